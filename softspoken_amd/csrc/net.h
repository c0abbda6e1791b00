// SpecUNet_2D's graph (pytorch_neural_nets.py:142-197), written down once: the tensors of an activation workspace and the ResBlocks in
// launch order.  Host only -- no kernel, no HIP call; it compiles alone.  engine.hip sizes the workspace and runs a pass from these tables,
// weights.hip builds the model from them; tests/test_net_table.py holds them to each other and to the tests' own copies of the graph.
#pragma once

namespace ss {

// one id per workspace tensor, in the arena's order
enum Act : int {
    kNoAct = -1,
    kH1, kC1, kP1, kH2, kC2, kP2, kH3, kC3, kP3, kH4, kC4, kP4, kHb, kBott, kHe, kEnc, kH6, kC6, kH7, kC7, kH8, kC8, kH9, kC9, kHs, kS9,
    // r = residual projection written by A launches that keep it (conv6, conv8, the spec head; every block in fp32 / f16x2)
    kR2, kR3, kR4, kRb, kRe, kR6, kR7, kR8, kR9, kRs,
    kActCount
};

// frag_order: stored in MFMA fragment order in f16x2 (the r tensors), never chunk-planar and not readable as [window][H][W][C]
struct ActInfo { const char* name; int H, W, C; bool frag_order; };
constexpr ActInfo kActs[kActCount] = {
    {"h1", 128, 256, 32, false}, {"c1", 128, 256, 32, false}, {"p1", 64, 128, 32, false}, {"h2", 64, 128, 64, false}, {"c2", 64, 128, 64, false},
    {"p2", 32, 64, 64, false},   {"h3", 32, 64, 96, false},   {"c3", 32, 64, 96, false},  {"p3", 16, 32, 96, false},  {"h4", 16, 32, 128, false},
    {"c4", 16, 32, 128, false},  {"p4", 8, 16, 128, false},   {"hb", 8, 16, 128, false},  {"bott", 8, 16, 128, false}, {"he", 8, 16, 128, false},
    {"enc", 8, 16, 128, false},  {"h6", 16, 32, 96, false},   {"c6", 16, 32, 96, false},  {"h7", 32, 64, 64, false},  {"c7", 32, 64, 64, false},
    {"h8", 64, 128, 32, false},  {"c8", 64, 128, 32, false},  {"h9", 128, 256, 32, false}, {"c9", 128, 256, 32, false},
    {"hs", 128, 256, 32, false}, {"s9", 128, 256, 32, false},
    {"r2", 64, 128, 64, true},   {"r3", 32, 64, 96, true},    {"r4", 16, 32, 128, true},  {"rb", 8, 16, 128, true},   {"re", 8, 16, 128, true},
    {"r6", 16, 32, 96, true},    {"r7", 32, 64, 64, true},    {"r8", 64, 128, 32, true},  {"r9", 128, 256, 32, true}, {"rs", 128, 256, 32, true}};

// the names ss_debug_activation knows beyond the workspace tensors (their exponents and "written" bits follow the tensors')
constexpr int kDbgFeat = kActCount, kDbgFlatPart = kActCount + 1, kDbgCount = kActCount + 2;

// One ResBlock (pytorch_neural_nets.py:7-41): launch A computes h (and the residual projection r) from the block input cat[x0, up2(x1)]
// (c0 + c1 channels; x1 at half resolution), launch B the block output y from h (and pool = maxpool2x2(y)).
struct Block {
    const char* name;
    int c0, c1, cout, H, W;
    Act x0, x1, h, r, y, pool;
    bool first_in_loader;      // conv1_1: no A launch -- B's loader computes the first conv from the features (h1 only exists on chip), and the
                               // 1 -> 32 residual is a rank-1 term of B
    bool flat_in_b;            // conv9_1: conv_flatten rides in B's epilogue; y itself is stored only when the spec head runs
    bool spec_only;            // the reference's dead head (worker.py:78-79 drops it): runs on request, always as A + r / B
};
constexpr Block kBlocks[] = {
    {"conv1_1", 1, 0, 32, 128, 256, kNoAct, kNoAct, kH1, kNoAct, kC1, kP1, true, false, false},
    {"conv2_1", 32, 0, 64, 64, 128, kP1, kNoAct, kH2, kR2, kC2, kP2, false, false, false},
    {"conv3_1", 64, 0, 96, 32, 64, kP2, kNoAct, kH3, kR3, kC3, kP3, false, false, false},
    {"conv4_1", 96, 0, 128, 16, 32, kP3, kNoAct, kH4, kR4, kC4, kP4, false, false, false},
    {"conv_bottleneck", 128, 0, 128, 8, 16, kP4, kNoAct, kHb, kRb, kBott, kNoAct, false, false, false},
    {"encoder_out", 128, 0, 128, 8, 16, kBott, kNoAct, kHe, kRe, kEnc, kNoAct, false, false, false},
    {"conv6", 128, 128, 96, 16, 32, kC4, kEnc, kH6, kR6, kC6, kNoAct, false, false, false},
    {"conv7", 96, 96, 64, 32, 64, kC3, kC6, kH7, kR7, kC7, kNoAct, false, false, false},
    {"conv8", 64, 64, 32, 64, 128, kC2, kC7, kH8, kR8, kC8, kNoAct, false, false, false},
    {"conv9_1", 32, 32, 32, 128, 256, kC1, kC8, kH9, kR9, kC9, kNoAct, false, true, false},
    {"spec_output_conv.0", 32, 0, 32, 128, 256, kC9, kNoAct, kHs, kRs, kS9, kNoAct, false, false, true}};
constexpr int kBlockCount = (int)(sizeof kBlocks / sizeof kBlocks[0]);

}  // namespace ss
