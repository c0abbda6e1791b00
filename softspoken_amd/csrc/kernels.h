// Internal launch interface between the host engine (engine.cpp) and the HIP kernels.
// Not part of the C ABI (include/softspoken.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <cstdlib>

#include "stream_desc.h"
#include "ingest_plan.h"

namespace ss {

// Development switches (tools/, tests of alternate kernel forms): compiled into libsoftspoken_hip_dev.so only (-DSS_DEVBUILD).
// The product library has every default fixed at build time and reads two environment variables in all: SOFTSPOKEN_CHUNK and
// SOFTSPOKEN_PRECISION.
#ifdef SS_DEVBUILD
static inline int dev_env(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
#else
static constexpr int dev_env(const char*, int dflt) { return dflt; }
#endif

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel: a process with contexts on several devices
// (ss_create takes a device id) must set it on each, and contexts run on several host threads.  done: one bit per device, per kernel.
inline hipError_t allow_full_lds(const void* kernel, std::atomic<uint64_t>& done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
    return e;
}

// ---- byte order of a 16-bit activation tensor ---------------------------------------------------------------------------------
// Every loader and storer of the 16-bit conv kernels works on (32-channel chunk x pixels), so a tensor's place of (n, y, x, c) is
// given by two strides beside the window stride H W C 2:
//   offset = n (H W C 2) + (c / 32) chunk + (y W + x) pix + (c % 32) 2
//   pixel-major, [window][H][W][C]:               pix = 2 C, chunk = 64        (bf16; f16x2 tensors of 32 channels; SOFTSPOKEN_LAYOUT=0)
//   chunk-planar, [window][C / 32][H][W][32]:     pix = 64,  chunk = H W 64    (f16x2 tensors wider than 32 channels)
// Both fill the same H W C 2 bytes of a window, and for C = 32 they are the same order.  Chunk-planar, a chunk's patch row is 18
// pixels x 64 B of contiguous memory: every 128-byte line a stage fetches is consumed by that stage, and a wave's 16-byte-per-lane
// load or store covers 1 KB of whole lines (pixel-major it covers sixteen half-used lines, and the line's other half is fetched
// again two stages later -- profiles/r05_fetch_order.md, profiles/r08_chunk_planar.md).
// fp32 tensors (conv2*.hip) are [window][H][W][C] and do not use the rule.
static constexpr bool kActChunkPlanar = true;       // the product's order for the f16x2 tensors wider than 32 channels
struct ActStride { uint32_t pix, chunk; };          // bytes from a pixel to the next / from a 32-channel chunk to the next
__host__ __device__ inline ActStride act_stride(int H, int W, int C, bool planar) {
    return (planar && C > 32) ? ActStride{64u, (uint32_t)H * (uint32_t)W * 64u} : ActStride{2u * (uint32_t)C, 64u};
}
__host__ __device__ inline uint32_t act_window_bytes(int H, int W, int C) { return (uint32_t)H * (uint32_t)W * (uint32_t)C * 2u; }
// byte offset of (n, y, x, c) from the tensor's first byte, mod 2^32 (the supports predicates hold a tensor below 4 GB).  y and x may
// be -1 (a patch origin): the pieces that are read lie inside the picture, and their offsets come out right mod 2^32
__host__ __device__ inline uint32_t act_offset(ActStride s, int H, int W, int C, int n, int y, int x, int c) {
    return (uint32_t)n * act_window_bytes(H, W, C) + (uint32_t)(c >> 5) * s.chunk + (uint32_t)(y * W + x) * s.pix + (uint32_t)(c & 31) * 2u;
}

// ---- implicit-GEMM 3x3 (+ fused 1x1 residual) convolution on MFMA ---------------------------------
// Element type float (conv2*.hip, [window][H][W][C]) or 16 bits (byte order: ActStride above).  One launch computes
//   out = act( conv3x3(cat[src0, up2(src1)]) + conv1x1(cat[res0, up2(res1)]) + rank1 + bias )
// where every term but the 3x3 is optional, and optionally also writes maxpool2x2(out).
struct ConvArgs {
    const void* src0; const void* src1;   // 3x3 input: [N][H][W][C0] and (nullable) [N][H/2][W/2][C1], nearest-upsampled
    const void* res0; const void* res1;   // 1x1 input, same convention (R0 / R1 channels)
    const void* wpk;                      // weights in MFMA fragment order (pack_conv_weights in engine.cpp)
    const float* bias;                    // [Cout] folded BatchNorm shift(s)
    const float* rank1_src;               // (nullable) [N][H][W] fp32 single-channel input of a 1->Cout 1x1 conv
    const float* rank1_w;                 // [Cout]
    void* out;                            // [N][H][W][Cout]
    void* pool_out;                       // (nullable) [N][H/2][W/2][Cout]
    int N, H, W, C0, C1, R0, R1, Cout;
    int relu;
    int tiles_y, tiles_x;
    int dbg;                              // ablation switches for tools/ (0 in production)
    // conv2.hip fusions (null = off)
    const float* first_w; const float* first_b;   // FIRST: conv1_1.conv1 folded weights [9][32] + bias [32]; input = rank1_src
    const void* flat_w; float* flat_part;         // FLAT: conv_flatten weights as MFMA fragments per mel row pair (columns 0-3 / 4-7); partial sums [N][H/4][4][W]
    int store_out;                                // FLAT: also write `out` (needed when the spec head runs)
    const void* flat_w4;                          // FLAT in conv4.hip: [128 rows][2 steps][64 lanes][8 bf16], channel order of the packed results
    void* res_out; const float* res_bias;         // A launch (RES): r = conv1x1(x) + br -> [N][H][W][Cout], weights = tap 9 of each chunk
    const void* res_in;                           // B launch: r, added before the ReLU
    const void* wpk_b; const float* bias_a;       // fused ResBlock (conv3.hip): launch-B weights, b1 (bias = b2 + br)
    // conv4.hip, "projection in B": launch A writes h only (plain = 1); launch B computes the block's 1x1 projection itself from the
    // centre pixels of the block input x = cat[xp0 (C0x channels), up2(xp1) (C1x channels)], read straight from memory as MFMA operands
    int plain;
    const void* proj_w;                           // [(C0x + C1x) / 16 steps][NT][64 lanes][8 bf16]: projection weights, A-operand order
    const void* xp0; const void* xp1; int C0x, C1x;
    // f16x2 mode: every activation tensor is two f16 planes (high and low halves of the values); a tensor pointer names the high
    // plane and the low plane lies lo_delta bytes behind it (the same distance for every tensor of a workspace)
    int64_t lo_delta;
    int* range_flag;                              // f16x2: set to 1 when a value that is being split does not fit an f16 (overflow, NaN)
    void* stamps;                                 // dev build: [grid][waves][8] uint32 segment times of a stage (null otherwise)
    // 16-bit kernels (conv4.hip, conv4_ups.hip): byte order of src0 / src1 / out / pool_out / xp0 / xp1 (res_in and a bf16 res_out: as out)
    ActStride s_src0, s_src1, s_out, s_pool, s_xp0, s_xp1;
};
// ---- work order of the four-tile ring kernels (conv4.hip RING, conv4_ups.hip conv3x3_upsr_kernel) ----------------
// A launch has total_pos positions (8 x 16-pixel tiles) x ngroups groups of 32 output channels.  XCD x owns the positions
// [x per_pos, x per_pos + lim), per_pos = ceil(total_pos / 8); a QUAD is four consecutive positions of that range, one per tile of a
// workgroup.  The XCD's G = gridDim.x / 8 workgroups walk items; all four tiles of a workgroup carry the same group in an item (they
// share one bank ring), and a tile whose position lies past the range has no work in that item and only keeps the beat.
//   side by side (the product): the XCD's items are (quad, group), group fastest, and workgroup w takes items w, w + G, w + 2 G, ...:
//     a quad's groups run at the same time on neighbouring workgroups of one XCD, so the quad's input patches are fetched from the
//     fabric once and found in that XCD's L2 (or merged with the miss in flight) by the other groups' readers;
//   sequential (development build, SOFTSPOKEN_ORDER=0; the order up to round 4): workgroup w takes quads w, w + G, ... and walks each
//     quad's groups one after the other -- between two readings of a patch the XCD's other tiles pull several L2s' worth through.
// Both orders give every (position, group) to exactly one tile, and with one group they are the same map.
static constexpr bool kOrderSideBySide = true;      // the product's order
struct RingItem { int pos, g; };                    // pos < 0: no work for this tile (g is the workgroup's group all the same)
__host__ __device__ inline int ring_lim(int xcd, int total_pos) {   // positions of the XCD
    const int per_pos = (total_pos + 7) >> 3, left = total_pos - xcd * per_pos;
    return left < 0 ? 0 : left < per_pos ? left : per_pos;
}
// group of a workgroup's item i: g0 + i * step (mod ngroups)
__host__ __device__ inline int ring_group0(int wg, int ngroups, bool seq) { return seq ? 0 : wg % ngroups; }
__host__ __device__ inline int ring_group_step(int G, int ngroups, bool seq) { return seq ? 1 % ngroups : G % ngroups; }
// item `item` of tile `tile` (0..3) of workgroup `wg` (0..G-1) on XCD `xcd`
__host__ __device__ inline RingItem ring_item(int xcd, int wg, int G, int item, int tile, int total_pos, int ngroups, bool seq) {
    const int lim = ring_lim(xcd, total_pos);
    int quad, g;
    if (seq) { quad = wg + (item / ngroups) * G; g = item % ngroups; }
    else { const int j = wg + item * G; quad = j / ngroups; g = j - quad * ngroups; }
    const int idx = 4 * quad + tile;
    return RingItem{idx < lim ? xcd * ((total_pos + 7) >> 3) + idx : -1, g};
}
// items in which that tile has work: its first ring_items items (a tile never has work again behind an item without)
__host__ __device__ inline int ring_items(int xcd, int wg, int G, int tile, int total_pos, int ngroups, bool seq) {
    const int lim = ring_lim(xcd, total_pos);
    const int quads = lim > tile ? (lim - tile + 3) >> 2 : 0;             // quads in which the tile's position exists
    if (seq) return quads > wg ? (quads - wg + G - 1) / G * ngroups : 0;
    const int n = quads * ngroups;
    return n > wg ? (n - wg + G - 1) / G : 0;
}

// ---- work order "one group per workgroup" (conv4.hip GRES: a group's banks resident in the workgroup's LDS) ----------------------
// The XCDs own the positions as above (ring_lim).  Of an XCD's G workgroups, workgroup w carries group w mod ngroups for its whole life
// and belongs to slot w / ngroups; the S = G / ngroups slots deal the XCD's positions among themselves, nh consecutive ones per item
// (one per tile of the workgroup): item i of slot s is the positions (s + i S) nh + tile.  The ngroups workgroups of a slot are
// neighbours on one XCD and walk the SAME position sequence at the same time, so a position's patches come from the fabric once and
// the siblings find them in that XCD's L2 -- and a workgroup loads its group's banks once per launch.
// The form needs G to be a multiple of ngroups: gres_grid_ok is the chooser's predicate, gres_grid the grid it asks for.
__host__ __device__ inline bool gres_grid_ok(int grid, int ngroups) { return grid > 0 && ngroups > 0 && grid % (8 * ngroups) == 0; }
// workgroups of a launch on num_cus CUs: one per CU, fewer when the busiest XCD has fewer items than slots; 0 = the form does not apply
__host__ __device__ inline int gres_grid(int num_cus, int total_pos, int ngroups, int nh) {
    int G = (num_cus + 7) / 8;
    if (ngroups <= 0 || G % ngroups) return 0;
    const int units = (((total_pos + 7) >> 3) + nh - 1) / nh;        // items of the busiest XCD (XCD 0)
    if (units < G / ngroups) G = (units > 0 ? units : 1) * ngroups;
    return 8 * G;
}
__host__ __device__ inline int gres_group(int wg, int ngroups) { return wg % ngroups; }
// item `item` of tile `tile` (0..nh-1) of workgroup `wg` (0..G-1) on XCD `xcd`; pos < 0: no work for this tile
__host__ __device__ inline RingItem gres_item(int xcd, int wg, int G, int item, int tile, int total_pos, int ngroups, int nh) {
    const int lim = ring_lim(xcd, total_pos), S = G / ngroups;
    const int idx = (wg / ngroups + item * S) * nh + tile;
    return RingItem{idx < lim ? xcd * ((total_pos + 7) >> 3) + idx : -1, wg % ngroups};
}
// items in which that tile has work: its first gres_items items
__host__ __device__ inline int gres_items(int xcd, int wg, int G, int tile, int total_pos, int ngroups, int nh) {
    const int lim = ring_lim(xcd, total_pos), S = G / ngroups, s = wg / ngroups;
    const int units = lim > tile ? (lim - tile + nh - 1) / nh : 0;    // items of the XCD in which the tile's position exists
    return units > s ? (units - s + S - 1) / S : 0;
}

// NT = number of 32-wide output-channel tiles per block (1..3); Cout % (32*NT) == 0.
// second structure (conv2.hip): persistent blocks, register prefetch, resident weights, staged stores
hipError_t launch_conv3x3_v2(const ConvArgs& a, bool bf16, int NT, int num_cus, hipStream_t s);
const char* conv_v2_variant(const ConvArgs& a, bool bf16, int NT, int num_cus);   // instantiation name, as rocprofv3 prints it
int conv_v2_flat_groups(bool bf16);   // row groups per window in ConvArgs::flat_part
// conv4.hip: 16-bit operands on the bf16 / f16 matrix instructions, A / B launches of a ResBlock (inputs need the engine's 256-byte
// zero header).  prec: 1 = bf16 (one plane per tensor), 2 = f16x2 (two f16 planes per tensor, three products per term)
bool conv_v4_supports(const ConvArgs& a, int NT, int num_cus, int prec);
const char* conv_v4_variant(const ConvArgs& a, int NT, int num_cus, int prec);
int conv_v4_flat_groups();           // row groups per window in ConvArgs::flat_part when conv4.hip's FLAT launch ran
hipError_t launch_conv3x3_v4(const ConvArgs& a, int NT, int num_cus, int prec, hipStream_t s);

// conv4_ups.hip (f16x2): the plain A launch of a decoder block whose upsampled input half runs at low resolution with four pre-summed
// taps per output parity class (weights: weights.hip pack_conv_split_ups, conv_ups_weight_bytes of them)
bool conv_ups_supports(const ConvArgs& a, int num_cus);
const char* conv_ups_variant();
size_t conv_ups_weight_bytes(int C0, int C1);
hipError_t launch_conv3x3_ups(const ConvArgs& a, int num_cus, hipStream_t s);
// ... and the A launch that also writes the block's 1x1 projection r (res_out), any number of 32-channel output groups, its banks
// streamed through a three-slot ring of half-chunk entries (weights: pack_conv_split_upsr; biases travel inside them)
bool conv_upsr_supports(const ConvArgs& a, int num_cus);
const char* conv_upsr_variant();
size_t conv_upsr_weight_bytes(int C0, int C1, int Cout);
hipError_t launch_conv3x3_upsr(const ConvArgs& a, int num_cus, hipStream_t s);

// conv2_ups.hip (fp32): the A launch of a decoder block (h -> out, r -> res_out) with four pre-summed taps per output parity class on
// the upsampled input half (weights: weights.hip pack_conv_v2_ups, conv_ups32_weight_bytes of them); Cout = 32, 64 or 96
// NT: 32-channel output tiles per block (the bank is packed for it); Cout / (32 NT) output-channel groups are separate tiles
// MTW: M-tiles per wave (1: 8 waves per block, 2: 4 waves, each the two halves of one parity class)
bool conv_ups32_supports(const ConvArgs& a, int NT, int MTW, int num_cus);
const char* conv_ups32_variant(int NT, int MTW);
size_t conv_ups32_weight_bytes(int C0, int C1, int Cout);
hipError_t launch_conv3x3_ups32(const ConvArgs& a, int NT, int MTW, int num_cus, hipStream_t s);

// conv1s.hip (f16x2): conv1_1 as a row-streaming kernel -- a wave owns a 32-column strip, h1 stays in registers, no LDS traffic but the
// weight fragments, no barrier after the prologue.  wpk: pack_conv_stream's banks (conv1_stream_weight_bytes); the other fields as for
// conv4.hip's FIRST + RANK1 + POOL launch (first_w / first_b, rank1_src = features, rank1_w, bias = b2 + br, out, pool_out).
// rows_per_unit: rows of a (window, band, strip) work unit (even, divides 128)
bool conv1_stream_supports(const ConvArgs& a);
const char* conv1_stream_variant(const ConvArgs& a, int form);   // (a.plain = 1: the f16 range of h1 and c1 is proven from the weights, no run-time test)
size_t conv1_stream_weight_bytes();
// form: 32 = one 32-column tile per strip row on v_mfma_f32_32x32x16_f16 (wpk: pack_conv_stream), 16 = two interleaved 16-pixel tiles on
// v_mfma_f32_16x16x32_f16 (wpk: pack_conv_stream16; same size)
hipError_t launch_conv1_stream(const ConvArgs& a, int form, int rows_per_unit, int num_cus, hipStream_t s);

// conv9s.hip (f16x2): conv9_1.B as a row-streaming kernel on the same core (stream16.h) -- h9, c1 and c8 are read from memory as MFMA
// operands, no patch image, no barrier after the prologue; conv_flatten in the epilogue, c9 written when store_out is set.  Fields as for
// conv4.hip's projection-in-B FLAT launch, except: wpk = pack_conv_stream16's banks of the second conv, proj_w = pack_proj_stream16's
// fragments (conv9_stream_proj_bytes), flat_w4 = pack_flat_rows' table (conv9_stream_flat_bytes).  flat_part receives
// conv9_stream_flat_groups(rows_per_unit) row groups per window.  grid_override > 0: at most that many workgroups (development build).
bool conv9_stream_supports(const ConvArgs& a);
const char* conv9_stream_variant();
size_t conv9_stream_proj_bytes();
size_t conv9_stream_flat_bytes();
bool conv9_stream_rows_ok(int rows_per_unit);        // even, divides 128, at most 32
int conv9_stream_flat_groups(int rows_per_unit);
double conv9_stream_issued_macs(int N);
hipError_t launch_conv9_stream(const ConvArgs& a, int rows_per_unit, int grid_override, int num_cus, hipStream_t s);

// conv9a.hip (f16x2): conv9_1.A as a row-streaming kernel on stream16.h's core without overlap columns -- c1 and c8 are read from memory
// as MFMA operands, the upsampled half at c8's resolution against pre-summed taps.  Fields as for conv4_ups.hip's plain A launch, except:
// wpk = pack_conv_stream16's banks of the conv's first 32 input channels, wpk_b = pack_ups_stream16's sets (conv9a_stream_ups_bytes).
// rows_per_unit, grid_override: as for conv9s.hip.
bool conv9a_stream_supports(const ConvArgs& a);
const char* conv9a_stream_variant();
size_t conv9a_stream_ups_bytes();
bool conv9a_stream_rows_ok(int rows_per_unit);       // even, divides 128, at most 32
double conv9a_stream_issued_macs(int N);
hipError_t launch_conv9a_stream(const ConvArgs& a, int rows_per_unit, int grid_override, int num_cus, hipStream_t s);

// heads.hip
// ResBlock1D(4,4) + Conv1d(4,1,1) fed by the FLAT partial sums [N][n_parts][4][256]: sums them in order, adds conv_flatten's bias,
// ReLU, then the 1-D head -> logits [N][256]
// fscale: exact power of two that takes conv_flatten's partial sums back to true units (f16x2 channel normalisation; 1 otherwise)
struct Head1dWeights { float w1[4][4][3], b1[4], w2[4][4][3], wr[4][4], b2r[4], wo[4], bo, fscale; };
hipError_t launch_mask_head_parts(const float* parts, int n_parts, const float* flat_bias, const Head1dWeights& hw, float* logits,
                                  int N, hipStream_t s);
// spec head tail: Conv2d(32,2,1) + bias + ReLU: x NHWC [N][128][256][32] -> spec NCHW [N][2][128][256] fp32
// prec: 0 = fp32 activations, 1 = bf16, 2 = two f16 planes (lo_delta apart)
hipError_t launch_spec_tail(const void* x, int64_t lo_delta, const float* w /*[2][32]*/, const float* bias, float* spec, int N, int prec,
                            hipStream_t s);

// ---- front-end ----------------------------------------------------------------------------------------
static constexpr int kMelLo = 10, kMelHi = 32, kMelPitch = 43;   // taps of a lane's narrow / wide filter; odd LDS pitch
struct FrontendTables {
    const float4* pretw;    // [4][256]: window x pre-twiddle, (w0*c, w1*s, w0*s, w1*c) for z[n] * W1024^(n r)
    const float2* w2048;    // [2048]: exp(-2 pi i j / 2048)
    const int* mel_start;   // [128] first bin of filter j
    const int* mel_count;   // [128] number of bins
    const int* mel_off;     // [128] offset into mel_w
    const float* mel_w;     // packed non-zero weights, ascending bin
    int mel_nw;             // number of packed weights (<= 1536)
    const float* mel_wp;    // [64][kMelPitch]: lane l's filters l (kMelLo taps) and 127 - l (kMelHi taps), zero-padded
    int dbg;                // ablation switches for tools/ (0 in production); bit 8: the first kernel (dev build A/B runs)
    // second kernel (16 lanes per frame, passes r = 0..3)
    const float2* win2;     // [256]: (w[2n], w[2n+1])
    const float2* twt;      // [4][16 n0][16 m0]: W1024^(n0 (4 m0 + r)), the twiddle between the two radix-16 passes
    const float2* wkt;      // [4][16 m1][16 m0]: W2048^(4 (m0 + 16 m1) + r), the real-FFT untangle's twiddle
    const float* mel_wq;    // [64][kMelRow]: lane l's weights for paired reads: 2 kMelPairsLo of filter l, 2 kMelPairsHi of filter 127 - l
    const int* mel_p0;      // [64][2]: first word of those two runs in the padded power-spectrum buffer (even)
};
static constexpr int kMelPairsLo = 9, kMelPairsHi = 20, kMelRow = 60;    // 8-byte reads per narrow / wide filter; row pitch (16-byte multiple)
static constexpr int kPwWords = 816;                                      // 768 bins + 4 pad words behind every 64
// windows: arena offsets of each window's first sample.  feat: [n][128][256] fp32.
hipError_t launch_frontend(const float* arena, const int64_t* win_off, int n, const FrontendTables& t, float* feat,
                           int num_cus, hipStream_t s);

// ---- decode / mixdown / resample ----------------------------------------------------------------------
// (ingest.hip; descriptors BatchFile / ChanFile: stream_desc.h; geometries Res3Geom / ResGeom: ingest_plan.h)
// batched: every file of a job in one launch; sr == 22050 files go mono -> arena directly
hipError_t launch_decode_mono_batch(const void* pcm, int format, int channels, const BatchFile* d_files, int n_files,
                                    int64_t max_frames, float* mono, hipStream_t s);
// review-screen spectrogram: |STFT| with n_fft = win = 512, hop 256, centred, zero-padded -> [257][n_frames]
hipError_t launch_stft512_mag(const float* x, int64_t n, int64_t n_frames, float* out, int num_cus, hipStream_t s);
// silencer: decode -> zero [begin,end) frame ranges (disjoint, ascending) -> 16-bit PCM
hipError_t launch_silence_encode(const void* pcm, int format, int channels, int64_t frames, const int64_t* d_ranges, int n_ranges,
                                 short* out, hipStream_t s);
// source-encoding silencer: the nbytes of pcm with the bytes inside d_byte_ranges (disjoint ascending [begin, end) byte pairs) replaced
// by the zero byte of `format`; pcm and out 16-byte aligned
hipError_t launch_silence_source(const void* pcm, int64_t nbytes, const int64_t* d_byte_ranges, int n_ranges, int format, void* out, hipStream_t s);
// decode + mixdown + polyphase resampling in one launch (no mono tensor), where res3_geometry applies; ipf: items per file
hipError_t launch_resample_fused(const void* pcm, int format, int channels, const BatchFile* d_files, int n_files, const Res3Geom& gm, int64_t ipf,
                                 int L, int M, int half, const float* taps, float* arena, int num_cus, hipStream_t s);
hipError_t launch_resample_batch(const float* mono, const BatchFile* d_files, int n_files, int64_t max_out, const ResGeom& gm, int L, int M, int half,
                                 const float* taps, float* arena, int num_cus, hipStream_t s);
// per-channel ingest (no mixdown): channel c of a recording is decoded to dst[mono_off + c mono_stride ..) / resampled to
// arena[out_off + c out_stride ..); one descriptor per recording, the channels' planes a constant stride apart
hipError_t launch_decode_channels_batch(const void* pcm, int format, int channels, const ChanFile* d_files, int n_files, int64_t max_frames,
                                        float* dst, hipStream_t s);
// the fused form: the PCM of a tile fetched once for two channels, the channels taking turns in the one LDS tile
hipError_t launch_resample_fused_channels(const void* pcm, int format, int channels, const ChanFile* d_files, int n_files, const Res3Geom& gm,
                                          int64_t ipf, int L, int M, int half, const float* taps, float* arena, int num_cus, hipStream_t s);

// ---- overlap averaging (NNDetector.py:153-190), double accumulation ---------------------------------
// s_b: bins between window starts (window step x 256 / 3), from which a bin's candidate windows are bounded; starts: the windows' first bins
struct AvgFile { int64_t logit_off; int64_t bin_off; int32_t W; int32_t n_bins; int64_t start_off; };
hipError_t launch_average(const float* logits, const AvgFile* files, int n_files, const int32_t* starts, double s_b, double* avg,
                          int32_t* count, int max_bins, hipStream_t s);
// covered / above-threshold bit per bin, 64 bins per word (words = ceil(total_bins / 64), both arrays)
hipError_t launch_bin_masks(const double* avg, const int32_t* count, int64_t total_bins, double threshold, unsigned long long* above,
                            unsigned long long* covered, hipStream_t s);
// ss_get_region_peaks: peaks[r * n_channels + c] = max of avg[chan_off[c] + j] over the covered, non-NaN bins j of [rng[2 r], rng[2 r + 1]]
// (-inf when there is none); one block per (region, channel)
hipError_t launch_region_peaks(const double* avg, const int32_t* count, const int64_t* chan_off, int n_channels, const int64_t* rng,
                               int64_t n_regions, double* peaks, hipStream_t s);

// ---- streaming detection (stream.hip): one launch per step for all streams, a descriptor per stream ----------------------------
// (the descriptors: stream_desc.h)
hipError_t launch_stream_silence(const StreamSilence* d, int n, int64_t max_samples, short* out, hipStream_t s);
hipError_t launch_stream_copy_bytes(const StreamCopyBytes* d, int n, int64_t max_bytes, hipStream_t s);
hipError_t launch_stream_silence_source(const StreamSilenceSource* d, int n, int64_t max_bytes, unsigned char* out, hipStream_t s);
hipError_t launch_stream_copy(const StreamCopy* d, int n, int64_t max_n, hipStream_t s);
hipError_t launch_stream_decode(const void* pcm, const StreamDecode* d, int n, int64_t max_frames, hipStream_t s);
hipError_t launch_stream_resample(const StreamResample* d, int n, int64_t max_n, hipStream_t s);
hipError_t launch_stream_average(const StreamAvg* d, int n, int64_t max_bins, double* avg, unsigned char* flags, hipStream_t s);
hipError_t launch_stream_decode_channels(const void* pcm, const StreamDecodeChannels* d, int n, int64_t max_frames, hipStream_t s);
hipError_t launch_stream_union(const StreamUnion* d, int n, int64_t max_bins, double* avg, unsigned char* flags, hipStream_t s);

}  // namespace ss
