// Plan + launch unit: the activation workspace, the launch sequence of SpecUNet_2D for one chunk of windows, and the two
// halves of a job (plan + enqueue, wait).  Reference files are cited per function (paths relative to the reference root).
#include "engine.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace ss {

// ------------------------------------------------------------------------------------------------------
// errors, profiling events
// ------------------------------------------------------------------------------------------------------
static thread_local std::string g_err;

int fail(ss_ctx* c, int code, const std::string& msg) {
    g_err = msg;
    if (c) c->err = msg;
    return code;
}
const char* thread_error() { return g_err.c_str(); }

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static int stat_id(ss_ctx* c, const std::string& name) {
    for (size_t i = 0; i < c->stats.size(); ++i) if (c->stats[i].name == name) return (int)i;
    KStat k; k.name = name; c->stats.push_back(k);
    return (int)c->stats.size() - 1;
}

ScopedLaunch::ScopedLaunch(ss_ctx* c_, hipStream_t stream_, const std::string& name, double flops, double bytes, double issued_macs)
    : c(c_), stream(stream_) {
    sid = stat_id(c, name);
    c->stats[sid].launches++; c->stats[sid].flops += flops; c->stats[sid].bytes += bytes;
    c->stats[sid].issued += 2.0 * (c->prec == kF16x2 ? 3.0 : 1.0) * (issued_macs >= 0 ? issued_macs : flops / 2.0);
    if (c->profile) {
        auto get = [&]() { hipEvent_t e; if (!c->evpool.empty()) { e = c->evpool.back(); c->evpool.pop_back(); } else hipEventCreate(&e); return e; };
        a = get(); b = get();
        hipEventRecord(a, stream);
    }
}
ScopedLaunch::~ScopedLaunch() {
    if (c->profile) { hipEventRecord(b, stream); c->pending.push_back({sid, a, b}); }
}

int range_clear(ss_ctx* c, hipStream_t stream) {
    if (c->d_range_flag) HIPCHK(c, hipMemsetAsync(c->d_range_flag, 0, 4, stream));
    return SS_OK;
}
int range_fetch(ss_ctx* c, hipStream_t stream) {
    if (c->d_range_flag) HIPCHK(c, hipMemcpyAsync(c->h_range_flag, c->d_range_flag, 4, hipMemcpyDeviceToHost, stream));
    return SS_OK;
}

void resolve_events(ss_ctx* c) {
    for (auto& p : c->pending) {
        float ms = 0;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) c->stats[p.sid].ms += ms;
        c->evpool.push_back(p.a); c->evpool.push_back(p.b);
    }
    c->pending.clear();
}

// ------------------------------------------------------------------------------------------------------
// activation workspace: tensors for `n` windows.  Every tensor is preceded by a 256-byte zero header (conv4.hip reads it
// for out-of-image patch pieces).  f16x2 mode keeps two planes per tensor (high and low halves of every value, both f16) in two
// arenas of identical layout, so that one byte distance (Workspace::lo_delta) leads from any high plane to its low plane.
// Byte order inside a tensor (kernels.h ActStride): [window][H][W][C] in fp32 and bf16; in f16x2 the tensors wider than 32 channels are
// chunk-planar, [window][C / 32][H][W][32] (the r tensors are in MFMA fragment order in f16x2 and have no such order).  The order is
// chosen per tensor here, when the workspace is built, and travels to the kernels as two strides per tensor; the window stride, the
// headers and lo_delta are the same in both orders.  Development build: SOFTSPOKEN_LAYOUT=0 keeps every tensor [window][H][W][C].
// ------------------------------------------------------------------------------------------------------
static constexpr size_t kActHeader = 256;

static void free_ws(Workspace& w) {
    // pointers are cleared BEFORE anything else can fail: a context whose growth failed holds no workspace at all (chunk = 0)
    // and the next call allocates afresh -- never a stale chunk over freed tensors
    void* const ps[] = {w.arena, w.feat, w.flat};
    w = Workspace();
    for (void* p : ps) if (p) hipFree(p);
}

void free_workspace(ss_ctx* c) {
    c->dbg_n = 0; c->dbg_ws = 0; c->dbg_written = 0;
    for (Workspace& w : c->ws) free_ws(w);
}

static hipError_t ws_malloc(ss_ctx* c, void** p, size_t bytes) {
    if (c->fail_alloc_after >= 0 && c->fail_alloc_after-- == 0) { *p = nullptr; return hipErrorOutOfMemory; }   // test hook
    return hipMalloc(p, bytes);
}

// one workspace for n windows, filled in place: arena (+ its tensors, net.h's kActs), feature and flatten-partial buffers; the zero headers
// are written on `stream`.  On failure everything it allocated is freed again (w is empty) and *what names the step.
static hipError_t alloc_ws(ss_ctx* c, int n, hipStream_t stream, Workspace& w, std::string& what) {
    const size_t es = c->prec == kFp32 ? 4 : 2;
    // one arena, one size (the spec head's tensors included): the workspace is sized once per context and chunk
    size_t total = 0;
    std::vector<size_t> offs;
    for (const ActInfo& t : kActs) {
        offs.push_back(total + kActHeader);
        total += kActHeader + (((size_t)n * t.H * t.W * t.C * es + 255) & ~(size_t)255);
    }
    const int planes = c->prec == kF16x2 ? 2 : 1;
    const size_t feat_b = (size_t)n * 128 * 256 * 4, flat_b = (size_t)n * 64 * 4 * 256 * 4;
    hipError_t e = ws_malloc(c, &w.arena, total * planes);
    if (e != hipSuccess) { what = "activation workspace (" + std::to_string(total * planes >> 20) + " MiB)"; free_ws(w); return e; }
    if ((e = ws_malloc(c, (void**)&w.feat, feat_b)) != hipSuccess || (e = ws_malloc(c, (void**)&w.flat, flat_b)) != hipSuccess) {
        what = "activation workspace"; free_ws(w); return e;
    }
    for (int pl = 0; pl < planes; ++pl)
        for (size_t off : offs) {
            e = hipMemsetAsync((char*)w.arena + pl * total + off - kActHeader, 0, kActHeader, stream);
            if (e != hipSuccess) { what = "hipMemsetAsync"; free_ws(w); return e; }
        }
    const bool planar = c->prec == kF16x2 && dev_env("SOFTSPOKEN_LAYOUT", kActChunkPlanar ? 1 : 0) != 0;
    for (int i = 0; i < kActCount; ++i) {
        const ActInfo& t = kActs[i];
        w.t[i].p = (char*)w.arena + offs[i];
        if (c->prec != kFp32) w.t[i].s = act_stride(t.H, t.W, t.C, planar && !t.frag_order);     // (fp32: no byte order, {0, 0})
    }
    w.lo_delta = planes == 2 ? (int64_t)total : 0;
    w.bytes = (int64_t)(total * planes + feat_b + flat_b);
    w.chunk = n;
    return hipSuccess;
}

int ensure_workspace(ss_ctx* c, int n) {
    if (n <= c->ws[0].chunk) return SS_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->lane_stream) HIPCHK(c, hipStreamSynchronize(c->lane_stream));
    free_workspace(c);
    std::string what;
    const hipError_t e = alloc_ws(c, n, c->stream, c->ws[0], what);
    if (e != hipSuccess) return fail(c, what == "hipMemsetAsync" ? SS_ERR_HIP : SS_ERR_NOMEM, what + ": " + hipGetErrorString(e));
    return SS_OK;
}

// the second lane for passes of n windows; false (and no lane) when the memory is not there -- the run then uses one lane
static bool ensure_lane(ss_ctx* c, int n) {
    Workspace& w = c->ws[1];
    if (w.chunk >= n) return true;
    if (!c->lane_stream) {
        if (hipStreamCreateWithFlags(&c->lane_stream, hipStreamNonBlocking) != hipSuccess) { c->lane_stream = nullptr; return false; }
        if (hipEventCreateWithFlags(&c->lane_ev_in, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->lane_ev_out, hipEventDisableTiming) != hipSuccess) return false;
    }
    hipStreamSynchronize(c->lane_stream);
    free_ws(w);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || (int64_t)free_b < c->ws[0].bytes + ((int64_t)4 << 30)) return false;   // (leave room for the caller's buffers)
    std::string what;
    if (alloc_ws(c, n, c->lane_stream, w, what) != hipSuccess) { (void)hipGetLastError(); return false; }
    return true;
}

// ------------------------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------------------------
static int base_dbg() {
    // product build: 32 (raised wave priority inside conv4.hip's MFMA loop: the measured default); dev build: + SOFTSPOKEN_DBG bits, and bit 9 =
    // the ring kernels' side-by-side work order (kernels.h; SOFTSPOKEN_ORDER=0: the sequential one; the product's order is compiled in)
    return (dev_env("SOFTSPOKEN_PRIO", 1) ? 32 : 0) | (dev_env("SOFTSPOKEN_ORDER", kOrderSideBySide ? 1 : 0) ? 512 : 0) | dev_env("SOFTSPOKEN_DBG", 0);
}

#ifdef SS_DEVBUILD
// SOFTSPOKEN_STAMP_LAYER=<layer name>: segment times of that launch's stages (shader clock, summed per wave) on stderr
struct StageStamps {
    void* d_st = nullptr;
    static constexpr size_t st_bytes = (size_t)4096 * 8 * 16 * 4;
    int begin(ss_ctx* c, hipStream_t stream, const std::string& name, ConvArgs& a) {
        const char* want = getenv("SOFTSPOKEN_STAMP_LAYER");
        if (want && name == want) { HIPCHK(c, hipMalloc(&d_st, st_bytes)); HIPCHK(c, hipMemsetAsync(d_st, 0, st_bytes, stream)); a.stamps = d_st; }
        return SS_OK;
    }
    int end(ss_ctx* c, hipStream_t stream, const std::string& name, int n) {
        if (!d_st) return SS_OK;
        std::vector<uint32_t> h(st_bytes / 4);
        HIPCHK(c, hipMemcpyAsync(h.data(), d_st, st_bytes, hipMemcpyDeviceToHost, stream));
        HIPCHK(c, hipStreamSynchronize(stream));
        double sum[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, stages = 0; int waves = 0;
        for (size_t w = 0; w < h.size() / 16; ++w) if (h[w * 16 + 5]) {
            ++waves; stages += h[w * 16 + 5];
            for (int i = 0; i < 5; ++i) sum[i] += h[w * 16 + i];
            for (int i = 5; i < 12; ++i) sum[i] += h[w * 16 + i + 1];
        }
        if (waves)
            fprintf(stderr, "[stamps] %s n=%d: %d waves, %.1f stages/wave; cycles per stage: mfma %.0f | barrier1 %.0f | commit+issue %.0f (wait for loads %.0f, LDS writes %.0f, next stage %.0f, patch loads %.0f, one stamp %.0f) | barrier2 %.0f | epilogue %.0f (f16x2: residual add incl. its wait %.0f, the last stage's work %.0f)\n",
                    name.c_str(), n, waves, stages / waves, sum[0] / stages, sum[1] / stages, sum[2] / stages, sum[5] / stages, sum[6] / stages, sum[7] / stages, sum[8] / stages, sum[9] / stages, sum[3] / stages, sum[4] / stages, sum[10] / stages, sum[11] / stages);
        hipFree(d_st); d_st = nullptr;
        return SS_OK;
    }
};
#else
struct StageStamps {
    int begin(ss_ctx*, hipStream_t, const std::string&, ConvArgs&) { return SS_OK; }
    int end(ss_ctx*, hipStream_t, const std::string&, int) { return SS_OK; }
};
#endif

// One conv launch with its bookkeeping: the stat entry "<instantiation as rocprofv3 prints it>/<layer>", the dev build's stage stamps
// when this layer's are asked for (stamped: the form takes them), the launch on `stream`, its error.  issued: as ScopedLaunch's issued_macs.
template <typename LaunchFn>
static int conv_launch(ss_ctx* c, hipStream_t stream, const char* variant, const std::string& layer, ConvArgs& a, double flops, double bytes,
                       double issued, bool stamped, LaunchFn&& launch) {
    StageStamps stamps;
    if (stamped) if (int rc = stamps.begin(c, stream, layer, a)) return rc;
    {
        ScopedLaunch sl(c, stream, std::string(variant) + "/" + layer, flops, bytes, issued);
        HIPCHK(c, launch(a));
    }
    return stamps.end(c, stream, layer, a.N);
}

// The kernel forms that can serve a launch of a ResBlock half
enum Form {
    kNoForm,            // no launch
    kConv2,             // conv2.hip: fp32, and bf16 under SOFTSPOKEN_CONV4=0
    kConv4,             // conv4.hip: bf16 / f16x2
    kConv4UpsPlain,     // conv4_ups.hip, plain A launch: the upsampled input half at low resolution, four pre-summed taps per parity class
    kConv4UpsRing,      // conv4_ups.hip, ring form: the same for the A launch that also writes r
    kConv2Ups,          // conv2_ups.hip: the same idea on the fp32 matrix instruction
    kConv1Stream16,     // conv1s.hip: conv1_1 as a row-streaming kernel, 16-pixel form
    kConv1Stream32,     // ... its 32-column form (development build, SOFTSPOKEN_C1S_FORM=32)
    kConv9aStream,      // conv9a.hip: conv9_1.A row-streaming
    kConv9Stream        // conv9s.hip: conv9_1.B row-streaming, conv_flatten in its epilogue
};
struct Launch { Form form = kNoForm; ConvArgs a{}; };
// How one block runs.  proj: "projection in B" (conv4.hip RP) -- A writes h alone, B reads h and the centre pixels of the block input;
// otherwise A + r / B -- A computes h and the residual projection r, B computes the block output from h and adds r.  conv1_1 has no A.
// B2: development build, SOFTSPOKEN_C1S=2: conv4.hip's form of conv1_1 runs as well, behind the stream form -- an A/B aid.
struct BlockRun { bool proj = false; Launch A, B, B2; };

static int prec4(const ss_ctx* c) { return c->prec == kF16x2 ? 2 : 1; }
static int ups32_mtw(const ConvPlan& p) { return dev_env("SOFTSPOKEN_UPS32_MTW", 2) == 2 && p.ups32_nt < 3 ? 2 : 1; }

// The ConvArgs of block bi's two launches for n windows, in either way of running it -- the one place where tensors become ConvArgs fields.
// (The form chosen below may still swap in its own weight banks.)
static void fill_args(const ss_ctx* c, const Workspace& ws, int bi, int n, bool with_spec, BlockRun& r) {
    const Block& k = kBlocks[bi];
    const BlockPlan& p = c->convs[bi];
    auto T = [&](Act t) { return t == kNoAct ? ActTensor() : ws.t[t]; };
    // (conv1_1's B reads the fp32 features, not an h1 tensor: h1 only exists on chip)
    const ActTensor x0 = T(k.x0), x1 = T(k.x1), h = T(k.first_in_loader ? kNoAct : k.h), rr = T(k.r), y = T(k.y), pool = T(k.pool);
    ConvArgs& a = r.A.a; ConvArgs& b = r.B.a;
    a = b = ConvArgs{};
    a.N = b.N = n; a.H = b.H = k.H; a.W = b.W = k.W; a.Cout = b.Cout = k.cout; a.relu = b.relu = 1; a.store_out = b.store_out = 1;
    a.lo_delta = b.lo_delta = ws.lo_delta; a.range_flag = b.range_flag = c->d_range_flag; a.dbg = b.dbg = base_dbg();
    a.src0 = x0.p; a.s_src0 = x0.s; a.src1 = x1.p; a.s_src1 = x1.s; a.C0 = k.c0; a.C1 = k.c1; a.out = h.p; a.s_out = h.s; a.bias = p.A.d_bias2;
    b.src0 = h.p; b.s_src0 = h.s; b.C0 = k.cout; b.out = y.p; b.s_out = y.s; b.pool_out = pool.p; b.s_pool = pool.s; b.wpk = p.B.d_w2;   // B's 3x3 input is h
    if (r.proj) {
        a.wpk = p.A.d_w3; a.plain = 1;
        b.bias = p.B.d_bias3; b.proj_w = p.B.d_proj; b.xp0 = x0.p; b.s_xp0 = x0.s; b.xp1 = x1.p; b.s_xp1 = x1.s; b.C0x = k.c0; b.C1x = k.c1;
    } else {
        a.wpk = p.A.d_w2; a.res_out = rr.p; a.res_bias = p.A.d_res_bias;
        b.bias = p.B.d_bias2; b.res_in = rr.p; b.rank1_w = p.B.d_rank1;
    }
    if (k.first_in_loader) { b.first_w = c->d_first_w; b.first_b = c->d_first_b; b.rank1_src = ws.feat; }
    if (k.flat_in_b) { b.flat_w = r.proj ? nullptr : c->d_flat_frag; b.flat_w4 = c->d_flat_frag4; b.flat_part = ws.flat; b.store_out = with_spec ? 1 : 0; }
}

// the tile forms every launch can end on; false: none (f16x2 has only conv4.hip)
static bool choose_tile(const ss_ctx* c, const ConvPlan& p, Launch& l) {
    if (c->prec != kFp32 && dev_env("SOFTSPOKEN_CONV4", 1) && conv_v4_supports(l.a, p.NT, c->num_cus, prec4(c))) l.form = kConv4;
    else if (c->prec != kF16x2) l.form = kConv2;
    return l.form != kNoForm;
}

// an A launch that also writes r: the decoder forms with the upsampled input half at low resolution first
static bool choose_A(const ss_ctx* c, const ConvPlan& p, Launch& l) {
    Launch u = l;
    if (c->prec == kF16x2 && p.d_w_upsr) {
        u.form = kConv4UpsRing; u.a.wpk = p.d_w_upsr;
        if (conv_upsr_supports(u.a, c->num_cus)) { l = u; return true; }
    }
    if (c->prec == kFp32 && p.d_w_ups32 && l.a.src1) {
        u.form = kConv2Ups; u.a.wpk = p.d_w_ups32;
        if (conv_ups32_supports(u.a, p.ups32_nt, ups32_mtw(p), c->num_cus)) { l = u; return true; }
    }
    return choose_tile(c, p, l);
}

// a B launch that adds r (conv1_1: the rank-1 term): conv1_1 has its row-streaming form, the others the tile forms alone
static bool choose_B(const ss_ctx* c, const Block& k, const ConvPlan& p, BlockRun& r) {
    if (c->prec == kF16x2 && k.first_in_loader && p.d_w_s16 && dev_env("SOFTSPOKEN_C1S", 1)) {
        Launch s = r.B;
        s.form = dev_env("SOFTSPOKEN_C1S_FORM", 16) == 32 && p.d_w_s1 ? kConv1Stream32 : kConv1Stream16;
        s.a.wpk = s.form == kConv1Stream16 ? p.d_w_s16 : p.d_w_s1;
        s.a.relu = 1 | (dev_env("SOFTSPOKEN_C1S_ABLATE", 0) << 4);    // (dev build, timing only: 1 no stores, 2 no second-conv products, 4 no pooled rows)
        s.a.plain = p.s1_range_proven && dev_env("SOFTSPOKEN_C1S_TRACK", 0) == 0;
        if (conv1_stream_supports(s.a)) {
            if (dev_env("SOFTSPOKEN_C1S", 1) == 2) { r.B2 = r.B; if (!choose_tile(c, p, r.B2)) return false; }
            r.B = s;
            return true;
        }
    }
    return choose_tile(c, p, r.B);
}

// "projection in B" (bf16, and f16x2 for the blocks conv4.hip has the form for); false: conv4.hip has no instantiation for this block, it
// runs as A + r / B.  (It gives up when conv4.hip cannot serve B even where conv9s.hip could.)
static bool choose_proj(const ss_ctx* c, const Block& k, const BlockPlan& p, BlockRun& r) {
    if (!p.A.d_w3 || !p.B.d_proj) return false;
    const int cus = c->num_cus;
    // f16x2: the A launch with the upsampled input half at low resolution where that form exists -- conv9_1.A
    Launch ups = r.A;
    ups.form = kConv4UpsPlain; ups.a.wpk = p.A.d_w_ups;
    const bool has_ups = c->prec == kF16x2 && p.A.d_w_ups && ups.a.src1 && conv_ups_supports(ups.a, cus);
    if ((!has_ups && !conv_v4_supports(r.A.a, p.A.NT, cus, prec4(c))) || !conv_v4_supports(r.B.a, p.B.NT, cus, prec4(c))) return false;
    r.A.form = r.B.form = kConv4;
    if (has_ups) {
        // conv9_1.A: the row-streaming form (conv9a.hip) -- the same pre-summed taps on stream16.h's core, no patch images, no barriers.
        // (Development build, SOFTSPOKEN_C9A=0: conv4_ups.hip's form; SOFTSPOKEN_UPS=0 switches both off.)
        Launch s = r.A;
        s.form = kConv9aStream; s.a.wpk = p.A.d_w_a16; s.a.wpk_b = p.A.d_w_ups16;
        const bool stream = p.A.d_w_a16 && p.A.d_w_ups16 && dev_env("SOFTSPOKEN_C9A", 1) && conv9a_stream_supports(s.a) &&
                            conv9a_stream_rows_ok(dev_env("SOFTSPOKEN_C9A_ROWS", 32));
        r.A = stream ? s : ups;
    }
    if (c->prec == kF16x2 && k.flat_in_b && c->d_flat_rows && p.B.d_w_s16 && p.B.d_proj_s16 && dev_env("SOFTSPOKEN_C9S", 1)) {
        // conv9_1.B: the row-streaming form (conv9s.hip), in the mask-only pass and in the spec pass alike (store_out): the two passes'
        // flatten sums are the same bits.  (Development build, SOFTSPOKEN_C9S=0: conv4.hip's form.)
        Launch s = r.B;
        s.form = kConv9Stream; s.a.wpk = p.B.d_w_s16; s.a.proj_w = p.B.d_proj_s16; s.a.flat_w4 = c->d_flat_rows;
        if (conv9_stream_supports(s.a) && conv9_stream_rows_ok(dev_env("SOFTSPOKEN_C9S_ROWS", 32))) r.B = s;
    }
    return true;
}

// How block bi runs for n windows and which form serves each of its launches, with their arguments; nothing is launched.  false: a launch
// has no form (its Launch is left at kNoForm).
static bool choose_block(const ss_ctx* c, const Workspace& ws, int bi, int n, bool with_spec, BlockRun& r) {
    const Block& k = kBlocks[bi];
    const BlockPlan& p = c->convs[bi];
    // (running A and B over Infinity-Cache-sized sub-chunks of windows was measured twice: no gain)
    // Blocks whose input is narrower than their output (encoder) move fewer bytes when B recomputes the 1x1 projection from
    // the block input than when A writes r and B reads it back; conv4.hip has that form for the blocks where it pays.
    if (c->prec != kFp32 && !k.spec_only && dev_env("SOFTSPOKEN_CONV4", 1) && dev_env("SOFTSPOKEN_RPROJ", 1)) {
        r.proj = true;
        fill_args(c, ws, bi, n, with_spec, r);
        if (choose_proj(c, k, p, r)) return true;
        r = BlockRun();
    }
    fill_args(c, ws, bi, n, with_spec, r);
    if (!k.first_in_loader && !choose_A(c, p.A, r.A)) return false;
    return choose_B(c, k, p.B, r);
}

// ---- what a launch is booked with: functions of the block, the launch (A or B), the way the block runs, the form and n ----
// multiply-adds of the layer as the reference computes it (FLOPs booked: twice these, whatever the form issues)
static double launch_macs(const Block& k, bool isA, bool proj, int n) {
    const double px = (double)n * k.H * k.W, cin = k.c0 + k.c1;
    if (isA) return px * k.cout * (9.0 * cin + (proj ? 0.0 : cin));
    return px * k.cout * (9.0 * k.cout + (proj ? cin : 0.0) + (k.first_in_loader ? 1 : 0)) + (k.first_in_loader ? px * 32 * 9 : 0.0) +
           (k.flat_in_b ? px * 32 * 4 : 0.0);
}
// bytes moved; es: bytes per stored activation value (f16x2: two f16 planes).  A reads the block input (its upsampled half at a quarter of
// the pixels) and writes h (+ r); B reads h (conv1_1: the fp32 features) and r or the block input, and writes y (store_y) and the pooled y.
static double launch_bytes(const Block& k, bool isA, bool proj, int n, double es, bool store_y) {
    const double px = (double)n * k.H * k.W, x = k.c0 + k.c1 / 4.0;
    if (isA) return px * es * (x + k.cout + (proj ? 0 : k.cout));
    return px * es * ((k.first_in_loader ? 4.0 / es : k.cout) + (proj ? x : k.r != kNoAct ? k.cout : 0) + (store_y ? k.cout : 0) + (k.pool != kNoAct ? k.cout / 4.0 : 0));
}
// multiply-adds the form issues when they are not the layer's (< 0: the same).  The decoder forms with the upsampled input half at low
// resolution issue 9 C0 + 4 C1 per output value (+ cin: the 1x1 projection, where A computes it); the stream forms count their own.
static double launch_issued(const Block& k, Form f, int n) {
    const double px = (double)n * k.H * k.W;
    switch (f) {
        case kConv4UpsRing: case kConv2Ups: return px * k.cout * (9.0 * k.c0 + 4.0 * k.c1 + (k.c0 + k.c1));
        case kConv4UpsPlain: return px * k.cout * (9.0 * k.c0 + 4.0 * k.c1);
        case kConv9aStream: return conv9a_stream_issued_macs(n);
        case kConv9Stream: return conv9_stream_issued_macs(n);
        default: return -1.0;
    }
}
// row groups per window that the form serving conv9_1.B writes into the flatten's partial sums
static int flat_groups_of(const ss_ctx* c, Form f) {
    return f == kConv9Stream ? conv9_stream_flat_groups(dev_env("SOFTSPOKEN_C9S_ROWS", 32)) : f == kConv4 ? conv_v4_flat_groups() : conv_v2_flat_groups(c->bf16);
}

// one chosen launch, under its stat name "<instantiation>/<layer>"
static int launch_form(ss_ctx* c, hipStream_t stream, const ConvPlan& p, Launch& l, double flops, double bytes, double issued) {
    const int cus = c->num_cus;
    // (conv4_ups.hip's plain form takes no stage stamps)
    auto go = [&](const char* variant, auto&& launch) { return conv_launch(c, stream, variant, p.name, l.a, flops, bytes, issued, l.form != kConv4UpsPlain, launch); };
    switch (l.form) {
        case kConv2: return go(conv_v2_variant(l.a, c->bf16, p.NT, cus), [&](ConvArgs& x) { return launch_conv3x3_v2(x, c->bf16, p.NT, cus, stream); });
        case kConv4: return go(conv_v4_variant(l.a, p.NT, cus, prec4(c)), [&](ConvArgs& x) { return launch_conv3x3_v4(x, p.NT, cus, prec4(c), stream); });
        case kConv4UpsPlain: return go(conv_ups_variant(), [&](ConvArgs& x) { return launch_conv3x3_ups(x, cus, stream); });
        case kConv4UpsRing: return go(conv_upsr_variant(), [&](ConvArgs& x) { return launch_conv3x3_upsr(x, cus, stream); });
        case kConv2Ups: return go(conv_ups32_variant(p.ups32_nt, ups32_mtw(p)), [&](ConvArgs& x) { return launch_conv3x3_ups32(x, p.ups32_nt, ups32_mtw(p), cus, stream); });
        case kConv1Stream16: case kConv1Stream32: {
            const int form = l.form == kConv1Stream16 ? 16 : 32;
            return go(conv1_stream_variant(l.a, form), [&](ConvArgs& x) { return launch_conv1_stream(x, form, dev_env("SOFTSPOKEN_C1S_ROWS", 32), cus, stream); });
        }
        case kConv9aStream:
            return go(conv9a_stream_variant(), [&](ConvArgs& x) { return launch_conv9a_stream(x, dev_env("SOFTSPOKEN_C9A_ROWS", 32), dev_env("SOFTSPOKEN_C9A_GRID", 0), cus, stream); });
        case kConv9Stream:
            return go(conv9_stream_variant(), [&](ConvArgs& x) { return launch_conv9_stream(x, dev_env("SOFTSPOKEN_C9S_ROWS", 32), dev_env("SOFTSPOKEN_C9S_GRID", 0), cus, stream); });
        case kNoForm: break;
    }
    return fail(c, SS_ERR_STATE, "no kernel form chosen for " + p.name);
}

// Block bi of net.h's kBlocks for n windows: choose, then launch.
static int run_block(ss_ctx* c, Workspace& ws, hipStream_t stream, int bi, int n, bool with_spec) {
    const Block& k = kBlocks[bi];
    const BlockPlan& p = c->convs[bi];
    BlockRun r;
    if (!choose_block(c, ws, bi, n, with_spec, r))
        return fail(c, SS_ERR_STATE, "f16x2: no kernel form for " + (k.first_in_loader || r.A.form != kNoForm ? p.B.name : p.A.name));
    // the tensors the block writes (ss_debug_activation refuses the others)
    const bool hasA = r.A.form != kNoForm, store_y = r.B.a.store_out != 0;
    for (Act t : {hasA ? k.h : kNoAct, hasA && !r.proj ? k.r : kNoAct, store_y ? k.y : kNoAct, k.pool})
        if (t != kNoAct) c->dbg_written |= (uint64_t)1 << t;
    const double es = c->prec == kBf16 ? 2 : 4;
    for (Launch* l : {&r.A, &r.B, &r.B2}) {
        if (l->form == kNoForm) continue;
        const bool isA = l == &r.A;
        if (int rc = launch_form(c, stream, isA ? p.A : p.B, *l, 2.0 * launch_macs(k, isA, r.proj, n), launch_bytes(k, isA, r.proj, n, es, store_y),
                                 launch_issued(k, l->form, n)))
            return rc;
    }
    if (k.flat_in_b) ws.flat_groups = flat_groups_of(c, r.B.form);
    return SS_OK;
}

static int forward_chunk_(ss_ctx* c, Workspace& ws, hipStream_t stream, const float* signal, const int64_t* d_winoff, int n, float* d_logits, float* d_spec) {
    FrontendTables tb{c->d_pretw, c->d_w2048, c->d_mel_start, c->d_mel_count, c->d_mel_off, c->d_mel_w, c->mel_nw, c->d_mel_wp, dev_env("SOFTSPOKEN_FEDBG", 0),
                      c->d_win2, c->d_twt, c->d_wkt, c->d_mel_wq, c->d_mel_p0};
    {
        ScopedLaunch sl(c, stream, "frontend", 0.0, (double)n * (66150.0 * 4 + 128.0 * 256 * 4));
        HIPCHK(c, launch_frontend(signal, d_winoff, n, tb, ws.feat, c->num_cus, stream));
    }
    if (!d_logits) return SS_OK;
    for (int bi = 0; bi < kBlockCount && !(kBlocks[bi].spec_only && !d_spec); ++bi)
        if (int rc = run_block(c, ws, stream, bi, n, d_spec != nullptr)) return rc;
    if (d_spec) {   // the spec head's 1x1 (its ResBlock ran above)
        const double es = c->prec == kBf16 ? 2 : 4;
        ScopedLaunch sl(c, stream, "spec_tail", 2.0 * n * 32768 * 64, (double)n * 32768 * (32 * es + 8));
        HIPCHK(c, launch_spec_tail(ws.t[kS9].p, ws.lo_delta, c->d_spec_w, c->d_spec_b, d_spec, n, (int)c->prec, stream));
    }
    const int groups = ws.flat_groups;
    ScopedLaunch sl(c, stream, "mask_head_parts", 0.0, (double)n * (groups * 4 * 256 * 4 + 1024));
    HIPCHK(c, launch_mask_head_parts(ws.flat, groups, c->d_flat_b, c->head, d_logits, n, stream));
    return SS_OK;
}

// SpecUNet_2D.forward (pytorch_neural_nets.py:142-197) for n <= ws.chunk windows that start at signal + d_winoff[0..n)
int forward_chunk(ss_ctx* c, Workspace& ws, hipStream_t stream, const float* signal, const int64_t* d_winoff, int n, float* d_logits, float* d_spec) {
    // the pass's record for the dev build's ss_debug_activation
    c->dbg_n = n; c->dbg_ws = (int)(&ws - c->ws);
    c->dbg_written = (uint64_t)1 << kDbgFeat | (uint64_t)(d_logits ? 1 : 0) << kDbgFlatPart;
    const int rc = forward_chunk_(c, ws, stream, signal, d_winoff, n, d_logits, d_spec);
    if (rc) { c->dbg_written = 0; c->dbg_n = 0; }
    return rc;
}

#ifdef SS_DEVBUILD
// ss_debug_activation: one plane of a tensor of the last pass as [n][H][W][C], whatever its stored order (a chunk-planar tensor is
// gathered on the host), and its channel exponents
int debug_activation(ss_ctx* c, const char* name, int plane, int64_t first, int64_t n, void* out, int64_t out_bytes, int32_t* shape,
                     int32_t* exponents) {
    if (!c || !name) return fail(c, SS_ERR_ARG, "ss_debug_activation: null argument");
    const std::string k = name;
    const Workspace& w = c->ws[0];
    int id = k == "feat" ? kDbgFeat : k == "flat_part" ? kDbgFlatPart : -1;
    for (int i = 0; i < kActCount && id < 0; ++i) if (k == kActs[i].name) id = i;
    if (id < 0) return fail(c, SS_ERR_ARG, "ss_debug_activation: no tensor named '" + k + "'");
    const bool act = id < kActCount;                      // a workspace tensor
    int H = 128, W = 256, C = 1, es = 4;                  // (the features)
    if (id == kDbgFlatPart) { H = std::max(w.flat_groups, 1); W = 4; C = 256; }      // conv_flatten's row-group partial sums [n][groups][4][256] (heads.hip)
    if (act) { H = kActs[id].H; W = kActs[id].W; C = kActs[id].C; es = c->prec == kFp32 ? 4 : 2; }
    if (shape) { shape[0] = H; shape[1] = W; shape[2] = C; shape[3] = es; }
    if (exponents) {
        const std::vector<int>& e = c->act_exp[id];
        for (int i = 0; i < C; ++i) exponents[i] = i < (int)e.size() ? e[i] : 0;
    }
    if (!out) return SS_OK;                               // (shape and exponents are the model's: no pass needed)
    if (c->run_pending) return fail(c, SS_ERR_STATE, "ss_debug_activation: a run is in flight");
    if (!w.chunk || !w.arena) return fail(c, SS_ERR_STATE, "ss_debug_activation: the context has no workspace");
    if (c->dbg_ws != 0) return fail(c, SS_ERR_STATE, "ss_debug_activation: the last pass ran on the second lane's workspace");
    if (!(c->dbg_written >> id & 1)) return fail(c, SS_ERR_STATE, "ss_debug_activation: the last pass did not write " + k);
    // (after the staleness test: SS_ERR_ARG for an r tensor tells the caller that the pass ran the block as A + r / B)
    if (act && kActs[id].frag_order) return fail(c, SS_ERR_ARG, "ss_debug_activation: " + k + " is stored in MFMA fragment order; check it through its B launch");
    const void* base = act ? w.t[id].p : id == kDbgFeat ? (const void*)w.feat : w.flat;
    const bool two = act && c->prec == kF16x2;
    if (plane < 0 || plane > (two ? 1 : 0)) return fail(c, SS_ERR_ARG, "ss_debug_activation: no plane " + std::to_string(plane) + " in " + k);
    if (first < 0 || n < 0 || first + n > c->dbg_n)
        return fail(c, SS_ERR_ARG, "ss_debug_activation: windows [" + std::to_string(first) + ", " + std::to_string(first + n) + ") are outside the last pass (" +
                                   std::to_string(c->dbg_n) + " windows)");
    const int64_t per = (int64_t)H * W * C * es, need = n * per;
    if (out_bytes < need) return fail(c, SS_ERR_ARG, "ss_debug_activation: output buffer too small");
    if (need) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const char* src = (const char*)base + (plane ? w.lo_delta : 0) + first * per;
        const ActStride s = act ? w.t[id].s : ActStride{0u, 0u};
        if (s.pix == 0 || s.pix == (uint32_t)(C * es)) {     // (no byte order: fp32, the features, the partial sums)
            HIPCHK(c, hipMemcpy(out, src, (size_t)need, hipMemcpyDeviceToHost));
        } else {                                          // stored [n][C / 32][H][W][32]: 64-byte pieces to their pixels
            std::vector<char> tmp((size_t)need);
            HIPCHK(c, hipMemcpy(tmp.data(), src, (size_t)need, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < n; ++i)
                for (int k = 0; k < C / 32; ++k)
                    for (int64_t px = 0; px < (int64_t)H * W; ++px)
                        memcpy((char*)out + i * per + px * C * 2 + k * 64, tmp.data() + i * per + (int64_t)k * s.chunk + px * s.pix, 64);
        }
    }
    return SS_OK;
}
#endif

int upload_winoff(ss_ctx* c, const std::vector<int64_t>& off) {
    int rc = ensure(c, &c->d_winoff, &c->winoff_cap, off.size());
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_winoff, off.data(), off.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));     // `off` is a host temporary
    return SS_OK;
}

// ------------------------------------------------------------------------------------------------------
// a job in two halves (worker.py:49-100 over every file of the arena): everything up to the last device -> host copy is
// enqueued by run_begin; run_end waits for it; the regions are found on the host when first asked for.
// ------------------------------------------------------------------------------------------------------
// device side of the post-processing (NNDetector.py:153-190 averaging, the comparison of :118): logits of `af` files -> two bit masks
static int enqueue_post(ss_ctx* c, const std::vector<AvgFile>& af, int64_t total_bins) {
    int rc;
    if ((rc = ensure(c, &c->d_avgfiles, &c->avgfiles_cap, af.size()))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_avgfiles, af.data(), af.size() * sizeof(AvgFile), hipMemcpyHostToDevice, c->stream));   // af lives in the context
    {
        size_t cap = c->avg_cap, cap2 = c->avg_cap;
        if ((rc = ensure(c, &c->d_avg, &cap, (size_t)std::max<int64_t>(total_bins, 1)))) return rc;
        if ((rc = ensure(c, &c->d_count, &cap2, (size_t)std::max<int64_t>(total_bins, 1)))) return rc;
        c->avg_cap = std::min(cap, cap2);
    }
    const size_t words = (size_t)((total_bins + 255) / 256) * 4 + 1;     // bin_masks_kernel writes whole blocks of 4 words
    if ((rc = ensure(c, &c->d_above, &c->mask_cap, words))) return rc;
    if ((rc = ensure(c, &c->d_cov, &c->cov_cap, words))) return rc;
    if (words > c->hmask_cap) {                           // pinned result buffers
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->h_above) hipHostFree(c->h_above);
        if (c->h_cov) hipHostFree(c->h_cov);
        c->h_above = nullptr; c->h_cov = nullptr; c->hmask_cap = 0;
        const size_t cap = words + words / 2;
        HIPCHK(c, hipHostMalloc((void**)&c->h_above, cap * 8, hipHostMallocDefault));
        HIPCHK(c, hipHostMalloc((void**)&c->h_cov, cap * 8, hipHostMallocDefault));
        c->hmask_cap = cap;
    }
    return SS_OK;
}

static int launch_post(ss_ctx* c, size_t n_files, int64_t total, int64_t total_bins, int max_bins, double threshold) {
    const size_t words = (size_t)((total_bins + 255) / 256) * 4 + 1;
    {
        ScopedLaunch sl(c, c->stream, "average", 0.0, (double)total * 1024 * 5 + (double)total_bins * 12);
        // (c->step is the run's: ss_set_window_step is refused while it is in flight)
        HIPCHK(c, launch_average(c->d_logits, c->d_avgfiles, (int)n_files, c->d_starts, step_bins(c->step), c->d_avg, c->d_count, max_bins, c->stream));
    }
    if (total_bins) {
        ScopedLaunch sl(c, c->stream, "bin_masks", 0.0, (double)total_bins * 12 + (double)words * 16);
        HIPCHK(c, launch_bin_masks(c->d_avg, c->d_count, total_bins, threshold, c->d_above, c->d_cov, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->ev_run1, c->stream));
    if (int rc = range_fetch(c, c->stream)) return rc;
    if (total_bins) {
        HIPCHK(c, hipMemcpyAsync(c->h_above, c->d_above, words * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->h_cov, c->d_cov, words * 8, hipMemcpyDeviceToHost, c->stream));
    }
    return SS_OK;
}

// ext_logits != nullptr: the windows' logits come from the caller (ss_run_from_logits: a recording whose window ranges were
// inferred on several GPUs) instead of from the network; everything after them is the same code.
// Progress of the run in flight (ss_run_poll).  A caller that watches the progress gets the reference's SEQUENCE of values
// (worker.py:71-84: one emit per batch of settings.prediction_batch_size = 32 windows, done = 32, 64, ..., total) without its pass
// size: the values that fall into a pass are reported, in order, once that pass's event has completed.  block: wait for every
// pass; otherwise report what has completed and return.  (Round 2 ran min(chunk, 32)-window passes for this: a tenth of the rate.)
int run_poll(ss_ctx* c, ss_progress_fn progress, void* user, int block, const volatile int* stop_flag) {
    if (!c) return fail(nullptr, SS_ERR_ARG, "null context");
    if (!c->run_pending) return fail(c, SS_ERR_STATE, "ss_run_poll: no run in flight");
    hipSetDevice(c->device);
    constexpr int64_t kBatch = 32;
    while (c->pass_reported < c->pass_done_at.size()) {
        if (stop_flag && *stop_flag) return SS_ERR_STOPPED;          // (the caller ends the run and discards it)
        hipEvent_t e = c->pass_ev[c->pass_reported];
        if (block) HIPCHK(c, hipEventSynchronize(e));
        else {
            const hipError_t q = hipEventQuery(e);
            if (q == hipErrorNotReady) break;
            if (q != hipSuccess) return fail(c, SS_ERR_HIP, std::string("hipEventQuery: ") + hipGetErrorString(q));
        }
        const int64_t upto = c->pass_done_at[c->pass_reported], total = c->track_total;
        while (c->progress_reported < upto) {
            const int64_t next = std::min<int64_t>(c->progress_reported + kBatch, total);
            if (next > upto) break;                           // a batch that straddles two passes is reported with the later one
            c->progress_reported = next;
            if (progress) progress(user, next, total);
        }
        ++c->pass_reported;
    }
    return SS_OK;
}

int run_begin(ss_ctx* c, double threshold, double break_s, bool track, const volatile int* stop_flag,
              const float* ext_logits, int64_t ext_windows) {
    if (!c) return fail(nullptr, SS_ERR_ARG, "null context");
    if (!c->has_model && !ext_logits) return fail(c, SS_ERR_STATE, "context was created without weights (audio-only)");
    if (c->run_pending) return fail(c, SS_ERR_STATE, "a run is in flight: ss_run_end first");
    if (c->files.empty()) return fail(c, SS_ERR_STATE, "ss_run: no files added since ss_reset");
    hipSetDevice(c->device);
    int rc;
    c->t_in = now_ms();
    // ---- plan (NNDetector.py:55-82) with the context's window step (settings.step_size) ----
    const double step = c->step;
    const int64_t per_step = step_samples(step);
    int64_t total = 0, total_bins = 0; int max_bins = 0;
    std::vector<int64_t> off;
    std::vector<int32_t> starts;
    std::vector<AvgFile>& af = c->pend_af;
    af.assign(c->files.size(), AvgFile{});
    for (size_t fi = 0; fi < c->files.size(); ++fi) {
        FileRec& f = c->files[fi];
        f.W = ss_plan_windows_step(f.duration, step, nullptr, 0);
        // the plan comes from the header duration, the data from the resampler: clamp to what fits
        while (f.W > 0 && (f.W - 1) * per_step + SS_WINDOW_SAMPLES > f.n_padded) --f.W;
        f.win_base = total;
        const double secs = (double)f.n_padded / 22050.0;
        const int n_bins = (int)std::nearbyint(secs * 256.0 / 3.0);          // NNDetector.py:168
        af[fi].logit_off = total; af[fi].bin_off = total_bins; af[fi].W = (int32_t)f.W; af[fi].n_bins = n_bins; af[fi].start_off = total;
        for (int64_t i = 0; i < f.W; ++i) {
            off.push_back(f.off + i * per_step);
            starts.push_back((int32_t)ss_window_start_bin(i, step));                       // NNDetector.py:175
        }
        total += f.W; total_bins += n_bins; max_bins = std::max(max_bins, n_bins);
    }
    if (ext_logits && ext_windows != total)
        return fail(c, SS_ERR_ARG, "ss_run_from_logits: " + std::to_string(ext_windows) + " windows given, the plan has " + std::to_string(total));
    c->total_windows = total;
    c->logits_valid = false;
    if (total > 0) {
        if ((rc = ensure(c, &c->d_logits, &c->logits_cap, (size_t)total * 256))) return rc;
        if ((rc = ensure(c, &c->d_starts, &c->starts_cap, (size_t)total))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->d_starts, starts.data(), starts.size() * 4, hipMemcpyHostToDevice, c->stream));
        if (ext_logits) HIPCHK(c, hipMemcpyAsync(c->d_logits, ext_logits, (size_t)total * 1024, hipMemcpyHostToDevice, c->stream));
        if ((rc = upload_winoff(c, off))) return rc;      // (synchronises: off, starts and the caller's logits are free again)
    }
    if ((rc = enqueue_post(c, af, total_bins))) return rc;
    c->total_bins = total_bins; c->avg_on_host = false; ++c->begin_gen;
    c->t_plan = now_ms();
    c->t_sync = c->t_plan;
    HIPCHK(c, hipEventRecord(c->ev_run0, c->stream));
    if ((rc = range_clear(c, c->stream))) return rc;
    c->pass_done_at.clear(); c->pass_reported = 0; c->progress_reported = 0; c->track_total = total;
    if (!ext_logits) {
        // passes of equal size (2560 windows: 3 x 854, not 1024 + 1024 + 512: a short last pass has the launch overheads and tail
        // effects of a full one)
        const int64_t n_pass = std::max<int64_t>(1, (total + c->chunk - 1) / c->chunk);
        const int ch = (int)std::max<int64_t>(1, (total + n_pass - 1) / n_pass);
        if ((rc = ensure_workspace(c, ch))) return rc;        // (waits for the stream itself when it has to reallocate)
        // Two lanes: odd passes run on a second stream over a second workspace.  Every launch fills the chip with one workgroup per CU, and
        // its last workgroups leave CUs idle until the slowest is done; with another pass's launches queued beside it those CUs take the
        // other lane's workgroups (two processes sharing the card showed it: 30.6 k audio-s/s against 29.6 k).  Same kernels, same
        // results; not with per-launch profiling (the launch times would overlap) and not when the memory for the lane is not there.
        // Off in the product build (SOFTSPOKEN_LANES=2 in the dev build): under rocprofv3 the overlapped launches' durations no longer are
        // the per-launch times the bench line's roofline is computed from (its profiled passes run one lane), and + 0.5-1 % is not worth two
        // sets of numbers that disagree.
        const bool two = n_pass >= 2 && !c->profile && dev_env("SOFTSPOKEN_LANES", 1) >= 2 && ensure_lane(c, ch);
        // (the lane starts behind what the main stream holds so far: the uploads, the cleared range flag)
        if (two) { HIPCHK(c, hipEventRecord(c->lane_ev_in, c->stream)); HIPCHK(c, hipStreamWaitEvent(c->lane_stream, c->lane_ev_in, 0)); }
        // ---- windows in chunks, across file boundaries (worker.py:71-84 batches per file of 32) ----
        // track: an event behind every pass, on that pass's stream, from which run_poll reports the progress (below).  The passes keep
        // their full size and are all enqueued here; nothing waits for the device.
        int64_t pass_no = 0;
        for (int64_t i0 = 0; i0 < total; i0 += ch, ++pass_no) {
            if (stop_flag && *stop_flag) {
                hipStreamSynchronize(c->stream);
                if (two) hipStreamSynchronize(c->lane_stream);
                return fail(c, SS_ERR_STOPPED, "stopped on request");
            }
            const int m = (int)std::min<int64_t>(ch, total - i0);
            const int lane = two ? (int)(pass_no & 1) : 0;
            const hipStream_t st = lane ? c->lane_stream : c->stream;
            if ((rc = forward_chunk(c, c->ws[lane], st, c->d_arena, c->d_winoff + i0, m, c->d_logits + (size_t)i0 * 256, nullptr))) return rc;
            if (track) {
                const size_t k = c->pass_done_at.size();
                if (k >= c->pass_ev.size()) {
                    hipEvent_t e = nullptr;
                    HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
                    c->pass_ev.push_back(e);
                }
                HIPCHK(c, hipEventRecord(c->pass_ev[k], st));
                c->pass_done_at.push_back(i0 + m);
            }
        }
        // (the main stream's averaging below reads both lanes' logits)
        if (two) { HIPCHK(c, hipEventRecord(c->lane_ev_out, c->lane_stream)); HIPCHK(c, hipStreamWaitEvent(c->stream, c->lane_ev_out, 0)); }
    }
    // ---- overlap averaging on the device (NNDetector.py:153-190), then two bits per bin ----
    if ((rc = launch_post(c, af.size(), total, total_bins, max_bins, threshold))) return rc;
    c->t_loop = now_ms();
    c->pend_thr = threshold; c->pend_brk = break_s;
    c->run_pending = true;
    return SS_OK;
}

int run_end(ss_ctx* c) {
    if (!c) return fail(nullptr, SS_ERR_ARG, "null context");
    if (!c->run_pending) return fail(c, SS_ERR_STATE, "ss_run_end: no run in flight");
    hipSetDevice(c->device);
    const bool timing = dev_env("SOFTSPOKEN_TIMING", 0) != 0;      // development aid: host-side phases of a run on stderr
    c->run_pending = false;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    { float ms = 0; if (hipEventElapsedTime(&ms, c->ev_run0, c->ev_run1) == hipSuccess) c->last_run_ms = ms; }
    resolve_events(c);
    if (range_left(c))
        return fail(c, SS_ERR_RANGE, "f16x2: an activation left the f16 range (|x| > 65504) or was not finite; run this checkpoint with the fp32 mode");
    const double t_d2h = now_ms();
    // the run's results leave the working set: file bookkeeping is copied, the mask buffers change places with the previous result's
    const std::vector<AvgFile>& af = c->pend_af;
    c->res_files.resize(c->files.size());
    for (size_t fi = 0; fi < c->files.size(); ++fi) {
        FileRec& f = c->files[fi];
        f.bin_off = af[fi].bin_off; f.n_bins = af[fi].n_bins;
        ss_ctx::ResFile& r = c->res_files[fi];
        r.W = f.W; r.win_base = f.win_base; r.bin_off = f.bin_off; r.n_bins = f.n_bins; r.regions.clear();
    }
    std::swap(c->h_above, c->r_above); std::swap(c->h_cov, c->r_cov); std::swap(c->hmask_cap, c->rmask_cap);
    c->res_thr = c->pend_thr; c->res_brk = c->pend_brk;
    c->res_valid = true; c->res_regions = false; c->res_gen = c->begin_gen;
    c->logits_valid = true;
    if (timing)
        fprintf(stderr, "[ss_run] plan+uploads %.3f ms, enqueue %.3f, drain+D2H %.3f (device %.3f), end %.3f\n",
                c->t_plan - c->t_in, c->t_loop - c->t_sync, t_d2h - c->t_loop, c->last_run_ms, now_ms() - t_d2h);
    return SS_OK;
}

// Run lengths + gap merge on the host (NNDetector.py:103-143, worker.py:100) from the two bit masks of the ended run, when a getter
// first asks: a run opens at a bin above the threshold and closes at the next COVERED bin that is not; uncovered bins are absent from
// the reference's series and neither extend nor close a run.  The same decisions ss_find_regions takes on the compacted series.
void ensure_regions(ss_ctx* c) {
    if (c->res_regions) return;
    const bool timing = dev_env("SOFTSPOKEN_TIMING", 0) != 0;
    const double t0 = now_ms();
    const unsigned long long* AB = c->r_above;
    const unsigned long long* CV = c->r_cov;
    // first set bit of (word(k) for k >= pos) in [pos, hi), or hi
    auto next_bit = [&](auto&& word, int64_t pos, int64_t hi) -> int64_t {
        while (pos < hi) {
            unsigned long long w = word(pos >> 6) >> (pos & 63);
            if (w) { const int64_t p = pos + __builtin_ctzll(w); return p < hi ? p : hi; }
            pos = (pos | 63) + 1;
        }
        return hi;
    };
    // last set bit of `above` in [lo, hi), or -1
    auto prev_above = [&](int64_t lo, int64_t hi) -> int64_t {
        int64_t pos = hi - 1;
        while (pos >= lo) {
            unsigned long long w = AB[pos >> 6] << (63 - (pos & 63));
            if (w) { const int64_t p = pos - __builtin_clzll(w); return p >= lo ? p : -1; }
            pos = (pos & ~(int64_t)63) - 1;
        }
        return -1;
    };
    auto above_w = [&](int64_t k) { return AB[k]; };
    auto closer_w = [&](int64_t k) { return CV[k] & ~AB[k]; };
    for (ss_ctx::ResFile& f : c->res_files) {
        f.regions.clear();
        const int64_t lo = f.bin_off, hi = f.bin_off + f.n_bins;
        RunMerger mg; mg.brk = c->res_brk;
        int64_t pos = lo;
        while (pos < hi) {
            const int64_t first = next_bit(above_w, pos, hi);
            if (first == hi) break;
            const int64_t q = next_bit(closer_w, first + 1, hi);              // the covered bin that ends the run, or the file's end
            const int64_t last = prev_above(first, q);                         // (>= first: `first` itself is above)
            mg.add(first - lo, last - lo, f.regions);
            pos = q + 1;
        }
        mg.flush(f.regions);
    }
    c->res_regions = true;
    if (timing) fprintf(stderr, "[ss_run] regions %.3f ms\n", now_ms() - t0);
}

// The merged table of files [first, first + n_ch) of the ended run (ss_get_regions_union): a bin is above when it is above on any of the
// channels -- the OR of their `above` bits at their bit offsets --, and closes a run when it is covered and above on none; then the run
// lengths; bin times and gap merge by the same RunMerger.  bins (optional): first and last bin of every merged region.
int union_regions(ss_ctx* c, int first, int n_ch, std::vector<ss_region>& regions, std::vector<int64_t>* bins) {
    regions.clear();
    if (bins) bins->clear();
    if (!c->res_valid) return fail(c, SS_ERR_STATE, "ss_get_regions_union: no completed ss_run");
    if (first < 0 || n_ch < 1 || (size_t)first + (size_t)n_ch > c->res_files.size())
        return fail(c, SS_ERR_ARG, "ss_get_regions_union: files outside the run");
    const ss_ctx::ResFile& f0 = c->res_files[first];
    for (int k = 1; k < n_ch; ++k)
        if (c->res_files[first + k].n_bins != f0.n_bins) return fail(c, SS_ERR_ARG, "ss_get_regions_union: the files differ in their number of bins");
    auto bit = [](const unsigned long long* w, int64_t j) { return (w[j >> 6] >> (j & 63)) & 1ull; };
    RunMerger mg; mg.brk = c->res_brk;
    bool open = false;
    int64_t run0 = 0, run1 = 0;
    for (int64_t j = 0; j < f0.n_bins; ++j) {
        bool above = false, covered = false;
        for (int k = 0; k < n_ch; ++k) {
            const int64_t at = c->res_files[first + k].bin_off + j;
            above = above || bit(c->r_above, at);
            covered = covered || bit(c->r_cov, at);
        }
        if (above) { if (!open) { run0 = j; open = true; } run1 = j; }
        else if (covered && open) { mg.add(run0, run1, regions, bins); open = false; }
    }
    if (open) mg.add(run0, run1, regions, bins);
    mg.flush(regions, bins);
    return SS_OK;
}

}  // namespace ss
