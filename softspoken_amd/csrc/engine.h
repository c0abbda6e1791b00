// Internal state of a context, shared by the host-side units of the library:
//   weights.hip   weights blob -> folded BatchNorm -> MFMA fragment packing, front-end tables      (ss_create's work)
//   engine.hip    activation workspaces (ss::Workspace), launch sequence of one pass of the U-Net on a workspace and a stream, job halves
//                 (plan + enqueue / wait), the region scans of an ended run
//   net.h         the network's graph, stated once: workspace tensors (ss::Act, kActs) and ResBlocks (kBlocks); the arrays below are indexed by it
//   host.hip      host-only pieces of the path: WAV header walk, window plan, run merger (ss::RunMerger) and regions, CSV text
//   sep_plan.h    the separation silencer's and the region bands' host plan (no HIP): the small rules host.hip and abi.hip call too
//   ingest_plan.h the host plan of PCM ingest (no HIP): rate rule, tap table, resampler geometries, slot rule, plan_ingest
//   abi.hip       the C ABI (include/softspoken.h): argument checks, arena, getters, measurement
// Not part of the C ABI.
#pragma once
#include "../../include/softspoken.h"
#include "hostdefs.h"
#include "sep_plan.h"
#include "kernels.h"
#include "net.h"

#include <map>
#include <string>
#include <vector>

namespace ss {

// ---- errors --------------------------------------------------------------------------------------------
int fail(ss_ctx* c, int code, const std::string& msg);       // records the message (context + calling thread), returns code
const char* thread_error();

#define HIPCHK(c, expr)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            return ss::fail((c), SS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

// ---- weights blob ("SSWBLOB1") ---------------------------------------------------------------------------
struct BlobEntry { char name[96]; uint32_t dtype, ndim; int64_t shape[4]; uint64_t offset, nbytes; };
static_assert(sizeof(BlobEntry) == 152, "blob entry layout");
struct Blob {
    std::map<std::string, BlobEntry> e;
    const char* base = nullptr;
    size_t size = 0;
    bool has(const std::string& k) const { return e.count(k) != 0; }
    const float* f32(const std::string& k, size_t count, std::string& err) const;
};
bool parse_blob(const void* p, size_t n, Blob& b, std::string& err);

// ---- context ---------------------------------------------------------------------------------------------
enum Precision { kFp32 = 0, kBf16 = 1, kF16x2 = 2 };

struct ConvPlan {          // one launch of a ResBlock half
    std::string name;
    // conv2.hip (fp32; also the bf16 fallback): A = conv1 + residual projection (10 taps per chunk), B = conv2 only
    void* d_w2 = nullptr; float* d_bias2 = nullptr; float* d_res_bias = nullptr; float* d_rank1 = nullptr;
    // conv4.hip "projection in B": A = conv1 alone (9 taps per chunk); B = conv2 + the block's 1x1 projection of its own
    // input, weights in MFMA A-operand order per 16-channel step, bias b2 + br
    void* d_w3 = nullptr; void* d_proj = nullptr; float* d_bias3 = nullptr;
    void* d_w_ups = nullptr;                              // conv4_ups.hip: A's banks with the upsampled input half as four taps per parity class
    bool s1_range_proven = false;                         // conv1s.hip: |h1| and |c1| bounded below the f16 limit by the weights alone (weights.hip)
    void* d_w_s1 = nullptr;                               // conv1s.hip: conv1_1's second conv, banks in the K order of the first conv's accumulator registers
    void* d_w_s16 = nullptr;                              // ... and for its 16-pixel form (v_mfma_f32_16x16x32_f16: natural K order, channel rows 8 g + 4 u + r)
    void* d_proj_s16 = nullptr;                           // conv9s.hip: conv9_1.B's projection as 16x16x32 A fragments (its 3 x 3 banks: d_w_s16)
    void* d_w_a16 = nullptr; void* d_w_ups16 = nullptr;   // conv9a.hip: conv9_1.A's skip half as pack_conv_stream16's banks, its upsampled half as pre-summed 16x16x32 sets
    void* d_w_upsr = nullptr;                           // conv4_ups.hip, ring form: the same for the A launch that also writes r (entries in walk order)
    void* d_w_ups32 = nullptr;                            // conv2_ups.hip (fp32): the A launch with the upsampled half at low resolution
    int ups32_nt = 1;                                     // ... packed for this many 32-channel tiles per block
    int Cout = 0, NT = 1, C0 = 0, C1 = 0, R0 = 0, R1 = 0, H = 0, W = 0;
};

struct BlockPlan { ConvPlan A, B; };    // the two launches of a ResBlock

// (FileRec, a signal's place in the arena: ingest_plan.h)

struct StreamSet;                                         // stream.hip: the context's streams and their step buffers
struct SepState;                                          // separate.hip: the separation silencer's tables and buffers

// An activation workspace for `chunk` windows (engine.hip alloc_ws): what one pass of the network writes.  A context has two -- the main
// one, and the second lane's of a run with several passes.
struct ActTensor { void* p = nullptr; ActStride s{0u, 0u}; };   // first byte (high plane in f16x2 mode) inside the arena; 16-bit modes: byte order
struct Workspace {
    int chunk = 0; int64_t bytes = 0;
    ActTensor t[kActCount];                               // the tensors of net.h, by Act
    void* arena = nullptr;
    int64_t lo_delta = 0;                                 // f16x2: byte distance from a tensor's high plane to its low plane
    float* feat = nullptr; float* flat = nullptr;         // front-end features; conv_flatten's row-group partial sums
    int flat_groups = 0;                                  // row groups the last FLAT launch wrote per window into `flat`
};

struct KStat { std::string name; int64_t launches = 0; double ms = 0, flops = 0, bytes = 0, issued = 0; };
struct PendingEvt { int sid; hipEvent_t a, b; };

}  // namespace ss

struct ss_ctx {
    int device = 0;
    uint32_t flags = 0;
    ss::Precision prec = ss::kFp32;
    bool bf16 = false;                                    // storage element is 2 bytes wide in the conv stack (bf16 mode)
    bool profile = false, has_model = false;
    hipStream_t stream = nullptr;
    // ingest: host -> device copies of the NEXT job's files run here, beside the compute stream's kernels; ev_copy is recorded behind
    // the last copy enqueued, and the next ss_add_pcm*_device makes the compute stream wait for it (copy_pending)
    hipStream_t copy_stream = nullptr; hipEvent_t ev_copy = nullptr; bool copy_pending = false;
    std::string err;
    int chunk = 1024;                                      // most windows per pass of the network
    double step = SS_STEP_DEFAULT;                         // window step, seconds (ss_set_window_step): the next run's plan, the streams opened from now on
    int num_cus = 256;

    // tables + weights on device
    float4* d_pretw = nullptr; float2* d_w2048 = nullptr;
    int *d_mel_start = nullptr, *d_mel_count = nullptr, *d_mel_off = nullptr; float* d_mel_w = nullptr; float* d_mel_wp = nullptr; int mel_nw = 0;
    float2 *d_win2 = nullptr, *d_twt = nullptr, *d_wkt = nullptr; float* d_mel_wq = nullptr; int* d_mel_p0 = nullptr;   // second front-end kernel
    float *d_first_w = nullptr, *d_first_b = nullptr;
    float* d_flat_b = nullptr; void* d_flat_frag = nullptr; void* d_flat_frag4 = nullptr;
    void* d_flat_rows = nullptr;                          // conv9s.hip: conv_flatten's filter per mel row as 16x16x32 A fragments (weights.hip pack_flat_rows)
    float *d_spec_w = nullptr, *d_spec_b = nullptr;
    ss::Head1dWeights head{};
    ss::BlockPlan convs[ss::kBlockCount];   // by block of net.h's kBlocks (conv1_1 has only B)
    std::vector<void*> owned;        // device allocations to free
    std::vector<void*> user_dev, user_host;   // ss_device_alloc / ss_host_alloc memory the caller has not freed: released with the context

    // bin masks of the last run, all files (covered by a window / average above the threshold; 64 bins per word): pinned, so that
    // ss_run_begin's copies are asynchronous.  The averages themselves stay on the device until ss_get_avg asks for them.
    unsigned long long *d_above = nullptr, *d_cov = nullptr, *h_above = nullptr, *h_cov = nullptr; size_t mask_cap = 0, cov_cap = 0, hmask_cap = 0;
    // The last ENDED run: its files' window / bin bookkeeping and its two masks (the pinned buffers swap places with h_above / h_cov
    // at ss_run_end), from which the regions are found when they are first asked for.  It stays readable while the next job is added
    // and in flight -- the host half of job k can run behind the device half of job k + 1 in ONE context.
    struct ResFile { int64_t W = 0, win_base = 0, bin_off = 0; int n_bins = 0; std::vector<ss_region> regions; };
    std::vector<ResFile> res_files; bool res_valid = false, res_regions = false; double res_thr = 0, res_brk = 0;
    unsigned long long *r_above = nullptr, *r_cov = nullptr; size_t rmask_cap = 0;
    uint64_t begin_gen = 0, res_gen = 0;               // avg / logits of the ended run live in device buffers the next ss_run_begin reuses
    std::vector<double> h_avg; std::vector<int32_t> h_cnt; bool avg_on_host = false; int64_t total_bins = 0;
    // a run between ss_run_begin and ss_run_end
    bool run_pending = false; double pend_thr = 0, pend_brk = 0; std::vector<ss::AvgFile> pend_af;
    double t_in = 0, t_plan = 0, t_sync = 0, t_loop = 0;
    // progress of the run in flight (ss_run_begin_tracked): an event behind every pass and the windows done at it
    std::vector<hipEvent_t> pass_ev; std::vector<int64_t> pass_done_at; size_t pass_reported = 0; int64_t progress_reported = 0, track_total = 0;
    // ws[0]: the main workspace (passes on `stream`).  ws[1]: the second lane of a run with several passes, with a stream of its own, so
    // that a pass's launches fill the CUs that the other lane's launch tails leave idle (engine.hip run_begin); allocated when such a run
    // first asks, dropped with the main workspace
    ss::Workspace ws[2];
    hipStream_t lane_stream = nullptr; hipEvent_t lane_ev_in = nullptr, lane_ev_out = nullptr;
    int* d_range_flag = nullptr; int* h_range_flag = nullptr;    // f16x2: set by the conv kernels when a value does not fit an f16
    int fail_alloc_after = -1;                            // dev build's test hook (ss_debug_fail_workspace_alloc): the n-th workspace allocation from now fails
    int64_t sep_budget = 0;                               // dev build's test hook (ss_debug_set_separation_budget): frames per chunk of ss_separate_pcm; 0: from kSepFrameBytes
    int64_t bands_budget = 0;                             // dev build's test hook (ss_debug_set_bands_budget): bins per piece of ss_region_bands; 0: kBandsPieceBins
    bool split_range_ok = true;                           // f16x2: cleared while packing when a folded weight has no f16 representation
    // f16x2: power-of-two channel exponents of every activation tensor, by Act, then of the features and of conv_flatten's partial sums
    // (weights.hip; all zero in the other modes and under SOFTSPOKEN_NORM=0): a tensor T holds 2^act_exp[T][c] x the value of channel c
    std::vector<int> act_exp[ss::kDbgCount];
    // the last network pass, for the dev build's ss_debug_activation (kept in both builds: the units shared by the two libraries must see
    // one layout of this struct): its windows, the index of the workspace it ran on, the tensors it wrote (bit Act; kDbgFeat, kDbgFlatPart)
    int dbg_n = 0, dbg_ws = 0; uint64_t dbg_written = 0;

    // arena
    float* d_arena = nullptr; size_t arena_cap = 0, arena_used = 0;
    uint64_t reset_gen = 0;                               // bumped by every ss_reset (callers caching file ids compare it)
    std::vector<ss::FileRec> files;
    void* d_pcm = nullptr; size_t pcm_cap = 0;
    float* d_sx = nullptr; size_t sx_cap = 0;                    // review-screen spectrogram: samples in, magnitudes out
    float* d_sm = nullptr; size_t sm_cap = 0;
    short* d_sil_out = nullptr; size_t sil_out_cap = 0;          // silencer output / frame ranges
    int64_t* d_sil_ranges = nullptr; size_t sil_ranges_cap = 0;
    unsigned char* d_src_out = nullptr; size_t src_out_cap = 0;  // source-encoding output (ss_silence_pcm_source, ss_separate_pcm*_source): bytes
    float* d_mono = nullptr; size_t mono_cap = 0;
    double* d_peaks = nullptr; size_t peaks_cap = 0;             // ss_get_region_peaks: results, then the regions' bin ranges and the channels' offsets
    unsigned char* d_desc = nullptr; size_t desc_cap = 0;         // the descriptor image of the ingest call at work (IngestPlan::desc)
    std::map<int, float*> taps;                                   // sr_in -> device taps (ingest_plan.h design_taps)

    // run state
    int64_t* d_winoff = nullptr; size_t winoff_cap = 0;
    float* d_logits = nullptr; size_t logits_cap = 0;
    float* d_spec = nullptr; size_t spec_cap = 0;
    double* d_avg = nullptr; int32_t* d_count = nullptr; size_t avg_cap = 0;
    int32_t* d_starts = nullptr; size_t starts_cap = 0;
    ss::AvgFile* d_avgfiles = nullptr; size_t avgfiles_cap = 0;
    bool logits_valid = false; int64_t total_windows = 0;
    hipEvent_t ev_run0 = nullptr, ev_run1 = nullptr; double last_run_ms = 0;

    // streaming detection (stream.hip): separate from the job above -- ss_reset / ss_run do not touch it
    ss::StreamSet* streams = nullptr;
    // separation silencer (separate.hip): per-rate FFT / band tables and its device buffers, allocated when first used
    ss::SepState* sep = nullptr;

    // profiling
    std::vector<ss::KStat> stats; std::vector<ss::PendingEvt> pending; std::vector<hipEvent_t> evpool;
};

namespace ss {

struct ScopedLaunch {      // times one launch with HIP events on its stream when profiling
    ss_ctx* c; hipStream_t stream; int sid; hipEvent_t a = nullptr, b = nullptr;
    // issued_macs: multiply-adds of the form that runs, when it differs from the layer's algorithmic count (< 0: flops / 2)
    ScopedLaunch(ss_ctx* c_, hipStream_t stream_, const std::string& name, double flops, double bytes, double issued_macs = -1.0);
    ~ScopedLaunch();
};
void resolve_events(ss_ctx* c);

template <typename T>
int dev_upload(ss_ctx* c, T** dst, const void* src, size_t bytes) {
    void* p = nullptr;
    HIPCHK(c, hipMalloc(&p, bytes ? bytes : 16));
    c->owned.push_back(p);
    if (bytes) HIPCHK(c, hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    *dst = (T*)p;
    return SS_OK;
}

// grow-only device buffer (1.5x); keep = carry the old contents over
template <typename T>
int ensure(ss_ctx* c, T** p, size_t* cap, size_t need_elems, bool keep = false) {
    if (need_elems <= *cap && *p) return SS_OK;
    size_t ncap = need_elems > *cap + *cap / 2 ? need_elems : *cap + *cap / 2;
    void* np = nullptr;
    size_t nb = ncap * sizeof(T);
    HIPCHK(c, hipMalloc(&np, nb > 256 ? nb : 256));
    if (keep && *p && *cap) {
        HIPCHK(c, hipMemcpyAsync(np, *p, *cap * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (*p) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(*p)); }
    *p = (T*)np; *cap = ncap;
    return SS_OK;
}

// ... that frees itself with its owner (the streams' and the separation's state)
template <typename T>
struct DevBuf {
    T* p = nullptr; size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) hipFree(p); }
    int reserve(ss_ctx* c, size_t n) { return ensure(c, &p, &cap, n); }
    int reserve_bytes(ss_ctx* c, size_t bytes) { return reserve(c, bytes / sizeof(T)); }
};

// weights.hip
int build_tables(ss_ctx* c, const Blob& bl);
int build_model(ss_ctx* c, const Blob& bl);
const float* mel_edges_hz();                              // the filterbank's 130 band edges (the front-end's table)
// engine.hip
int ensure_workspace(ss_ctx* c, int n);                  // the main workspace holds >= n windows, or an error
void free_workspace(ss_ctx* c);                           // both workspaces
// one pass: n <= ws.chunk windows at signal + d_winoff[0..n) through the network, on `stream` (d_logits == nullptr: the front end only)
int forward_chunk(ss_ctx* c, Workspace& ws, hipStream_t stream, const float* signal, const int64_t* d_winoff, int n, float* d_logits, float* d_spec);
// f16x2's range flag (no-ops in the other modes): clear it on a stream; enqueue its copy to the pinned word; test that word after the
// stream has been synchronised.  The caller reports SS_ERR_RANGE in its own words.
int range_clear(ss_ctx* c, hipStream_t stream);
int range_fetch(ss_ctx* c, hipStream_t stream);
inline bool range_left(const ss_ctx* c) { return c->h_range_flag && *c->h_range_flag; }
int run_begin(ss_ctx* c, double threshold, double break_s, bool track, const volatile int* stop_flag,
              const float* ext_logits = nullptr, int64_t ext_windows = 0);
int run_poll(ss_ctx* c, ss_progress_fn progress, void* user, int block, const volatile int* stop_flag);
int run_end(ss_ctx* c);
#ifdef SS_DEVBUILD
int debug_activation(ss_ctx* c, const char* name, int plane, int64_t first, int64_t n, void* out, int64_t out_bytes, int32_t* shape,
                     int32_t* exponents);
#endif
void ensure_regions(ss_ctx* c);
int union_regions(ss_ctx* c, int first, int n_ch, std::vector<ss_region>& regions, std::vector<int64_t>* bins);
int upload_winoff(ss_ctx* c, const std::vector<int64_t>& off);
// abi.hip
int check_pcm_args(ss_ctx* c, const void* pcm, int format, int sr, int ch, int64_t frames);
int get_taps(ss_ctx* c, int sr_in, int& L, int& M, int& half, float** d_taps);    // polyphase table of sr_in -> 22 050 Hz (cached)
// stream.hip
void free_streams(ss_ctx* c);
// separate.hip (sep_fft_size, check_separation_params, separation_defaults, separation_plan, check_band_args: sep_plan.h)
int separation_maps(ss_ctx* c, int file_id, int64_t first_bin, int64_t n_bins, float* out);
// each: every channel's gains from its own passes (ss_separate_pcm_channels, ch > 1); src: the output in the recording's own encoding
// (frames x channels x bytes-per-sample bytes), otherwise int16
int separate_run(ss_ctx* c, bool each, bool src, const void* pcm, int format, int sr, int ch, int64_t frames, const ss_region* regions,
                 int64_t n_regions, const ss_separation_params* params, void* out);
void free_separation(ss_ctx* c);
// separate.hip, band silencer (plan_boxes, check_box_args, box_defaults: sep_plan.h); the recording is in c->d_pcm
int box_run(ss_ctx* c, bool src, int format, int sr, int ch, int64_t frames, const ss_box* boxes, int64_t n_boxes, const ss_box_params* params,
            void* out);
// separate.hip, region bands (include/softspoken.h "region bands")
void band_edges(double* hz130);
// maps == nullptr: the spec head on files fid .. fid + nsig - 1; otherwise the caller's maps of bins first_bin .. first_bin + n_bins - 1
int region_bands(ss_ctx* c, const float* maps, int fid, int nsig, int64_t first_bin, int64_t n_bins, const ss_region* regions, int64_t n,
                 const ss_band_params* params, ss_region_band* out, double* profile);
// host.hip (and the rules of hostdefs.h)
double now_ms();

}  // namespace ss
