// Streaming detection (include/softspoken.h, ss_stream_*): recordings whose PCM arrives in pieces, stepped together.  A step plans
// every stream on the host, uploads all staged pieces and its descriptors in one copy, and rebuilds the streams' carried state in the
// other half of a double-buffered arena:
//   copy (carried samples / logits, padding zeros) -> decode + mixdown -> resample -> windows (forward_chunk, passes across streams)
//   -> new logits behind the carried ones -> averaging of the bins that became final -> regions continued on the host.
// A stream opened in each-channel mode (ss_stream_open_channels, more than one channel) carries one lane per channel instead of the one
// mixdown lane: the lanes share the stream's plan and differ only in their arena segments; its pieces are decoded to one plane per
// channel, every lane goes through the copies, the resampler, the passes and the averaging with a descriptor of its own, and the bins
// that became final are merged (OR of the flags, fmax of the averages) into the series the host walks.
// Nothing of the stream state changes before the step has completed without SS_ERR_RANGE: the arena half the streams live in is only
// read, and the host records are updated at the end (commit), so a refused step leaves every stream as it was.
// Streams opened with output (ss_stream_open_output) then get their decided frames back as 16-bit PCM with the detected speech zeroed
// (step_output, behind the commit): the raw PCM not returned yet is carried in a byte arena of the same two-half discipline.
// Streams opened with bands (ss_stream_open_bands; include/softspoken.h "stream bands") return with every region its ss_region_band,
// bytes equal to ss_region_bands on the whole file: their windows run in passes of their own that store the spec head's output,
// stream_map_kernel adds each pass to float64 sums per non-final bin carried in the arena and turns the bins that became final into the
// float32 averaged maps, and -- behind the commit's region walk, whose decisions arrive as a short event list -- stream_band_kernel walks
// the final bins in order over one running accumulator and a snapshot per lane and evaluates the regions the walk returned.
#include "engine.h"
#include "bands.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

namespace ss {

namespace {

constexpr int64_t kPad = SS_WINDOW_SAMPLES;          // 3 s of zeros in front of and behind the recording (worker.py:58-62)

// ---- bands: descriptors and kernels ----
constexpr int kBandAcc = 5;                           // 256-double vectors per lane: done, cur, snap_done, snap_cur, parked
enum { kEvReset = 0, kEvSnap = 1, kEvPark = 2, kEvEmitSnap = 3, kEvEmitPark = 4 };
// one decision of the host's region walk.  Reset / snap act before bin `pos` is added: reset clears both accumulators (a candidate region
// starts at pos), snap copies them (the candidate's bins end before pos).  Park forms the snapshot's profile and sets it aside (the region
// is final, the walk returns it later); emit evaluates record `rec` of the step (n_bins bins) from the snapshot or from the parked vector.
struct StreamBandEv { int64_t pos; int32_t type, n_bins; int64_t rec; };
// one launch's work on one band lane's map sums [256][stride] over the bins [b0, b0 + n) of the step.  Flags: kMapInit -- the sums start
// from the carried ones and zeros (the lane's first entry of the step); the windows [i0, i1) of this pass, the first at spec slot slot0,
// are added (none when i0 == i1); kMapFin -- the first fin_n bins become float32 maps fmap [256][fin_n] (the lane's last entry)
enum { kMapInit = 1, kMapFin = 2 };
struct StreamMap {
    const double* old_sum; int64_t old_stride, old_b0, old_n;
    double* sum; int64_t stride, b0, n;
    int64_t i0, i1, slot0;
    float* fmap; int64_t fin_n, i_end;
    int32_t flags, pad;
};
// one band lane's walk over the step's final bins [b0, b0 + nb) (fmap [256][nb]) under the stream's events ev0 .. ev0 + nev - 1
struct StreamBand {
    const double* acc_old; double* acc;
    const float* fmap; int64_t b0, nb;
    int64_t out0;                                     // record (rec, lane) of the stream: out0 + rec lanes + lane
    int32_t ev0, nev, lanes, lane, speech_ch, want_prof;
    double q_low, q_high;
};

__device__ __forceinline__ int band_win_start(int i) { return (int)(((int64_t)512 * i + 5) / 10); }   // round(51.2 i), as sep_accumulate_kernel

// Thread = (bin t of the lane's step range, channel x band blockIdx.y), descriptor blockIdx.z.  A thread owns its sum through all the
// launches of a step, so start, addition and the final value follow one another in one thread.  The addition is
// sep_accumulate_kernel's arithmetic: the pass's windows over the bin are added to its float64 sum in ascending window order; passes and
// steps arrive in ascending window order too, so the sum is the whole-file one.  The final value is sep_finalize_kernel's: sum / count
// as float32, 0 for a bin no window covers (only behind the last window of a closed stream).  Loads of spec and stores of sums and
// maps run along the bins: consecutive threads, consecutive addresses.
__global__ __launch_bounds__(256) void stream_map_kernel(const StreamMap* __restrict__ ds, int nd, const float* __restrict__ spec) {
    const int cm = blockIdx.y;
    for (int k = blockIdx.z; k < nd; k += gridDim.z) {
        const StreamMap d = ds[k];
        for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < d.n; t += (int64_t)gridDim.x * 256) {
            const int64_t jb = d.b0 + t;
            const int j = (int)jb;
            double* sp = d.sum + (size_t)cm * d.stride + t;
            double s;
            if (d.flags & kMapInit) s = (d.old_sum && jb >= d.old_b0 && jb < d.old_b0 + d.old_n) ? d.old_sum[(size_t)cm * d.old_stride + (jb - d.old_b0)] : 0.0;
            else s = *sp;
            int lo = (int)((double)(j - 255) / 51.2) - 1;
            if (lo < 0) lo = 0;
            const int hi = (int)((double)j / 51.2) + 1;
            {
                const int a = lo < d.i0 ? (int)d.i0 : lo, b = hi > d.i1 - 1 ? (int)d.i1 - 1 : hi;
                for (int i = a; i <= b; ++i) {
                    const int dd = j - band_win_start(i);
                    if (dd < 0 || dd >= 256) continue;
                    s += (double)spec[((size_t)(d.slot0 + (i - d.i0)) * 256 + cm) * 256 + dd];
                }
            }
            *sp = s;
            if ((d.flags & kMapFin) && t < d.fin_n) {
                const int b = hi > d.i_end - 1 ? (int)d.i_end - 1 : hi;
                int n = 0;
                for (int i = lo; i <= b; ++i) {
                    const int dd = j - band_win_start(i);
                    n += dd >= 0 && dd < 256;
                }
                d.fmap[(size_t)cm * d.fin_n + t] = n ? (float)(s / (double)n) : 0.f;
            }
        }
    }
}

// Block = one band lane, thread = (spec channel, band).  The step's final bins are walked in ascending order: P(y) is added to the
// current tile's sum, and a tile is closed into the completed-tile sum behind every bin whose number ends a multiple of 64 -- a region's
// E is then completed tiles + current tile at its snapshot, term for term band_profile_kernel's tile sums added by band_bounds_kernel.
// The events are applied in the host's order (their positions never decrease); records and profiles leave by ordinary vector stores.
__global__ __launch_bounds__(256) void stream_band_kernel(const StreamBand* __restrict__ ds, const StreamBandEv* __restrict__ evs,
                                                          const double* __restrict__ hz, ss_region_band* __restrict__ out,
                                                          double* __restrict__ profile) {
#pragma clang fp contract(off)
    const StreamBand d = ds[blockIdx.x];
    const int t = threadIdx.x;
    double done = 0.0, cur = 0.0, sd = 0.0, sc = 0.0, pk = 0.0;
    if (d.acc_old) { done = d.acc_old[t]; cur = d.acc_old[256 + t]; sd = d.acc_old[512 + t]; sc = d.acc_old[768 + t]; pk = d.acc_old[1024 + t]; }
    int64_t j = d.b0;
    const int64_t end = d.b0 + d.nb;
    auto advance = [&](int64_t to) {
        if (to > end) to = end;
        for (; j < to; ++j) {
            cur += band_power(d.fmap[(size_t)t * d.nb + (j - d.b0)]);
            if ((j & 63) == 63) { done += cur; cur = 0.0; }
        }
    };
    for (int k = 0; k < d.nev; ++k) {
        const StreamBandEv ev = evs[d.ev0 + k];
        switch (ev.type) {
            case kEvReset: advance(ev.pos); done = 0.0; cur = 0.0; break;
            case kEvSnap: advance(ev.pos); sd = done; sc = cur; break;
            case kEvPark: pk = sd + sc; break;
            default: {
                const double e = ev.type == kEvEmitPark ? pk : sd + sc;
                const size_t o = (size_t)(d.out0 + ev.rec * d.lanes + d.lane);
                if (d.want_prof) profile[o * 256 + t] = e;
                band_bounds_block(e, ev.n_bins, d.speech_ch, d.q_low, d.q_high, hz, out + o);
            }
        }
    }
    advance(end);
    d.acc[t] = done; d.acc[256 + t] = cur; d.acc[512 + t] = sd; d.acc[768 + t] = sc; d.acc[1024 + t] = pk;
}

struct StreamRec {
    int format = 0, sr = 0, ch = 0;
    double thr = 0;                                   // (break_s: mg.brk)
    // the window step the stream was opened with (the context's then, or its image's): seconds, and floor(22050 step) samples
    double step = SS_STEP_DEFAULT; int64_t per_step = SS_STEP_SAMPLES;
    int L = 1, M = 1, half = 0;                       // 22 050 Hz: decoded straight into the signal (no resampler)
    float* d_taps = nullptr;
    int64_t frames_in = 0;                            // frames decoded so far
    std::vector<unsigned char> staged; int64_t staged_frames = 0;
    bool closed = false, finished = false;
    // carried state, in the current arena half (float offsets) -- or in the host vectors after an import (on_host)
    int64_t mono_off = 0, mono_base = 0, mono_n = 0;  // decoded input frames [mono_base, mono_base + mono_n)
    int64_t sig_off = 0, sig_base = 0, sig_n = 0;     // padded 22 050 Hz samples [sig_base, sig_base + sig_n)
    int64_t lg_off = 0, lg_w0 = 0, lg_n = 0;          // logits of windows [lg_w0, lg_w0 + lg_n)
    bool on_host = false; std::vector<float> h_mono, h_sig, h_lg;
    int64_t m_next = 0;                               // next resampled output (index into the unpadded signal)
    int64_t win_run = 0, bins_done = 0;
    // region walk, carried across steps: the open run of bins above the threshold, and the merge of the closed ones
    bool run_open = false; int64_t run_first = 0, run_last = 0; RunMerger mg;
    // the last step's results
    std::vector<ss_region> r_out; std::vector<double> a_out; std::vector<int64_t> b_out;
    // output (ss_stream_open_output): frames [0, frames_out) are returned; the raw PCM of [frames_out, frames_in) is carried in the
    // current half of the byte arena (byte offset raw_off, a multiple of 16) -- or in h_raw after an import (on_host); er_rng: the frame
    // ranges [begin, end) of the returned regions' erase table that reach past frames_out (ascending, merged)
    bool out_on = false; ss_stream_erase er{0, 0};
    bool src_out = false;                                 // the output in the stream's own encoding (ss_stream_open_source): o_off counts bytes
    int64_t frames_out = 0, erased = 0, raw_off = 0;
    std::vector<int64_t> er_rng; std::vector<unsigned char> h_raw;
    int64_t o_first = 0, o_n = 0, o_off = 0;          // the last step's frames: o_n of them at the pinned output buffer + o_off (int16s)
    // each-channel mode: `lanes` = ch lanes (1: a plain stream); lane l's carried segments lie l x mono_ls / sig_ls / lg_ls floats behind
    // lane 0's (mono_off, sig_off, lg_off) in the current arena half, and back to back in h_mono / h_sig / h_lg after an import
    int lanes = 1; int64_t mono_ls = 0, sig_ls = 0, lg_ls = 0;
    // running per-channel peaks (fmax over covered bins; -inf: none yet) of the open run, of the pending merged region (mg.cur, the gaps it
    // has merged included) and of the covered bins since the last run closed (the gap the next run may still merge)
    std::vector<double> pk_run, pk_cur, pk_gap;
    // the last step's results per lane: the lanes' averages of the bins in b_out (lane-major), peaks[r * lanes + c] of r_out
    std::vector<double> la_out, p_out;
    // bands (ss_stream_open_bands).  Per lane, in the current arena half at bs_off + l bs_ls (floats; doubles inside): kBandAcc vectors
    // of 256 doubles (completed tiles, current tile, the snapshot of both, the parked profile), then the float64 map sums of the bs_n
    // non-final bins [bins_done, bins_done + bs_n) as [256][bs_stride], the first carried bin at bs_sum_off floats behind the lane's base
    // -- or all of it in h_band after an import (per lane the vectors, then [256][bs_n]).  b_parked: a final region waits in the parked
    // vector for the walk to return it.  b_ev / b_b0: the event list of the step being committed and the step's first bin.
    bool bands_on = false, want_prof = false, b_parked = false; ss_band_params bprm{0.05, 0.95, 1, 0};
    int64_t bs_off = 0, bs_ls = 0, bs_stride = 0, bs_sum_off = 0, bs_n = 0;
    std::vector<double> h_band;
    std::vector<StreamBandEv> b_ev; int64_t b_b0 = 0;
    std::vector<ss_region_band> bd_out; std::vector<double> bp_out;      // the last step's records [n][lanes] and profiles [n][lanes][256]
    int64_t frame_bytes() const { return (int64_t)ch * (int64_t)pcm_bytes_per_sample(format); }
    void set_lanes(int n) { lanes = n; const double ninf = -HUGE_VAL; pk_run.assign(n > 1 ? n : 0, ninf); pk_cur = pk_run; pk_gap = pk_run; }
};

// what the next step does with a stream (host arithmetic only)
struct StreamPlan {
    int64_t F = 0;                                    // frames decoded after the step
    bool closing = false;
    int64_t kb = 0, mono_keep = 0;                    // mono history kept: [kb, frames_in), then the new frames
    int64_t m_end = 0;                                // outputs [m_next, m_end) are computed
    int64_t base_new = 0, sig_keep = 0, pre = 0, post = 0;   // signal: carried [base_new, +sig_keep), pre zeros, outputs, post zeros
    int64_t i_end = 0;                                // windows [win_run, i_end) run
    int64_t b_end = 0; int W_avg = 0;                 // bins [bins_done, b_end) become final
    int64_t lw0 = 0;                                  // logits in the step's arena: windows [lw0, i_end)
    // offsets in the next arena half
    int64_t mono_off = 0, sig_off = 0, lg_off = 0, up_off = 0, host_off = 0, raw_up_off = 0;
    int64_t mono_ls = 0, sig_ls = 0, lg_ls = 0;       // floats from a lane's segment to the next lane's
    int64_t f0 = 0; bool was_host = false;            // frames decoded before the step; the carried state came from an image
    // bands: the step's map sums cover bins [bins_done, bins_done + bs_n) per lane ([256][bs_stride] behind the accumulators at bs_off +
    // l bs_ls of the next half); the carried band state of an imported stream lies at band_up_off of the upload; the lane's final maps
    // at fmap_at floats of the step's map buffer
    int64_t bs_off = 0, bs_ls = 0, bs_stride = 0, bs_n = 0, band_up_off = 0, fmap_at = 0;
    const double* acc_old = nullptr; int64_t acc_old_ls = 0;   // lane 0's carried accumulators (nullptr: a stream without a step yet), doubles to the next lane's
    int64_t mono_len() const { return F - kb; }
    int64_t sig_len() const { return sig_keep + pre + (m_end - m_next_) + post; }
    int64_t m_next_ = 0;
};

int64_t n22_of(const StreamRec& s, int64_t F) { return ss_resampled_length(F, s.sr); }

// first bin of the stream's window i (NNDetector.py:175): the whole-file run's start table
int64_t win_start_bin(const StreamRec& s, int64_t i) { return ss_window_start_bin(i, s.step); }

// run_begin's plan of a file of F frames: window count (clamped to the padded signal) and bin count
void file_plan(const StreamRec& s, int64_t F, int64_t& W, int64_t& n_bins) {
    const int64_t n_padded = n22_of(s, F) + 2 * kPad;
    W = ss_plan_windows_step((double)F / (double)s.sr, s.step, nullptr, 0);
    while (W > 0 && (W - 1) * s.per_step + SS_WINDOW_SAMPLES > n_padded) --W;
    n_bins = (int64_t)std::nearbyint((double)n_padded / 22050.0 * 256.0 / 3.0);
}

StreamPlan plan_stream(const StreamRec& s) {
    StreamPlan p;
    p.m_next_ = s.m_next;
    p.F = s.frames_in + s.staged_frames;
    p.f0 = s.frames_in; p.was_host = s.on_host;
    p.closing = s.closed;
    const bool direct = s.sr == SS_SAMPLE_RATE;
    // outputs whose taps all lie inside the input (or past a closed stream's end)
    int64_t m_end;
    if (direct) m_end = p.F;
    else if (p.closing) m_end = n22_of(s, p.F);
    else {
        const int64_t X = p.F - s.half;               // output m needs input frames up to floor(m M / L) + half
        m_end = X > 0 ? std::min((X * s.L + s.M - 1) / s.M, n22_of(s, p.F)) : 0;
    }
    p.m_end = std::max(m_end, s.m_next);
    if (!direct) {
        const int64_t k0 = std::max<int64_t>(0, (s.m_next * s.M) / s.L - s.half + 1);   // first input the next outputs read
        p.kb = std::min(std::max(k0, s.mono_base), s.frames_in);
        p.mono_keep = s.frames_in - p.kb;
    }
    p.base_new = s.win_run * s.per_step;
    const int64_t sig_end = s.sig_base + s.sig_n;
    p.sig_keep = sig_end - p.base_new;
    p.pre = sig_end < kPad ? kPad - sig_end : 0;      // a new stream: the 3 s in front
    int64_t W_plan, nb_plan;
    file_plan(s, p.F, W_plan, nb_plan);
    if (p.closing) {
        p.post = kPad;
        p.i_end = W_plan;
        p.b_end = nb_plan;
    } else {
        // window i reads the unpadded samples [i per_step - 66150, i per_step) (13230 i at the default step); the plan of F frames is a
        // lower bound of the final one
        p.i_end = std::min(p.m_end / s.per_step + 1, W_plan);
        p.b_end = std::min(win_start_bin(s, p.i_end), nb_plan);    // every window that starts at or before such a bin has run
    }
    p.i_end = std::max(p.i_end, s.win_run);
    p.b_end = std::max(p.b_end, s.bins_done);
    p.W_avg = (int)p.i_end;
    p.lw0 = s.lg_n > 0 ? s.lg_w0 : s.win_run;
    return p;
}

// windows whose logits the bins from b on still need: start(i) + 256 > b (start(i) lies within half a bin of i s_b: the first guess
// is at or below the answer)
int64_t first_window_for_bin(const StreamRec& s, int64_t b) {
    int64_t i = std::max<int64_t>(0, (int64_t)std::floor((double)(b - 256) / step_bins(s.step)) - 1);
    while (win_start_bin(s, i) + 256 <= b) ++i;
    return i;
}

}  // namespace

struct StreamSet {
    std::map<int, StreamRec> s;
    int next_id = 0;
    float* arena[2] = {nullptr, nullptr}; size_t arena_cap[2] = {0, 0}; int cur = 0;
    unsigned char* d_up = nullptr; size_t up_cap = 0;                    // the step's upload: PCM, host carries, descriptors, window offsets
    unsigned char* h_up = nullptr; size_t h_up_cap = 0;                  // pinned
    float* d_newlg = nullptr; size_t newlg_cap = 0;
    double* d_avg = nullptr; size_t avg_cap = 0;
    unsigned char* d_flags = nullptr; size_t flags_cap = 0;
    std::vector<double> h_avg; std::vector<unsigned char> h_flags;
    // streams with output: the carried raw PCM in two halves like the arena, the step's second (small) upload of descriptors and
    // ranges, the step's output on the device and in pinned memory
    unsigned char* barena[2] = {nullptr, nullptr}; size_t barena_cap[2] = {0, 0}; int bcur = 0;
    unsigned char* d_up2 = nullptr; size_t up2_cap = 0;
    unsigned char* h_up2 = nullptr; size_t h_up2_cap = 0;
    short* d_out = nullptr; size_t out_cap = 0;
    unsigned char* h_out = nullptr; size_t h_out_cap = 0;
    unsigned char* d_outb = nullptr; size_t outb_cap = 0;               // the source-encoding streams' output, bytes
    unsigned char* h_outb = nullptr; size_t h_outb_cap = 0;
    // streams with bands: the step's final maps [bins][256] of every band lane, the upload of the walk's events and the lanes'
    // descriptors behind the flags download, the records and profiles on the device and in pinned memory, the 130 band edges
    float* d_fmap = nullptr; size_t fmap_cap = 0;
    unsigned char* d_up3 = nullptr; size_t up3_cap = 0;
    unsigned char* h_up3 = nullptr; size_t h_up3_cap = 0;
    ss_region_band* d_bout = nullptr; size_t bout_cap = 0;
    double* d_bprof = nullptr; size_t bprof_cap = 0;
    unsigned char* h_bres = nullptr; size_t h_bres_cap = 0;
    double* d_hz = nullptr;
    float* d_spec = nullptr; size_t spec_cap = 0;                        // the spec head's output of one pass of band windows
};

void free_streams(ss_ctx* c) {
    StreamSet* S = c->streams;
    if (!S) return;
    for (float* a : S->arena) if (a) hipFree(a);
    void* ds[] = {S->d_up, S->d_newlg, S->d_avg, S->d_flags, S->barena[0], S->barena[1], S->d_up2, S->d_out, S->d_outb, S->d_fmap, S->d_up3, S->d_bout, S->d_bprof, S->d_hz, S->d_spec};
    for (void* p : ds) if (p) hipFree(p);
    void* hs[] = {S->h_up, S->h_up2, S->h_out, S->h_outb, S->h_up3, S->h_bres};
    for (void* p : hs) if (p) hipHostFree(p);
    delete S;
    c->streams = nullptr;
}

}  // namespace ss

using namespace ss;

static StreamSet& streams_of(ss_ctx* c) {
    if (!c->streams) c->streams = new StreamSet();
    return *c->streams;
}

static StreamRec* find_stream(ss_ctx* c, int id) {
    if (!c || !c->streams) return nullptr;
    auto it = c->streams->s.find(id);
    return it == c->streams->s.end() ? nullptr : &it->second;
}

static int64_t state_bytes(const StreamRec& s) {
    return (int64_t)sizeof(StreamRec) + 4 * s.lanes * (s.mono_n + s.sig_n + s.lg_n * 256) + 8 * (int64_t)(3 * s.pk_run.size()) +
           (s.bands_on && !s.finished ? 8 * (int64_t)s.lanes * 256 * (kBandAcc + s.bs_n) : 0) +
           (s.out_on ? (s.frames_in - s.frames_out) * s.frame_bytes() + 8 * (int64_t)s.er_rng.size() : 0);
}

static int init_rates(ss_ctx* c, StreamRec& s) {
    if (s.sr == SS_SAMPLE_RATE) { s.L = s.M = 1; s.half = 0; s.d_taps = nullptr; return SS_OK; }
    return get_taps(c, s.sr, s.L, s.M, s.half, &s.d_taps);
}

static int open_stream(ss_ctx* c, int format, int sr, int ch, double threshold, double break_s, const ss_stream_erase* erase, bool out_on, int* id,
                       bool each = false, bool bands = false, const ss_band_params* bprm = nullptr, bool want_prof = false) {
    static const unsigned char one[8] = {0};
    int rc = check_pcm_args(c, one, format, sr, ch, 0);
    if (rc) return rc;
    // (a stream with output takes an infinite threshold: +inf is the plain transcode, -inf erases everything a window covers)
    if (!id || (out_on ? std::isnan(threshold) : !std::isfinite(threshold)) || !std::isfinite(break_s)) return fail(c, SS_ERR_ARG, "ss_stream_open: bad argument");
    if (!erase_ok(erase)) return fail(c, SS_ERR_ARG, "ss_stream_open_output: pad_s and min_len_s must be finite and >= 0");
    if (bands) {
        std::string err;
        if (check_band_args(nullptr, 0, bprm, err)) return fail(c, SS_ERR_ARG, "ss_stream_open_bands: " + err);
    }
    if (!c->has_model) return fail(c, SS_ERR_STATE, "context was created without weights (audio-only)");
    if (bands && c->step != SS_STEP_DEFAULT)
        return fail(c, SS_ERR_STATE, "ss_stream_open_bands: bands need the default window step (the maps are defined on 0.6 s windows)");
    hipSetDevice(c->device);
    StreamRec s;
    s.bands_on = bands; s.want_prof = bands && want_prof; if (bands && bprm) s.bprm = *bprm;
    s.format = format; s.sr = sr; s.ch = ch; s.thr = threshold; s.mg.brk = break_s;
    s.step = c->step; s.per_step = step_samples(c->step);
    s.out_on = out_on; if (erase) s.er = *erase;
    s.set_lanes(each ? ch : 1);                          // (one channel in each-channel mode: a plain stream)
    if ((rc = init_rates(c, s))) return rc;
    StreamSet& S = streams_of(c);
    *id = S.next_id++;
    S.s.emplace(*id, std::move(s));
    return SS_OK;
}

extern "C" int ss_stream_open(ss_ctx* c, int format, int sr, int ch, double threshold, double break_s, int* id) {
    return open_stream(c, format, sr, ch, threshold, break_s, nullptr, false, id);
}

extern "C" int ss_stream_open_output(ss_ctx* c, int format, int sr, int ch, double threshold, double break_s, const ss_stream_erase* erase,
                                     int* id) {
    return open_stream(c, format, sr, ch, threshold, break_s, erase, true, id);
}

extern "C" int ss_stream_open_channels(ss_ctx* c, int format, int sr, int ch, double threshold, double break_s, const ss_stream_erase* erase,
                                       int with_output, int* id) {
    return open_stream(c, format, sr, ch, threshold, break_s, erase, erase != nullptr || with_output != 0, id, true);
}

// a stream with output in its own encoding: ss_stream_open_channels' stream (each_channel == 0: the mix's) read through
// ss_stream_output_bytes
extern "C" int ss_stream_open_source(ss_ctx* c, int format, int sr, int ch, double threshold, double break_s, const ss_stream_erase* erase,
                                     int each_channel, int* id) {
    int rc = open_stream(c, format, sr, ch, threshold, break_s, erase, true, id, each_channel != 0);
    if (rc) return rc;
    find_stream(c, *id)->src_out = true;
    return SS_OK;
}

extern "C" int ss_stream_open_bands(ss_ctx* c, int format, int sr, int ch, double threshold, double break_s, const ss_stream_erase* erase,
                                    int with_output, int each_channel, const ss_band_params* params, int want_profile, int* id) {
    return open_stream(c, format, sr, ch, threshold, break_s, erase, erase != nullptr || with_output != 0, id, each_channel != 0, true, params,
                       want_profile != 0);
}

extern "C" int ss_stream_push(ss_ctx* c, int id, const void* pcm, int64_t frames) {
    StreamRec* s = find_stream(c, id);
    if (!s) return fail(c, SS_ERR_ARG, "ss_stream_push: no such stream");
    if (s->closed) return fail(c, SS_ERR_STATE, "ss_stream_push: the stream is closed");
    int rc = check_pcm_args(c, pcm, s->format, s->sr, s->ch, frames);
    if (rc) return rc;
    if (s->frames_in + s->staged_frames + frames > ((int64_t)1 << 36)) return fail(c, SS_ERR_ARG, "ss_stream_push: stream too long");
    const size_t nb = (size_t)frames * s->ch * pcm_bytes_per_sample(s->format);
    if (nb) s->staged.insert(s->staged.end(), (const unsigned char*)pcm, (const unsigned char*)pcm + nb);
    s->staged_frames += frames;
    return SS_OK;
}

extern "C" int ss_stream_close(ss_ctx* c, int id) {
    StreamRec* s = find_stream(c, id);
    if (!s) return fail(c, SS_ERR_ARG, "ss_stream_close: no such stream");
    s->closed = true;
    return SS_OK;
}

extern "C" int ss_stream_free(ss_ctx* c, int id) {
    if (!find_stream(c, id)) return fail(c, SS_ERR_ARG, "ss_stream_free: no such stream");
    c->streams->s.erase(id);
    return SS_OK;
}

extern "C" int ss_stream_get_info(ss_ctx* c, int id, ss_stream_info* out) {
    StreamRec* s = find_stream(c, id);
    if (!s || !out) return fail(c, SS_ERR_ARG, "ss_stream_get_info: bad argument");
    memset(out, 0, sizeof(*out));
    out->frames_pushed = s->frames_in + s->staged_frames;
    out->frames_staged = s->staged_frames;
    out->windows_run = s->win_run;
    out->windows_ready = s->finished ? 0 : plan_stream(*s).i_end - s->win_run;
    out->final_until_s = (double)s->bins_done * 3.0 / 256.0 - 3.0;
    out->closed = s->closed; out->finished = s->finished;
    out->state_bytes = state_bytes(*s);
    return SS_OK;
}

extern "C" int ss_stream_regions(ss_ctx* c, int id, ss_region* out, int64_t cap, int64_t* n_out) {
    StreamRec* s = find_stream(c, id);
    if (!s || !n_out) return fail(c, SS_ERR_ARG, "ss_stream_regions: bad argument");
    *n_out = (int64_t)s->r_out.size();
    if (!out) return SS_OK;
    if (cap < *n_out) return fail(c, SS_ERR_CAPACITY, "ss_stream_regions: capacity < " + std::to_string(*n_out));
    if (*n_out) memcpy(out, s->r_out.data(), s->r_out.size() * sizeof(ss_region));
    return SS_OK;
}

extern "C" int ss_stream_avg(ss_ctx* c, int id, double* avg, int64_t* bin_idx, int64_t cap, int64_t* n_out) {
    StreamRec* s = find_stream(c, id);
    if (!s || !n_out) return fail(c, SS_ERR_ARG, "ss_stream_avg: bad argument");
    *n_out = (int64_t)s->a_out.size();
    if (!avg && !bin_idx) return SS_OK;
    if (cap < *n_out) return fail(c, SS_ERR_CAPACITY, "ss_stream_avg: capacity < " + std::to_string(*n_out));
    if (*n_out && avg) memcpy(avg, s->a_out.data(), s->a_out.size() * 8);
    if (*n_out && bin_idx) memcpy(bin_idx, s->b_out.data(), s->b_out.size() * 8);
    return SS_OK;
}

extern "C" int ss_stream_avg_channel(ss_ctx* c, int id, int channel, double* avg, int64_t* bin_idx, int64_t cap, int64_t* n_out) {
    StreamRec* s = find_stream(c, id);
    if (!s || !n_out) return fail(c, SS_ERR_ARG, "ss_stream_avg_channel: bad argument");
    if (channel < 0 || channel >= s->lanes) return fail(c, SS_ERR_ARG, "ss_stream_avg_channel: no such channel (a mix stream has channel 0 only)");
    if (s->lanes == 1) return ss_stream_avg(c, id, avg, bin_idx, cap, n_out);
    *n_out = (int64_t)s->b_out.size();
    if (!avg && !bin_idx) return SS_OK;
    if (cap < *n_out) return fail(c, SS_ERR_CAPACITY, "ss_stream_avg_channel: capacity < " + std::to_string(*n_out));
    if (*n_out && avg) memcpy(avg, s->la_out.data() + (size_t)channel * s->b_out.size(), s->b_out.size() * 8);
    if (*n_out && bin_idx) memcpy(bin_idx, s->b_out.data(), s->b_out.size() * 8);
    return SS_OK;
}

extern "C" int ss_stream_region_peaks(ss_ctx* c, int id, double* peaks, int64_t cap_regions, int64_t* n_out) {
    StreamRec* s = find_stream(c, id);
    if (!s || !n_out) return fail(c, SS_ERR_ARG, "ss_stream_region_peaks: bad argument");
    if (s->lanes == 1) return fail(c, SS_ERR_STATE, "ss_stream_region_peaks: not an each-channel stream of several channels (ss_stream_open_channels)");
    *n_out = (int64_t)s->r_out.size();
    if (!peaks) return SS_OK;
    if (cap_regions < *n_out) return fail(c, SS_ERR_CAPACITY, "ss_stream_region_peaks: capacity < " + std::to_string(*n_out) + " regions");
    if (!s->p_out.empty()) memcpy(peaks, s->p_out.data(), s->p_out.size() * 8);
    return SS_OK;
}

extern "C" int ss_stream_bands(ss_ctx* c, int id, ss_region_band* out, double* profile, int64_t cap_regions, int64_t* n_out) {
    StreamRec* s = find_stream(c, id);
    if (!s || !n_out) return fail(c, SS_ERR_ARG, "ss_stream_bands: bad argument");
    if (!s->bands_on) return fail(c, SS_ERR_STATE, "ss_stream_bands: the stream was opened without bands (ss_stream_open_bands)");
    if (profile && !s->want_prof) return fail(c, SS_ERR_STATE, "ss_stream_bands: the stream was opened without want_profile");
    *n_out = (int64_t)s->r_out.size();
    if (!out && !profile) return SS_OK;
    if (cap_regions < *n_out) return fail(c, SS_ERR_CAPACITY, "ss_stream_bands: capacity < " + std::to_string(*n_out) + " regions");
    if (out && !s->bd_out.empty()) memcpy(out, s->bd_out.data(), s->bd_out.size() * sizeof(ss_region_band));
    if (profile && !s->bp_out.empty()) memcpy(profile, s->bp_out.data(), s->bp_out.size() * 8);
    return SS_OK;
}

extern "C" int ss_stream_output(ss_ctx* c, int id, int16_t* out, int64_t cap_frames, int64_t* first_frame, int64_t* n_frames) {
    StreamRec* s = find_stream(c, id);
    if (!s || !first_frame || !n_frames) return fail(c, SS_ERR_ARG, "ss_stream_output: bad argument");
    if (!s->out_on) return fail(c, SS_ERR_STATE, "ss_stream_output: the stream was opened without output (ss_stream_open_output)");
    if (s->src_out) return fail(c, SS_ERR_STATE, "ss_stream_output: the stream's output is in its own encoding (ss_stream_output_bytes)");
    *first_frame = s->o_first; *n_frames = s->o_n;
    if (!out) return SS_OK;
    if (cap_frames < s->o_n) return fail(c, SS_ERR_CAPACITY, "ss_stream_output: capacity < " + std::to_string(s->o_n));
    if (s->o_n) memcpy(out, (const int16_t*)c->streams->h_out + s->o_off, (size_t)(s->o_n * s->ch) * 2);
    return SS_OK;
}

extern "C" int ss_stream_output_bytes(ss_ctx* c, int id, void* out, int64_t cap_bytes, int64_t* first_frame, int64_t* n_frames) {
    StreamRec* s = find_stream(c, id);
    if (!s || !first_frame || !n_frames) return fail(c, SS_ERR_ARG, "ss_stream_output_bytes: bad argument");
    if (!s->src_out) return fail(c, SS_ERR_STATE, "ss_stream_output_bytes: the stream was not opened with ss_stream_open_source");
    *first_frame = s->o_first; *n_frames = s->o_n;
    if (!out) return SS_OK;
    const int64_t bytes = s->o_n * s->frame_bytes();
    if (cap_bytes < bytes) return fail(c, SS_ERR_CAPACITY, "ss_stream_output_bytes: capacity < " + std::to_string(bytes));
    if (bytes) memcpy(out, c->streams->h_outb + s->o_off, (size_t)bytes);
    return SS_OK;
}

extern "C" int ss_stream_get_output_info(ss_ctx* c, int id, ss_stream_output_info* out) {
    StreamRec* s = find_stream(c, id);
    if (!s || !out) return fail(c, SS_ERR_ARG, "ss_stream_get_output_info: bad argument");
    if (!s->out_on) return fail(c, SS_ERR_STATE, "ss_stream_get_output_info: the stream was opened without output (ss_stream_open_output)");
    memset(out, 0, sizeof(*out));
    out->frames_out = s->frames_out; out->frames_held = s->frames_in + s->staged_frames - s->frames_out; out->frames_erased = s->erased;
    out->pad_s = s->er.pad_s; out->min_len_s = s->er.min_len_s;
    return SS_OK;
}

// ------------------------------------------------------------------------------------------------------
// the step
// ------------------------------------------------------------------------------------------------------
// the region walk over bins in order, one bin at a time: a run opens at a bin above the threshold and closes at the next covered bin
// that is not; closed runs go through the stream's RunMerger.  A merged region is final once a covered bin lies more than brk after
// its end (bin times never decrease, so no later run can merge into it).
// An each-channel stream walks its merged flags, and beside them keeps every channel's peak (ss_stream_region_peaks): v[l vs] is lane l's
// average of the bin (v == nullptr: a plain stream, which keeps none).  A region's peaks are the fmax over its covered bins from its first to its last one -- the runs, and the gaps
// between them that the merger joined -- so the gap behind the last closed run is held apart until the next run decides whether it
// belongs.  fmax of doubles is exact in any order: the values are ss_get_region_peaks' of the whole-file run.
// Bands: the walk's decisions as events for stream_band_kernel (StreamBandEv).  Positions come from rule 1 on the very ss_region values
// the stream returns (start = bin_time(first) - 3, end = bin_time(last) - 3: a region's bins run from its first bin to just before the
// last bin of its last run).  A run that opens within brk of the pending region will merge (RunMerger::add's own test, decided by
// the run's first bin): the accumulators run on across the gap.  Any other run starts a candidate: reset at its first bin -- the pending
// region, now final though the walk returns it only when this run closes or a later bin passes brk, has its profile parked first.  The
// snapshot is taken where a run closes and, for a run still open at the end of a step, at its last bin so far: the next step may find
// that bin to have been the last.
static int64_t band_pos(double bin_t) {
    int64_t first, count;
    const double x = bin_t - 3.0;
    region_bins(x, x, 0, (int64_t)1 << 40, first, count);
    return first;
}
static void band_emit(StreamRec& s, size_t n0) {          // the walk has just returned regions n0 .. (at most one)
    for (size_t r = n0; r < s.r_out.size(); ++r) {
        int64_t first, count;
        region_bins(s.r_out[r].start, s.r_out[r].end, 0, (int64_t)1 << 40, first, count);
        s.b_ev.push_back(StreamBandEv{0, s.b_parked ? kEvEmitPark : kEvEmitSnap, (int32_t)count, (int64_t)r});
        s.b_parked = false;
    }
}
static void band_snap(StreamRec& s) {                     // the candidate's bins end before run_last (a snapshot of an earlier step holds otherwise)
    const int64_t pos = band_pos(bin_time(s.run_last));
    if (pos >= s.b_b0) s.b_ev.push_back(StreamBandEv{pos, kEvSnap, 0, 0});
}

static void close_run(StreamRec& s) {
    const bool had = s.mg.have;
    const size_t n0 = s.r_out.size();
    s.mg.add(s.run_first, s.run_last, s.r_out);
    s.run_open = false;
    if (s.bands_on) { band_emit(s, n0); band_snap(s); }
    if (s.lanes == 1) return;
    const bool emitted = s.r_out.size() > n0;             // the run did not reach the pending region: that one is final
    if (emitted) s.p_out.insert(s.p_out.end(), s.pk_cur.begin(), s.pk_cur.end());
    for (int l = 0; l < s.lanes; ++l) {
        s.pk_cur[l] = had && !emitted ? std::fmax(std::fmax(s.pk_cur[l], s.pk_gap[l]), s.pk_run[l]) : s.pk_run[l];
        s.pk_run[l] = s.pk_gap[l] = -HUGE_VAL;
    }
}

static void flush_merged(StreamRec& s) {
    const size_t n0 = s.r_out.size();
    s.mg.flush(s.r_out);
    if (s.bands_on) band_emit(s, n0);
    if (s.lanes > 1 && s.r_out.size() > n0) s.p_out.insert(s.p_out.end(), s.pk_cur.begin(), s.pk_cur.end());
}

static void walk_bin(StreamRec& s, int64_t j, unsigned char f, const double* v, int64_t vs) {
    if (!(f & 1)) return;                                 // not covered: absent from the reference's series
    if (f & 2) {
        if (!s.run_open) {
            s.run_open = true; s.run_first = j;
            if (s.bands_on && !(s.mg.have && bin_time(j) - s.mg.cur.end <= s.mg.brk)) {
                if (s.mg.have) { s.b_ev.push_back(StreamBandEv{0, kEvPark, 0, 0}); s.b_parked = true; }
                s.b_ev.push_back(StreamBandEv{band_pos(bin_time(j)), kEvReset, 0, 0});
            }
        }
        s.run_last = j;
        if (v) for (int l = 0; l < s.lanes; ++l) s.pk_run[l] = std::fmax(s.pk_run[l], v[l * vs]);
        return;
    }
    if (s.run_open) close_run(s);
    if (v) for (int l = 0; l < s.lanes; ++l) s.pk_gap[l] = std::fmax(s.pk_gap[l], v[l * vs]);
    if (s.mg.have && bin_time(j) - s.mg.cur.end > s.mg.brk) flush_merged(s);
}

static void finish_regions(StreamRec& s) {
    if (s.run_open) close_run(s);
    flush_merged(s);
}

static int ensure_pinned(ss_ctx* c, unsigned char** p, size_t* cap, size_t need) {
    if (need <= *cap && *p) return SS_OK;
    if (*p) { HIPCHK(c, hipHostFree(*p)); *p = nullptr; *cap = 0; }
    const size_t nc = std::max(need + need / 2, (size_t)1 << 16);
    HIPCHK(c, hipHostMalloc((void**)p, nc, hipHostMallocDefault));
    *cap = nc;
    return SS_OK;
}

// ---- the output of the streams opened with it (include/softspoken.h: which frames a step returns) ----
// [begin, end) of one region of the erase table as silence_ranges rounds it, clamped at frame 0 (the clamp to the recording's length
// is the limit's: no frame at or past it is looked at)
static void erase_frames(const ss_region& padded, int sr, int64_t& lo, int64_t& hi) {
    const double a = std::nearbyint(padded.start * (double)sr), b = std::nearbyint(padded.end * (double)sr);
    lo = (int64_t)std::min(std::max(a, 0.0), 9.0e18); hi = (int64_t)std::min(std::max(b, 0.0), 9.0e18);
}

static void merge_ranges(std::vector<int64_t>& r) {      // sorted by begin, overlapping and touching ranges joined, as silence_ranges
    std::vector<std::pair<int64_t, int64_t>> v;
    for (size_t i = 0; i + 1 < r.size(); i += 2) if (r[i + 1] > r[i]) v.emplace_back(r[i], r[i + 1]);
    std::sort(v.begin(), v.end());
    r.clear();
    for (const auto& p : v) {
        if (!r.empty() && p.first <= r.back()) r.back() = std::max(r.back(), p.second);
        else { r.push_back(p.first); r.push_back(p.second); }
    }
}

// After the commit: the streams' walks have taken in the step's bins, frames_in counts the step's frames, the staged bytes still lie
// in the upload.  One launch encodes every stream's decided frames, one copies the raw PCM that stays into the other half of the byte
// arena, one copy brings all output to pinned memory.
static int step_output(ss_ctx* c, StreamSet& S, std::vector<std::pair<StreamRec*, StreamPlan>>& act) {
    struct OutPlan { StreamRec* s; const StreamPlan* p; int64_t limit, rng_at, n_rng, out_off, raw_off, erased; };
    std::vector<OutPlan> ops;
    std::vector<int64_t> rng_all;
    auto al = [](int64_t x, int64_t a) { return (x + a - 1) / a * a; };
    int64_t total_out = 0, total_outb = 0, raw_need = 0;      // int16 samples; bytes of the source-encoding streams; carried bytes
    for (auto& [sp, p] : act) {
        StreamRec& s = *sp;
        if (!s.out_on) continue;
        OutPlan o{sp, &p, 0, (int64_t)rng_all.size(), 0, 0, 0, 0};
        auto add_region = [&](std::vector<int64_t>& to, const ss_region& r) {
            if (!erase_keeps(r, s.er.min_len_s)) return;
            int64_t lo, hi;
            erase_frames(erase_padded(r, s.er.pad_s), s.sr, lo, hi);
            if (hi > lo) { to.push_back(lo); to.push_back(hi); }
        };
        for (const ss_region& r : s.r_out) add_region(s.er_rng, r);       // what the step returned (everything, at close)
        merge_ranges(s.er_rng);
        std::vector<int64_t> rng = s.er_rng;
        if (s.finished) o.limit = s.frames_in;
        else {
            // P: the current region joined with the open run where RunMerger::add would join them; a current region the open run
            // cannot reach any more is final (the walk returns it when the run closes) and is erased as a decided one
            bool pending = false; double ps = 0, pe = 0;
            if (s.run_open) {
                const double rs = bin_time(s.run_first), re = bin_time(s.run_last);
                pending = true; ps = rs; pe = re;
                if (s.mg.have) {
                    if (rs - s.mg.cur.end <= s.mg.brk) ps = s.mg.cur.start;
                    else add_region(rng, ss_region{s.mg.cur.start - 3.0, s.mg.cur.end - 3.0});
                }
            } else if (s.mg.have) { pending = true; ps = s.mg.cur.start; pe = s.mg.cur.end; }
            if (pending) add_region(rng, ss_region{ps - 3.0, pe - 3.0});   // its certain part (nothing when it fails the filter)
            const int64_t lim = ss_stream_output_limit(s.sr, s.bins_done, pending, ps, pe, &s.er);
            o.limit = std::min(std::max(lim, s.frames_out), s.frames_in);
            merge_ranges(rng);
        }
        for (size_t i = 0; i + 1 < rng.size(); i += 2) {                   // the part inside [frames_out, limit)
            const int64_t lo = std::max(rng[i], s.frames_out), hi = std::min(rng[i + 1], o.limit);
            if (hi > lo) { rng_all.push_back(lo); rng_all.push_back(hi); o.erased += hi - lo; }
        }
        o.n_rng = ((int64_t)rng_all.size() - o.rng_at) / 2;
        if (s.src_out) { o.out_off = total_outb; total_outb = al(total_outb + (o.limit - s.frames_out) * s.frame_bytes(), 16); }
        else { o.out_off = total_out; total_out = al(total_out + (o.limit - s.frames_out) * s.ch, 8); }
        o.raw_off = raw_need; raw_need = al(raw_need + (s.frames_in - o.limit) * s.frame_bytes(), 16);
        ops.push_back(o);
    }
    if (ops.empty()) return SS_OK;
    int rc;
    const int bnxt = S.bcur ^ 1;
    if ((rc = ensure(c, &S.barena[bnxt], &S.barena_cap[bnxt], (size_t)std::max<int64_t>(raw_need, 16)))) return rc;
    if ((rc = ensure(c, &S.d_out, &S.out_cap, (size_t)std::max<int64_t>(total_out, 8)))) return rc;
    if ((rc = ensure_pinned(c, &S.h_out, &S.h_out_cap, (size_t)std::max<int64_t>(total_out, 8) * 2))) return rc;
    if (total_outb > 0) {
        if ((rc = ensure(c, &S.d_outb, &S.outb_cap, (size_t)total_outb + 16))) return rc;
        if ((rc = ensure_pinned(c, &S.h_outb, &S.h_outb_cap, (size_t)total_outb + 16))) return rc;
    }
    const size_t o_sil = 0, o_cpb = (size_t)al((int64_t)(ops.size() * sizeof(StreamSilence)), 64);
    const size_t o_src = o_cpb + (size_t)al((int64_t)(2 * ops.size() * sizeof(StreamCopyBytes)), 64);
    const size_t o_rng = o_src + (size_t)al((int64_t)(ops.size() * sizeof(StreamSilenceSource)), 64);
    const size_t up2 = o_rng + rng_all.size() * 8 + 64;
    if ((rc = ensure(c, &S.d_up2, &S.up2_cap, up2))) return rc;
    if ((rc = ensure_pinned(c, &S.h_up2, &S.h_up2_cap, up2))) return rc;
    std::vector<StreamSilence> sil;
    std::vector<StreamCopyBytes> cpb;
    std::vector<StreamSilenceSource> srcs;
    int64_t max_samples = 0, max_bytes = 0, max_src = 0;
    double in_bytes = 0, carried = 0, src_bytes = 0;
    for (const OutPlan& o : ops) {
        StreamRec& s = *o.s;
        const StreamPlan& p = *o.p;
        const int64_t fb = s.frame_bytes(), n = o.limit - s.frames_out;
        // the frames [frames_out, f0) carried from earlier steps, and the step's own [f0, frames_in) in the upload
        const unsigned char* seg0 = p.was_host ? S.d_up + p.raw_up_off : S.barena[S.bcur] + s.raw_off;
        const unsigned char* seg1 = S.d_up + p.up_off;
        if (n > 0 && s.src_out) {   // bytes in, bytes out: the ranges as byte numbers of the recording
            for (int64_t i = o.rng_at; i < o.rng_at + 2 * o.n_rng; ++i) rng_all[(size_t)i] *= fb;
            srcs.push_back(StreamSilenceSource{seg0, seg1, (const int64_t*)(S.d_up2 + o_rng) + o.rng_at, std::min(n, p.f0 - s.frames_out) * fb,
                                               s.frames_out * fb, n * fb, o.out_off, (int32_t)o.n_rng, s.format == SS_PCM_U8 ? 0x80808080u : 0u});
            max_src = std::max(max_src, n * fb);
            src_bytes += (double)(n * fb);
        } else if (n > 0) {
            sil.push_back(StreamSilence{seg0, seg1, (const int64_t*)(S.d_up2 + o_rng) + o.rng_at, std::min(n, p.f0 - s.frames_out), s.frames_out, n,
                                        o.out_off, (int32_t)o.n_rng, s.format, s.ch, 0});
            max_samples = std::max(max_samples, n * s.ch);
            in_bytes += (double)(n * fb);
        }
        unsigned char* dst = S.barena[bnxt] + o.raw_off;
        const size_t k0 = cpb.size();
        if (o.limit < p.f0) {
            cpb.push_back(StreamCopyBytes{seg0 + (o.limit - s.frames_out) * fb, dst, (p.f0 - o.limit) * fb});
            dst += (p.f0 - o.limit) * fb;
        }
        const int64_t from = std::max(o.limit, p.f0);
        if (from < s.frames_in) cpb.push_back(StreamCopyBytes{seg1 + (from - p.f0) * fb, dst, (s.frames_in - from) * fb});
        for (size_t k = k0; k < cpb.size(); ++k) { max_bytes = std::max(max_bytes, cpb[k].n); carried += (double)cpb[k].n; }
    }
    if (!sil.empty()) memcpy(S.h_up2 + o_sil, sil.data(), sil.size() * sizeof(StreamSilence));
    if (!cpb.empty()) memcpy(S.h_up2 + o_cpb, cpb.data(), cpb.size() * sizeof(StreamCopyBytes));
    if (!srcs.empty()) memcpy(S.h_up2 + o_src, srcs.data(), srcs.size() * sizeof(StreamSilenceSource));
    if (!rng_all.empty()) memcpy(S.h_up2 + o_rng, rng_all.data(), rng_all.size() * 8);
    HIPCHK(c, hipMemcpyAsync(S.d_up2, S.h_up2, o_rng + rng_all.size() * 8, hipMemcpyHostToDevice, c->stream));
    {
        ScopedLaunch sl(c, c->stream, "stream_silence_kernel", 0.0, in_bytes + 2.0 * (double)total_out);
        HIPCHK(c, launch_stream_silence((const StreamSilence*)(S.d_up2 + o_sil), (int)sil.size(), max_samples, S.d_out, c->stream));
    }
    if (!srcs.empty()) {        // (the copy of the carried PCM below writes the other half of the byte arena: either order will do)
        ScopedLaunch sl(c, c->stream, "stream_silence_source_kernel", 0.0, 2.0 * src_bytes);
        HIPCHK(c, launch_stream_silence_source((const StreamSilenceSource*)(S.d_up2 + o_src), (int)srcs.size(), max_src, S.d_outb, c->stream));
    }
    {
        ScopedLaunch sl(c, c->stream, "stream_copy_bytes", 0.0, 2.0 * carried);
        HIPCHK(c, launch_stream_copy_bytes((const StreamCopyBytes*)(S.d_up2 + o_cpb), (int)cpb.size(), max_bytes, c->stream));
    }
    if (!sil.empty()) HIPCHK(c, hipMemcpyAsync(S.h_out, S.d_out, (size_t)total_out * 2, hipMemcpyDeviceToHost, c->stream));
    if (!srcs.empty()) HIPCHK(c, hipMemcpyAsync(S.h_outb, S.d_outb, (size_t)total_outb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    for (const OutPlan& o : ops) {
        StreamRec& s = *o.s;
        s.o_first = s.frames_out; s.o_n = o.limit - s.frames_out; s.o_off = o.out_off;
        s.frames_out = o.limit; s.erased += o.erased; s.raw_off = o.raw_off;
        std::vector<int64_t> keep;
        for (size_t i = 0; i + 1 < s.er_rng.size(); i += 2) if (s.er_rng[i + 1] > o.limit) { keep.push_back(s.er_rng[i]); keep.push_back(s.er_rng[i + 1]); }
        s.er_rng.swap(keep);
    }
    S.bcur = bnxt;
    return SS_OK;
}

// Behind the commit's walks: every band lane's accumulators move to the other arena half through stream_band_kernel, which takes in the
// step's final bins under the stream's events and evaluates the regions the walk returned; one copy brings the records (and profiles)
// to pinned memory.  `A`: the half the step built.
static int step_bands(ss_ctx* c, StreamSet& S, std::vector<std::pair<StreamRec*, StreamPlan>>& act, float* A) {
    std::vector<StreamBand> bd;
    std::vector<StreamBandEv> evs;
    int64_t n_rec = 0; bool any_prof = false;
    for (auto& [sp, p] : act) {
        StreamRec& s = *sp;
        if (!s.bands_on) continue;
        const int64_t nb = s.bins_done - s.b_b0;
        for (int l = 0; l < s.lanes; ++l)
            bd.push_back(StreamBand{p.acc_old ? p.acc_old + l * p.acc_old_ls : nullptr, (double*)(A + p.bs_off + l * p.bs_ls), S.d_fmap + p.fmap_at + l * nb * 256,
                                    s.b_b0, nb, n_rec, (int32_t)evs.size(), (int32_t)s.b_ev.size(), s.lanes, l, s.bprm.speech_channel, s.want_prof ? 1 : 0,
                                    s.bprm.q_low, s.bprm.q_high});
        evs.insert(evs.end(), s.b_ev.begin(), s.b_ev.end());
        n_rec += (int64_t)s.r_out.size() * s.lanes;
        any_prof = any_prof || s.want_prof;
    }
    if (bd.empty()) return SS_OK;
    int rc;
    auto al = [](size_t x) { return (x + 63) / 64 * 64; };
    const size_t o_ev = al(bd.size() * sizeof(StreamBand)), up3 = o_ev + al(evs.size() * sizeof(StreamBandEv)) + 64;
    const size_t rec_bytes = al((size_t)n_rec * sizeof(ss_region_band)), prof_bytes = any_prof ? (size_t)n_rec * 256 * 8 : 0;
    if ((rc = ensure(c, &S.d_up3, &S.up3_cap, up3))) return rc;
    if ((rc = ensure_pinned(c, &S.h_up3, &S.h_up3_cap, up3))) return rc;
    if ((rc = ensure(c, &S.d_bout, &S.bout_cap, (size_t)std::max<int64_t>(n_rec, 1)))) return rc;
    if ((rc = ensure(c, &S.d_bprof, &S.bprof_cap, (size_t)std::max<int64_t>(any_prof ? n_rec * 256 : 1, 1)))) return rc;
    if ((rc = ensure_pinned(c, &S.h_bres, &S.h_bres_cap, rec_bytes + prof_bytes + 64))) return rc;
    if (!S.d_hz) {
        double f[130];
        band_edges(f);
        HIPCHK(c, hipMalloc((void**)&S.d_hz, sizeof f));
        HIPCHK(c, hipMemcpy(S.d_hz, f, sizeof f, hipMemcpyHostToDevice));
    }
    memcpy(S.h_up3, bd.data(), bd.size() * sizeof(StreamBand));
    if (!evs.empty()) memcpy(S.h_up3 + o_ev, evs.data(), evs.size() * sizeof(StreamBandEv));
    HIPCHK(c, hipMemcpyAsync(S.d_up3, S.h_up3, o_ev + evs.size() * sizeof(StreamBandEv), hipMemcpyHostToDevice, c->stream));
    {
        double bins = 0; for (const StreamBand& b : bd) bins += (double)b.nb;
        ScopedLaunch sl(c, c->stream, "stream_band_kernel", 0.0, bins * 1024 + (double)bd.size() * kBandAcc * 4096 + (double)n_rec * (48 + (any_prof ? 2048 : 0)));
        hipLaunchKernelGGL(stream_band_kernel, dim3((unsigned)bd.size()), dim3(256), 0, c->stream, (const StreamBand*)S.d_up3, (const StreamBandEv*)(S.d_up3 + o_ev),
                           S.d_hz, S.d_bout, S.d_bprof);
        HIPCHK(c, hipGetLastError());
    }
    if (n_rec) {
        HIPCHK(c, hipMemcpyAsync(S.h_bres, S.d_bout, (size_t)n_rec * sizeof(ss_region_band), hipMemcpyDeviceToHost, c->stream));
        if (any_prof) HIPCHK(c, hipMemcpyAsync(S.h_bres + rec_bytes, S.d_bprof, prof_bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    int64_t at = 0;
    for (auto& [sp, p] : act) {
        StreamRec& s = *sp;
        if (!s.bands_on) continue;
        const int64_t n = (int64_t)s.r_out.size() * s.lanes;
        if (n) {
            s.bd_out.assign((const ss_region_band*)S.h_bres + at, (const ss_region_band*)S.h_bres + at + n);
            if (s.want_prof) s.bp_out.assign((const double*)(S.h_bres + rec_bytes) + at * 256, (const double*)(S.h_bres + rec_bytes) + (at + n) * 256);
        }
        at += n;
        s.b_ev.clear();
    }
    return SS_OK;
}

extern "C" int ss_stream_step(ss_ctx* c) {
    if (!c) return fail(nullptr, SS_ERR_ARG, "null context");
    if (!c->has_model) return fail(c, SS_ERR_STATE, "context was created without weights (audio-only)");
    if (c->run_pending) return fail(c, SS_ERR_STATE, "a run is in flight: ss_run_end first");
    hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));             // (the pinned upload buffer is rewritten below)
    StreamSet& S = streams_of(c);
    int rc;
    // ---- plan every unfinished stream (host only; nothing is changed before the commit) ----
    std::vector<std::pair<StreamRec*, StreamPlan>> act;
    for (auto& kv : S.s) if (!kv.second.finished) act.emplace_back(&kv.second, plan_stream(kv.second));
    // arena layout of the next half, upload layout, descriptors
    const int nxt = S.cur ^ 1;
    float* cur_arena = S.arena[S.cur];
    auto al = [](int64_t x, int64_t a) { return (x + a - 1) / a * a; };
    int64_t arena_need = 0, up_bytes = 0, total_w = 0, total_b = 0, n_lanes = 0, n_each = 0;
    // windows of streams with bands run in passes of their own, behind the others': those passes store the spec head's output
    int64_t total_w_band = 0, n_band_lanes = 0, fmap_need = 0;
    double avg_reads = 0;                                   // logits the averaging reads: 256 / s_b windows per bin
    for (auto& [sp, p] : act) {
        const StreamRec& s = *sp;
        // (arena_need stays a multiple of 64; a plain stream has one lane)
        if (s.sr != SS_SAMPLE_RATE) { p.mono_off = arena_need; p.mono_ls = al(p.mono_len(), 64); arena_need += s.lanes * p.mono_ls; }
        p.sig_off = arena_need; p.sig_ls = al(p.sig_len() + 64, 64); arena_need += s.lanes * p.sig_ls;    // (+ 64: slack behind the last window, as the file arena)
        p.lg_off = arena_need; p.lg_ls = al((p.i_end - p.lw0) * 256, 64); arena_need += s.lanes * p.lg_ls;
        p.up_off = up_bytes; up_bytes = al(up_bytes + (int64_t)s.staged.size(), 16);
        p.host_off = up_bytes;
        if (s.on_host) up_bytes = al(up_bytes + 4 * (int64_t)(s.h_mono.size() + s.h_sig.size() + s.h_lg.size()), 16);
        p.raw_up_off = up_bytes;
        if (s.on_host && s.out_on) up_bytes = al(up_bytes + (int64_t)s.h_raw.size(), 16);
        if (s.bands_on) {
            // the step's sums reach from the first non-final bin to the last bin a window of the step covers (or a carried sum, or the
            // last bin that becomes final: behind a closed stream's last window there are bins without a window)
            const int64_t top = std::max({p.b_end, s.bins_done + s.bs_n, p.i_end > 0 ? ss_window_start_bin(p.i_end - 1, SS_STEP_DEFAULT) + 256 : (int64_t)0});
            p.bs_n = top - s.bins_done; p.bs_stride = al(std::max<int64_t>(p.bs_n, 1), 8);
            p.bs_off = arena_need; p.bs_ls = al(2 * 256 * (kBandAcc + p.bs_stride), 64); arena_need += s.lanes * p.bs_ls;
            p.band_up_off = up_bytes;
            if (s.on_host) up_bytes = al(up_bytes + 8 * (int64_t)s.h_band.size(), 16);
            p.fmap_at = fmap_need; fmap_need += s.lanes * (p.b_end - s.bins_done) * 256;
            total_w_band += s.lanes * (p.i_end - s.win_run); n_band_lanes += s.lanes;
        }
        total_w += s.lanes * (p.i_end - s.win_run);
        total_b += (s.lanes > 1 ? s.lanes + 1 : 1) * (p.b_end - s.bins_done);      // every lane's bins, then the merged ones
        n_lanes += s.lanes; n_each += s.lanes > 1;
    }
    std::vector<StreamCopy> pre, post;
    std::vector<StreamDecode> dec;
    std::vector<StreamDecodeChannels> decc;                 // each-channel streams only: a step without one launches neither kernel
    std::vector<StreamUnion> uni;
    std::vector<StreamResample> res;
    std::vector<StreamAvg> avg;
    std::vector<int64_t> winoff((size_t)total_w);
    // passes of equal size, as run_begin; each of the two groups of windows has its own
    const int64_t total_w_plain = total_w - total_w_band;
    auto pass_size = [&](int64_t tw) { const int64_t n_pass = std::max<int64_t>(1, (tw + c->chunk - 1) / c->chunk); return (int)std::max<int64_t>(1, (tw + n_pass - 1) / n_pass); };
    const int ch_plain = pass_size(total_w_plain), ch_band = pass_size(total_w_band);
    const int64_t n_pass_band = total_w_band > 0 ? (total_w_band + ch_band - 1) / ch_band : 0;
    std::vector<StreamMap> map_idle;                        // band lanes without a window in this step: their sums move on all the same
    std::vector<std::vector<StreamMap>> map_pass((size_t)n_pass_band);
    int64_t max_map_n = 1;
    int64_t max_copy = 0, max_dec = 0, max_decc = 0, max_res = 0, max_bins = 0, max_uni = 0;
    double decc_bytes = 0, uni_bytes = 0;
    if ((rc = ensure(c, &S.arena[nxt], &S.arena_cap[nxt], (size_t)std::max<int64_t>(arena_need, 64)))) return rc;
    float* A = S.arena[nxt];
    const size_t desc_off = (size_t)al(up_bytes, 64);
    // descriptors behind the data (they hold device addresses of the upload's copy, so its buffer is sized first): at most 5 copies
    // before the passes, one after, one resample, one averaging per lane, one decode (and one merge) per stream, the window offsets,
    // 64-byte alignment of each
    const size_t n_desc_bytes = (size_t)n_lanes * (6 * sizeof(StreamCopy) + sizeof(StreamResample) + sizeof(StreamAvg)) + act.size() * sizeof(StreamDecode) +
                                (size_t)n_each * (sizeof(StreamDecodeChannels) + sizeof(StreamUnion)) + (size_t)total_w * 8 + 8 * 64 +
                                (size_t)(4 * n_band_lanes + n_pass_band + 2) * sizeof(StreamMap) + (size_t)(n_pass_band + 2) * 64;
    const size_t up_total = desc_off + n_desc_bytes;
    if ((rc = ensure(c, &S.d_up, &S.up_cap, up_total))) return rc;
    if ((rc = ensure_pinned(c, &S.h_up, &S.h_up_cap, up_total))) return rc;
    if ((rc = ensure(c, &S.d_newlg, &S.newlg_cap, (size_t)std::max<int64_t>(total_w, 1) * 256))) return rc;
    if ((rc = ensure(c, &S.d_avg, &S.avg_cap, (size_t)std::max<int64_t>(total_b, 1)))) return rc;
    if ((rc = ensure(c, &S.d_flags, &S.flags_cap, (size_t)std::max<int64_t>(total_b, 1)))) return rc;
    if (n_band_lanes) {
        if ((rc = ensure(c, &S.d_fmap, &S.fmap_cap, (size_t)std::max<int64_t>(fmap_need, 256)))) return rc;
        if ((rc = ensure(c, &S.d_spec, &S.spec_cap, (size_t)ch_band * 2 * 32768))) return rc;
    }
    int64_t w_plain_at = 0, w_band_at = total_w_plain, b_at = 0;
    for (auto& [sp, p] : act) {
        const StreamRec& s = *sp;
        int64_t& w_at = s.bands_on ? w_band_at : w_plain_at;
        unsigned char* hu = S.h_up;
        if (!s.staged.empty()) memcpy(hu + p.up_off, s.staged.data(), s.staged.size());
        if (s.on_host && s.out_on && !s.h_raw.empty()) memcpy(hu + p.raw_up_off, s.h_raw.data(), s.h_raw.size());
        const float* hm = nullptr; const float* hs = nullptr; const float* hl = nullptr;
        if (s.on_host) {
            float* h = (float*)(hu + p.host_off);
            memcpy(h, s.h_mono.data(), s.h_mono.size() * 4);
            memcpy(h + s.h_mono.size(), s.h_sig.data(), s.h_sig.size() * 4);
            memcpy(h + s.h_mono.size() + s.h_sig.size(), s.h_lg.data(), s.h_lg.size() * 4);
            const float* dh = (const float*)(S.d_up + p.host_off);
            hm = dh; hs = dh + s.h_mono.size(); hl = hs + s.h_sig.size();
        } else {
            hm = cur_arena + s.mono_off; hs = cur_arena + s.sig_off; hl = cur_arena + s.lg_off;
        }
        const bool direct = s.sr == SS_SAMPLE_RATE;
        if (s.bands_on) {
            if (s.on_host) { p.acc_old = (const double*)(S.d_up + p.band_up_off); p.acc_old_ls = 256 * kBandAcc; if (!s.h_band.empty()) memcpy(hu + p.band_up_off, s.h_band.data(), s.h_band.size() * 8); }
            else if (s.bs_ls) { p.acc_old = (const double*)(cur_arena + s.bs_off); p.acc_old_ls = s.bs_ls / 2; }
        }
        // lane l's carried segments, and its segments in the next half
        const int64_t src_mono_ls = s.on_host ? s.mono_n : s.mono_ls, src_sig_ls = s.on_host ? s.sig_n : s.sig_ls,
                      src_lg_ls = s.on_host ? s.lg_n * 256 : s.lg_ls;
        const int64_t n_new_out = p.m_end - s.m_next, nw = p.i_end - s.win_run, nb = p.b_end - s.bins_done;
        for (int l = 0; l < s.lanes; ++l) {
            const float* hm_l = hm + l * src_mono_ls; const float* hs_l = hs + l * src_sig_ls; const float* hl_l = hl + l * src_lg_ls;
            float* Am = A + p.mono_off + l * p.mono_ls; float* As = A + p.sig_off + l * p.sig_ls; float* Al = A + p.lg_off + l * p.lg_ls;
            // carried mono history [kb, frames_in), then the new frames
            if (!direct && p.mono_keep > 0) {
                pre.push_back(StreamCopy{hm_l + (p.kb - s.mono_base), Am, p.mono_keep});
                max_copy = std::max(max_copy, p.mono_keep);
            }
            // signal: carried [base_new, sig_end), the leading zeros of a new stream, outputs, the trailing zeros at close
            if (p.sig_keep > 0) { pre.push_back(StreamCopy{hs_l + (p.base_new - s.sig_base), As, p.sig_keep}); max_copy = std::max(max_copy, p.sig_keep); }
            if (p.pre > 0) { pre.push_back(StreamCopy{nullptr, As + p.sig_keep, p.pre}); max_copy = std::max(max_copy, p.pre); }
            float* out0 = As + p.sig_keep + p.pre;              // = padded index kPad + m_next
            pre.push_back(StreamCopy{nullptr, out0 + n_new_out, p.post + 64});      // (+ 64: the slack behind the signal is zero, as in the file arena)
            max_copy = std::max(max_copy, p.post + 64);
            // logits carried [lw0, win_run)
            if (s.lg_n > 0) { pre.push_back(StreamCopy{hl_l, Al, s.lg_n * 256}); max_copy = std::max(max_copy, s.lg_n * 256); }
            if (s.staged_frames > 0 && l == 0) {
                float* dst = direct ? out0 : Am + p.mono_keep;
                if (s.lanes == 1) {
                    dec.push_back(StreamDecode{(int64_t)p.up_off, s.staged_frames, dst, s.format, s.ch});
                    max_dec = std::max(max_dec, s.staged_frames);
                } else {                                         // every lane's plane from the one reading of the frames
                    decc.push_back(StreamDecodeChannels{(int64_t)p.up_off, s.staged_frames, dst, direct ? p.sig_ls : p.mono_ls, s.format, s.ch});
                    max_decc = std::max(max_decc, s.staged_frames);
                    decc_bytes += (double)s.staged.size() + 4.0 * (double)(s.staged_frames * s.lanes);
                }
            }
            if (!direct && n_new_out > 0) {
                res.push_back(StreamResample{Am, p.kb, p.F, s.d_taps, out0, s.m_next, n_new_out, s.L, s.M, s.half, 0});
                max_res = std::max(max_res, n_new_out);
            }
            // windows [win_run, i_end): arena offsets, their logits behind the carried ones
            for (int64_t i = s.win_run; i < p.i_end; ++i) winoff[(size_t)(w_at + i - s.win_run)] = p.sig_off + l * p.sig_ls + (i * s.per_step - p.base_new);
            if (s.bands_on) {
                // the lane's sums: from the carried ones, one entry per pass that holds windows of the lane, the final bins' maps
                double* lane = (double*)(A + p.bs_off + l * p.bs_ls);
                StreamMap m{};
                if (s.on_host) {
                    if (s.bs_n) { m.old_sum = (const double*)(S.d_up + p.band_up_off) + (size_t)s.lanes * 256 * kBandAcc + (size_t)l * 256 * s.bs_n; m.old_stride = s.bs_n; }
                } else if (s.bs_n) { m.old_sum = (const double*)(cur_arena + s.bs_off + l * s.bs_ls + s.bs_sum_off); m.old_stride = s.bs_stride; }
                m.old_b0 = s.bins_done; m.old_n = s.bs_n;
                m.sum = lane + 256 * kBandAcc; m.stride = p.bs_stride; m.b0 = s.bins_done; m.n = p.bs_n;
                m.fmap = S.d_fmap + p.fmap_at + l * nb * 256; m.fin_n = nb; m.i_end = p.i_end;
                m.i0 = m.i1 = s.win_run;
                max_map_n = std::max(max_map_n, p.bs_n);
                const int64_t g0 = w_at - total_w_plain;                 // the lane's first window among the band windows
                if (nw == 0) { m.flags = kMapInit | kMapFin; map_idle.push_back(m); }
                for (int64_t q = g0 / ch_band; nw > 0 && q * ch_band < g0 + nw; ++q) {
                    StreamMap a = m;
                    a.i0 = s.win_run + std::max<int64_t>(0, q * ch_band - g0);
                    a.i1 = s.win_run + std::min<int64_t>(nw, (q + 1) * ch_band - g0);
                    a.slot0 = g0 + (a.i0 - s.win_run) - q * ch_band;
                    a.flags = (a.i0 == s.win_run ? kMapInit : 0) | (a.i1 == p.i_end ? kMapFin : 0);
                    map_pass[(size_t)q].push_back(a);
                }
            }
            if (nw > 0) post.push_back(StreamCopy{S.d_newlg + (size_t)w_at * 256, Al + (s.win_run - p.lw0) * 256, nw * 256});
            w_at += nw;
            if (nb > 0) {
                avg.push_back(StreamAvg{Al, p.lw0, p.W_avg, 0, s.bins_done, nb, b_at, s.thr, s.step, step_bins(s.step)});
                max_bins = std::max(max_bins, nb);
                avg_reads += (double)nb * 256.0 / step_bins(s.step);
            }
            b_at += nb;
        }
        if (s.lanes > 1) {                                       // the merged bins behind the lanes'
            if (nb > 0) {
                uni.push_back(StreamUnion{b_at - s.lanes * nb, nb, b_at, s.lanes, 0});
                max_uni = std::max(max_uni, nb);
                uni_bytes += 9.0 * (double)(nb * (s.lanes + 1));
            }
            b_at += nb;
        }
    }
    // pack the descriptors behind the data
    size_t at = desc_off;
    auto put = [&](const void* src, size_t bytes) -> size_t { const size_t o = at; if (bytes) memcpy(S.h_up + at, src, bytes); at = (size_t)al((int64_t)(at + bytes), 64); return o; };
    const size_t o_pre = put(pre.data(), pre.size() * sizeof(StreamCopy));
    const size_t o_post = put(post.data(), post.size() * sizeof(StreamCopy));
    const size_t o_dec = put(dec.data(), dec.size() * sizeof(StreamDecode));
    const size_t o_res = put(res.data(), res.size() * sizeof(StreamResample));
    const size_t o_avg = put(avg.data(), avg.size() * sizeof(StreamAvg));
    const size_t o_win = put(winoff.data(), winoff.size() * 8);
    const size_t o_decc = put(decc.data(), decc.size() * sizeof(StreamDecodeChannels));     // (nothing, and no bytes, without an each-channel stream)
    const size_t o_uni = put(uni.data(), uni.size() * sizeof(StreamUnion));
    const size_t o_midle = put(map_idle.data(), map_idle.size() * sizeof(StreamMap));
    std::vector<size_t> o_mpass;
    for (const auto& v : map_pass) o_mpass.push_back(put(v.data(), v.size() * sizeof(StreamMap)));
    if (at > up_total) return fail(c, SS_ERR_STATE, "ss_stream_step: upload layout overflow");   // (cannot happen: sized above)
    // ---- device work ----
    HIPCHK(c, hipMemcpyAsync(S.d_up, S.h_up, at, hipMemcpyHostToDevice, c->stream));
    {
        ScopedLaunch sl(c, c->stream, "stream_copy", 0.0, 8.0 * max_copy * pre.size());
        HIPCHK(c, launch_stream_copy((const StreamCopy*)(S.d_up + o_pre), (int)pre.size(), max_copy, c->stream));
    }
    {
        ScopedLaunch sl(c, c->stream, "stream_decode", 0.0, 0.0);
        HIPCHK(c, launch_stream_decode(S.d_up, (const StreamDecode*)(S.d_up + o_dec), (int)dec.size(), max_dec, c->stream));
    }
    if (!decc.empty()) {
        ScopedLaunch sl(c, c->stream, "stream_decode_channels", 0.0, decc_bytes);
        HIPCHK(c, launch_stream_decode_channels(S.d_up, (const StreamDecodeChannels*)(S.d_up + o_decc), (int)decc.size(), max_decc, c->stream));
    }
    {
        ScopedLaunch sl(c, c->stream, "stream_resample", 0.0, 0.0);
        HIPCHK(c, launch_stream_resample((const StreamResample*)(S.d_up + o_res), (int)res.size(), max_res, c->stream));
    }
    if ((rc = range_clear(c, c->stream))) return rc;
    auto launch_maps = [&](size_t off, size_t n, int64_t max_n, const float* spec, double bytes) -> int {
        if (!n) return SS_OK;
        ScopedLaunch sl(c, c->stream, "stream_map_kernel", 0.0, bytes);
        hipLaunchKernelGGL(stream_map_kernel, dim3((unsigned)std::min<int64_t>((max_n + 255) / 256, 64), 256, (unsigned)std::min<size_t>(n, 4096)), dim3(256), 0,
                           c->stream, (const StreamMap*)(S.d_up + off), (int)n, spec);
        HIPCHK(c, hipGetLastError());
        return SS_OK;
    };
    if (total_w > 0) {
        if ((rc = ensure_workspace(c, std::max(total_w_plain > 0 ? ch_plain : 1, total_w_band > 0 ? ch_band : 1)))) return rc;
        const int64_t* d_win = (const int64_t*)(S.d_up + o_win);
        for (int64_t i0 = 0; i0 < total_w_plain; i0 += ch_plain) {
            const int m = (int)std::min<int64_t>(ch_plain, total_w_plain - i0);
            if ((rc = forward_chunk(c, c->ws[0], c->stream, A, d_win + i0, m, S.d_newlg + (size_t)i0 * 256, nullptr))) return rc;
        }
    }
    if (n_band_lanes) {
        // a lane's first entry starts its sums from the carried ones, every pass of its windows adds that pass's spec output, its last
        // entry turns the final bins into maps (lanes without a window: one entry of their own, before the passes)
        if ((rc = launch_maps(o_midle, map_idle.size(), max_map_n, nullptr, 16.0 * 256 * max_map_n * map_idle.size()))) return rc;
        const int64_t* d_win = (const int64_t*)(S.d_up + o_win);
        for (int64_t q = 0; q < n_pass_band; ++q) {
            const int64_t i0 = total_w_plain + q * ch_band;
            const int m = (int)std::min<int64_t>(ch_band, total_w - i0);
            if ((rc = forward_chunk(c, c->ws[0], c->stream, A, d_win + i0, m, S.d_newlg + (size_t)i0 * 256, S.d_spec))) return rc;
            if ((rc = launch_maps(o_mpass[(size_t)q], map_pass[(size_t)q].size(), max_map_n, S.d_spec, (double)m * 2 * 32768 * 4 + 16.0 * 256 * max_map_n * map_pass[(size_t)q].size()))) return rc;
        }
    }
    {
        int64_t mx = 0; for (const StreamCopy& p : post) mx = std::max(mx, p.n);
        ScopedLaunch sl(c, c->stream, "stream_copy", 0.0, 8.0 * mx * post.size());
        HIPCHK(c, launch_stream_copy((const StreamCopy*)(S.d_up + o_post), (int)post.size(), mx, c->stream));
    }
    {
        ScopedLaunch sl(c, c->stream, "stream_average", 0.0, avg_reads * 4 + (double)total_b * 9);
        HIPCHK(c, launch_stream_average((const StreamAvg*)(S.d_up + o_avg), (int)avg.size(), max_bins, S.d_avg, S.d_flags, c->stream));
    }
    if (!uni.empty()) {
        ScopedLaunch sl(c, c->stream, "stream_union", 0.0, uni_bytes);
        HIPCHK(c, launch_stream_union((const StreamUnion*)(S.d_up + o_uni), (int)uni.size(), max_uni, S.d_avg, S.d_flags, c->stream));
    }
    S.h_avg.resize((size_t)total_b); S.h_flags.resize((size_t)total_b);
    if (total_b) {
        HIPCHK(c, hipMemcpyAsync(S.h_avg.data(), S.d_avg, (size_t)total_b * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(S.h_flags.data(), S.d_flags, (size_t)total_b, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = range_fetch(c, c->stream))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    if (range_left(c))
        return fail(c, SS_ERR_RANGE, "f16x2: an activation left the f16 range (|x| > 65504) or was not finite; nothing of the step is committed: "
                                     "move the streams that had windows in it to an fp32 context (ss_stream_export / ss_stream_import)");
    // ---- commit ----
    for (auto& kv : S.s) {
        StreamRec& s = kv.second;
        s.r_out.clear(); s.a_out.clear(); s.b_out.clear(); s.la_out.clear(); s.p_out.clear(); s.o_first = s.frames_out; s.o_n = 0;
        s.bd_out.clear(); s.bp_out.clear();
    }
    b_at = 0;
    for (auto& [sp, p] : act) {
        StreamRec& s = *sp;
        const int64_t nb = p.b_end - s.bins_done;
        // a plain stream's bins; an each-channel stream's lanes, then its merged bins: the series it returns and walks
        const int64_t m_at = b_at + (s.lanes > 1 ? s.lanes * nb : 0);
        s.b_ev.clear(); s.b_b0 = s.bins_done;
        const double* lane_avg = s.lanes > 1 ? S.h_avg.data() + b_at : nullptr;
        for (int64_t k = 0; k < nb; ++k) {
            const int64_t j = s.bins_done + k;
            const unsigned char f = S.h_flags[(size_t)(m_at + k)];
            if (f & 1) { s.a_out.push_back(S.h_avg[(size_t)(m_at + k)]); s.b_out.push_back(j); }
            walk_bin(s, j, f, lane_avg ? lane_avg + k : nullptr, nb);
        }
        if (s.lanes > 1)
            for (int l = 0; l < s.lanes; ++l)
                for (int64_t k = 0; k < nb; ++k)
                    if (S.h_flags[(size_t)(m_at + k)] & 1) s.la_out.push_back(S.h_avg[(size_t)(b_at + l * nb + k)]);
        b_at = m_at + nb;
        s.mono_ls = p.mono_ls; s.sig_ls = p.sig_ls; s.lg_ls = p.lg_ls;
        const bool direct = s.sr == SS_SAMPLE_RATE;
        const int64_t sig_end = p.base_new + p.sig_len();
        s.frames_in = p.F; s.m_next = p.m_end; s.win_run = p.i_end; s.bins_done = p.b_end;
        s.staged.clear(); s.staged.shrink_to_fit(); s.staged_frames = 0;
        s.on_host = false; s.h_mono.clear(); s.h_sig.clear(); s.h_lg.clear(); s.h_raw.clear(); s.h_raw.shrink_to_fit();
        if (s.bands_on) {
            if (!p.closing && s.run_open) band_snap(s);
            // the sums of the bins still not final, inside the segment this step wrote
            s.bs_off = p.bs_off; s.bs_ls = p.bs_ls; s.bs_stride = p.bs_stride; s.bs_n = p.bs_n - nb;
            s.bs_sum_off = 2 * (256 * kBandAcc + nb);
            // a finished stream is planned no more, so nothing of it moves to the other half when the arena flips: it keeps no band
            // state on the device (its last regions have been evaluated; an image of it holds zeros, as of a stream without a step yet)
            if (p.closing) { s.bs_off = s.bs_ls = s.bs_stride = s.bs_sum_off = s.bs_n = 0; s.b_parked = false; }
            s.h_band.clear(); s.h_band.shrink_to_fit();
        }
        if (p.closing) {
            finish_regions(s);
            s.finished = true;
            s.mono_n = s.sig_n = s.lg_n = 0; s.mono_base = s.frames_in; s.sig_base = sig_end; s.lg_w0 = s.win_run;
            continue;
        }
        // what the next step needs, inside the segments this step wrote
        if (!direct) {
            const int64_t k0 = std::min(std::max(p.kb, (p.m_end * s.M) / s.L - s.half + 1), p.F);
            s.mono_base = k0; s.mono_n = p.F - k0; s.mono_off = p.mono_off + (k0 - p.kb);
        }
        s.sig_base = p.i_end * s.per_step; s.sig_n = sig_end - s.sig_base; s.sig_off = p.sig_off + (s.sig_base - p.base_new);
        const int64_t w0 = std::min(std::max(first_window_for_bin(s, p.b_end), p.lw0), p.i_end);
        s.lg_w0 = w0; s.lg_n = p.i_end - w0; s.lg_off = p.lg_off + (w0 - p.lw0) * 256;
    }
    S.cur = nxt;                                            // (the records describe the half just built from here on, as for step_output)
    if (n_band_lanes && (rc = step_bands(c, S, act, A))) return rc;
    return step_output(c, S, act);
}

// ------------------------------------------------------------------------------------------------------
// export / import: a stream's whole state as a byte image
// ------------------------------------------------------------------------------------------------------
namespace {
struct ImageHdr {
    char magic[8];
    int32_t format, sr, ch, closed, finished, have, run_open, pad;
    double thr, brk, cur_start, cur_end;
    int64_t frames_in, staged_frames, staged_bytes, mono_base, mono_n, sig_base, sig_n, lg_w0, lg_n, m_next, win_run, bins_done, run_first, run_last;
};
// "SSSTRM01": a stream with the default window step -- the header, then the data.  "SSSTRM02": any other step -- the header, the step
// (a double), then the data.
constexpr char kMagic[8] = {'S', 'S', 'S', 'T', 'R', 'M', '0', '1'};
constexpr char kMagicStep[8] = {'S', 'S', 'S', 'T', 'R', 'M', '0', '2'};
// "SSSTRM03": a stream with output -- the header, the step, ImageOut, n_er int64s (the decided ranges still ahead), the staged bytes,
// the floats, then the held raw PCM (raw_bytes: frames [frames_out, frames_in) in the stream's encoding)
constexpr char kMagicOut[8] = {'S', 'S', 'S', 'T', 'R', 'M', '0', '3'};
struct ImageOut { double pad_s, min_len_s; int64_t frames_out, erased, raw_bytes, n_er; };
// "SSSTRM04": an each-channel stream of several channels -- the header, the step, ImageLanes, the peak state (3 x lanes doubles: open
// run, pending region, gap), then with_out ? the output block of "SSSTRM03" (ImageOut, the ranges) : nothing, the staged bytes, the
// floats (every lane's mono history, then every lane's signal, then every lane's logits), then the held raw PCM of a stream with output
constexpr char kMagicLanes[8] = {'S', 'S', 'S', 'T', 'R', 'M', '0', '4'};
struct ImageLanes { int32_t lanes, with_out; };
// "SSSTRM05": a stream with bands (of any other kind: mix or each-channel, with or without output) -- the header, the step (the default
// one: bands know no other), ImageBands, lanes > 1 ? the peak state of "SSSTRM04" : nothing, with_out ? the output block of "SSSTRM03" :
// nothing, the staged bytes, the floats as in "SSSTRM04", the band state as doubles (every lane's accumulator vectors [kBandAcc][256],
// then every lane's map sums [256][bs_n] of the bins [bins_done, bins_done + bs_n)), then the held raw PCM of a stream with output
constexpr char kMagicBands[8] = {'S', 'S', 'S', 'T', 'R', 'M', '0', '5'};
struct ImageBands { int32_t lanes, with_out, want_prof, parked, speech_channel, reserved; double q_low, q_high; int64_t bs_n; };
// "SSSTRM06": a stream with output in its own encoding (ss_stream_open_source) -- these eight bytes, then the image the stream would
// write without that property ("SSSTRM03" or "SSSTRM04"), whole
constexpr char kMagicSource[8] = {'S', 'S', 'S', 'T', 'R', 'M', '0', '6'};
constexpr int64_t kMaxCarriedBins = 4096;             // (a stream carries the sums of about 300 bins)
}  // namespace

static int export_image(ss_ctx* c, StreamRec* s, void* buf, int64_t cap, int64_t* n_out);
static int import_image(ss_ctx* c, const void* buf, int64_t n, int* id);

extern "C" int ss_stream_export(ss_ctx* c, int id, void* buf, int64_t cap, int64_t* n_out) {
    StreamRec* s = find_stream(c, id);
    if (!s || !n_out) return fail(c, SS_ERR_ARG, "ss_stream_export: bad argument");
    if (!s->src_out) return export_image(c, s, buf, cap, n_out);
    int rc = export_image(c, s, buf ? (unsigned char*)buf + 8 : nullptr, buf ? std::max<int64_t>(cap - 8, 0) : 0, n_out);
    *n_out += 8;
    if (rc == SS_OK && buf) memcpy(buf, kMagicSource, 8);
    return rc;
}

extern "C" int ss_stream_import(ss_ctx* c, const void* buf, int64_t n, int* id) {
    if (!c || !buf || !id || n < (int64_t)sizeof(ImageHdr)) return fail(c, SS_ERR_ARG, "ss_stream_import: bad argument");
    if (memcmp(buf, kMagicSource, 8) != 0) return import_image(c, buf, n, id);
    const unsigned char* inner = (const unsigned char*)buf + 8;
    if (n < 8 + (int64_t)sizeof(ImageHdr) || (memcmp(inner, kMagicOut, 8) != 0 && memcmp(inner, kMagicLanes, 8) != 0))
        return fail(c, SS_ERR_FORMAT, "ss_stream_import: not a stream image");
    int rc = import_image(c, inner, n - 8, id);
    if (rc) return rc;
    StreamRec* s = find_stream(c, *id);
    if (!s->out_on) { ss_stream_free(c, *id); return fail(c, SS_ERR_FORMAT, "ss_stream_import: a source-output image of a stream without output"); }
    s->src_out = true;
    return SS_OK;
}

static int export_image(ss_ctx* c, StreamRec* s, void* buf, int64_t cap, int64_t* n_out) {
    const bool each = s->lanes > 1, bands = s->bands_on;
    const bool with_step = bands || each || s->out_on || s->step != SS_STEP_DEFAULT;
    const int64_t band_doubles = bands ? (int64_t)s->lanes * 256 * (kBandAcc + s->bs_n) : 0;
    const int64_t raw_bytes = s->out_on ? (s->frames_in - s->frames_out) * s->frame_bytes() : 0;
    const int64_t nl = s->lanes;
    const int64_t need = (int64_t)sizeof(ImageHdr) + (with_step ? 8 : 0) + (bands ? (int64_t)sizeof(ImageBands) : each ? (int64_t)sizeof(ImageLanes) : 0) +
                         (each ? 24 * nl : 0) + (int64_t)s->staged.size() + 4 * nl * (s->mono_n + s->sig_n + s->lg_n * 256) + 8 * band_doubles +
                         (s->out_on ? (int64_t)sizeof(ImageOut) + 8 * (int64_t)s->er_rng.size() + raw_bytes : 0);
    *n_out = need;
    if (!buf) return SS_OK;
    if (cap < need) return fail(c, SS_ERR_CAPACITY, "ss_stream_export: capacity < " + std::to_string(need));
    ImageHdr h{};
    memcpy(h.magic, bands ? kMagicBands : each ? kMagicLanes : s->out_on ? kMagicOut : with_step ? kMagicStep : kMagic, 8);
    h.format = s->format; h.sr = s->sr; h.ch = s->ch; h.closed = s->closed; h.finished = s->finished; h.have = s->mg.have; h.run_open = s->run_open;
    h.thr = s->thr; h.brk = s->mg.brk; h.cur_start = s->mg.cur.start; h.cur_end = s->mg.cur.end;
    h.frames_in = s->frames_in; h.staged_frames = s->staged_frames; h.staged_bytes = (int64_t)s->staged.size();
    h.mono_base = s->mono_base; h.mono_n = s->mono_n; h.sig_base = s->sig_base; h.sig_n = s->sig_n; h.lg_w0 = s->lg_w0; h.lg_n = s->lg_n;
    h.m_next = s->m_next; h.win_run = s->win_run; h.bins_done = s->bins_done; h.run_first = s->run_first; h.run_last = s->run_last;
    unsigned char* o = (unsigned char*)buf;
    memcpy(o, &h, sizeof h); o += sizeof h;
    if (with_step) { memcpy(o, &s->step, 8); o += 8; }
    if (bands) {
        const ImageBands ib{s->lanes, s->out_on ? 1 : 0, s->want_prof ? 1 : 0, s->b_parked ? 1 : 0, s->bprm.speech_channel, 0, s->bprm.q_low, s->bprm.q_high, s->bs_n};
        memcpy(o, &ib, sizeof ib); o += sizeof ib;
    } else if (each) {
        const ImageLanes il{s->lanes, s->out_on ? 1 : 0};
        memcpy(o, &il, sizeof il); o += sizeof il;
    }
    if (each) {
        for (const std::vector<double>* v : {&s->pk_run, &s->pk_cur, &s->pk_gap}) { memcpy(o, v->data(), 8 * nl); o += 8 * nl; }
    }
    if (s->out_on) {
        const ImageOut io{s->er.pad_s, s->er.min_len_s, s->frames_out, s->erased, raw_bytes, (int64_t)s->er_rng.size()};
        memcpy(o, &io, sizeof io); o += sizeof io;
        if (!s->er_rng.empty()) memcpy(o, s->er_rng.data(), s->er_rng.size() * 8);
        o += s->er_rng.size() * 8;
    }
    if (!s->staged.empty()) memcpy(o, s->staged.data(), s->staged.size());
    o += s->staged.size();
    float* f = (float*)o;                                 // (unaligned host memory is fine for memcpy / hipMemcpy)
    unsigned char* bnd = o + 4 * nl * (s->mono_n + s->sig_n + s->lg_n * 256);        // (doubles at any alignment: written by memcpy only)
    unsigned char* raw = bnd + 8 * band_doubles;
    float* f_sig = f + nl * s->mono_n; float* f_lg = f_sig + nl * s->sig_n;       // the lanes back to back, as the host vectors hold them
    if (s->on_host) {
        memcpy(f, s->h_mono.data(), nl * s->mono_n * 4); memcpy(f_sig, s->h_sig.data(), nl * s->sig_n * 4);
        memcpy(f_lg, s->h_lg.data(), nl * s->lg_n * 1024);
        if (raw_bytes) memcpy(raw, s->h_raw.data(), (size_t)raw_bytes);
        if (band_doubles) memcpy(bnd, s->h_band.data(), (size_t)band_doubles * 8);
        return SS_OK;
    }
    hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const float* a = c->streams->arena[c->streams->cur];
    for (int64_t l = 0; l < nl; ++l) {
        if (s->mono_n) HIPCHK(c, hipMemcpy(f + l * s->mono_n, a + s->mono_off + l * s->mono_ls, s->mono_n * 4, hipMemcpyDeviceToHost));
        if (s->sig_n) HIPCHK(c, hipMemcpy(f_sig + l * s->sig_n, a + s->sig_off + l * s->sig_ls, s->sig_n * 4, hipMemcpyDeviceToHost));
        if (s->lg_n) HIPCHK(c, hipMemcpy(f_lg + l * s->lg_n * 256, a + s->lg_off + l * s->lg_ls, s->lg_n * 1024, hipMemcpyDeviceToHost));
    }
    if (raw_bytes) HIPCHK(c, hipMemcpy(raw, c->streams->barena[c->streams->bcur] + s->raw_off, (size_t)raw_bytes, hipMemcpyDeviceToHost));
    if (bands && !s->bs_ls) memset(bnd, 0, (size_t)band_doubles * 8);                  // no step yet: nothing carried, the accumulators zero
    else if (bands) {
        unsigned char* sums = bnd + (size_t)nl * 256 * kBandAcc * 8;
        for (int64_t l = 0; l < nl; ++l) {
            const float* lane = a + s->bs_off + l * s->bs_ls;
            HIPCHK(c, hipMemcpy(bnd + (size_t)l * 256 * kBandAcc * 8, lane, 256 * kBandAcc * 8, hipMemcpyDeviceToHost));
            if (s->bs_n)
                HIPCHK(c, hipMemcpy2D(sums + (size_t)l * 256 * s->bs_n * 8, (size_t)s->bs_n * 8, lane + s->bs_sum_off, (size_t)s->bs_stride * 8, (size_t)s->bs_n * 8, 256,
                                      hipMemcpyDeviceToHost));
        }
    }
    return SS_OK;
}

static int import_image(ss_ctx* c, const void* buf, int64_t n, int* id) {
    if (!c || !buf || !id || n < (int64_t)sizeof(ImageHdr)) return fail(c, SS_ERR_ARG, "ss_stream_import: bad argument");
    if (!c->has_model) return fail(c, SS_ERR_STATE, "context was created without weights (audio-only)");
    ImageHdr h;
    memcpy(&h, buf, sizeof h);
    static const unsigned char one[8] = {0};
    // an "SSSTRM04" image that does not hold together is an argument error (SS_ERR_ARG); the older images keep SS_ERR_FORMAT
    const bool bands = memcmp(h.magic, kMagicBands, 8) == 0;
    const bool each = bands || memcmp(h.magic, kMagicLanes, 8) == 0;    // (the lanes' block: ImageLanes, or ImageBands which begins like it)
    const int bad = each ? SS_ERR_ARG : SS_ERR_FORMAT;
    bool with_out = memcmp(h.magic, kMagicOut, 8) == 0;
    const bool with_step = each || with_out || memcmp(h.magic, kMagicStep, 8) == 0;
    int64_t hdr_bytes = (int64_t)sizeof h;
    double step = SS_STEP_DEFAULT;
    if (with_step && n >= hdr_bytes + 8) { memcpy(&step, (const unsigned char*)buf + hdr_bytes, 8); hdr_bytes += 8; }
    ImageLanes il{1, 0};
    ImageBands ib{1, 0, 0, 0, 1, 0, 0.05, 0.95, 0};
    int64_t pk_at = 0;                                    // the peak state's place in the image
    if (each) {
        const int64_t blk = bands ? (int64_t)sizeof ib : (int64_t)sizeof il;
        bool ok = hdr_bytes == (int64_t)sizeof h + 8 && n >= hdr_bytes + blk;
        if (ok) {
            memcpy(&il, (const unsigned char*)buf + hdr_bytes, sizeof il);
            const int64_t pk = !bands || il.lanes > 1 ? 24 * (int64_t)il.lanes : 0;       // (an "SSSTRM04" image always holds the peak block)
            ok = il.lanes >= 1 && (il.lanes == 1 || il.lanes == h.ch) && il.lanes <= 64 && (il.with_out == 0 || il.with_out == 1) && n >= hdr_bytes + blk + pk;
            if (ok && bands) {
                memcpy(&ib, (const unsigned char*)buf + hdr_bytes, sizeof ib);
                const ss_band_params bp{ib.q_low, ib.q_high, ib.speech_channel, 0};
                std::string err;
                ok = (ib.want_prof == 0 || ib.want_prof == 1) && (ib.parked == 0 || ib.parked == 1) && ib.reserved == 0 && ib.bs_n >= 0 && ib.bs_n <= kMaxCarriedBins &&
                     check_band_args(nullptr, 0, &bp, err) == SS_OK && step == SS_STEP_DEFAULT;
            }
            pk_at = hdr_bytes + blk;
            hdr_bytes = pk_at + pk;
        }
        if (!ok)
            return fail(c, SS_ERR_ARG, bands ? "ss_stream_import: a band image that does not hold together (lane count, parameters, a step other than the default, or cut short)"
                                             : "ss_stream_import: an each-channel image whose lane count is neither 1 nor its channel count, or cut short");
        with_out = il.with_out != 0;
    }
    const int64_t nl = il.lanes;
    const int64_t band_bytes = bands ? 8 * nl * 256 * (kBandAcc + ib.bs_n) : 0;
    ImageOut io{0, 0, 0, 0, 0, 0};
    int64_t out_bytes = 0;                                // what an image with output holds beyond the others: ImageOut, the ranges, the raw PCM
    if (with_out) {
        bool ok = n >= hdr_bytes + (int64_t)sizeof io;
        if (ok) {
            memcpy(&io, (const unsigned char*)buf + hdr_bytes, sizeof io);
            const ss_stream_erase e{io.pad_s, io.min_len_s};
            ok = erase_ok(&e) && io.n_er >= 0 && io.n_er <= ((int64_t)1 << 24) && io.n_er % 2 == 0 && io.frames_out >= 0 && io.frames_out <= h.frames_in &&
                 io.erased >= 0 && io.erased <= io.frames_out && h.ch > 0 && h.ch <= 64 && io.raw_bytes >= 0 && io.raw_bytes <= n;
        }
        if (!ok) return fail(c, bad, "ss_stream_import: not a stream image");
        hdr_bytes += (int64_t)sizeof io + 8 * io.n_er;
        out_bytes = io.raw_bytes;
    }
    if ((memcmp(h.magic, kMagic, 8) != 0 && !(with_step && hdr_bytes > (int64_t)sizeof h && step_ok(step))) || check_pcm_args(c, one, h.format, h.sr, h.ch, 0) != SS_OK || h.staged_bytes < 0 || h.mono_n < 0 ||
        h.sig_n < 0 || h.lg_n < 0 || h.lg_n > 64 || h.mono_n > ((int64_t)1 << 32) || h.sig_n > ((int64_t)1 << 32) ||
        n != hdr_bytes + h.staged_bytes + 4 * nl * (h.mono_n + h.sig_n + h.lg_n * 256) + band_bytes + out_bytes ||
        (with_out && io.raw_bytes != (h.frames_in - io.frames_out) * h.ch * (int64_t)pcm_bytes_per_sample(h.format)) ||
        h.staged_bytes != h.staged_frames * h.ch * (int64_t)pcm_bytes_per_sample(h.format))
        return fail(c, bad, "ss_stream_import: not a stream image");
    hipSetDevice(c->device);
    StreamRec s;
    s.format = h.format; s.sr = h.sr; s.ch = h.ch; s.closed = h.closed; s.finished = h.finished; s.mg.have = h.have; s.run_open = h.run_open;
    s.thr = h.thr; s.mg.brk = h.brk; s.mg.cur = ss_region{h.cur_start, h.cur_end};
    s.step = step; s.per_step = step_samples(step);
    s.frames_in = h.frames_in; s.staged_frames = h.staged_frames;
    s.mono_base = h.mono_base; s.mono_n = h.mono_n; s.sig_base = h.sig_base; s.sig_n = h.sig_n; s.lg_w0 = h.lg_w0; s.lg_n = h.lg_n;
    s.m_next = h.m_next; s.win_run = h.win_run; s.bins_done = h.bins_done; s.run_first = h.run_first; s.run_last = h.run_last;
    int rc = init_rates(c, s);
    if (rc) return rc;
    const unsigned char* p = (const unsigned char*)buf + hdr_bytes;
    s.staged.assign(p, p + h.staged_bytes); p += h.staged_bytes;
    s.set_lanes((int)nl);
    if (nl > 1)
        for (std::vector<double>* v : {&s.pk_run, &s.pk_cur, &s.pk_gap}) { memcpy(v->data(), (const unsigned char*)buf + pk_at, 8 * nl); pk_at += 8 * nl; }
    s.h_mono.resize(nl * h.mono_n); s.h_sig.resize(nl * h.sig_n); s.h_lg.resize(nl * h.lg_n * 256);
    memcpy(s.h_mono.data(), p, nl * h.mono_n * 4); p += nl * h.mono_n * 4;
    memcpy(s.h_sig.data(), p, nl * h.sig_n * 4); p += nl * h.sig_n * 4;
    memcpy(s.h_lg.data(), p, nl * h.lg_n * 1024); p += nl * h.lg_n * 1024;
    if (bands) {
        s.bands_on = true; s.want_prof = ib.want_prof != 0; s.b_parked = ib.parked != 0; s.bprm = ss_band_params{ib.q_low, ib.q_high, ib.speech_channel, 0};
        s.bs_n = ib.bs_n;
        s.h_band.resize((size_t)(band_bytes / 8));
        memcpy(s.h_band.data(), p, (size_t)band_bytes); p += band_bytes;
    }
    if (with_out) {
        s.out_on = true; s.er = ss_stream_erase{io.pad_s, io.min_len_s}; s.frames_out = io.frames_out; s.erased = io.erased;
        const unsigned char* q = (const unsigned char*)buf + hdr_bytes - 8 * io.n_er;
        s.er_rng.resize((size_t)io.n_er);
        if (io.n_er) memcpy(s.er_rng.data(), q, (size_t)io.n_er * 8);
        s.h_raw.assign(p, p + io.raw_bytes);
        s.o_first = s.frames_out;
    }
    s.on_host = true;
    StreamSet& S = streams_of(c);
    *id = S.next_id++;
    S.s.emplace(*id, std::move(s));
    return SS_OK;
}
