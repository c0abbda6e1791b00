// The host-only stages of a stream step (stream.hip): what a step does with every stream, where everything lies, every descriptor
// of every launch -- and, behind the device work, what the records carry into the next step.  No HIP call and no HIP header:
// tests/stream_extents.cpp drives these stages over seeded stream populations without a device and checks every range a descriptor
// addresses against the buffer it names.
//   layout:  plan_step (plans, buffer sizes) -> the caller grows the buffers -> build_step (descriptors on the buffers' bases)
//   commit:  commit_step (region walk, band events, the carried extents)
//   then, planned from the committed records: layout_bands / commit_bands and layout_output / commit_output
// The layout stages read the records and change none; the commits make no address.
#pragma once
#include "hostdefs.h"
#include "stream_desc.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

namespace ss {

constexpr int64_t kPad = SS_WINDOW_SAMPLES;          // 3 s of zeros in front of and behind the recording (worker.py:58-62)

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

// The buffers of a step, by name.  Every address in a descriptor is base[buffer] + an offset, and need[buffer] is what the layout
// demands of that buffer, in bytes.  kCur / kRawCur -- the arena halves the streams live in -- are only read; what lies there is what
// the last commit recorded.  kNext is the half the step builds (the band walk behind the commit still calls it that).
enum StepBuf { kCur, kNext, kUp, kNewlg, kAvg, kFlags, kFmap, kSpec, kUp3, kBout, kBprof, kRawCur, kRawNext, kUp2, kOut, kOutb, kStepBufs };
struct StepBuffers {
    unsigned char* base[kStepBufs] = {};
    size_t need[kStepBufs] = {};
    template <typename T> T* at(StepBuf b, int64_t off) const { return reinterpret_cast<T*>(base[b]) + off; }
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
    // lane 0's carried accumulators: acc_off doubles into acc_buf (kUp: an image's; kCur), acc_ls doubles to the next lane's (acc_have
    // false: a stream without a step yet)
    bool acc_have = false; StepBuf acc_buf = kCur; int64_t acc_off = 0, acc_ls = 0;
    int64_t w_at = 0, b_at = 0;                       // the stream's first window among the step's, its first bin in the avg / flags download
    int64_t mono_len() const { return F - kb; }
    int64_t sig_len() const { return sig_keep + pre + (m_end - m_next_) + post; }
    int64_t m_next_ = 0;
};

inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

inline int64_t n22_of(const StreamRec& s, int64_t F) { return ss_resampled_length(F, s.sr); }

// first bin of the stream's window i (NNDetector.py:175): the whole-file run's start table
inline int64_t win_start_bin(const StreamRec& s, int64_t i) { return ss_window_start_bin(i, s.step); }

// run_begin's plan of a file of F frames: window count (clamped to the padded signal) and bin count
inline void file_plan(const StreamRec& s, int64_t F, int64_t& W, int64_t& n_bins) {
    const int64_t n_padded = n22_of(s, F) + 2 * kPad;
    W = ss_plan_windows_step((double)F / (double)s.sr, s.step, nullptr, 0);
    while (W > 0 && (W - 1) * s.per_step + SS_WINDOW_SAMPLES > n_padded) --W;
    n_bins = (int64_t)std::nearbyint((double)n_padded / 22050.0 * 256.0 / 3.0);
}

inline StreamPlan plan_stream(const StreamRec& s) {
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
inline int64_t first_window_for_bin(const StreamRec& s, int64_t b) {
    int64_t i = std::max<int64_t>(0, (int64_t)std::floor((double)(b - 256) / step_bins(s.step)) - 1);
    while (win_start_bin(s, i) + 256 <= b) ++i;
    return i;
}

// ------------------------------------------------------------------------------------------------------
// layout of the step: plans and buffer sizes, then the descriptors
// ------------------------------------------------------------------------------------------------------
struct HostPiece { int64_t off; const void* src; size_t bytes; };       // host bytes the run stage copies to the upload's `off`

struct StepBuild {
    std::vector<StreamPlan> plans;                    // one per stream of the step, in the order given
    int64_t total_w = 0, total_w_plain = 0, total_w_band = 0, total_b = 0, n_lanes = 0, n_each = 0, n_band_lanes = 0, n_pass_band = 0;
    int ch_plain = 1, ch_band = 1;                    // windows per pass of the streams without / with bands
    int64_t desc_off = 0;                             // the descriptors lie behind the data of the upload
    std::vector<HostPiece> pieces;
    std::vector<StreamCopy> pre, post;
    std::vector<StreamDecode> dec;
    std::vector<StreamDecodeChannels> decc;           // each-channel streams only: a step without one launches neither kernel
    std::vector<StreamUnion> uni;
    std::vector<StreamResample> res;
    std::vector<StreamAvg> avg;
    std::vector<int64_t> winoff;
    std::vector<StreamMap> map_idle;                  // band lanes without a window in this step: their sums move on all the same
    std::vector<std::vector<StreamMap>> map_pass;
    // the launches' grid extents and byte figures
    int64_t max_copy = 0, max_dec = 0, max_decc = 0, max_res = 0, max_bins = 0, max_uni = 0, max_map_n = 1;
    double decc_bytes = 0, uni_bytes = 0, avg_reads = 0;      // avg_reads: logits the averaging reads, 256 / s_b windows per bin
};

// The most descriptors one lane or one stream adds to each vector: stated here, beside the builders below that push them.  plan_step
// sizes the upload's descriptor region from them, build_step checks its own counts against them before anything is packed.
constexpr int kLanePre = 5;                           // copies before the passes: mono history, signal, leading zeros, trailing zeros, logits
constexpr int kLanePost = 1, kLaneRes = 1, kLaneAvg = 1;
constexpr int kStreamDec = 1, kStreamDecc = 1, kStreamUni = 1;
// a band lane adds one idle entry, or one entry per pass its windows lie in: a pass boundary inside the lane adds one more, and all
// the lanes together cross each of the passes' boundaries once
inline int64_t map_entries_max(int64_t band_lanes, int64_t passes) { return band_lanes + passes; }

inline size_t desc_bytes_max(const StepBuild& b, size_t n_streams) {
    auto al = [](size_t x) { return (size_t)align_up((int64_t)x, 64); };
    return al((size_t)b.n_lanes * kLanePre * sizeof(StreamCopy)) + al((size_t)b.n_lanes * kLanePost * sizeof(StreamCopy)) +
           al(n_streams * kStreamDec * sizeof(StreamDecode)) + al((size_t)b.n_lanes * kLaneRes * sizeof(StreamResample)) +
           al((size_t)b.n_lanes * kLaneAvg * sizeof(StreamAvg)) + al((size_t)b.total_w * 8) + al((size_t)b.n_each * kStreamDecc * sizeof(StreamDecodeChannels)) +
           al((size_t)b.n_each * kStreamUni * sizeof(StreamUnion)) + (size_t)map_entries_max(b.n_band_lanes, b.n_pass_band) * sizeof(StreamMap) +
           (size_t)(b.n_pass_band + 1) * 64;
}

inline bool desc_counts_ok(const StepBuild& b, size_t n_streams) {
    size_t maps = b.map_idle.size();
    for (const auto& v : b.map_pass) maps += v.size();
    return b.pre.size() <= (size_t)b.n_lanes * kLanePre && b.post.size() <= (size_t)b.n_lanes * kLanePost && b.dec.size() <= n_streams * kStreamDec &&
           b.res.size() <= (size_t)b.n_lanes * kLaneRes && b.avg.size() <= (size_t)b.n_lanes * kLaneAvg && b.winoff.size() == (size_t)b.total_w &&
           b.decc.size() <= (size_t)b.n_each * kStreamDecc && b.uni.size() <= (size_t)b.n_each * kStreamUni &&
           maps <= (size_t)map_entries_max(b.n_band_lanes, b.n_pass_band);
}

// passes of equal size, as run_begin
inline int pass_size(int64_t tw, int chunk) {
    const int64_t n_pass = std::max<int64_t>(1, (tw + chunk - 1) / chunk);
    return (int)std::max<int64_t>(1, (tw + n_pass - 1) / n_pass);
}

// Plans every stream, lays out the next arena half and the data of the upload, and states what the step needs of every buffer.
// Windows of streams with bands run in passes of their own, behind the others': those passes store the spec head's output.
inline StepBuild plan_step(const std::vector<StreamRec*>& act, int chunk, StepBuffers& B) {
    StepBuild b;
    int64_t arena_need = 0, up_bytes = 0, fmap_need = 0;
    for (const StreamRec* sp : act) {
        const StreamRec& s = *sp;
        StreamPlan p = plan_stream(s);
        // (arena_need stays a multiple of 64; a plain stream has one lane)
        if (s.sr != SS_SAMPLE_RATE) { p.mono_off = arena_need; p.mono_ls = align_up(p.mono_len(), 64); arena_need += s.lanes * p.mono_ls; }
        p.sig_off = arena_need; p.sig_ls = align_up(p.sig_len() + 64, 64); arena_need += s.lanes * p.sig_ls;    // (+ 64: slack behind the last window, as the file arena)
        p.lg_off = arena_need; p.lg_ls = align_up((p.i_end - p.lw0) * 256, 64); arena_need += s.lanes * p.lg_ls;
        p.up_off = up_bytes; up_bytes = align_up(up_bytes + (int64_t)s.staged.size(), 16);
        p.host_off = up_bytes;
        if (s.on_host) up_bytes = align_up(up_bytes + 4 * (int64_t)(s.h_mono.size() + s.h_sig.size() + s.h_lg.size()), 16);
        p.raw_up_off = up_bytes;
        if (s.on_host && s.out_on) up_bytes = align_up(up_bytes + (int64_t)s.h_raw.size(), 16);
        if (s.bands_on) {
            // the step's sums reach from the first non-final bin to the last bin a window of the step covers (or a carried sum, or the
            // last bin that becomes final: behind a closed stream's last window there are bins without a window)
            const int64_t top = std::max({p.b_end, s.bins_done + s.bs_n, p.i_end > 0 ? ss_window_start_bin(p.i_end - 1, SS_STEP_DEFAULT) + 256 : (int64_t)0});
            p.bs_n = top - s.bins_done; p.bs_stride = align_up(std::max<int64_t>(p.bs_n, 1), 8);
            p.bs_off = arena_need; p.bs_ls = align_up(2 * 256 * (kBandAcc + p.bs_stride), 64); arena_need += s.lanes * p.bs_ls;
            p.band_up_off = up_bytes;
            if (s.on_host) up_bytes = align_up(up_bytes + 8 * (int64_t)s.h_band.size(), 16);
            p.fmap_at = fmap_need; fmap_need += s.lanes * (p.b_end - s.bins_done) * 256;
            b.total_w_band += s.lanes * (p.i_end - s.win_run); b.n_band_lanes += s.lanes;
        }
        b.total_w += s.lanes * (p.i_end - s.win_run);
        b.total_b += (s.lanes > 1 ? s.lanes + 1 : 1) * (p.b_end - s.bins_done);      // every lane's bins, then the merged ones
        b.n_lanes += s.lanes; b.n_each += s.lanes > 1;
        b.plans.push_back(p);
    }
    b.total_w_plain = b.total_w - b.total_w_band;
    b.ch_plain = pass_size(b.total_w_plain, chunk); b.ch_band = pass_size(b.total_w_band, chunk);
    b.n_pass_band = b.total_w_band > 0 ? (b.total_w_band + b.ch_band - 1) / b.ch_band : 0;
    // the streams' places among the step's windows (the band streams' behind the others') and in the avg / flags download
    int64_t w_plain_at = 0, w_band_at = b.total_w_plain, b_at = 0;
    for (size_t k = 0; k < act.size(); ++k) {
        const StreamRec& s = *act[k];
        StreamPlan& p = b.plans[k];
        int64_t& w_at = s.bands_on ? w_band_at : w_plain_at;
        p.w_at = w_at; w_at += s.lanes * (p.i_end - s.win_run);
        p.b_at = b_at; b_at += (s.lanes > 1 ? s.lanes + 1 : 1) * (p.b_end - s.bins_done);
    }
    b.desc_off = align_up(up_bytes, 64);
    B.need[kNext] = (size_t)std::max<int64_t>(arena_need, 64) * 4;
    B.need[kUp] = (size_t)b.desc_off + desc_bytes_max(b, act.size());
    B.need[kNewlg] = (size_t)std::max<int64_t>(b.total_w, 1) * 256 * 4;
    B.need[kAvg] = (size_t)std::max<int64_t>(b.total_b, 1) * 8;
    B.need[kFlags] = (size_t)std::max<int64_t>(b.total_b, 1);
    B.need[kFmap] = b.n_band_lanes ? (size_t)std::max<int64_t>(fmap_need, 256) * 4 : 0;
    B.need[kSpec] = b.n_band_lanes ? (size_t)b.ch_band * 2 * 32768 * 4 : 0;
    return b;
}

// one lane of one stream while its descriptors are built
struct LaneAt {
    const StreamRec& s; const StreamPlan& p; int l;
    const float* hm; const float* hs; const float* hl;    // the lane's carried mono history, signal and logits
    float* Am; float* As; float* Al;                      // its segments in the next half
    float* out0;                                          // the step's first new signal sample (padded index kPad + m_next)
    int64_t n_new_out, nw, nb, w_at, b_at;                // new samples, windows, final bins; the lane's first window and bin of the step
    bool direct;
};

// where lane 0's carried segments lie: in the stream's place of the upload after an import (the host vectors, copied there lanes back
// to back), otherwise in the current half where the last commit left them; `ls`: floats from a lane's segment to the next lane's
struct CarriedSrc { const float* hm; const float* hs; const float* hl; int64_t mono_ls, sig_ls, lg_ls; };
inline CarriedSrc carried_sources(StepBuild& b, const StreamRec& s, const StreamPlan& p, const StepBuffers& B) {
    if (!s.on_host) return CarriedSrc{B.at<const float>(kCur, s.mono_off), B.at<const float>(kCur, s.sig_off), B.at<const float>(kCur, s.lg_off), s.mono_ls, s.sig_ls, s.lg_ls};
    const int64_t o = p.host_off / 4, nm = (int64_t)s.h_mono.size(), ns = (int64_t)s.h_sig.size();
    b.pieces.push_back(HostPiece{p.host_off, s.h_mono.data(), s.h_mono.size() * 4});
    b.pieces.push_back(HostPiece{p.host_off + 4 * nm, s.h_sig.data(), s.h_sig.size() * 4});
    b.pieces.push_back(HostPiece{p.host_off + 4 * (nm + ns), s.h_lg.data(), s.h_lg.size() * 4});
    return CarriedSrc{B.at<const float>(kUp, o), B.at<const float>(kUp, o + nm), B.at<const float>(kUp, o + nm + ns), s.mono_n, s.sig_n, s.lg_n * 256};
}

// the stream's carried band accumulators (nothing before its first step)
inline void carried_band_source(StepBuild& b, const StreamRec& s, StreamPlan& p) {
    if (s.on_host) {
        p.acc_have = true; p.acc_buf = kUp; p.acc_off = p.band_up_off / 8; p.acc_ls = 256 * kBandAcc;
        b.pieces.push_back(HostPiece{p.band_up_off, s.h_band.data(), s.h_band.size() * 8});
    } else if (s.bs_ls) { p.acc_have = true; p.acc_buf = kCur; p.acc_off = s.bs_off / 2; p.acc_ls = s.bs_ls / 2; }
}

// copies before the passes (kLanePre): carried mono history [kb, frames_in); signal: carried [base_new, sig_end), the leading zeros of a
// new stream, the trailing zeros at close; the logits carried [lw0, win_run)
inline void lane_copies(StepBuild& b, const LaneAt& a) {
    const StreamRec& s = a.s; const StreamPlan& p = a.p;
    auto copy = [&](const float* src, float* dst, int64_t n) { b.pre.push_back(StreamCopy{src, dst, n}); b.max_copy = std::max(b.max_copy, n); };
    if (!a.direct && p.mono_keep > 0) copy(a.hm + (p.kb - s.mono_base), a.Am, p.mono_keep);
    if (p.sig_keep > 0) copy(a.hs + (p.base_new - s.sig_base), a.As, p.sig_keep);
    if (p.pre > 0) copy(nullptr, a.As + p.sig_keep, p.pre);
    copy(nullptr, a.out0 + a.n_new_out, p.post + 64);      // (+ 64: the slack behind the signal is zero, as in the file arena)
    if (s.lg_n > 0) copy(a.hl, a.Al, s.lg_n * 256);
}

// the stream's staged frames, decoded behind the mono history (or straight into the signal): lane 0 decodes for all lanes
// (kStreamDec / kStreamDecc)
inline void lane_decode(StepBuild& b, const LaneAt& a) {
    const StreamRec& s = a.s; const StreamPlan& p = a.p;
    if (s.staged_frames <= 0 || a.l != 0) return;
    float* dst = a.direct ? a.out0 : a.Am + p.mono_keep;
    if (s.lanes == 1) {
        b.dec.push_back(StreamDecode{p.up_off, s.staged_frames, dst, s.format, s.ch});
        b.max_dec = std::max(b.max_dec, s.staged_frames);
    } else {                                              // every lane's plane from the one reading of the frames
        b.decc.push_back(StreamDecodeChannels{p.up_off, s.staged_frames, dst, a.direct ? p.sig_ls : p.mono_ls, s.format, s.ch});
        b.max_decc = std::max(b.max_decc, s.staged_frames);
        b.decc_bytes += (double)s.staged.size() + 4.0 * (double)(s.staged_frames * s.lanes);
    }
}

inline void lane_resample(StepBuild& b, const LaneAt& a) {      // (kLaneRes)
    if (a.direct || a.n_new_out <= 0) return;
    b.res.push_back(StreamResample{a.Am, a.p.kb, a.p.F, a.s.d_taps, a.out0, a.s.m_next, a.n_new_out, a.s.L, a.s.M, a.s.half, 0});
    b.max_res = std::max(b.max_res, a.n_new_out);
}

// windows [win_run, i_end): arena offsets of their first samples
inline void lane_windows(StepBuild& b, const LaneAt& a) {
    const StreamRec& s = a.s; const StreamPlan& p = a.p;
    for (int64_t i = s.win_run; i < p.i_end; ++i) b.winoff[(size_t)(a.w_at + i - s.win_run)] = p.sig_off + a.l * p.sig_ls + (i * s.per_step - p.base_new);
}

// a band lane's sums: from the carried ones, one entry per pass that holds windows of the lane, the final bins' maps
// (map_entries_max)
inline void lane_maps(StepBuild& b, const LaneAt& a, const StepBuffers& B) {
    const StreamRec& s = a.s; const StreamPlan& p = a.p;
    StreamMap m{};
    if (s.on_host) {
        if (s.bs_n) { m.old_sum = B.at<const double>(kUp, p.band_up_off / 8 + (int64_t)s.lanes * 256 * kBandAcc + (int64_t)a.l * 256 * s.bs_n); m.old_stride = s.bs_n; }
    } else if (s.bs_n) { m.old_sum = B.at<const double>(kCur, (s.bs_off + a.l * s.bs_ls + s.bs_sum_off) / 2); m.old_stride = s.bs_stride; }
    m.old_b0 = s.bins_done; m.old_n = s.bs_n;
    m.sum = B.at<double>(kNext, (p.bs_off + a.l * p.bs_ls) / 2 + 256 * kBandAcc); m.stride = p.bs_stride; m.b0 = s.bins_done; m.n = p.bs_n;
    m.fmap = B.at<float>(kFmap, p.fmap_at + a.l * a.nb * 256); m.fin_n = a.nb; m.i_end = p.i_end;
    m.i0 = m.i1 = s.win_run;
    b.max_map_n = std::max(b.max_map_n, p.bs_n);
    const int64_t g0 = a.w_at - b.total_w_plain;             // the lane's first window among the band windows
    if (a.nw == 0) { m.flags = kMapInit | kMapFin; b.map_idle.push_back(m); }
    for (int64_t q = g0 / b.ch_band; a.nw > 0 && q * b.ch_band < g0 + a.nw; ++q) {
        StreamMap e = m;
        e.i0 = s.win_run + std::max<int64_t>(0, q * b.ch_band - g0);
        e.i1 = s.win_run + std::min<int64_t>(a.nw, (q + 1) * b.ch_band - g0);
        e.slot0 = g0 + (e.i0 - s.win_run) - q * b.ch_band;
        e.flags = (e.i0 == s.win_run ? kMapInit : 0) | (e.i1 == p.i_end ? kMapFin : 0);
        b.map_pass[(size_t)q].push_back(e);
    }
}

// behind the passes: the lane's new logits behind the carried ones (kLanePost), the averaging of the bins that became final (kLaneAvg)
inline void lane_average(StepBuild& b, const LaneAt& a, const StepBuffers& B) {
    const StreamRec& s = a.s; const StreamPlan& p = a.p;
    if (a.nw > 0) b.post.push_back(StreamCopy{B.at<const float>(kNewlg, a.w_at * 256), a.Al + (s.win_run - p.lw0) * 256, a.nw * 256});
    if (a.nb <= 0) return;
    b.avg.push_back(StreamAvg{a.Al, p.lw0, p.W_avg, 0, s.bins_done, a.nb, a.b_at, s.thr, s.step, step_bins(s.step)});
    b.max_bins = std::max(b.max_bins, a.nb);
    b.avg_reads += (double)a.nb * 256.0 / step_bins(s.step);
}

// Every descriptor of the step on the buffers' bases, and the host bytes the upload takes.  False: a vector outgrew the maxima the
// upload was sized from (nothing has been written anywhere).
inline bool build_step(StepBuild& b, const std::vector<StreamRec*>& act, const StepBuffers& B) {
    b.winoff.assign((size_t)b.total_w, 0);
    b.map_pass.assign((size_t)b.n_pass_band, {});
    for (size_t k = 0; k < act.size(); ++k) {
        const StreamRec& s = *act[k];
        StreamPlan& p = b.plans[k];
        if (!s.staged.empty()) b.pieces.push_back(HostPiece{p.up_off, s.staged.data(), s.staged.size()});
        if (s.on_host && s.out_on && !s.h_raw.empty()) b.pieces.push_back(HostPiece{p.raw_up_off, s.h_raw.data(), s.h_raw.size()});
        const CarriedSrc src = carried_sources(b, s, p, B);
        if (s.bands_on) carried_band_source(b, s, p);
        const bool direct = s.sr == SS_SAMPLE_RATE;
        const int64_t n_new_out = p.m_end - s.m_next, nw = p.i_end - s.win_run, nb = p.b_end - s.bins_done;
        for (int l = 0; l < s.lanes; ++l) {
            float* As = B.at<float>(kNext, p.sig_off + l * p.sig_ls);
            const LaneAt a{s, p, l, src.hm + l * src.mono_ls, src.hs + l * src.sig_ls, src.hl + l * src.lg_ls,
                           B.at<float>(kNext, p.mono_off + l * p.mono_ls), As, B.at<float>(kNext, p.lg_off + l * p.lg_ls), As + p.sig_keep + p.pre,
                           n_new_out, nw, nb, p.w_at + l * nw, p.b_at + l * nb, direct};
            lane_copies(b, a);
            lane_decode(b, a);
            lane_resample(b, a);
            lane_windows(b, a);
            if (s.bands_on) lane_maps(b, a, B);
            lane_average(b, a, B);
        }
        if (s.lanes > 1 && nb > 0) {                          // the merged bins behind the lanes' (kStreamUni)
            b.uni.push_back(StreamUnion{p.b_at, nb, p.b_at + s.lanes * nb, s.lanes, 0});
            b.max_uni = std::max(b.max_uni, nb);
            b.uni_bytes += 9.0 * (double)(nb * (s.lanes + 1));
        }
    }
    return desc_counts_ok(b, act.size());
}

// ------------------------------------------------------------------------------------------------------
// one packer for the step's three uploads: regions of a pinned buffer, each 64-byte aligned
// ------------------------------------------------------------------------------------------------------
struct UploadPacker {
    unsigned char* base; size_t cap, at;
    size_t used = 0;                                  // the end of the last region's bytes (`at`: that end, aligned)
    bool ok = true;
    UploadPacker(unsigned char* base_, size_t cap_, size_t at_ = 0) : base(base_), cap(cap_), at(at_), used(at_) { ok = at <= cap; }
    // -> the region's offset.  A region that does not fit is not written and fails the packer: the caller tests ok before it uploads.
    // room: the region takes that many bytes whatever it holds (its successors' offsets were stated before it was complete)
    size_t put(const void* src, size_t bytes, size_t room = 0) {
        const size_t o = at, end = (size_t)align_up((int64_t)(at + std::max(bytes, room)), 64);
        if (!ok || end > cap || (room && bytes > room)) { ok = false; return o; }
        if (bytes) memcpy(base + at, src, bytes);
        used = at + bytes; at = end;
        return o;
    }
    template <typename T> size_t put(const std::vector<T>& v) { return put(v.data(), v.size() * sizeof(T)); }
    bool piece(const HostPiece& h) {                  // data at a place the layout chose, in front of the packed regions
        if (!ok || h.off < 0 || (size_t)h.off + h.bytes > cap) return ok = false;
        if (h.bytes) memcpy(base + h.off, h.src, h.bytes);
        return true;
    }
};

// ------------------------------------------------------------------------------------------------------
// commit: the region walk
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
inline int64_t band_pos(double bin_t) {
    int64_t first, count;
    const double x = bin_t - 3.0;
    region_bins(x, x, 0, (int64_t)1 << 40, first, count);
    return first;
}
inline void band_emit(StreamRec& s, size_t n0) {          // the walk has just returned regions n0 .. (at most one)
    for (size_t r = n0; r < s.r_out.size(); ++r) {
        int64_t first, count;
        region_bins(s.r_out[r].start, s.r_out[r].end, 0, (int64_t)1 << 40, first, count);
        s.b_ev.push_back(StreamBandEv{0, s.b_parked ? kEvEmitPark : kEvEmitSnap, (int32_t)count, (int64_t)r});
        s.b_parked = false;
    }
}
inline void band_snap(StreamRec& s) {                     // the candidate's bins end before run_last (a snapshot of an earlier step holds otherwise)
    const int64_t pos = band_pos(bin_time(s.run_last));
    if (pos >= s.b_b0) s.b_ev.push_back(StreamBandEv{pos, kEvSnap, 0, 0});
}

inline void close_run(StreamRec& s) {
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

inline void flush_merged(StreamRec& s) {
    const size_t n0 = s.r_out.size();
    s.mg.flush(s.r_out);
    if (s.bands_on) band_emit(s, n0);
    if (s.lanes > 1 && s.r_out.size() > n0) s.p_out.insert(s.p_out.end(), s.pk_cur.begin(), s.pk_cur.end());
}

inline void walk_bin(StreamRec& s, int64_t j, unsigned char f, const double* v, int64_t vs) {
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

inline void finish_regions(StreamRec& s) {
    if (s.run_open) close_run(s);
    flush_merged(s);
}

// the step's final bins of one stream from the download (a plain stream's bins; an each-channel stream's lanes, then its merged bins:
// the series it returns and walks)
inline void commit_bins(StreamRec& s, const StreamPlan& p, const double* h_avg, const unsigned char* h_flags) {
    const int64_t nb = p.b_end - s.bins_done, m_at = p.b_at + (s.lanes > 1 ? s.lanes * nb : 0);
    s.b_ev.clear(); s.b_b0 = s.bins_done;
    const double* lane_avg = s.lanes > 1 ? h_avg + p.b_at : nullptr;
    for (int64_t k = 0; k < nb; ++k) {
        const int64_t j = s.bins_done + k;
        const unsigned char f = h_flags[m_at + k];
        if (f & 1) { s.a_out.push_back(h_avg[m_at + k]); s.b_out.push_back(j); }
        walk_bin(s, j, f, lane_avg ? lane_avg + k : nullptr, nb);
    }
    if (s.lanes > 1)
        for (int l = 0; l < s.lanes; ++l)
            for (int64_t k = 0; k < nb; ++k)
                if (h_flags[m_at + k] & 1) s.la_out.push_back(h_avg[p.b_at + l * nb + k]);
}

// what the next step needs, inside the segments this step wrote
inline void commit_carried(StreamRec& s, const StreamPlan& p, int64_t sig_end) {
    if (s.sr != SS_SAMPLE_RATE) {
        const int64_t k0 = std::min(std::max(p.kb, (p.m_end * s.M) / s.L - s.half + 1), p.F);
        s.mono_base = k0; s.mono_n = p.F - k0; s.mono_off = p.mono_off + (k0 - p.kb);
    }
    s.sig_base = p.i_end * s.per_step; s.sig_n = sig_end - s.sig_base; s.sig_off = p.sig_off + (s.sig_base - p.base_new);
    const int64_t w0 = std::min(std::max(first_window_for_bin(s, p.b_end), p.lw0), p.i_end);
    s.lg_w0 = w0; s.lg_n = p.i_end - w0; s.lg_off = p.lg_off + (w0 - p.lw0) * 256;
}

// The records take in the step: `all` -- every stream of the context, whose last results are cleared --, `act` -- the streams of the
// step --, the downloaded averages and flags.  The caller flips the arena behind it.
template <typename AllStreams>
inline void commit_step(AllStreams& all, const std::vector<StreamRec*>& act, const StepBuild& b, const double* h_avg, const unsigned char* h_flags) {
    for (auto& kv : all) {
        StreamRec& s = kv.second;
        s.r_out.clear(); s.a_out.clear(); s.b_out.clear(); s.la_out.clear(); s.p_out.clear(); s.o_first = s.frames_out; s.o_n = 0;
        s.bd_out.clear(); s.bp_out.clear();
    }
    for (size_t k = 0; k < act.size(); ++k) {
        StreamRec& s = *act[k];
        const StreamPlan& p = b.plans[k];
        const int64_t nb = p.b_end - s.bins_done;
        commit_bins(s, p, h_avg, h_flags);
        s.mono_ls = p.mono_ls; s.sig_ls = p.sig_ls; s.lg_ls = p.lg_ls;
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
        commit_carried(s, p, sig_end);
    }
}

// ------------------------------------------------------------------------------------------------------
// bands, behind the commit's walks: every band lane's accumulators move to the half the step built through stream_band_kernel, which
// takes in the step's final bins under the stream's events and evaluates the regions the walk returned
// ------------------------------------------------------------------------------------------------------
struct BandBuild {
    std::vector<StreamBand> bd;
    std::vector<StreamBandEv> evs;
    int64_t n_rec = 0; bool any_prof = false;
    size_t rec_bytes = 0, prof_bytes = 0;             // the records, then the profiles, in the pinned result buffer
    double bins = 0;
};

inline BandBuild layout_bands(const std::vector<StreamRec*>& act, const StepBuild& b, StepBuffers& B) {
    BandBuild o;
    for (size_t k = 0; k < act.size(); ++k) {
        const StreamRec& s = *act[k];
        const StreamPlan& p = b.plans[k];
        if (!s.bands_on) continue;
        const int64_t nb = s.bins_done - s.b_b0;
        for (int l = 0; l < s.lanes; ++l)
            o.bd.push_back(StreamBand{p.acc_have ? B.at<const double>(p.acc_buf, p.acc_off + l * p.acc_ls) : nullptr, B.at<double>(kNext, (p.bs_off + l * p.bs_ls) / 2),
                                      B.at<const float>(kFmap, p.fmap_at + l * nb * 256), s.b_b0, nb, o.n_rec, (int32_t)o.evs.size(), (int32_t)s.b_ev.size(), s.lanes, l,
                                      s.bprm.speech_channel, s.want_prof ? 1 : 0, s.bprm.q_low, s.bprm.q_high});
        o.evs.insert(o.evs.end(), s.b_ev.begin(), s.b_ev.end());
        o.n_rec += (int64_t)s.r_out.size() * s.lanes;
        o.any_prof = o.any_prof || s.want_prof;
        o.bins += (double)(nb * s.lanes);
    }
    if (o.bd.empty()) return o;
    o.rec_bytes = (size_t)align_up(o.n_rec * (int64_t)sizeof(ss_region_band), 64); o.prof_bytes = o.any_prof ? (size_t)o.n_rec * 256 * 8 : 0;
    B.need[kUp3] = (size_t)align_up((int64_t)(o.bd.size() * sizeof(StreamBand)), 64) + (size_t)align_up((int64_t)(o.evs.size() * sizeof(StreamBandEv)), 64);
    B.need[kBout] = (size_t)std::max<int64_t>(o.n_rec, 1) * sizeof(ss_region_band);
    B.need[kBprof] = (size_t)std::max<int64_t>(o.any_prof ? o.n_rec * 256 : 1, 1) * 8;
    return o;
}

// the records [n][lanes] (and profiles [n][lanes][256]) of every band stream, in the step's order, from the download
inline void commit_bands(const std::vector<StreamRec*>& act, const ss_region_band* rec, const double* prof) {
    int64_t at = 0;
    for (StreamRec* sp : act) {
        StreamRec& s = *sp;
        if (!s.bands_on) continue;
        const int64_t n = (int64_t)s.r_out.size() * s.lanes;
        if (n) {
            s.bd_out.assign(rec + at, rec + at + n);
            if (s.want_prof) s.bp_out.assign(prof + at * 256, prof + (at + n) * 256);
        }
        at += n;
        s.b_ev.clear();
    }
}

// ------------------------------------------------------------------------------------------------------
// the output of the streams opened with it (include/softspoken.h: which frames a step returns), behind the commit: the streams' walks
// have taken in the step's bins, frames_in counts the step's frames, the staged bytes still lie in the upload.  One launch encodes
// every stream's decided frames, one copies the raw PCM that stays into the other half of the byte arena.
// ------------------------------------------------------------------------------------------------------
// [begin, end) of one region of the erase table as silence_ranges rounds it, clamped at frame 0 (the clamp to the recording's length
// is the limit's: no frame at or past it is looked at)
inline void erase_frames(const ss_region& padded, int sr, int64_t& lo, int64_t& hi) {
    const double a = std::nearbyint(padded.start * (double)sr), b = std::nearbyint(padded.end * (double)sr);
    lo = (int64_t)std::min(std::max(a, 0.0), 9.0e18); hi = (int64_t)std::min(std::max(b, 0.0), 9.0e18);
}

inline void merge_ranges(std::vector<int64_t>& r) {      // sorted by begin, overlapping and touching ranges joined, as silence_ranges
    std::vector<std::pair<int64_t, int64_t>> v;
    for (size_t i = 0; i + 1 < r.size(); i += 2) if (r[i + 1] > r[i]) v.emplace_back(r[i], r[i + 1]);
    std::sort(v.begin(), v.end());
    r.clear();
    for (const auto& p : v) {
        if (!r.empty() && p.first <= r.back()) r.back() = std::max(r.back(), p.second);
        else { r.push_back(p.first); r.push_back(p.second); }
    }
}

// one stream's output of the step: frames [frames_out, limit) leave, the raw PCM of [limit, frames_in) stays at raw_off of the next
// half of the byte arena; er_rng: the stream's erase table with the step's regions taken in
struct OutPlan { size_t k; int64_t limit, rng_at, n_rng, out_off, raw_off, erased; std::vector<int64_t> er_rng; };
struct OutBuild {
    std::vector<OutPlan> ops;
    std::vector<int64_t> rng_all;                     // the ranges inside [frames_out, limit) of every stream (byte numbers for a source stream)
    std::vector<StreamSilence> sil;
    std::vector<StreamCopyBytes> cpb;
    std::vector<StreamSilenceSource> srcs;
    int64_t total_out = 0, total_outb = 0;            // int16 samples; bytes of the source-encoding streams
    int64_t max_samples = 0, max_bytes = 0, max_src = 0;
    double in_bytes = 0, carried = 0, src_bytes = 0;
};

// the frames a stream returns in this step and the ranges of them that are erased
inline OutPlan plan_output(const StreamRec& s, size_t k, std::vector<int64_t>& rng_all) {
    OutPlan o{k, 0, (int64_t)rng_all.size(), 0, 0, 0, 0, s.er_rng};
    auto add_region = [&](std::vector<int64_t>& to, const ss_region& r) {
        if (!erase_keeps(r, s.er.min_len_s)) return;
        int64_t lo, hi;
        erase_frames(erase_padded(r, s.er.pad_s), s.sr, lo, hi);
        if (hi > lo) { to.push_back(lo); to.push_back(hi); }
    };
    for (const ss_region& r : s.r_out) add_region(o.er_rng, r);       // what the step returned (everything, at close)
    merge_ranges(o.er_rng);
    std::vector<int64_t> rng = o.er_rng;
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
    return o;
}

// a stream's descriptors: its decided frames encoded, its raw PCM that stays copied on
inline void output_descs(OutBuild& ob, const OutPlan& o, const StreamRec& s, const StreamPlan& p, const StepBuffers& B, int64_t o_rng) {
    const int64_t fb = s.frame_bytes(), n = o.limit - s.frames_out;
    // the frames [frames_out, f0) carried from earlier steps, and the step's own [f0, frames_in) in the upload
    const unsigned char* seg0 = p.was_host ? B.at<const unsigned char>(kUp, p.raw_up_off) : B.at<const unsigned char>(kRawCur, s.raw_off);
    const unsigned char* seg1 = B.at<const unsigned char>(kUp, p.up_off);
    const int64_t* ranges = B.at<const int64_t>(kUp2, o_rng / 8 + o.rng_at);
    if (n > 0 && s.src_out) {   // bytes in, bytes out: the ranges as byte numbers of the recording
        for (int64_t i = o.rng_at; i < o.rng_at + 2 * o.n_rng; ++i) ob.rng_all[(size_t)i] *= fb;
        ob.srcs.push_back(StreamSilenceSource{seg0, seg1, ranges, std::min(n, p.f0 - s.frames_out) * fb, s.frames_out * fb, n * fb, o.out_off, (int32_t)o.n_rng,
                                              s.format == SS_PCM_U8 ? 0x80808080u : 0u});
        ob.max_src = std::max(ob.max_src, n * fb);
        ob.src_bytes += (double)(n * fb);
    } else if (n > 0) {
        ob.sil.push_back(StreamSilence{seg0, seg1, ranges, std::min(n, p.f0 - s.frames_out), s.frames_out, n, o.out_off, (int32_t)o.n_rng, s.format, s.ch, 0});
        ob.max_samples = std::max(ob.max_samples, n * s.ch);
        ob.in_bytes += (double)(n * fb);
    }
    unsigned char* dst = B.at<unsigned char>(kRawNext, o.raw_off);
    const size_t k0 = ob.cpb.size();
    if (o.limit < p.f0) {
        ob.cpb.push_back(StreamCopyBytes{seg0 + (o.limit - s.frames_out) * fb, dst, (p.f0 - o.limit) * fb});
        dst += (p.f0 - o.limit) * fb;
    }
    const int64_t from = std::max(o.limit, p.f0);
    if (from < s.frames_in) ob.cpb.push_back(StreamCopyBytes{seg1 + (from - p.f0) * fb, dst, (s.frames_in - from) * fb});
    for (size_t k = k0; k < ob.cpb.size(); ++k) { ob.max_bytes = std::max(ob.max_bytes, ob.cpb[k].n); ob.carried += (double)ob.cpb[k].n; }
}

// the regions of the output's upload, in the packer's order: silence, copy, source descriptors (one, two, one per stream at most), ranges
inline int64_t output_ranges_off(size_t n_ops) {
    return align_up((int64_t)(n_ops * sizeof(StreamSilence)), 64) + align_up((int64_t)(2 * n_ops * sizeof(StreamCopyBytes)), 64) +
           align_up((int64_t)(n_ops * sizeof(StreamSilenceSource)), 64);
}

// plans first (they state the sizes), then -- the caller has grown the buffers -- the descriptors
inline OutBuild plan_outputs(const std::vector<StreamRec*>& act, StepBuffers& B) {
    OutBuild ob;
    int64_t raw_need = 0;                             // carried bytes
    for (size_t k = 0; k < act.size(); ++k) {
        const StreamRec& s = *act[k];
        if (!s.out_on) continue;
        OutPlan o = plan_output(s, k, ob.rng_all);
        if (s.src_out) { o.out_off = ob.total_outb; ob.total_outb = align_up(ob.total_outb + (o.limit - s.frames_out) * s.frame_bytes(), 16); }
        else { o.out_off = ob.total_out; ob.total_out = align_up(ob.total_out + (o.limit - s.frames_out) * s.ch, 8); }
        o.raw_off = raw_need; raw_need = align_up(raw_need + (s.frames_in - o.limit) * s.frame_bytes(), 16);
        ob.ops.push_back(std::move(o));
    }
    if (ob.ops.empty()) return ob;
    B.need[kRawNext] = (size_t)std::max<int64_t>(raw_need, 16);
    B.need[kOut] = (size_t)std::max<int64_t>(ob.total_out, 8) * 2;
    B.need[kOutb] = ob.total_outb > 0 ? (size_t)ob.total_outb + 16 : 0;
    B.need[kUp2] = (size_t)output_ranges_off(ob.ops.size()) + (size_t)align_up((int64_t)ob.rng_all.size() * 8, 64);
    return ob;
}

inline void build_outputs(OutBuild& ob, const std::vector<StreamRec*>& act, const StepBuild& b, const StepBuffers& B) {
    const int64_t o_rng = output_ranges_off(ob.ops.size());
    for (const OutPlan& o : ob.ops) output_descs(ob, o, *act[o.k], b.plans[o.k], B, o_rng);
}

inline void commit_outputs(const std::vector<StreamRec*>& act, OutBuild& ob) {
    for (OutPlan& o : ob.ops) {
        StreamRec& s = *act[o.k];
        s.o_first = s.frames_out; s.o_n = o.limit - s.frames_out; s.o_off = o.out_off;
        s.frames_out = o.limit; s.erased += o.erased; s.raw_off = o.raw_off;
        s.er_rng.clear();
        for (size_t i = 0; i + 1 < o.er_rng.size(); i += 2) if (o.er_rng[i + 1] > o.limit) { s.er_rng.push_back(o.er_rng[i]); s.er_rng.push_back(o.er_rng[i + 1]); }
    }
}

}  // namespace ss
