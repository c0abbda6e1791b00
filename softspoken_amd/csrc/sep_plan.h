// The host plan of the separation silencer and the region bands (separate.hip): which STFT frames, bins and windows a call needs,
// and every index a kernel reads -- gain rows, records, window slots, compact bins.  No HIP call, no HIP header and no ss_ctx:
// tests/sep_plan_check.cpp holds every plan to a brute-force restatement without a device.
//   small rules   FFT size, file geometry, a frame's two bins, the windows over a bin range, ss_separation_plan, argument checks
//   plan_maps       merged bin and window ranges -> compact bins, window slots, the run list       (separate.hip sep_run_maps)
//   plan_ranges, plan_synthesis  a SepPlan -> merged ranges; frames, interval pieces, chunks of a frame budget  (separate_run)
//   plan_boxes      a box table -> merged intervals, box rows, each frame's active boxes; the same pieces and chunks  (box_run)
//   plan_bands      regions -> rule 1, the disjoint union, pieces of a bin budget, tile segments   (region_bands)
#pragma once
#include "hostdefs.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

namespace ss {

// the layouts the kernels read
struct SepFrame { int64_t k; int32_t cb0, cb1; float alpha; int32_t pad; };     // an STFT frame: centre k hop, gain rows cb0 / cb1
struct SepSeg { int64_t a, b, s0, s1, k0, rec0, out0; };                          // an interval piece: interval [a, b), samples [s0, s1),
                                                                                  // frames k0.. in records rec0.., first output slot out0
struct BandSeg { int32_t cb0, n, out, pad; };         // (region, tile): compact bins cb0 .. cb0 + n - 1 of the piece's maps -> tile sum `out`
struct BandRegion { int32_t seg0, nseg, n_bins, pad; };   // a region's tile sums seg0 .. seg0 + nseg - 1 (ascending tiles), its bins

using Ranges = std::vector<std::pair<int64_t, int64_t>>;  // inclusive ranges, ascending and merged

struct SepPlan {                                          // ss_separation_plan's result
    int N = 0, hop = 0;
    int64_t W = 0, n_bins = 0, windows_run = 0;
    std::vector<ss_separation_range> ranges;
};

// ---- small rules ----------------------------------------------------------------------------------------------------
inline int64_t floordiv(int64_t a, int64_t b) { int64_t q = a / b; if ((a % b != 0) && ((a < 0) != (b < 0))) --q; return q; }
inline int64_t win_start(int64_t i) { return (512 * i + 5) / 10; }

inline int sep_fft_size(int sr) {
    const double l = std::log2((double)sr * 512.0 / 22050.0);
    const long e = std::lround(l);
    return 1 << std::min<long>(13, std::max<long>(8, e));
}

// W and covered bins of a file whose padded signal holds n_padded samples and whose header says duration_s (ss_run's plan)
inline void file_geometry(double duration_s, int64_t n_padded, int64_t& W, int64_t& n_bins) {
    W = ss_plan_windows(duration_s, nullptr, 0);
    while (W > 0 && (W - 1) * (int64_t)SS_STEP_SAMPLES + SS_WINDOW_SAMPLES > n_padded) --W;
    const int64_t nb = (int64_t)std::nearbyint((double)n_padded / 22050.0 * 256.0 / 3.0);
    n_bins = W > 0 ? std::min(nb, win_start(W - 1) + 256) : 0;
}

// the two bins around frame k's time k hop / sr (centres (j + 0.5) 3 / 256 - 3 s) and the weight of the second; exact integers:
// u = (k hop / sr + 3) 256 / 3 - 0.5 = (512 (k hop + 3 sr) - 3 sr) / (6 sr).  Clamped to bins 0 .. n_bins - 1.
inline void frame_bins(int64_t k, int hop, int sr, int64_t n_bins, int64_t& j0, int64_t& j1, double& alpha) {
    const int64_t num = 512 * (k * hop + 3 * (int64_t)sr) - 3 * (int64_t)sr, den = 6 * (int64_t)sr;
    j0 = floordiv(num, den);
    alpha = (double)(num - j0 * den) / (double)den;
    if (j0 < 0) { j0 = j1 = 0; alpha = 0.0; }
    else if (j0 >= n_bins - 1) { j0 = j1 = n_bins - 1; alpha = 0.0; }
    else j1 = j0 + 1;
}

// windows (inclusive) that cover any bin of [b0, b1]
inline void covering_windows(int64_t b0, int64_t b1, int64_t W, int64_t& w0, int64_t& w1) {
    w0 = std::max<int64_t>(0, (int64_t)((double)(b0 - 255) / 51.2) - 2);
    while (w0 < W - 1 && win_start(w0) + 255 < b0) ++w0;
    w1 = std::min<int64_t>(W - 1, (int64_t)((double)b1 / 51.2) + 2);
    while (w1 > 0 && win_start(w1) > b1) --w1;
}

inline int check_separation_params(const ss_separation_params* p, std::string& err) {
    if (!p) return SS_OK;
    if (p->speech_channel != 0 && p->speech_channel != 1) { err = "speech_channel must be 0 or 1"; return SS_ERR_ARG; }
    if (!(p->fade_s >= 0.0) || !std::isfinite(p->fade_s)) { err = "fade_s must be a finite value >= 0"; return SS_ERR_ARG; }
    if (!(p->min_gain >= 0.0 && p->min_gain <= 1.0)) { err = "min_gain must lie in [0, 1]"; return SS_ERR_ARG; }
    if (p->above_fmax != SS_ABOVE_FMAX_MUTE && p->above_fmax != SS_ABOVE_FMAX_KEEP) { err = "above_fmax must be SS_ABOVE_FMAX_MUTE or _KEEP"; return SS_ERR_ARG; }
    return SS_OK;
}

inline ss_separation_params separation_defaults() { return ss_separation_params{0.01, 0.0, SS_ABOVE_FMAX_MUTE, 1}; }

inline void separation_plan(int sr, int64_t frames, const ss_region* regions, int64_t n_regions, SepPlan& pl) {
    pl.N = sep_fft_size(sr); pl.hop = pl.N / 4;
    const int64_t n_padded = ss_resampled_length(frames, sr) + 2 * (int64_t)SS_WINDOW_SAMPLES;
    file_geometry((double)frames / (double)sr, n_padded, pl.W, pl.n_bins);
    pl.ranges.clear(); pl.windows_run = 0;
    const std::vector<int64_t> r = silence_ranges(regions, n_regions, sr, frames);
    int64_t last_win = -1;
    for (size_t i = 0; i + 1 < r.size(); i += 2) {
        ss_separation_range g{};
        g.frame_begin = r[i]; g.frame_end = r[i + 1];
        g.stft_first = floordiv(g.frame_begin - pl.N / 2, pl.hop) + 1;
        g.stft_last = -floordiv(-(g.frame_end + pl.N / 2), pl.hop) - 1;
        int64_t a0, a1, b0, b1; double al;
        frame_bins(g.stft_first, pl.hop, sr, pl.n_bins, a0, a1, al);
        frame_bins(g.stft_last, pl.hop, sr, pl.n_bins, b0, b1, al);
        g.bin_first = a0; g.bin_last = b1;
        covering_windows(g.bin_first, g.bin_last, pl.W, g.win_first, g.win_last);
        const int64_t from = std::max(g.win_first, last_win + 1);
        if (g.win_last >= from) pl.windows_run += g.win_last - from + 1;
        last_win = std::max(last_win, g.win_last);
        pl.ranges.push_back(g);
    }
}

inline int check_band_args(const ss_region* regions, int64_t n, const ss_band_params* p, std::string& err) {
    if (n < 0 || (n > 0 && !regions)) { err = "bad region table"; return SS_ERR_ARG; }
    if (n > (int64_t)1 << 24) { err = "too many regions"; return SS_ERR_ARG; }
    if (p) {
        if (!(p->q_low > 0.0 && p->q_low < p->q_high && p->q_high <= 1.0)) { err = "need 0 < q_low < q_high <= 1"; return SS_ERR_ARG; }
        if (p->speech_channel != 0 && p->speech_channel != 1) { err = "speech_channel must be 0 or 1"; return SS_ERR_ARG; }
    }
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(regions[i].start) || !std::isfinite(regions[i].end) || regions[i].end < regions[i].start) {
            err = "region " + std::to_string(i) + " is not finite or ends before it starts";
            return SS_ERR_ARG;
        }
    return SS_OK;
}

// a range joins the last one of `to` where it overlaps or touches it
inline void join_range(Ranges& to, int64_t first, int64_t last) {
    if (!to.empty() && first <= to.back().second + 1) to.back().second = std::max(to.back().second, last);
    else to.emplace_back(first, last);
}

// ---- maps plan: what sep_accumulate_kernel reads --------------------------------------------------------------------
// cbin [ncb]: the bins of bin_ranges, ascending.  slot [W]: a window's place among the nw windows of win_ranges, -1 for the others.
// off: the run list -- signal s's windows (arena offset sig_off[s] + i SS_STEP_SAMPLES) behind signal s - 1's.
struct MapsPlan { std::vector<int32_t> cbin, slot; std::vector<int64_t> off; int ncb = 0, nw = 0; };

// false: more windows than an int32 slot counts
inline bool plan_maps(const Ranges& bin_ranges, const Ranges& win_ranges, int64_t W, int nsig, const int64_t* sig_off, MapsPlan& m) {
    m.cbin.clear(); m.off.clear(); m.slot.assign((size_t)W, -1);
    for (auto& r : bin_ranges) for (int64_t j = r.first; j <= r.second; ++j) m.cbin.push_back((int32_t)j);
    for (int s = 0; s < nsig; ++s) {
        int32_t t = 0;
        for (auto& r : win_ranges)
            for (int64_t i = r.first; i <= r.second; ++i) { m.slot[i] = t++; m.off.push_back(sig_off[s] + i * SS_STEP_SAMPLES); }
    }
    if (m.off.size() > (size_t)INT32_MAX) return false;
    m.ncb = (int)m.cbin.size(); m.nw = (int)m.off.size() / nsig;
    return true;
}

// ---- synthesis plan: what sep_stft_kernel<N> and sep_blend_kernel read ----------------------------------------------
struct SepChunk { size_t seg0, nseg, rec0, nrec; int64_t total; };   // segments, frame records and output samples of one round of the frame buffer
struct SepRanges {
    Ranges br, wr;                                        // the intervals' bins and windows, merged: what the maps are made over
    std::vector<int64_t> cbase;                           // compact index of each interval's first bin
};
// The cuts of a frame budget, shared by the separation silencer and the band silencer (plan_boxes): interval pieces, their frame
// records (counted here, laid out by the caller) and the chunks of the frame buffer
struct SepCuts {
    std::vector<SepSeg> sg;
    std::vector<SepChunk> chunks;
    size_t n_rec = 0, max_rec = 0;                        // records in all; most records of a chunk
};
struct SynthPlan : SepCuts {
    std::vector<SepFrame> fr;
    size_t fout_need = 0;                                 // the frame buffer [max_rec][npairs][N], in float2
};

inline SepRanges plan_ranges(const SepPlan& pl) {
    SepRanges p;
    int64_t ncb_run = 0;
    for (const auto& g : pl.ranges) {
        if (!p.br.empty() && g.bin_first <= p.br.back().second + 1) {
            const int64_t at = ncb_run - (p.br.back().second - p.br.back().first + 1);
            p.cbase.push_back(at + (g.bin_first - p.br.back().first));
            if (g.bin_last > p.br.back().second) { ncb_run += g.bin_last - p.br.back().second; p.br.back().second = g.bin_last; }
        } else {
            p.cbase.push_back(ncb_run);
            p.br.emplace_back(g.bin_first, g.bin_last);
            ncb_run += g.bin_last - g.bin_first + 1;
        }
        join_range(p.wr, g.win_first, g.win_last);
    }
    return p;
}

// One merged interval [a, b) cut into pieces of at most (budget - 8) hop samples; a piece opens a new chunk when its frames would pass
// `budget` records (budget >= 16).  A piece holds every frame over its samples, so neighbours recompute the three frames they share.
// frame(k): called once per record, in record order -- the caller appends its own record for frame k.
template <class Frame>
inline void cut_interval(SepCuts& p, int N, int hop, int64_t budget, int64_t a, int64_t b, Frame&& frame) {
    const int64_t piece = (budget - 8) * hop;
    for (int64_t s0 = a; s0 < b; s0 += piece) {
        const int64_t s1 = std::min(b, s0 + piece);
        const int64_t k0 = floordiv(s0 - N / 2, hop) + 1, k1 = -floordiv(-(s1 + N / 2), hop) - 1;
        if (p.chunks.empty() || (int64_t)(p.n_rec - p.chunks.back().rec0) + (k1 - k0 + 1) > budget)
            p.chunks.push_back(SepChunk{p.sg.size(), 0, p.n_rec, 0, 0});
        SepChunk& ck = p.chunks.back();
        p.sg.push_back(SepSeg{a, b, s0, s1, k0, (int64_t)(p.n_rec - ck.rec0), ck.total});
        for (int64_t k = k0; k <= k1; ++k) { frame(k); ++p.n_rec; }
        ck.nseg++; ck.nrec = p.n_rec - ck.rec0; ck.total += s1 - s0;
    }
}
inline void finish_cuts(SepCuts& p) { for (const SepChunk& ck : p.chunks) p.max_rec = std::max(p.max_rec, ck.nrec); }

// pieces and chunks of a frame budget (cut_interval); cbase: plan_ranges' (made behind the maps' launches)
inline SynthPlan plan_synthesis(const SepPlan& pl, const std::vector<int64_t>& cbase, int sr, int ch, int64_t budget) {
    SynthPlan p;
    const int N = pl.N, hop = pl.hop;
    for (size_t r = 0; r < pl.ranges.size(); ++r) {
        const auto& g = pl.ranges[r];
        cut_interval(p, N, hop, budget, g.frame_begin, g.frame_end, [&](int64_t k) {
            int64_t j0, j1; double al;
            frame_bins(k, hop, sr, pl.n_bins, j0, j1, al);
            p.fr.push_back(SepFrame{k, (int32_t)(cbase[r] + (j0 - g.bin_first)), (int32_t)(cbase[r] + (j1 - g.bin_first)), (float)al, 0});
        });
    }
    finish_cuts(p);
    p.fout_need = p.max_rec * (size_t)((ch + 1) / 2) * N;
    return p;
}

// ---- box plan: what box_stft_kernel<N> reads (include/softspoken.h "band silencer") ------------------------------------
// a box's row: bins q_lo .. q_hi lie inside (q_lo clamped to 0 .. N/2 + 1, q_hi to -1 .. N/2; q_lo > q_hi: no bin inside).  The distances
// of the roll-off are kept as an exact integer and a fraction, so that float32 holds them at every N: below q_lo, d = (q_lo - q) - lo_f
// with lo_f = q_lo - lo_b; above q_hi, d = (q - q_hi) - hi_f with hi_f = hi_b - q_hi.  inv_e = 1 / e_b, 0 for the hard edge.
struct BoxRow { int32_t q_lo, q_hi; float lo_f, hi_f, inv_e; int32_t channel; };
struct BoxFrame { int64_t k; int32_t first, count; };     // frame k's active boxes: idx[first .. first + count - 1], ascending box index

struct BoxPlan : SepCuts {
    int N = 0, hop = 0;
    std::vector<ss_box_range> ranges;                     // the merged intervals and their frames
    int64_t n_frames = 0;                                 // distinct frames over them
    std::vector<BoxRow> rows;                             // one per box of the table (a dropped box's row is read by no frame)
    std::vector<BoxFrame> fr;                             // one per record
    std::vector<int32_t> idx;
    int32_t max_count = 0;                                // most active boxes of a frame
    size_t fout_need = 0;
};

inline ss_box_params box_defaults() { return ss_box_params{0.01, 0.0, 100.0}; }

// channels: the file's, or 0 when only the table is known (ss_box_plan: -1 .. 255)
inline int check_box_args(const ss_box* boxes, int64_t n, int channels, const ss_box_params* p, std::string& err) {
    if (n < 0 || (n > 0 && !boxes)) { err = "bad box table"; return SS_ERR_ARG; }
    if (n > (int64_t)1 << 24) { err = "too many boxes"; return SS_ERR_ARG; }
    if (p) {
        if (!(p->fade_s >= 0.0) || !std::isfinite(p->fade_s)) { err = "fade_s must be a finite value >= 0"; return SS_ERR_ARG; }
        if (!(p->min_gain >= 0.0 && p->min_gain <= 1.0)) { err = "min_gain must lie in [0, 1]"; return SS_ERR_ARG; }
        if (!(p->edge_hz >= 0.0) || !std::isfinite(p->edge_hz)) { err = "edge_hz must be a finite value >= 0"; return SS_ERR_ARG; }
    }
    const int top = channels > 0 ? channels : 256;
    for (int64_t i = 0; i < n; ++i) {
        const ss_box& b = boxes[i];
        const double lo = std::isnan(b.low_hz) ? 0.0 : b.low_hz, hi = std::isnan(b.high_hz) ? INFINITY : b.high_hz;
        const char* what = nullptr;
        if (!std::isfinite(b.start) || !std::isfinite(b.end) || b.end < b.start) what = "is not finite or ends before it starts";
        else if (lo > hi) what = "has low_hz above high_hz";
        else if (hi < 0.0) what = "has a negative high_hz";
        else if (b.channel < -1 || b.channel >= top) what = "names a channel the file does not have";
        else if (b.reserved != 0) what = "has a non-zero reserved field";
        if (what) { err = "box " + std::to_string(i) + " " + what; return SS_ERR_ARG; }
    }
    return SS_OK;
}

inline BoxRow box_row(const ss_box& b, int N, int sr, double edge_hz) {
    const double lo = std::isnan(b.low_hz) ? 0.0 : b.low_hz, hi = std::isnan(b.high_hz) ? INFINITY : b.high_hz;
    const double lo_b = lo * (double)N / (double)sr, hi_b = hi * (double)N / (double)sr, e_b = edge_hz * (double)N / (double)sr;
    const int half = N / 2;
    BoxRow r{};
    r.q_lo = lo_b > (double)half ? half + 1 : (int32_t)std::max(0.0, std::ceil(lo_b));
    r.q_hi = hi_b >= (double)half ? half : (int32_t)std::floor(hi_b);
    r.lo_f = (float)((double)r.q_lo - lo_b);
    r.hi_f = hi_b >= (double)half ? 0.f : (float)(hi_b - (double)r.q_hi);
    r.inv_e = e_b > 0.0 ? (float)(1.0 / e_b) : 0.f;
    r.channel = b.channel;
    return r;
}

// The table (checked: check_box_args) over a file of `frames` frames.  budget <= 0: the intervals and rows alone (ss_box_plan).
// false: more active-box entries than an int32 counts.
inline bool plan_boxes(int sr, int64_t frames, int ch, const ss_box* boxes, int64_t n, const ss_box_params& prm, int64_t budget, BoxPlan& p) {
    p = BoxPlan();
    const int N = p.N = sep_fft_size(sr), hop = p.hop = N / 4;
    auto first_frame = [&](int64_t a) { return floordiv(a - N / 2, hop) + 1; };
    auto last_frame = [&](int64_t b) { return -floordiv(-(b + N / 2), hop) - 1; };
    // rule 1 per box (silence_ranges' rounding and clamp), the merge of all
    std::vector<ss_region> reg((size_t)n);
    std::vector<int64_t> ka((size_t)n, 0), kb((size_t)n, -1);             // a box's active frames ka .. kb (none: an empty box)
    std::vector<int64_t> at((size_t)n, -1);                               // its first sample
    p.rows.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        reg[i] = ss_region{boxes[i].start, boxes[i].end};
        p.rows[i] = box_row(boxes[i], N, sr, prm.edge_hz);
        const std::vector<int64_t> r = silence_ranges(&reg[i], 1, sr, frames);
        if (r.empty()) continue;
        at[i] = r[0]; ka[i] = first_frame(r[0]); kb[i] = last_frame(r[1]);
    }
    const std::vector<int64_t> iv = silence_ranges(reg.data(), n, sr, frames);
    int64_t last_k = INT64_MIN;
    for (size_t r = 0; r + 1 < iv.size(); r += 2) {
        const ss_box_range g{iv[r], iv[r + 1], first_frame(iv[r]), last_frame(iv[r + 1])};
        p.n_frames += g.stft_last - std::max(g.stft_first, last_k + 1) + 1;
        last_k = g.stft_last;
        p.ranges.push_back(g);
    }
    if (budget <= 0 || p.ranges.empty()) return true;
    // the boxes of every interval, ascending box index
    std::vector<std::vector<int32_t>> members(p.ranges.size());
    for (int64_t i = 0; i < n; ++i) {
        if (at[i] < 0) continue;
        auto it = std::upper_bound(p.ranges.begin(), p.ranges.end(), at[i], [](int64_t v, const ss_box_range& g) { return v < g.frame_begin; });
        members[(size_t)(it - p.ranges.begin()) - 1].push_back((int32_t)i);
    }
    std::vector<int32_t> cand;
    for (size_t r = 0; r < p.ranges.size(); ++r) {
        const ss_box_range& g = p.ranges[r];
        // a frame of this interval may also lie over a box of a neighbour: the intervals whose frames meet this one's
        size_t r0 = r, r1 = r;
        while (r0 > 0 && p.ranges[r0 - 1].stft_last >= g.stft_first) --r0;
        while (r1 + 1 < p.ranges.size() && p.ranges[r1 + 1].stft_first <= g.stft_last) ++r1;
        cand.clear();
        for (size_t t = r0; t <= r1; ++t) cand.insert(cand.end(), members[t].begin(), members[t].end());
        std::sort(cand.begin(), cand.end());
        bool ok = true;
        cut_interval(p, N, hop, budget, g.frame_begin, g.frame_end, [&](int64_t k) {
            BoxFrame f{k, (int32_t)p.idx.size(), 0};
            for (int32_t i : cand)
                if (ka[i] <= k && k <= kb[i]) { p.idx.push_back(i); ++f.count; }
            if (p.idx.size() > (size_t)INT32_MAX / 2) ok = false;
            p.max_count = std::max(p.max_count, f.count);
            p.fr.push_back(f);
        });
        if (!ok) return false;
    }
    finish_cuts(p);
    p.fout_need = p.max_rec * (size_t)((ch + 1) / 2) * N;
    return true;
}

// ---- bands plan: what band_profile_kernel and band_bounds_kernel read -----------------------------------------------
// a round of sep_run_maps: the bins br (ncb of them) under the windows wr, the segments seg0 .. seg0 + nseg - 1 over its maps
struct BandPiece { Ranges br, wr; int64_t ncb = 0; size_t seg0 = 0, nseg = 0; };
struct BandsPlan {
    Ranges rb, un;                                        // rule 1 per region as [first, end); the disjoint union of the non-empty ones
    std::vector<BandPiece> pieces;
    std::vector<BandSeg> segs;                            // in piece order
    std::vector<BandRegion> regs;
    int64_t nseg_total = 0;
};

// The regions over the bins [lo, hi): the union cut at absolute tile boundaries (64 bins) into pieces of at most `budget` bins (a
// tile's share alone may exceed a budget below 64).  caller_maps: the maps hold [lo, hi) already -- one piece, no windows, compact bin
// = bin - lo.  false: too many region tiles.
inline bool plan_bands(const ss_region* regions, int64_t n, int64_t lo, int64_t hi, bool caller_maps, int64_t budget, int64_t W, BandsPlan& p) {
    p = BandsPlan();
    p.rb.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        int64_t b0, cnt;
        region_bins(regions[i].start, regions[i].end, lo, hi, b0, cnt);
        p.rb[i] = {b0, b0 + cnt};
        if (cnt > 0) p.un.emplace_back(b0, b0 + cnt - 1);
    }
    std::sort(p.un.begin(), p.un.end());
    Ranges un;
    for (const auto& u : p.un) join_range(un, u.first, u.second);
    p.un.swap(un);
    struct Chunk { int64_t b0, b1; int piece; int64_t cb0; };       // bins [b0, b1) of one tile, at compact bin cb0 of its piece
    std::vector<Chunk> chunks;
    if (caller_maps) {
        p.pieces.emplace_back();
        p.pieces[0].ncb = hi - lo;
        chunks.push_back(Chunk{lo, hi, 0, 0});
    } else {
        for (const auto& u : p.un)
            for (int64_t b = u.first; b <= u.second;) {
                const int64_t e = std::min(u.second + 1, ((b >> 6) + 1) << 6);
                if (p.pieces.empty() || p.pieces.back().ncb + (e - b) > budget) p.pieces.emplace_back();
                BandPiece& pc = p.pieces.back();
                chunks.push_back(Chunk{b, e, (int)p.pieces.size() - 1, pc.ncb});
                if (!pc.br.empty() && pc.br.back().second + 1 == b) pc.br.back().second = e - 1;
                else pc.br.emplace_back(b, e - 1);
                pc.ncb += e - b;
                b = e;
            }
        for (BandPiece& pc : p.pieces)
            for (const auto& b : pc.br) {
                int64_t w0, w1;
                covering_windows(b.first, b.second, W, w0, w1);
                join_range(pc.wr, w0, w1);
            }
    }
    // segments: region by region, ascending tiles; every one lies inside one chunk's piece
    p.regs.resize((size_t)n);
    std::vector<std::vector<BandSeg>> psegs(p.pieces.size());
    for (int64_t i = 0; i < n; ++i) {
        p.regs[i] = BandRegion{(int32_t)p.nseg_total, 0, (int32_t)(p.rb[i].second - p.rb[i].first), 0};
        for (int64_t b = p.rb[i].first; b < p.rb[i].second;) {
            const int64_t e = std::min(p.rb[i].second, ((b >> 6) + 1) << 6);
            size_t k = 0;
            if (!caller_maps) {
                auto it = std::upper_bound(chunks.begin(), chunks.end(), b, [](int64_t v, const Chunk& ck) { return v < ck.b0; });
                k = (size_t)(it - chunks.begin()) - 1;
            }
            const Chunk& ck = chunks[k];
            psegs[ck.piece].push_back(BandSeg{(int32_t)(ck.cb0 + (b - ck.b0)), (int32_t)(e - b), (int32_t)p.nseg_total, 0});
            ++p.nseg_total; ++p.regs[i].nseg;
            b = e;
        }
        if (p.nseg_total > (int64_t)INT32_MAX / 2) return false;
    }
    p.segs.reserve((size_t)p.nseg_total);
    for (size_t k = 0; k < p.pieces.size(); ++k) {
        p.pieces[k].seg0 = p.segs.size(); p.pieces[k].nseg = psegs[k].size();
        p.segs.insert(p.segs.end(), psegs[k].begin(), psegs[k].end());
    }
    return true;
}

}  // namespace ss
