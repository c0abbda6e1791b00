// The host plan of the band silencer, checked without a device (tests/test_box_plan.py builds this with -fsanitize=address,undefined and
// runs it).  Seeded box tables, recordings and budgets are put through plan_boxes of softspoken_amd/csrc/sep_plan.h and held to a
// brute-force restatement written here: the merged intervals by marking samples, every frame's active boxes by walking the samples of
// its support, the bins of every row by testing each bin, every segment, chunk, record and frame-buffer index the kernels would read.
// The cuts plan_boxes shares with plan_synthesis (cut_interval) are also held to the loop plan_synthesis had before they were shared,
// restated below, on the same inputs.  The library is linked for the rules the plans rest on (silence_ranges, ss_plan_windows,
// ss_resampled_length).
#include "../softspoken_amd/csrc/sep_plan.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>

namespace {

[[noreturn]] void die(const std::string& msg) {
    std::fprintf(stderr, "box_plan_check: FAILED: %s\n", msg.c_str());
    std::exit(1);
}
std::string g_case;
#define REQUIRE(cond, what) do { if (!(cond)) die(std::string(what) + " (" #cond ") in " + g_case); } while (0)

std::vector<std::string> g_order;
std::map<std::string, int64_t> g_count;
void hit(const char* prop, int64_t n = 1) {
    if (!g_count.count(prop)) g_order.push_back(prop);
    g_count[prop] += n;
}

int r_fft_size(int sr) {                                  // the power of two nearest (in log2) to 512 sr / 22050, within 256 .. 8192
    int best = 256; double bd = 1e300;
    for (int n = 256; n <= 8192; n *= 2) {
        const double d = std::fabs(std::log2((double)sr * 512.0 / 22050.0) - std::log2((double)n));
        if (d < bd) { bd = d; best = n; }
    }
    return best;
}

// [a, b) of a box: Python's round of the time x rate (half to even), clamped to the file; b <= a: empty
void r_box_range(const ss_box& bx, int sr, int64_t frames, int64_t& a, int64_t& b) {
    auto py_round = [](double v) { const double f = std::floor(v), d = v - f; return d > 0.5 ? f + 1 : d < 0.5 ? f : (std::fmod(f, 2.0) == 0.0 ? f : f + 1); };
    const double ra = py_round(bx.start * (double)sr), rb = py_round(bx.end * (double)sr);
    a = (int64_t)std::min(std::max(ra, 0.0), (double)frames);
    b = (int64_t)std::min(std::max(rb, 0.0), (double)frames);
}

// plan_synthesis as it stood before cut_interval was shared
ss::SynthPlan old_plan_synthesis(const ss::SepPlan& pl, const std::vector<int64_t>& cbase, int sr, int ch, int64_t budget) {
    using namespace ss;
    SynthPlan p;
    const int N = pl.N, hop = pl.hop;
    const int64_t piece = (budget - 8) * hop;
    for (size_t r = 0; r < pl.ranges.size(); ++r) {
        const auto& g = pl.ranges[r];
        for (int64_t s0 = g.frame_begin; s0 < g.frame_end; s0 += piece) {
            const int64_t s1 = std::min(g.frame_end, s0 + piece);
            const int64_t k0 = floordiv(s0 - N / 2, hop) + 1, k1 = -floordiv(-(s1 + N / 2), hop) - 1;
            if (p.chunks.empty() || (int64_t)(p.fr.size() - p.chunks.back().rec0) + (k1 - k0 + 1) > budget)
                p.chunks.push_back(SepChunk{p.sg.size(), 0, p.fr.size(), 0, 0});
            SepChunk& ck = p.chunks.back();
            p.sg.push_back(SepSeg{g.frame_begin, g.frame_end, s0, s1, k0, (int64_t)(p.fr.size() - ck.rec0), ck.total});
            for (int64_t k = k0; k <= k1; ++k) {
                int64_t j0, j1; double al;
                frame_bins(k, hop, sr, pl.n_bins, j0, j1, al);
                p.fr.push_back(SepFrame{k, (int32_t)(cbase[r] + (j0 - g.bin_first)), (int32_t)(cbase[r] + (j1 - g.bin_first)), (float)al, 0});
            }
            ck.nseg++; ck.nrec = p.fr.size() - ck.rec0; ck.total += s1 - s0;
        }
    }
    for (const SepChunk& ck : p.chunks) p.max_rec = std::max(p.max_rec, ck.nrec);
    p.fout_need = p.max_rec * (size_t)((ch + 1) / 2) * N;
    return p;
}

void check_synthesis_unchanged(int sr, int ch, int64_t frames, const std::vector<ss_box>& boxes, int64_t budget) {
    std::vector<ss_region> regions;
    for (const ss_box& b : boxes) regions.push_back(ss_region{b.start, b.end});
    ss::SepPlan pl;
    ss::separation_plan(sr, frames, regions.data(), (int64_t)regions.size(), pl);
    const ss::SepRanges rg = ss::plan_ranges(pl);
    const ss::SynthPlan a = ss::plan_synthesis(pl, rg.cbase, sr, ch, budget), b = old_plan_synthesis(pl, rg.cbase, sr, ch, budget);
    REQUIRE(a.fr.size() == b.fr.size() && a.sg.size() == b.sg.size() && a.chunks.size() == b.chunks.size(), "synthesis: vector sizes changed");
    REQUIRE(a.n_rec == a.fr.size(), "synthesis: records counted");
    for (size_t i = 0; i < a.fr.size(); ++i)
        REQUIRE(a.fr[i].k == b.fr[i].k && a.fr[i].cb0 == b.fr[i].cb0 && a.fr[i].cb1 == b.fr[i].cb1 && a.fr[i].alpha == b.fr[i].alpha && a.fr[i].pad == 0, "synthesis: a frame changed");
    for (size_t i = 0; i < a.sg.size(); ++i) {
        const ss::SepSeg &x = a.sg[i], &y = b.sg[i];
        REQUIRE(x.a == y.a && x.b == y.b && x.s0 == y.s0 && x.s1 == y.s1 && x.k0 == y.k0 && x.rec0 == y.rec0 && x.out0 == y.out0, "synthesis: a segment changed");
    }
    for (size_t i = 0; i < a.chunks.size(); ++i) {
        const ss::SepChunk &x = a.chunks[i], &y = b.chunks[i];
        REQUIRE(x.seg0 == y.seg0 && x.nseg == y.nseg && x.rec0 == y.rec0 && x.nrec == y.nrec && x.total == y.total, "synthesis: a chunk changed");
    }
    REQUIRE(a.max_rec == b.max_rec && a.fout_need == b.fout_need, "synthesis: buffer sizes changed");
    hit("synthesis: old vectors", (int64_t)(a.fr.size() + a.sg.size() + a.chunks.size()) + 1);
}

void check_boxes(int sr, int ch, int64_t frames, const std::vector<ss_box>& boxes, const ss_box_params& prm, int64_t budget) {
    const int64_t n = (int64_t)boxes.size();
    std::string err;
    REQUIRE(ss::check_box_args(boxes.data(), n, ch, &prm, err) == SS_OK, "a drawn table was refused");
    ss::BoxPlan bp;
    REQUIRE(ss::plan_boxes(sr, frames, ch, boxes.data(), n, prm, budget, bp), "boxes: refused");
    const int N = r_fft_size(sr), hop = N / 4, npairs = (ch + 1) / 2;
    REQUIRE(bp.N == N && bp.hop == hop, "boxes: FFT size");
    // merged intervals: the samples some box covers, in runs
    std::vector<int64_t> a((size_t)n), b((size_t)n);
    std::vector<char> mark((size_t)frames + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        r_box_range(boxes[i], sr, frames, a[i], b[i]);
        for (int64_t s = a[i]; s < b[i]; ++s) mark[(size_t)s] = 1;
    }
    std::vector<std::pair<int64_t, int64_t>> iv;
    for (int64_t s = 0; s < frames; ++s)
        if (mark[(size_t)s]) { if (!iv.empty() && iv.back().second == s) iv.back().second = s + 1; else iv.emplace_back(s, s + 1); }
    REQUIRE(bp.ranges.size() == iv.size(), "boxes: interval count");
    std::map<int64_t, int> frames_seen;
    for (size_t r = 0; r < iv.size(); ++r) {
        const ss_box_range& g = bp.ranges[r];
        REQUIRE(g.frame_begin == iv[r].first && g.frame_end == iv[r].second, "boxes: a merged interval");
        // its frames: those whose support [k hop - N/2, k hop + N/2) meets it
        REQUIRE(g.stft_first * hop + N / 2 > g.frame_begin && (g.stft_first - 1) * hop + N / 2 <= g.frame_begin, "boxes: stft_first");
        REQUIRE(g.stft_last * hop - N / 2 < g.frame_end && (g.stft_last + 1) * hop - N / 2 >= g.frame_end, "boxes: stft_last");
        for (int64_t k = g.stft_first; k <= g.stft_last; ++k) frames_seen[k] = 1;
        hit("boxes: merged intervals and their frames");
    }
    REQUIRE(bp.n_frames == (int64_t)frames_seen.size(), "boxes: n_frames");
    // rows: bin membership by testing every bin against the definition's doubles; the roll-off's distances
    REQUIRE((int64_t)bp.rows.size() == n, "boxes: a row per box");
    for (int64_t i = 0; i < n; ++i) {
        const ss::BoxRow& rw = bp.rows[i];
        const double lo = std::isnan(boxes[i].low_hz) ? 0.0 : boxes[i].low_hz, hi = std::isnan(boxes[i].high_hz) ? INFINITY : boxes[i].high_hz;
        const double lo_b = lo * N / sr, hi_b = hi * N / sr, e_b = prm.edge_hz * N / sr;
        int below = 0, inside = 0;                        // bins under lo_b, bins inside [lo_b, hi_b]
        for (int q = 0; q <= N / 2; ++q) { below += (double)q < lo_b; inside += (double)q >= lo_b && (double)q <= hi_b; }
        REQUIRE(rw.q_lo == below && rw.q_hi == below + inside - 1, "boxes: q_lo / q_hi");
        REQUIRE(rw.q_lo >= 0 && rw.q_lo <= N / 2 + 1 && rw.q_hi >= -1 && rw.q_hi <= N / 2 && rw.q_lo <= rw.q_hi + 1, "boxes: q_lo / q_hi outside their clamps");
        for (int q = 0; q <= N / 2; ++q) {                // the distance the kernel forms, against the definition's
            if (q >= rw.q_lo && q <= rw.q_hi) continue;
            const double d = q < rw.q_lo ? lo_b - q : q - hi_b;
            const double dk = q < rw.q_lo ? (double)(rw.q_lo - q) - (double)rw.lo_f : (double)(q - rw.q_hi) - (double)rw.hi_f;
            if (std::isfinite(d)) REQUIRE(d > 0.0 && std::fabs(dk - d) <= 1.2e-7 * std::max(1.0, std::fabs(d)), "boxes: a roll-off distance");
            else REQUIRE(dk == d, "boxes: an infinite roll-off distance");
        }
        REQUIRE(rw.channel == boxes[i].channel, "boxes: a row's channel");
        REQUIRE(e_b > 0.0 ? std::fabs((double)rw.inv_e * e_b - 1.0) <= 1e-6 : rw.inv_e == 0.f, "boxes: inv_e");
        hit("boxes: rows");
    }
    if (iv.empty()) { REQUIRE(bp.fr.empty() && bp.sg.empty() && bp.chunks.empty() && bp.idx.empty(), "boxes: work without an interval"); hit("boxes: nothing without an interval"); return; }
    // chunks, segments, records: plan_synthesis' properties
    REQUIRE(bp.n_rec == bp.fr.size(), "boxes: records counted");
    size_t seg_at = 0, rec_at = 0;
    for (const ss::SepChunk& ck : bp.chunks) {
        REQUIRE(ck.seg0 == seg_at && ck.rec0 == rec_at && ck.nseg > 0, "boxes: chunk table not consecutive");
        REQUIRE((int64_t)ck.nrec <= budget && ck.nrec <= bp.max_rec, "boxes: a chunk over the budget");
        hit("boxes: chunk within budget");
        int64_t out0 = 0, rec0 = 0;
        for (size_t s = ck.seg0; s < ck.seg0 + ck.nseg; ++s) {
            const ss::SepSeg& g = bp.sg[s];
            REQUIRE(g.out0 == out0 && g.rec0 == rec0, "boxes: out0 / rec0 do not ascend from 0");
            REQUIRE(g.s1 - g.s0 <= (budget - 8) * hop && g.s1 > g.s0, "boxes: a segment longer than (budget - 8) hop");
            out0 += g.s1 - g.s0;
            int64_t k = g.k0;
            REQUIRE(k * hop + N / 2 > g.s0 && (k - 1) * hop + N / 2 <= g.s0, "boxes: k0 is not the first frame over the segment");
            while (k * hop - N / 2 < g.s1) { ++k; ++rec0; }
            REQUIRE((size_t)rec0 <= ck.nrec, "boxes: a segment's frames past the chunk's records");
            // the blend's reads, every sample: frames kb - 1 .. kb + 2 at position n - k hop + N / 2
            for (int64_t s2 = g.s0; s2 < g.s1; ++s2) {
                const int64_t kb = s2 / hop;
                for (int64_t kk = kb - 1; kk <= kb + 2; ++kk) {
                    const int64_t rec = g.rec0 + (kk - g.k0), pos = s2 - kk * hop + N / 2;
                    REQUIRE(rec >= 0 && rec < (int64_t)ck.nrec && pos >= 0 && pos < N, "blend: a read outside the chunk's records");
                    REQUIRE(bp.fr[ck.rec0 + (size_t)rec].k == kk, "blend: the record is another frame's");
                    REQUIRE(((size_t)rec * npairs + (npairs - 1)) * N + (size_t)pos < bp.fout_need, "blend: a read past the frame buffer");
                }
            }
            hit("blend: reads inside the chunk's records", g.s1 - g.s0);
        }
        REQUIRE(out0 == ck.total && (size_t)rec0 == ck.nrec, "boxes: total / nrec");
        hit("boxes: segments of a chunk");
        seg_at += ck.nseg; rec_at += ck.nrec;
    }
    REQUIRE(seg_at == bp.sg.size() && rec_at == bp.fr.size(), "boxes: segments or frames outside every chunk");
    REQUIRE(bp.fout_need == bp.max_rec * (size_t)npairs * N, "boxes: frame buffer size");
    size_t s = 0;
    for (size_t r = 0; r < iv.size(); ++r) {
        int64_t at = iv[r].first;
        while (s < bp.sg.size() && at < iv[r].second) {
            REQUIRE(bp.sg[s].a == iv[r].first && bp.sg[s].b == iv[r].second && bp.sg[s].s0 == at, "boxes: segments do not partition the interval");
            at = bp.sg[s].s1; ++s;
        }
        REQUIRE(at == iv[r].second, "boxes: segments do not end at the interval's end");
        hit("boxes: segments partition the interval");
    }
    REQUIRE(s == bp.sg.size(), "boxes: segments beyond the intervals");
    // every record's active boxes: box i is active at k when a sample of the support lies in [a_i, b_i) -- walked sample by sample
    int32_t max_count = 0;
    for (const ss::BoxFrame& f : bp.fr) {
        REQUIRE(f.first >= 0 && f.count >= 1 && (size_t)f.first + (size_t)f.count <= bp.idx.size(), "boxes: a frame's index range");
        std::vector<int32_t> want;
        for (int64_t i = 0; i < n; ++i) {
            bool active = false;
            for (int64_t t = f.k * hop - N / 2; t < f.k * hop + N / 2 && !active; ++t) active = t >= a[i] && t < b[i];
            if (active) want.push_back((int32_t)i);
        }
        REQUIRE(std::vector<int32_t>(bp.idx.begin() + f.first, bp.idx.begin() + f.first + f.count) == want, "boxes: a frame's active boxes");
        max_count = std::max(max_count, f.count);
        hit("boxes: active boxes of a frame");
    }
    REQUIRE(bp.max_count == max_count, "boxes: max_count");
}

// 0 to 6 boxes over `dur` seconds: empty ones, touching and overlapping ones, ones before 0 and past the end, single samples; bands with
// NaN edges, below one bin, past Nyquist; channels -1 .. ch - 1
std::vector<ss_box> draw_boxes(std::mt19937_64& rng, double dur, int sr, int ch) {
    auto u = [&](double lo, double hi) { return lo + (hi - lo) * (double)(rng() % 1000001) / 1e6; };
    std::vector<ss_box> r;
    const int n = (int)(rng() % 7);
    for (int i = 0; i < n; ++i) {
        double a = u(-0.2 * dur - 0.01, 1.1 * dur + 0.01), len = u(0.0, 0.3 * dur + 0.01);
        switch (rng() % 8) {
            case 0: len = 0.0; break;
            case 1: if (!r.empty()) a = r.back().end; break;
            case 2: if (!r.empty()) a = u(r.back().start, r.back().end); break;
            case 3: a = u(-0.5, -0.01); len = u(0.0, 0.6); break;
            case 4: a = u(0.5 * dur, dur + 0.02); len = dur + 1.0; break;
            case 5: len = 1.0 / sr; break;
            default: break;
        }
        double lo = u(0.0, 0.3 * sr), hi = lo + u(0.0, 0.3 * sr);
        switch (rng() % 8) {
            case 0: lo = NAN; hi = NAN; break;
            case 1: lo = NAN; break;
            case 2: hi = NAN; break;
            case 3: hi = lo + u(0.0, 0.5 * sr / 8192.0); break;         // narrower than a bin of any N
            case 4: lo = 0.0; hi = (double)sr; break;
            case 5: lo = u(0.5 * sr, sr); hi = lo + 10.0; break;        // above Nyquist
            case 6: lo = -u(0.0, 100.0); hi = u(0.0, 0.3 * sr); break;
            default: break;
        }
        r.push_back(ss_box{a, a + len, lo, hi, (int32_t)(rng() % (uint64_t)(ch + 1)) - 1, 0});
    }
    return r;
}

}  // namespace

int main() {
    const int rates[8] = {8000, 16000, 22050, 44100, 48000, 96000, 192000, 384000};
    const int64_t budgets[4] = {16, 17, 23, 64};
    const double edges[4] = {0.0, 100.0, 100.0, 2500.0};
    std::mt19937_64 rng(20261021);
    int64_t cases = 0;
    for (int round = 0; round < 12; ++round)
        for (int ri = 0; ri < 8; ++ri)
            for (int bi = 0; bi < 4; ++bi) {
                const int sr = rates[ri], ch = 1 + (int)(rng() % 5);
                const int N = r_fft_size(sr);
                int64_t frames;
                switch (rng() % 8) {
                    case 0: frames = 0; break;
                    case 1: frames = 1 + (int64_t)(rng() % (uint64_t)N); break;          // shorter than an FFT
                    default: frames = (int64_t)(rng() % (uint64_t)(60 * N)); break;      // up to 240 hops
                }
                const double dur = (double)frames / sr;
                const std::vector<ss_box> boxes = draw_boxes(rng, dur, sr, ch);
                const ss_box_params prm{0.01, 0.0, edges[rng() % 4]};
                g_case = "case " + std::to_string(cases) + " (sr " + std::to_string(sr) + ", ch " + std::to_string(ch) + ", frames " + std::to_string(frames) +
                         ", budget " + std::to_string(budgets[bi]) + ", " + std::to_string(boxes.size()) + " boxes)";
                check_boxes(sr, ch, frames, boxes, prm, budgets[bi]);
                check_synthesis_unchanged(sr, ch, frames, boxes, budgets[bi]);
                ++cases;
            }
    std::printf("cases %lld\n", (long long)cases);
    for (const std::string& k : g_order) std::printf("  %-48s %lld\n", k.c_str(), (long long)g_count[k]);
    std::printf("box_plan_check: ok\n");
    return 0;
}
