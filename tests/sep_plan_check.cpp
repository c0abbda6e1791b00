// The host plan of the separation silencer and the region bands, checked without a device (tests/test_sep_plan.py builds this with
// -fsanitize=address,undefined and runs it).  Seeded recordings, region tables and budgets are put through the plans of
// softspoken_amd/csrc/sep_plan.h -- plan_maps, plan_synthesis, plan_bands -- and every index a kernel would read is held to a
// brute-force restatement written here: exact integers and loops over all windows, bins and samples, none of the header's own rules
// (window starts, frame bins, covering windows, the geometry and the cuts are restated below).  The library is linked for the rules the
// plans rest on and other tests hold: ss_plan_windows, ss_resampled_length, silence_ranges and rule 1 (region_bins).
#include "../softspoken_amd/csrc/sep_plan.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>

namespace {

typedef std::vector<std::pair<int64_t, int64_t>> Rg;      // inclusive ranges

[[noreturn]] void die(const std::string& msg) {
    std::fprintf(stderr, "sep_plan_check: FAILED: %s\n", msg.c_str());
    std::exit(1);
}
std::string g_case;                                       // the case being checked, for a failure's message
#define REQUIRE(cond, what) do { if (!(cond)) die(std::string(what) + " (" #cond ") in " + g_case); } while (0)

std::vector<std::string> g_order;
std::map<std::string, int64_t> g_count;                   // checks made, by property
void hit(const char* prop, int64_t n = 1) {
    if (!g_count.count(prop)) g_order.push_back(prop);
    g_count[prop] += n;
}

// ---- restated rules ------------------------------------------------------------------------------------------------------------
int64_t r_win_start(int64_t i) { return (256 * i + 2) / 5; }       // round(51.2 i): 256 i / 5 has no fraction of one half

int r_fft_size(int sr) {                                  // the power of two nearest (in log2) to 512 sr / 22050, within 256 .. 8192
    int best = 256; double bd = 1e300;
    for (int n = 256; n <= 8192; n *= 2) {
        const double d = std::fabs(std::log2((double)sr * 512.0 / 22050.0) - std::log2((double)n));
        if (d < bd) { bd = d; best = n; }
    }
    return best;
}

// Windows and covered bins of a recording, by counting: the planned windows that lie inside the padded signal, and the bins of the
// padded signal's round(n_padded / 22050 * 256 / 3) that lie under one of them.
void r_geometry(int sr, int64_t frames, int64_t& W, int64_t& n_bins) {
    const int64_t n_padded = ss_resampled_length(frames, sr) + 2 * (int64_t)SS_WINDOW_SAMPLES;
    const int64_t planned = ss_plan_windows((double)frames / (double)sr, nullptr, 0);
    W = 0;
    for (int64_t i = 0; i < planned; ++i) if (i * (int64_t)SS_STEP_SAMPLES + SS_WINDOW_SAMPLES <= n_padded) ++W;
    const int64_t nb = (int64_t)std::llround((long double)n_padded * 256.0L / (22050.0L * 3.0L));
    n_bins = 0;
    for (int64_t j = 0; j < nb; ++j) {
        bool covered = false;
        for (int64_t i = 0; i < W && !covered; ++i) covered = r_win_start(i) <= j && j < r_win_start(i) + 256;
        n_bins += covered;
    }
}

// Frame k's time k hop / sr against the bin centres (j + 0.5) 3 / 256 - 3 s, in integers: centre(j) <= t <=> (2 j + 1) 3 sr <= 512 (k hop
// + 3 sr).  j0: the last such bin, found by stepping; the weight of bin j0 + 1: (t - centre(j0)) / (3 / 256).
void r_frame_bins(int64_t k, int hop, int sr, int64_t n_bins, int64_t& j0, int64_t& j1, float& alpha) {
    const __int128 T = (__int128)512 * (k * (int64_t)hop + 3 * (int64_t)sr);
    auto at_or_before = [&](int64_t j) { return (__int128)(2 * j + 1) * 3 * sr <= T; };
    int64_t j = (int64_t)std::floor(((double)k * hop / sr + 3.0) * 256.0 / 3.0 - 0.5);
    while (at_or_before(j + 1)) ++j;
    while (!at_or_before(j)) --j;
    if (j < 0) { j0 = j1 = 0; alpha = 0.f; return; }
    if (j >= n_bins - 1) { j0 = j1 = n_bins - 1; alpha = 0.f; return; }
    j0 = j; j1 = j + 1;
    alpha = (float)((double)(int64_t)(T - (__int128)(2 * j + 1) * 3 * sr) / (double)(6 * (int64_t)sr));
}

int64_t count_bins(const Rg& r) { int64_t n = 0; for (auto& x : r) n += x.second - x.first + 1; return n; }

// ---- maps plan -----------------------------------------------------------------------------------------------------------------
void check_maps(const Rg& br, const Rg& wr, int64_t W, int nsig, std::mt19937_64& rng, std::vector<int32_t>* cbin_out = nullptr) {
    std::vector<int64_t> sig_off;
    for (int s = 0; s < nsig; ++s) sig_off.push_back((int64_t)(rng() % 1000000) * 64);
    ss::MapsPlan m;
    REQUIRE(ss::plan_maps(br, wr, W, nsig, sig_off.data(), m), "maps: refused");
    // cbin: strictly ascending, the union of the ranges' bins
    std::vector<int32_t> want;
    for (size_t i = 0; i < br.size(); ++i) {
        REQUIRE(br[i].first <= br[i].second && (i == 0 || br[i].first > br[i - 1].second), "maps: bin ranges not ascending");
        for (int64_t j = br[i].first; j <= br[i].second; ++j) want.push_back((int32_t)j);
    }
    REQUIRE(m.cbin == want && m.ncb == (int)want.size(), "maps: cbin is not the union of the ranges' bins");
    for (size_t i = 1; i < m.cbin.size(); ++i) REQUIRE(m.cbin[i] > m.cbin[i - 1], "maps: cbin not strictly ascending");
    hit("maps: cbin ascending union", (int64_t)m.cbin.size());
    // every window over a bin of cbin has a slot
    REQUIRE((int64_t)m.slot.size() == W, "maps: slot table size");
    int64_t covering = 0;
    for (int32_t j : m.cbin)
        for (int64_t i = 0; i < W; ++i)
            if (r_win_start(i) <= j && j < r_win_start(i) + 256) { REQUIRE(m.slot[(size_t)i] >= 0, "maps: a window over a bin has no slot"); ++covering; }
    hit("maps: covering window has a slot", covering);
    // slots 0 .. nw - 1 in ascending window order
    int32_t t = 0;
    for (int64_t i = 0; i < W; ++i) if (m.slot[(size_t)i] >= 0) { REQUIRE(m.slot[(size_t)i] == t, "maps: slots not 0 .. nw - 1 ascending"); ++t; }
    REQUIRE(t == m.nw, "maps: nw");
    hit("maps: slots ascending", m.nw);
    // the run list: signal s's windows behind signal s - 1's
    REQUIRE((int64_t)m.off.size() == (int64_t)nsig * m.nw, "maps: run list length");
    for (int s = 0; s < nsig; ++s)
        for (int64_t i = 0; i < W; ++i)
            if (m.slot[(size_t)i] >= 0) {
                REQUIRE(m.off[(size_t)s * m.nw + m.slot[(size_t)i]] == sig_off[s] + i * (int64_t)SS_STEP_SAMPLES, "maps: window offset");
            }
    hit("maps: window offsets", (int64_t)m.off.size());
    if (cbin_out) *cbin_out = m.cbin;
}

// ---- synthesis plan ------------------------------------------------------------------------------------------------------------
void check_synthesis(int sr, int ch, int64_t frames, const std::vector<ss_region>& regions, int64_t budget, std::mt19937_64& rng) {
    ss::SepPlan pl;
    ss::separation_plan(sr, frames, regions.data(), (int64_t)regions.size(), pl);
    int64_t W, n_bins;
    r_geometry(sr, frames, W, n_bins);
    const int N = r_fft_size(sr), hop = N / 4, npairs = (ch + 1) / 2;
    REQUIRE(pl.N == N && pl.hop == hop && pl.W == W && pl.n_bins == n_bins, "plan: FFT size or file geometry");
    hit("plan: FFT size and geometry");
    const std::vector<int64_t> iv = ss::silence_ranges(regions.data(), (int64_t)regions.size(), sr, frames);
    REQUIRE(pl.ranges.size() * 2 == iv.size(), "plan: interval count");
    const ss::SepRanges rg = ss::plan_ranges(pl);
    const ss::SynthPlan sp = ss::plan_synthesis(pl, rg.cbase, sr, ch, budget);
    REQUIRE(rg.cbase.size() == pl.ranges.size(), "synthesis: cbase per interval");
    if (pl.ranges.empty()) { REQUIRE(sp.fr.empty() && sp.sg.empty() && sp.chunks.empty(), "synthesis: work without an interval"); hit("synthesis: nothing without an interval"); return; }
    std::vector<int32_t> cbin;
    check_maps(rg.br, rg.wr, W, 1 + (int)(rng() % 3), rng, &cbin);
    const int64_t ncb = (int64_t)cbin.size();
    REQUIRE(ncb == count_bins(rg.br), "synthesis: ncb");
    // chunks: consecutive segments and records, at most `budget` frames, out0 from 0, lengths add up to total
    size_t seg_at = 0, rec_at = 0;
    for (const ss::SepChunk& ck : sp.chunks) {
        REQUIRE(ck.seg0 == seg_at && ck.rec0 == rec_at && ck.nseg > 0, "synthesis: chunk table not consecutive");
        REQUIRE((int64_t)ck.nrec <= budget, "synthesis: a chunk holds more than the budget's frames");
        REQUIRE(ck.nrec <= sp.max_rec, "synthesis: max_rec");
        hit("synthesis: chunk within budget");
        int64_t out0 = 0, rec0 = 0;
        for (size_t s = ck.seg0; s < ck.seg0 + ck.nseg; ++s) {
            const ss::SepSeg& g = sp.sg[s];
            REQUIRE(g.out0 == out0 && g.rec0 == rec0, "synthesis: out0 / rec0 do not ascend from 0");
            REQUIRE(g.s1 - g.s0 <= (budget - 8) * hop && g.s1 > g.s0, "synthesis: a segment longer than (budget - 8) hop");
            hit("synthesis: segment length");
            out0 += g.s1 - g.s0;
            // the segment's frames: every frame that overlaps [s0, s1) -- k hop - N / 2 < s1 and k hop + N / 2 > s0
            int64_t k = g.k0, nk = 0;
            REQUIRE(k * hop + N / 2 > g.s0 && (k - 1) * hop + N / 2 <= g.s0, "synthesis: k0 is not the first frame over the segment");
            while (k * hop - N / 2 < g.s1) { ++k; ++nk; }
            rec0 += nk;
            REQUIRE((size_t)rec0 <= ck.nrec, "synthesis: a segment's frames past the chunk's records");
        }
        REQUIRE(out0 == ck.total && (size_t)rec0 == ck.nrec, "synthesis: total / nrec");
        hit("synthesis: out0 ascends, lengths add up");
        seg_at += ck.nseg; rec_at += ck.nrec;
    }
    REQUIRE(seg_at == sp.sg.size() && rec_at == sp.fr.size(), "synthesis: segments or frames outside every chunk");
    REQUIRE(sp.fout_need == sp.max_rec * (size_t)npairs * N, "synthesis: frame buffer size");
    // the segments of an interval partition it, in ascending order
    size_t s = 0;
    for (size_t r = 0; r < pl.ranges.size(); ++r) {
        const int64_t a = iv[2 * r], b = iv[2 * r + 1];
        REQUIRE(pl.ranges[r].frame_begin == a && pl.ranges[r].frame_end == b, "plan: interval");
        int64_t at = a;
        while (s < sp.sg.size() && at < b) {
            REQUIRE(sp.sg[s].a == a && sp.sg[s].b == b && sp.sg[s].s0 == at, "synthesis: segments do not partition the interval");
            at = sp.sg[s].s1; ++s;
        }
        REQUIRE(at == b, "synthesis: segments do not end at the interval's end");
        hit("synthesis: segments partition the interval");
    }
    REQUIRE(s == sp.sg.size(), "synthesis: segments beyond the intervals");
    // every frame: its gain rows lie in the table and are the rows of the two bins around its time
    for (const ss::SepFrame& f : sp.fr) {
        REQUIRE(f.cb0 >= 0 && f.cb0 < ncb && f.cb1 >= 0 && f.cb1 < ncb, "synthesis: a gain row outside [0, ncb)");
        int64_t j0, j1; float al;
        r_frame_bins(f.k, hop, sr, n_bins, j0, j1, al);
        REQUIRE(cbin[(size_t)f.cb0] == j0 && cbin[(size_t)f.cb1] == j1 && f.alpha == al, "synthesis: a frame's bins or weight");
    }
    hit("synthesis: gain rows inside the table", (int64_t)sp.fr.size());
    hit("synthesis: frame bins and weight", (int64_t)sp.fr.size());
    // the blend's reads: sample n of a segment reads frames kb - 1 .. kb + 2 (kb = n / hop) at position n - k hop + N / 2.  Every sample
    // of the case when there are few; otherwise the first and last sample of every hop block (records and positions are monotonic in n
    // inside a block)
    int64_t erased = 0, reads = 0;
    for (const ss::SepSeg& g : sp.sg) erased += g.s1 - g.s0;
    const bool all_samples = erased <= 400000;
    for (const ss::SepChunk& ck : sp.chunks)
        for (size_t q = ck.seg0; q < ck.seg0 + ck.nseg; ++q) {
            const ss::SepSeg& g = sp.sg[q];
            auto sample = [&](int64_t n) {
                const int64_t kb = n / hop;
                for (int64_t k = kb - 1; k <= kb + 2; ++k) {
                    const int64_t rec = g.rec0 + (k - g.k0), pos = n - k * hop + N / 2;
                    REQUIRE(rec >= 0 && rec < (int64_t)ck.nrec, "blend: a record outside the chunk");
                    REQUIRE(pos >= 0 && pos < N, "blend: a position outside the frame");
                    REQUIRE(sp.fr[ck.rec0 + (size_t)rec].k == k, "blend: the record is another frame's");
                    REQUIRE(((size_t)rec * npairs + (npairs - 1)) * N + (size_t)pos < sp.fout_need, "blend: a read past the frame buffer");
                }
                ++reads;
            };
            if (all_samples) for (int64_t n = g.s0; n < g.s1; ++n) sample(n);
            else
                for (int64_t n = g.s0; n < g.s1;) {
                    const int64_t e = std::min(g.s1, (n / hop + 1) * hop);
                    sample(n); sample(e - 1);
                    n = e;
                }
        }
    hit("blend: reads inside the chunk's records", reads);
}

// ---- bands plan ----------------------------------------------------------------------------------------------------------------
void check_bands(const std::vector<ss_region>& regions, int64_t lo, int64_t hi, bool caller_maps, int64_t budget, int64_t W, std::mt19937_64& rng) {
    const int64_t n = (int64_t)regions.size();
    ss::BandsPlan bp;
    REQUIRE(ss::plan_bands(regions.data(), n, lo, hi, caller_maps, budget, W, bp), "bands: refused");
    REQUIRE((int64_t)bp.rb.size() == n && (int64_t)bp.regs.size() == n, "bands: tables per region");
    // rule 1 per region; the union by marking bins
    std::vector<char> mark((size_t)std::max<int64_t>(hi - lo, 0), 0);
    for (int64_t i = 0; i < n; ++i) {
        int64_t b0, cnt;
        ss::region_bins(regions[i].start, regions[i].end, lo, hi, b0, cnt);
        REQUIRE(bp.rb[i].first == b0 && bp.rb[i].second == b0 + cnt && bp.regs[i].n_bins == cnt, "bands: a region's bin range");
        for (int64_t j = b0; j < b0 + cnt; ++j) mark[(size_t)(j - lo)] = 1;
    }
    Rg un;
    for (int64_t j = lo; j < hi; ++j)
        if (mark[(size_t)(j - lo)]) { if (!un.empty() && un.back().second + 1 == j) un.back().second = j; else un.emplace_back(j, j); }
    REQUIRE(bp.un == un, "bands: the disjoint union");
    hit("bands: region ranges and union", n);
    // pieces: consistent seg0 / nseg; their bins are the union's, each once, ascending; within the budget unless one tile's share
    std::vector<std::vector<int32_t>> cb(bp.pieces.size());
    std::vector<int32_t> all;
    size_t seg_at = 0;
    for (size_t k = 0; k < bp.pieces.size(); ++k) {
        const ss::BandPiece& pc = bp.pieces[k];
        REQUIRE(pc.seg0 == seg_at && pc.seg0 + pc.nseg <= bp.segs.size(), "bands: a piece's seg0 / nseg");
        seg_at += pc.nseg;
        if (caller_maps) {
            REQUIRE(bp.pieces.size() == 1 && pc.ncb == hi - lo && pc.br.empty() && pc.wr.empty(), "bands: the caller's maps are one piece");
            for (int64_t j = lo; j < hi; ++j) cb[k].push_back((int32_t)j);
            hit("bands: caller's maps are one piece");
            continue;
        }
        check_maps(pc.br, pc.wr, W, 1 + (int)(rng() % 2), rng, &cb[k]);
        REQUIRE((int64_t)cb[k].size() == pc.ncb && pc.ncb > 0 && pc.nseg > 0, "bands: a piece's ncb");
        const bool one_tile = (cb[k].front() >> 6) == (cb[k].back() >> 6);
        REQUIRE(pc.ncb <= budget || one_tile, "bands: a piece over the budget");
        hit("bands: piece within budget");
        all.insert(all.end(), cb[k].begin(), cb[k].end());
    }
    REQUIRE(seg_at == bp.segs.size() && (int64_t)bp.segs.size() == bp.nseg_total, "bands: segments outside every piece");
    hit("bands: seg0 / nseg of the pieces");
    if (!caller_maps) {
        std::vector<int32_t> want;
        for (auto& u : un) for (int64_t j = u.first; j <= u.second; ++j) want.push_back((int32_t)j);
        REQUIRE(all == want, "bands: the pieces' bins are not the union's");
        hit("bands: pieces hold the union once");
    }
    // segments: inside their piece; absolute bins from the piece's compact bins; out indices 0 .. nseg_total - 1 once
    std::vector<int64_t> abs0((size_t)bp.nseg_total, -1), len((size_t)bp.nseg_total, 0);
    for (size_t k = 0; k < bp.pieces.size(); ++k)
        for (size_t q = bp.pieces[k].seg0; q < bp.pieces[k].seg0 + bp.pieces[k].nseg; ++q) {
            const ss::BandSeg& g = bp.segs[q];
            REQUIRE(g.cb0 >= 0 && g.n >= 1 && g.n <= 64 && (int64_t)g.cb0 + g.n <= bp.pieces[k].ncb, "bands: a segment outside its piece");
            for (int t = 1; t < g.n; ++t) REQUIRE(cb[k][(size_t)(g.cb0 + t)] == cb[k][(size_t)g.cb0] + t, "bands: a segment's compact bins are not consecutive bins");
            if (caller_maps) { REQUIRE(cb[k][(size_t)g.cb0] - lo == g.cb0, "bands: compact bin is not bin - first_bin"); hit("bands: caller's maps compact bin"); }
            REQUIRE(g.out >= 0 && g.out < bp.nseg_total && abs0[(size_t)g.out] < 0, "bands: an out index outside 0 .. nseg_total - 1 or used twice");
            abs0[(size_t)g.out] = cb[k][(size_t)g.cb0]; len[(size_t)g.out] = g.n;
            hit("bands: segment inside its piece");
        }
    for (int64_t o = 0; o < bp.nseg_total; ++o) REQUIRE(abs0[(size_t)o] >= 0, "bands: an out index not used");
    hit("bands: out indices each once", bp.nseg_total);
    // a region's segments tile its range in ascending 64-aligned tiles
    int64_t seg0 = 0;
    for (int64_t i = 0; i < n; ++i) {
        const ss::BandRegion& rg = bp.regs[i];
        REQUIRE(rg.seg0 == seg0 && rg.nseg >= 0, "bands: a region's seg0");
        int64_t at = bp.rb[i].first;
        for (int64_t o = rg.seg0; o < rg.seg0 + rg.nseg; ++o) {
            REQUIRE(abs0[(size_t)o] == at, "bands: a region's tiles are not consecutive");
            const int64_t e = at + len[(size_t)o];
            REQUIRE((at >> 6) == ((e - 1) >> 6), "bands: a segment across a tile boundary");
            REQUIRE(e == bp.rb[i].second || (e & 63) == 0, "bands: a segment ends inside a tile before the region does");
            at = e;
            hit("bands: tiles ascending and aligned");
        }
        REQUIRE(at == bp.rb[i].second, "bands: a region's tiles do not reach its end");
        seg0 += rg.nseg;
    }
    REQUIRE(seg0 == bp.nseg_total, "bands: nseg_total");
    hit("bands: seg0 / nseg of the regions", n);
}

// ---- cases ---------------------------------------------------------------------------------------------------------------------
// 0 to 6 regions over a recording of `dur` seconds: empty ones, ones that touch or overlap the one before, ones before 0 and past the end
std::vector<ss_region> draw_regions(std::mt19937_64& rng, double dur) {
    auto u = [&](double a, double b) { return a + (b - a) * (double)(rng() % 1000001) / 1e6; };
    std::vector<ss_region> r;
    const int n = (int)(rng() % 7);
    for (int i = 0; i < n; ++i) {
        double a = u(-0.2 * dur - 0.5, 1.1 * dur + 0.5), len = u(0.0, 0.3 * dur + 0.3);
        switch (rng() % 8) {
            case 0: len = 0.0; break;                                         // empty
            case 1: if (!r.empty()) a = r.back().end; break;                  // touches the one before
            case 2: if (!r.empty()) a = u(r.back().start, r.back().end); break;   // overlaps it
            case 3: a = u(-2.0, -0.1); len = u(0.0, 1.0); break;              // before 0 (ends before or after it)
            case 4: a = u(0.5 * dur, dur + 0.2); len = dur + 1.0; break;      // past the end
            case 5: len = u(0.0, 0.002); break;                               // a few samples
            default: break;
        }
        r.push_back(ss_region{a, a + len});
    }
    return r;
}

}  // namespace

int main() {
    const int rates[8] = {8000, 16000, 22050, 44100, 48000, 96000, 192000, 384000};
    const int64_t band_budgets[5] = {64, 65, 128, 200, 16384};
    std::mt19937_64 rng(20261021);
    int64_t cases = 0;
    for (int round = 0; round < 64; ++round)
        for (int ri = 0; ri < 8; ++ri) {
            const int sr = rates[ri], ch = 1 + (int)(rng() % 5);
            double dur;
            switch (rng() % 10) {
                case 0: dur = 0.0; break;
                case 1: case 2: dur = (double)(rng() % 40001) / 1000.0; break;                     // up to 40 s
                case 3: dur = (double)(1 + rng() % 2000) / (double)sr; break;                      // shorter than a few FFTs
                default: dur = (double)(rng() % 4001) / 1000.0; break;
            }
            if (round == 0) dur = 40.0;
            const int64_t frames = (int64_t)std::floor(dur * sr);
            const std::vector<ss_region> regions = draw_regions(rng, dur);
            const int N = r_fft_size(sr), npairs = (ch + 1) / 2;
            const int64_t dflt = std::max<int64_t>(16, (int64_t)(((size_t)256 << 20) / ((size_t)npairs * N * 8)));
            const int64_t budget = rng() % 4 == 0 ? dflt : 16 + (int64_t)(rng() % 25);
            g_case = "synthesis case " + std::to_string(cases) + " (sr " + std::to_string(sr) + ", ch " + std::to_string(ch) + ", frames " + std::to_string(frames) +
                     ", budget " + std::to_string(budget) + ", " + std::to_string(regions.size()) + " regions)";
            check_synthesis(sr, ch, frames, regions, budget, rng);
            // the bands over the same recording's bins, and over a caller's maps of a stretch of bins
            int64_t W, n_bins;
            r_geometry(sr, frames, W, n_bins);
            const int64_t bb = band_budgets[rng() % 5];
            g_case = "bands case " + std::to_string(cases) + " (bins " + std::to_string(n_bins) + ", budget " + std::to_string(bb) + ", " + std::to_string(regions.size()) + " regions)";
            check_bands(regions, 0, n_bins, false, bb, W, rng);
            const int64_t first = (int64_t)(rng() % 300), nb = 1 + (int64_t)(rng() % 700);
            g_case = "bands-from-maps case " + std::to_string(cases) + " (bins [" + std::to_string(first) + ", " + std::to_string(first + nb) + "))";
            check_bands(regions, first, first + nb, true, bb, 0, rng);
            ++cases;
        }
    std::printf("cases %lld\n", (long long)cases);
    for (const std::string& k : g_order) std::printf("  %-48s %lld\n", k.c_str(), (long long)g_count[k]);
    std::printf("sep_plan_check: ok\n");
    return 0;
}
