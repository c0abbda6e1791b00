// The host plan of PCM ingest, checked without a device (tests/test_ingest_plan.py builds this with -fsanitize=address,undefined and runs
// it).  Seeded batches are put through plan_ingest of softspoken_amd/csrc/ingest_plan.h, and every range a kernel would address through
// the plan's descriptors and geometries is held to a restatement written here: the slot rule as the sequential walk it replaced, the
// kernels' own index arithmetic (ingest.hip) as loops over threads, phases, taps and outputs.  The library is linked for
// ss_resampled_length, which other tests hold.
//   ingest_plan_check [DIR]     DIR: the tap table of every rate of the list is written there as taps_<rate>.f32 for the test to hash
#include "../softspoken_amd/csrc/ingest_plan.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <string>

namespace {

using namespace ss;

[[noreturn]] void die(const std::string& msg) {
    std::fprintf(stderr, "ingest_plan_check: FAILED: %s\n", msg.c_str());
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

const int kRates[] = {8000, 11025, 16000, 22050, 32000, 44100, 48000, 88200, 96000, 192000, 768000, 48001};
const int kChannels[] = {1, 2, 3, 5, 64};
const int64_t W = SS_WINDOW_SAMPLES;
const size_t kLds = 160 * 1024;

int r_gcd(int a, int b) { return b ? r_gcd(b, a % b) : a; }

// ---- the fused form, restated from the kernels -------------------------------------------------------------------------------------
int r_res3_slot(int k, int c) {                           // lane of position c in LDS service group k ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31})
    static const int even[16] = {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27};
    static const int odd[16] = {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31};
    return 32 * (k / 2) + (k % 2 ? odd[c] : even[c]);
}

// does the fused form apply: the conditions of the route, without the geometry's own walk
bool r_fused_applies(int L, int M, int half) {
    const int nt = 2 * half;
    if (L > 1024 || nt > M) return false;
    const int groups = 1024 / L, R = 4 * groups;
    if ((int64_t)R * M + M + nt > 9 * 1024) return false;
    int pv = R + 2;
    while (pv % 4 || (pv / 4) % 2 == 0) ++pv;
    std::map<int, int> cls;
    int nsg = 0;
    for (int p = 0; p < L; ++p) nsg = std::max(nsg, ++cls[(int)((int64_t)p * M / L) % 16]);
    const int dealt = 32 * ((nsg + 1) / 2);
    auto lds = [&](int lanes) { return 4 * ((size_t)(M + nt) * pv + (size_t)lanes * (nt | 1) + lanes + L); };
    return (M > L && dealt * groups <= 1024 && lds(dealt) <= kLds) || lds(L) <= kLds;
}

void check_fused_geometry(int L, int M, int half) {
    const Res3Geom gm = res3_geometry(L, M, half);
    REQUIRE(gm.groups > 0, "geometry of a rate the form applies to");
    const int nt = 2 * half, R = 4 * gm.groups, pv = gm.pitch_v, span = R * M + M + nt;
    REQUIRE(gm.lds <= kLds, "LDS bytes");
    REQUIRE(gm.lds == 4 * ((size_t)(M + nt) * pv + (size_t)gm.lpg * (nt | 1) + gm.lpg + L), "LDS bytes are the kernel's arrays");
    REQUIRE(span <= kRes3Stage * 1024, "span within what the threads stage");
    REQUIRE(gm.lpg * gm.groups <= 1024 && gm.groups * L <= 1024, "lanes within the block");
    REQUIRE(pv % 4 == 0 && (pv / 4) % 2 == 1, "an odd number of 16-byte slots per row");
    // staging: every sample of the span has a place in X, and its shifted twin where the reads ask for one
    std::set<int> x, x1;
    for (int ip = 0; ip < kRes3Stage * 1024; ++ip) {
        const int vv = ip / M, u = ip % M;
        if (ip < span) REQUIRE(vv < pv, "a sample of the span has a row of the tile");
        if (ip < span && vv < pv) { REQUIRE(u * pv + vv < M * pv, "X offset"); x.insert(u * pv + vv); }
        if (ip < span && u < nt && vv >= 1 && vv - 1 < pv) { REQUIRE(u * pv + vv - 1 < nt * pv, "X1 offset"); x1.insert(u * pv + vv - 1); }
    }
    REQUIRE((int)x.size() == span, "X places are distinct");
    // reads: phase p, group g, tap j -> rows 4 g .. 4 g + 3 of X[b + j], or of the shifted copy behind the wrap
    for (int p = 0; p < L; ++p) {
        const int b = (int)((int64_t)p * M / L), jx = std::min(M - b, nt);
        for (int g = 0; g < gm.groups; ++g)
            for (int j = 0; j < nt; ++j) {
                const int row = j < jx ? b + j : b + j - M;
                REQUIRE(row >= 0 && row < (j < jx ? M : nt), "row inside its array");
                const int off = row * pv + 4 * g;
                REQUIRE(off % 4 == 0 && 4 * g + 3 < pv, "16-byte read aligned and inside the row");
                for (int r = 0; r < 4; ++r) {             // ... and it is the sample (4 g + r) M + b + j of the tile
                    const int ip = (4 * g + r) * M + b + j;
                    REQUIRE(ip < span, "sample inside the span");
                    if (j < jx) REQUIRE(x.count(off + r) && ip % M == row && ip / M == 4 * g + r, "X holds the sample");
                    else REQUIRE(x1.count(off + r) && ip % M == row && ip / M - 1 == 4 * g + r, "X1 holds the sample");
                }
            }
    }
    // lanes: phases in lane order, or dealt by residue class to distinct lanes below lpg
    std::set<int> lanes;
    std::map<int, int> seen;
    for (int p = 0; p < L; ++p) {
        const int c = (int)((int64_t)p * M / L) & 15;
        const int lane = gm.lpg == L ? p : r_res3_slot(seen[c]++, c);
        REQUIRE(lane >= 0 && lane < gm.lpg && lanes.insert(lane).second, "dealt lane distinct and below lpg");
    }
    hit("fused geometry: LDS, span, tile places, 16-byte reads, lanes");
}

void check_unfused_geometry(int L, int M, int half, int64_t max_out, int n) {
    const ResGeom g = res_geometry(L, M, half, max_out, n);
    const size_t table = (size_t)L * ((2 * half) | 1) * 4;
    const bool want_lds = table <= 150 * 1024 && (int64_t)4096 * M < ((int64_t)1 << 30) && ((max_out + 4095) / 4096) * n < ((int64_t)1 << 30);
    REQUIRE(g.lds_kernel == want_lds, "which unfused kernel");
    if (!g.lds_kernel) { hit("unfused geometry: the plain kernel"); return; }
    REQUIRE(g.lds <= kLds && g.lds == table + (size_t)g.span * 4, "LDS bytes");
    REQUIRE(g.chunks_per_file * 4096 >= max_out && (g.chunks_per_file - 1) * 4096 < std::max<int64_t>(max_out, 1), "chunks cover the longest file");
    REQUIRE((int64_t)L - 1 + (int64_t)4095 * M < ((int64_t)1 << 31), "ph0 + k M in 32 bits");
    if (g.span > 0) {
        const int64_t db_max = ((int64_t)L - 1 + (int64_t)4095 * M) / L;       // the last output of an item that starts at phase L - 1
        REQUIRE(db_max + 2 * half - 1 < g.span, "span covers every input of a 4096-output item");
        hit("unfused geometry: LDS kernel, staged span");
    } else {
        REQUIRE(table + 4 * (size_t)(((int64_t)L - 1 + (int64_t)4095 * M) / L + 2 * half + 1) > kLds, "span dropped only when it does not fit");
        hit("unfused geometry: LDS kernel, no span");
    }
}

// ---- one batch ---------------------------------------------------------------------------------------------------------------------
void check_plan(int format, int sr, int ch, const std::vector<int64_t>& frames, bool each_arg, size_t used0, bool allow_fused) {
    const int n = (int)frames.size();
    const IngestPlan pl = plan_ingest(format, sr, ch, frames.data(), n, each_arg, used0, allow_fused);
    const bool each = each_arg && ch > 1;
    const int planes = each ? ch : 1;
    const int64_t bps = format == 1 || format == 7 ? 1 : format == 2 || format == 8 ? 2 : format == 3 || format == 9 ? 3 : format == 6 || format == 12 ? 8 : 4;
    const int g = r_gcd(sr, 22050), L = 22050 / g, M = sr / g;
    const int half = sr <= 22050 ? 32 : (int)((32 * (int64_t)sr + 22049) / 22050);
    const bool resample = sr != 22050;
    REQUIRE(pl.each == each && (int)pl.files.size() == n * planes, "signals of the batch");
    if (resample) REQUIRE(pl.rule.L == L && pl.rule.M == M && pl.rule.half == half, "rate rule");
    hit("plan: rate rule and signal count");

    // route
    const IngestRoute want = !resample ? kRouteDecode : (r_fused_applies(L, M, half) && allow_fused) ? kRouteFused : kRoutePair;
    REQUIRE(pl.route == want, "route");
    hit("route: the three conditions");

    // slots: the sequential walk of the slot rule
    size_t used = used0;
    int64_t total = 0, max_frames = 0, max_out = 0, prev_end = (int64_t)used0;
    double n22sum = 0;
    for (int i = 0, s = 0; i < n; ++i) {
        const int64_t n22 = sr == 22050 ? frames[i] : (frames[i] * 22050 + sr - 1) / sr;
        REQUIRE(n22 == ss_resampled_length(frames[i], sr), "resampled length");
        for (int k = 0; k < planes; ++k, ++s) {
            const FileRec& f = pl.files[s];
            const int64_t off = ((int64_t)used + 3) & ~(int64_t)3, need = n22 + 2 * W + 64;
            used = (size_t)(off + need);
            REQUIRE(f.off == off && f.n == n22 && f.n_padded == n22 + 2 * W && f.duration == (double)frames[i] / (double)sr, "FileRec by the parent's formulas");
            REQUIRE(f.off % 4 == 0 && f.off >= prev_end && f.off >= (int64_t)pl.fill_off, "slot aligned, ascending, disjoint");
            REQUIRE(f.off + f.n_padded + 64 <= (int64_t)pl.arena_used && f.off + f.n_padded + 64 <= (int64_t)(pl.fill_off + pl.fill_n), "slot and its slack inside the extent");
            prev_end = f.off + f.n_padded + 64;
            hit("slots: aligned, ascending, disjoint, inside the extent, slack behind");
        }
        total += frames[i]; max_frames = std::max(max_frames, frames[i]); max_out = std::max(max_out, n22); n22sum += (double)n22 * planes;
    }
    REQUIRE(pl.arena_used == used && pl.fill_off == ((used0 + 3) & ~(size_t)3) && pl.fill_off + pl.fill_n == used, "the fill is the new extent");
    REQUIRE(pl.fill_off + pl.fill_n == (size_t)prev_end, "the fill ends behind the last slot's slack");
    hit("slots: the fill covers exactly the new extent");
    REQUIRE(pl.max_frames == max_frames && pl.max_out == max_out, "maxima");

    // descriptor image
    REQUIRE(pl.n_chan == (each ? (size_t)n : 0), "ChanFiles: one per recording of a per-channel call");
    REQUIRE(pl.n_batch == (!each ? (size_t)n : pl.route == kRoutePair ? (size_t)n * ch : 0), "BatchFiles: one per file, or per signal of the pair route");
    const size_t chan_end = pl.chan_off + pl.n_chan * sizeof(ChanFile), batch_end = pl.batch_off + pl.n_batch * sizeof(BatchFile);
    REQUIRE(chan_end <= pl.batch_off && batch_end <= pl.desc.size() && pl.chan_off % alignof(ChanFile) == 0 && pl.batch_off % alignof(BatchFile) == 0,
            "descriptor regions disjoint, inside the image, aligned");
    hit("descriptors: regions disjoint, sized, aligned");

    // what the descriptors address
    const int64_t pcm_total = total * ch * bps;
    int64_t pcm_at = 0, mono_at = 0;
    const int64_t mono_n = (int64_t)pl.mono_n;
    REQUIRE((pl.route == kRoutePair) == (mono_n > 0), "a mono buffer for the pair route only");
    for (int i = 0; i < n; ++i) {
        const FileRec& f0 = pl.files[(size_t)i * planes];
        int64_t d_pcm, d_frames, d_mono, d_out, d_nout, d_mstride = 0, d_ostride = 0;
        if (each) {
            const ChanFile& d = pl.chan()[i];
            d_pcm = d.pcm_off; d_frames = d.frames; d_mono = d.mono_off; d_out = d.out_off; d_nout = d.n_out; d_mstride = d.mono_stride; d_ostride = d.out_stride;
            for (int k = 0; k < ch; ++k) REQUIRE(pl.files[(size_t)i * ch + k].off + W == d_out + k * d_ostride, "channel slots out_stride apart");
            hit("channels: slots exactly out_stride apart");
            if (pl.route == kRoutePair) {
                for (int k = 0; k < ch; ++k) {
                    const BatchFile& b = pl.batch()[(size_t)i * ch + k];
                    REQUIRE(b.frames == d_frames && b.n_out == d_nout && b.mono_off == d_mono + k * d_mstride && b.out_off == d_out + k * d_ostride,
                            "a signal's BatchFile addresses the ChanFile's planes");
                }
                hit("channels: the pair route's BatchFiles address the ChanFile's planes");
            }
        } else {
            const BatchFile& b = pl.batch()[i];
            d_pcm = b.pcm_off; d_frames = b.frames; d_mono = b.mono_off; d_out = b.out_off; d_nout = b.n_out;
        }
        REQUIRE(d_frames == frames[i] && d_nout == f0.n && d_out == f0.off + W, "descriptor frames, n_out, out_off");
        hit("slots: n_padded, out_off and duration by the parent's formulas");
        REQUIRE(d_pcm == pcm_at && d_pcm + frames[i] * ch * bps <= pcm_total, "PCM ranges back to back inside the buffer");
        pcm_at += frames[i] * ch * bps;
        hit("pcm: ranges back to back inside sum(frames) ch bps");
        if (pl.route == kRouteDecode) {                   // decoded straight into the slots
            REQUIRE(d_mono == d_out && (!each || d_mstride == d_ostride), "straight decode writes the arena planes");
            for (int k = 0; k < planes; ++k) REQUIRE(d_mono + k * d_mstride + frames[i] <= pl.files[(size_t)i * planes + k].off + W + f0.n, "decoded samples inside the slot");
            hit("decode: 22 050 Hz files go straight into their slots");
        } else if (pl.route == kRoutePair) {
            const int64_t stride = each ? d_mstride : ((frames[i] + 3) & ~(int64_t)3);
            REQUIRE(d_mono == mono_at && d_mono % 4 == 0 && stride % 4 == 0 && stride >= frames[i], "mono planes aligned and disjoint");
            REQUIRE(d_mono + (int64_t)planes * stride <= mono_n, "mono planes inside the stated size");
            mono_at += (int64_t)planes * stride;
            hit("mono: planes 16-byte aligned, disjoint, inside the mono size");
        }
        // resampler input reads of the first and last min(n_out, 2 L) outputs
        if (resample && d_nout > 0) {
            const int64_t cnt = std::min<int64_t>(d_nout, 2 * (int64_t)L);
            const int R = pl.route == kRouteFused ? 4 * pl.res3.groups : 0;
            for (int pass = 0; pass < 2; ++pass)
                for (int64_t q = 0; q < cnt; ++q) {
                    const int64_t m = pass ? d_nout - 1 - q : q, base = (m * M) / L;
                    for (int j = 0; j < 2 * half; j += (j == 0 ? 2 * half - 1 : 1)) {          // the first and the last tap bound the others
                        const int64_t idx = base + j - half + 1;
                        REQUIRE(idx > -half && idx < frames[i] + half, "an input index is inside the file or within `half` of it, where the kernels read zero");
                        if (pl.route == kRouteFused) {    // the item's tile holds it
                            const int64_t it = m / ((int64_t)L * R), i_lo = it * R * M - half + 1;
                            REQUIRE(idx >= i_lo && idx < i_lo + (int64_t)R * M + M + 2 * half, "input inside its item's tile");
                            REQUIRE(it < pl.items_per_file, "item counted");
                        } else if (idx >= 0 && idx < frames[i]) {
                            REQUIRE(idx < (each ? d_mstride : ((frames[i] + 3) & ~(int64_t)3)), "input inside its mono plane");
                        }
                    }
                }
            REQUIRE(((d_nout - 1) * M) / L < frames[i] + half, "the last output's base index is below frames + half");
            hit("resampler: input reads inside the file or on a zeroed side");
        }
    }
    if (pl.route == kRoutePair) REQUIRE(mono_n == mono_at + 16, "mono size");

    // geometries, items
    if (pl.route == kRouteFused) {
        const int64_t per_item = (int64_t)L * 4 * pl.res3.groups;
        REQUIRE(pl.items_per_file * per_item >= max_out && (pl.items_per_file - 1) * per_item < std::max<int64_t>(max_out, 1), "items cover the longest file");
        REQUIRE(pl.items_ok == (pl.items_per_file * n < ((int64_t)1 << 30)), "items below 2^30, or the plan refuses");
        hit("items: items_per_file n_files < 2^30, or refused");
    }
    if (pl.route == kRoutePair) check_unfused_geometry(L, M, half, max_out, (int)pl.n_batch);

    // what ScopedLaunch books
    const double pcm_bytes = (double)total * ch * bps;
    REQUIRE(pl.decode.flops == 0.0 && pl.decode.bytes == pcm_bytes + 4.0 * planes * total, "decode cost");
    if (resample) {
        REQUIRE(pl.fused.flops == 2.0 * 2 * half * n22sum && pl.fused.bytes == pcm_bytes + 4.0 * n22sum, "fused cost");
        REQUIRE(pl.resample.flops == 2.0 * 2 * half * n22sum && pl.resample.bytes == 4.0 * planes * total + 4.0 * n22sum, "resample cost");
    }
    hit("costs: the three (flops, bytes) pairs");
}

}  // namespace

int main(int argc, char** argv) {
    // per rate: the route, the unfused kernel, the fused geometry, the table
    std::printf("routes (mixdown call, one file of 10 000 frames):\n");
    for (int sr : kRates) {
        g_case = "rate " + std::to_string(sr);
        const ResampleRule r = resample_rule(sr);
        const int64_t fr = 10000;
        const IngestPlan pl = plan_ingest(SS_PCM_S16, sr, 2, &fr, 1, false, 0);
        const ResGeom ug = res_geometry(r.L, r.M, r.half, pl.max_out, 1);
        std::printf("    %6d Hz  L %4d  M %5d  half %4d  %-15s unfused: %s\n", sr, r.L, r.M, r.half,
                    pl.route == kRouteDecode ? "straight decode" : pl.route == kRouteFused ? "fused" : "pair",
                    sr == 22050 ? "-" : !ug.lds_kernel ? "plain kernel" : ug.span > 0 ? "LDS kernel, staged span" : "LDS kernel, no span");
        if (sr != 22050) {
            REQUIRE(r_fused_applies(r.L, r.M, r.half) == (res3_geometry(r.L, r.M, r.half).groups > 0), "fused form applies");
            if (res3_geometry(r.L, r.M, r.half).groups > 0) check_fused_geometry(r.L, r.M, r.half);
        }
        const std::vector<float> t = design_taps(sr);
        REQUIRE(t.size() == (size_t)r.L * 2 * r.half, "table size");
        hit("taps: [L][2 half] floats");
        if (argc > 1) {
            const std::string path = std::string(argv[1]) + "/taps_" + std::to_string(sr) + ".f32";
            FILE* f = std::fopen(path.c_str(), "wb");
            REQUIRE(f && std::fwrite(t.data(), 4, t.size(), f) == t.size() && std::fclose(f) == 0, "table written");
        }
    }
    // argument limits
    g_case = "argument limits";
    REQUIRE(pcm_args_ok(true, 1, 1, 1, 0) && pcm_args_ok(false, 12, 768000, 64, 0) && pcm_args_ok(true, 5, 48000, 2, (int64_t)1 << 36), "accepted");
    REQUIRE(!pcm_args_ok(false, 2, 48000, 2, 1) && !pcm_args_ok(true, 0, 48000, 2, 1) && !pcm_args_ok(true, 13, 48000, 2, 1) && !pcm_args_ok(true, 2, 0, 2, 1) &&
            !pcm_args_ok(true, 2, 768001, 2, 1) && !pcm_args_ok(true, 2, 48000, 0, 1) && !pcm_args_ok(true, 2, 48000, 65, 1) && !pcm_args_ok(true, 2, 48000, 2, -1) &&
            !pcm_args_ok(true, 2, 48000, 2, ((int64_t)1 << 36) + 1), "refused");
    REQUIRE(signal_count_ok(1, 64) && signal_count_ok((1 << 24) / 64 - 1, 64) && !signal_count_ok((1 << 24) / 64, 64), "signal count");
    hit("limits: check_pcm_args' bounds and the signal count");
    {   // a batch whose items pass 2^30: refused by the plan (no such batch fits a device; the launcher refuses it too)
        g_case = "items past 2^30";
        std::vector<int64_t> fr(128, (int64_t)1 << 36);
        const IngestPlan pl = plan_ingest(SS_PCM_S16, 48000, 1, fr.data(), (int)fr.size(), false, 0);
        REQUIRE(pl.route == kRouteFused && !pl.items_ok, "refused");
        hit("items: items_per_file n_files < 2^30, or refused");
    }

    std::mt19937_64 rng(20261021);
    auto pick = [&](int64_t n) { return (int64_t)(rng() % (uint64_t)n); };
    const int kCases = 640;
    for (int ci = 0; ci < kCases; ++ci) {
        const int format = 1 + ci % 12, sr = kRates[(ci / 12 + ci) % 12], ch = kChannels[pick(5)];
        const bool each = pick(2), allow_fused = pick(8) != 0;
        const int n = 1 + (int)pick(7);
        const ResampleRule r = resample_rule(sr);
        const Res3Geom gm = res3_geometry(r.L, r.M, r.half);
        const int64_t item_span = gm.groups ? (int64_t)4 * gm.groups * r.M : 4096;
        std::vector<int64_t> frames(n);
        for (int64_t& f : frames) {
            switch (pick(8)) {
                case 0: f = 0; break;
                case 1: f = 1; break;
                case 2: f = item_span - 1; break;
                case 3: f = item_span; break;
                case 4: f = item_span + 1; break;
                case 5: f = 1 + pick(3 * item_span); break;
                case 6: f = 1 + pick(400000); break;
                default: f = 1 + pick(3000); break;
            }
        }
        const size_t used0 = pick(3) == 0 ? 0 : (size_t)pick(5000000);
        g_case = "case " + std::to_string(ci) + ": format " + std::to_string(format) + " sr " + std::to_string(sr) + " ch " + std::to_string(ch) + " files " +
                 std::to_string(n) + (each ? " each" : " mix") + " used " + std::to_string(used0);
        check_plan(format, sr, ch, frames, each, used0, allow_fused);
    }
    std::printf("%d seeded cases; checks by property:\n", kCases);
    for (const std::string& p : g_order) std::printf("  %-78s %lld\n", p.c_str(), (long long)g_count[p]);
    std::printf("ingest_plan_check: ok\n");
    return 0;
}
