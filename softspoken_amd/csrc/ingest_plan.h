// The host plan of PCM ingest (ss_add_pcm*, ss_add_f32*): the rate rule and the polyphase tap table, the geometries of the resampler
// kernels, the arena's slot rule, the argument limits, and plan_ingest -- everything a batch call decides before it touches the device,
// as plain data.  No HIP header: abi.hip's ingest_run allocates, uploads and launches what the plan states, ingest.hip's launchers take
// the geometries, and tests/ingest_plan_check.cpp holds every index of every plan to a brute-force restatement without a device.
#pragma once
#include "hostdefs.h"
#include "stream_desc.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace ss {

// ---- argument limits -----------------------------------------------------------------------------------------------------------
// (frames: 99 h at 192 kHz; keeps frames * channels * bytes and frames * 22050 inside 64 bits)
inline bool pcm_args_ok(bool has_pcm, int format, int sr, int ch, int64_t frames) {
    return !((!has_pcm && frames > 0) || format < SS_PCM_U8 || format > SS_PCM_F64BE || sr <= 0 || sr > 768000 || ch < 1 || ch > 64 || frames < 0 ||
             frames > ((int64_t)1 << 36));
}
inline bool signal_count_ok(int n_files, int ch) { return (int64_t)n_files * ch < (int64_t)1 << 24; }   // signals of one per-channel batch

// ---- the rate rule: sr -> 22 050 Hz is L / M, the filter reaches `half` input samples to either side --------------------------------
struct ResampleRule { int L, M, half; };
inline ResampleRule resample_rule(int sr) {
    auto gcd = [](int a, int b) { while (b) { int t = a % b; a = b; b = t; } return a; };
    const int g = gcd(sr, SS_SAMPLE_RATE);
    const double scale = std::min(1.0, (double)SS_SAMPLE_RATE / sr);
    return ResampleRule{SS_SAMPLE_RATE / g, sr / g, (int)std::ceil(32.0 / scale)};
}

// ---- Kaiser-windowed sinc polyphase taps (the build's own design; oracle/oracle_np.py resample_plan states the same) ---------------
inline double bessel_i0(double x) {
    double s = 1.0, t = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 200; ++k) { t *= q / ((double)k * k); s += t; if (t < s * 1e-17) break; }
    return s;
}
// [L][2 half] floats
inline std::vector<float> design_taps(int sr) {
    const ResampleRule r = resample_rule(sr);
    const int L = r.L, M = r.M, half = r.half;
    const double scale = std::min(1.0, (double)SS_SAMPLE_RATE / sr);
    const double fc = 0.95 * scale, beta = 12.0;
    const double PI = 3.14159265358979323846;
    std::vector<float> t((size_t)L * 2 * half);
    const double i0b = bessel_i0(beta);
    for (int p = 0; p < L; ++p) {
        const double frac = (double)(((int64_t)p * M) % L) / L;
        for (int jj = 0; jj < 2 * half; ++jj) {
            const double d = (double)(jj - half + 1) - frac;
            const double xx = fc * d;
            const double sinc = xx == 0.0 ? 1.0 : std::sin(PI * xx) / (PI * xx);
            double w = 0.0;
            if (std::fabs(d) <= half) { const double u = 1.0 - (d / half) * (d / half); w = bessel_i0(beta * std::sqrt(u < 0 ? 0 : u)) / i0b; }
            t[(size_t)p * 2 * half + jj] = (float)(fc * sinc * w);
        }
    }
    return t;
}

// ---- geometry of the fused resampler (ingest.hip resample_fused*_kernel) -----------------------------------------------------------
constexpr int kRes3Threads = 1024;
constexpr int kRes3Stage = 9;                             // most tile samples a thread stages per item (the geometry checks the span)
// for a rate pair, or groups = 0 when the form does not apply (table or tile too large, 2 half > M, L > 1024)
struct Res3Geom { int groups, pitch_v, lpg; size_t lds; };
inline Res3Geom res3_geometry(int L, int M, int half) {
    Res3Geom gm{0, 0, 0, 0};
    const int nt = 2 * half;
    if (L > kRes3Threads || nt > M) return gm;
    const int groups = kRes3Threads / L;
    const int R = 4 * groups;
    int pv = R + 2;                                       // rows v the tile needs: r + (b + j) div M <= R - 1 + 1, + the shifted copy's read
    pv = (pv + 3) & ~3;                                   // 16-byte rows
    if (((pv / 4) & 1) == 0) pv += 4;                     // an odd number of 16-byte slots per row: rows u, u + 1, ... start 16 banks-of-four apart mod 16
    if ((size_t)R * M + M + nt > (size_t)kRes3Stage * kRes3Threads) return gm;
    // phases dealt to the LDS service groups by b(p) mod 16 (see the kernel): lanes per 4-row group = 32 ceil(largest class / 2)
    int cnt[16] = {0};
    for (int ph = 0; ph < L; ++ph) ++cnt[(int)(((int64_t)ph * M) / L) % 16];
    int nsg = 0;
    for (int c = 0; c < 16; ++c) nsg = std::max(nsg, cnt[c]);
    int lpg = 32 * ((nsg + 1) / 2);
    auto lds_of = [&](int lanes) { return ((size_t)M * pv + (size_t)nt * pv + (size_t)lanes * (nt | 1) + (size_t)lanes + (size_t)L) * sizeof(float); };
    // (interpolating pairs, M <= L: neighbouring lanes read the same or the next row -- broadcasts and adjacent banks -- and measured the
    // same or a little slower dealt: 16 k -> 22.05 k 118 -> 128 us per 1005 windows; decimating pairs spread a service group over ~35 rows:
    // 48 k -> 22.05 k 1.53 -> 1.41 ms on the C5 job)
    if (M <= L || lpg * groups > kRes3Threads || lds_of(lpg) > 160 * 1024) lpg = L;     // phases in lane order
    const size_t lds = lds_of(lpg);
    if (lds > 160 * 1024) return gm;
    gm.groups = groups; gm.pitch_v = pv; gm.lpg = lpg; gm.lds = lds;
    return gm;
}
// items a file of max_out outputs takes: an item is 4 groups rows of L outputs
inline int64_t res3_items_per_file(const Res3Geom& gm, int L, int64_t max_out) {
    const int64_t per_item = (int64_t)L * 4 * gm.groups;
    return (max_out + per_item - 1) / per_item;
}
constexpr int64_t kMaxItems = (int64_t)1 << 30;           // items of one launch, all files: the kernels count them in 32 bits

// ---- geometry of the unfused resampler (ingest.hip resample_batch*_kernel) ---------------------------------------------------------
constexpr int kResOut = 4096;                             // outputs of one item of the LDS form
constexpr int kResThreads = 1024;                         // 4 waves per SIMD; the 115 KB table allows one block per CU
// lds_kernel: the table in LDS, a block walking (file, 4096-output chunk) items; span > 0: an item's input samples staged beside it
// (floor((L - 1 + (kResOut - 1) M) / L) + 2 half of them, when they fit); otherwise the plain kernel, taps and samples from memory
struct ResGeom { bool lds_kernel; int64_t chunks_per_file; int span; size_t lds; };
inline ResGeom res_geometry(int L, int M, int half, int64_t max_out, int n_files) {
    const size_t lds = (size_t)L * ((2 * half) | 1) * sizeof(float);
    const int64_t cpf = (max_out + kResOut - 1) / kResOut;
    if (!(lds <= 150 * 1024 && (int64_t)kResOut * M < (int64_t)1 << 30 && cpf * n_files < kMaxItems)) return ResGeom{false, 0, 0, 0};
    const int span = (int)(((int64_t)L - 1 + (int64_t)(kResOut - 1) * M) / L) + 2 * half + 1;
    const size_t lds_all = lds + (size_t)span * sizeof(float);
    return lds_all > 160 * 1024 ? ResGeom{true, cpf, 0, lds} : ResGeom{true, cpf, span, lds_all};
}

// ---- the arena's slot rule ---------------------------------------------------------------------------------------------------------
struct FileRec {
    int64_t off = 0;        // arena offset of the padded signal
    int64_t n = 0;          // samples at 22 050 Hz (unpadded)
    int64_t n_padded = 0;
    double duration = 0;    // header duration in seconds (frames / sample_rate)
    int64_t W = 0, win_base = 0;                          // plan of the last ss_run_begin
    int64_t bin_off = 0; int n_bins = 0;
};
constexpr int64_t kSlotSlack = 64;                        // floats behind every padded signal
inline int64_t slot_floats(int64_t n_padded) { return n_padded + kSlotSlack; }
inline int64_t slot_align(int64_t off) { return (off + 3) & ~(int64_t)3; }    // every slot starts on 16 bytes
// the slot of a signal of n samples behind `used` floats of arena: its 3 s of padding either side (stored >= 0: the caller brings the
// padded signal, that many samples); used: the arena's extent behind the slot
inline FileRec arena_slot(size_t& used, int64_t n, int64_t stored = -1) {
    FileRec fr;
    fr.n = n < 0 ? 0 : n; fr.n_padded = stored >= 0 ? stored : n + 2 * (int64_t)SS_WINDOW_SAMPLES;
    fr.off = slot_align((int64_t)used);
    used = (size_t)(fr.off + slot_floats(fr.n_padded));
    return fr;
}

// ---- the plan of one batch call ----------------------------------------------------------------------------------------------------
enum IngestRoute { kRouteDecode = 0, kRouteFused = 1, kRoutePair = 2 };   // straight into the arena / one fused launch / decode + resample_batch
struct LaunchCost { double flops, bytes; };               // what ScopedLaunch books for a launch
struct IngestPlan {
    int format = 0, sr = 0, ch = 1, n_files = 0;
    bool each = false;                                    // a signal per channel (ch > 1), no mixdown
    ResampleRule rule{1, 1, 0};
    IngestRoute route = kRouteDecode;
    Res3Geom res3{0, 0, 0, 0}; int64_t items_per_file = 0; bool items_ok = true;   // fused route
    ResGeom res{false, 0, 0, 0};                          // pair route
    std::vector<FileRec> files;                           // the new signals, in file id order
    size_t fill_off = 0, fill_n = 0;                      // floats of arena the call zeroes: exactly the new slots
    size_t arena_used = 0;                                // ... and the arena's extent behind them
    size_t mono_n = 0;                                    // floats of the mono buffer (pair route; 0 otherwise)
    int64_t max_frames = 0, max_out = 0;
    LaunchCost decode{0, 0}, fused{0, 0}, resample{0, 0};
    // one descriptor image: a recording's ChanFile each (per-channel calls), then the BatchFiles -- a file's (mixdown calls) or, for
    // the pair route of a per-channel call, a signal's, which resample_batch reads
    std::vector<unsigned char> desc;
    size_t chan_off = 0, n_chan = 0, batch_off = 0, n_batch = 0;
    const ChanFile* chan() const { return (const ChanFile*)(desc.data() + chan_off); }
    const BatchFile* batch() const { return (const BatchFile*)(desc.data() + batch_off); }
};

// `frames[i]` frames per file back to back in one buffer, one format / rate / channel count; allow_fused: the development build's switch
inline IngestPlan plan_ingest(int format, int sr, int ch, const int64_t* frames, int n_files, bool each_channel, size_t arena_used,
                              bool allow_fused = true) {
    IngestPlan pl;
    pl.format = format; pl.sr = sr; pl.ch = ch; pl.n_files = n_files; pl.each = each_channel && ch > 1;
    const int planes = pl.each ? ch : 1;
    const int64_t bps = (int64_t)pcm_bytes_per_sample(format);
    const bool resample = sr != SS_SAMPLE_RATE;
    if (resample) {
        pl.rule = resample_rule(sr);
        pl.res3 = res3_geometry(pl.rule.L, pl.rule.M, pl.rule.half);
    }
    pl.route = !resample ? kRouteDecode : (pl.res3.groups > 0 && allow_fused) ? kRouteFused : kRoutePair;
    std::vector<ChanFile> cf;
    std::vector<BatchFile> bf;
    int64_t pcm_off = 0, mono_off = 0, total_frames = 0;
    double n22sum = 0;
    size_t used = arena_used;
    pl.fill_off = (size_t)slot_align((int64_t)used);
    for (int i = 0; i < n_files; ++i) {
        const int64_t n22 = ss_resampled_length(frames[i], sr);
        const int64_t mono_stride = slot_align(frames[i]);
        const int64_t out_stride = slot_align(slot_floats(n22 + 2 * (int64_t)SS_WINDOW_SAMPLES));   // a recording's slots have one length
        const int64_t out_off = slot_align((int64_t)used) + SS_WINDOW_SAMPLES;
        for (int k = 0; k < planes; ++k) {
            FileRec fr = arena_slot(used, n22);
            fr.duration = (double)frames[i] / (double)sr;
            pl.files.push_back(fr);
            // decode straight into the arena (no resampling), or to a plane of the mono buffer
            if (!pl.each || pl.route == kRoutePair)
                bf.push_back(BatchFile{pl.each ? 0 : pcm_off, frames[i], resample ? mono_off + k * mono_stride : out_off + k * out_stride,
                                       out_off + k * out_stride, n22});
        }
        if (pl.each)
            cf.push_back(ChanFile{pcm_off, frames[i], resample ? mono_off : out_off, out_off, n22, resample ? mono_stride : out_stride, out_stride});
        pcm_off += frames[i] * ch * bps; mono_off += mono_stride * planes;
        total_frames += frames[i];
        pl.max_frames = std::max(pl.max_frames, frames[i]); pl.max_out = std::max(pl.max_out, n22);
        n22sum += (double)n22 * planes;
    }
    pl.arena_used = used; pl.fill_n = used - pl.fill_off;
    if (pl.route == kRouteFused) {
        pl.items_per_file = res3_items_per_file(pl.res3, pl.rule.L, pl.max_out);
        pl.items_ok = pl.items_per_file * n_files < kMaxItems;
    }
    if (pl.route == kRoutePair) {
        pl.mono_n = (size_t)mono_off + 16;
        pl.res = res_geometry(pl.rule.L, pl.rule.M, pl.rule.half, pl.max_out, (int)bf.size());
    }
    const double pcm_bytes = (double)total_frames * ch * bps;
    const int half = pl.rule.half;
    pl.decode = LaunchCost{0.0, pcm_bytes + 4.0 * planes * total_frames};
    pl.fused = LaunchCost{2.0 * 2 * half * n22sum, pcm_bytes + 4.0 * n22sum};
    pl.resample = LaunchCost{2.0 * 2 * half * n22sum, 4.0 * planes * total_frames + 4.0 * n22sum};
    pl.n_chan = cf.size(); pl.n_batch = bf.size();
    pl.chan_off = 0; pl.batch_off = cf.size() * sizeof(ChanFile);
    pl.desc.resize(pl.batch_off + bf.size() * sizeof(BatchFile));
    if (!cf.empty()) memcpy(pl.desc.data() + pl.chan_off, cf.data(), cf.size() * sizeof(ChanFile));
    if (!bf.empty()) memcpy(pl.desc.data() + pl.batch_off, bf.data(), bf.size() * sizeof(BatchFile));
    return pl;
}

}  // namespace ss
