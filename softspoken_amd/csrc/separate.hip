// The separation silencer (include/softspoken.h "separation silencer"): inside the erased intervals, an STFT at the file's native rate
// whose bins are scaled by a gain from the network's spec head (pytorch_neural_nets.py:125-130,184-185, "env / speech separation";
// NNDetector.py:84-101 returns it as speech_pred, worker.py:78-79 drops it); outside them, ss_silence_pcm's transcode.
// Kernels and device runs only: each run asks sep_plan.h (host, no HIP) for its plan, grows its buffers, uploads, launches, downloads.
//
//   plan   separation_plan: merged intervals (silence_ranges) -> STFT frames -> averaged bins they read -> windows over those bins;
//          plan_ranges + plan_maps: merged bins and windows, window slots, run list; plan_synthesis (behind step 1): frames, pieces, chunks
//   1      spec head over those windows (forward_chunk, passes of ss_set_chunk_windows) -> sep_accumulate_kernel after each pass:
//          float64 sums per (bin, channel, band) in ascending window order, carried in memory across passes
//   2      sep_finalize_kernel: sum / count -> float32 maps, band gains G' (logistic of the log-power difference)
//   3      sep_stft_kernel<N>: per (frame, channel pair): decode + Hann -> FFT -> gain per STFT bin (two mel triangles x two bins in
//          time) -> inverse FFT (conj / forward / conj) -> synthesis Hann / (1.5 N), one frame per slot of a buffer
//   4      sep_blend_kernel: per output sample of an interval, the four overlapping frames gathered in ascending order, blended with
//          the decoded sample over the fade ramps, encoded as ss_silence_pcm encodes
// Everything else of the file is the transcode (silence_encode_kernel with no ranges), launched first.
// The band silencer (ss_box_silence_pcm, box_run below) is steps 3 and 4 alone: box_stft_kernel<N> shares step 3's frame body and takes
// its gains from a table of boxes instead of the maps.
//
// ss_separate_pcm_channels ("per-channel separation"): the signals of step 1 are the channels alone (ss_add_pcm_channels), their windows
// in one run list; sums, maps and gains carry a signal dimension, and step 3 runs as sep_stft_each_kernel<N>, which gives the two
// channels of a complex FFT their own gains.  Steps 2 and 4 and the plan are the mix's.
#include "engine.h"
#include "dsp.h"
#include "bands.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <type_traits>

namespace ss {

struct SepBand { int32_t m0, m1; float w0, w1; };                                // STFT bin -> two mel bands and weights (m0 < 0: >= 8 kHz)

struct SepTables { int N = 0; DevBuf<float2> tw; DevBuf<float> win; DevBuf<SepBand> band; };

struct SepState {
    std::map<int, SepTables> tables;                      // per sample rate
    DevBuf<int32_t> cbin, slot, count;
    DevBuf<double> sum;
    DevBuf<float> map, gain;
    DevBuf<SepFrame> frames;
    DevBuf<SepSeg> segs;
    DevBuf<float2> fout;
    // band silencer
    DevBuf<BoxFrame> bframes;
    DevBuf<int32_t> bidx;
    DevBuf<BoxRow> brows;
    // region bands
    DevBuf<BandSeg> bseg;
    DevBuf<BandRegion> breg;
    DevBuf<double> bpart, bprof, hz;
    DevBuf<ss_region_band> bout;
};

// =========================================================================================================
// kernels
// =========================================================================================================
// One pass of the spec head: spec [m][2][128][256] holds the windows whose run-list positions (win_slot) are slot_lo .. slot_lo + m - 1.
// Thread = (compact bin cb, channel x band cm); it adds the pass's windows over bin cbin[cb] to its float64 sum in ascending window order
// (average_bin's window walk), so that the sum over all passes is the whole-file average's sum, bit for bit.
// Signals (blockIdx.z: the channels of ss_separate_pcm_channels, one for the mix) share the plan: signal z's windows sit `nw` run-list
// positions behind signal z - 1's, its sums and counts one [256][ncb] / [ncb] block further on.
__global__ __launch_bounds__(256) void sep_accumulate_kernel(const float* __restrict__ spec, int slot_lo, int m, const int32_t* __restrict__ win_slot,
                                                             int W, int nw, const int32_t* __restrict__ cbin, int ncb, double* __restrict__ sum,
                                                             int32_t* __restrict__ count) {
    const int cb = blockIdx.x * 256 + threadIdx.x, cm = blockIdx.y, sig = blockIdx.z;
    if (cb >= ncb) return;
    const int j = cbin[cb];
    int lo = (int)((double)(j - 255) / 51.2) - 1;
    if (lo < 0) lo = 0;
    int hi = (int)((double)j / 51.2) + 1;
    if (hi > W - 1) hi = W - 1;
    sum += (size_t)sig * 256 * ncb;
    count += (size_t)sig * ncb;
    const int64_t first = (int64_t)sig * nw - slot_lo;                     // signal's first window in this pass's numbering
    if (first >= m || first + nw <= 0) return;                             // none of its windows ran in this pass
    double s = sum[(size_t)cm * ncb + cb];
    int n = 0;
    for (int i = lo; i <= hi; ++i) {
        const int d = j - (int)(((int64_t)512 * i + 5) / 10);             // start(i) = round(51.2 i) (no ties: 512 i is even)
        if (d < 0 || d >= 256) continue;
        if (win_slot[i] < 0) continue;
        const int64_t slot = first + win_slot[i];
        if (slot < 0 || slot >= m) continue;
        s += (double)spec[((size_t)slot * 256 + cm) * 256 + d];
        ++n;
    }
    sum[(size_t)cm * ncb + cb] = s;
    if (cm == 0) count[cb] += n;
}

// ln(10^(y^2) - 1): the log power behind a feature value y = sqrt(log10(P + 1)); -inf at y = 0, finite for every finite y
__device__ __forceinline__ double sep_log_power(double y) {
    const double a = y * y * 2.302585092994045684;
    if (a == 0.0) return -INFINITY;
    return a > 30.0 ? a + log1p(-exp(-a)) : log(expm1(a));
}

// maps [2][ncb][128] = sum / count as float32; gain (nullable) [ncb][128] = max(P_env / (P_env + P_speech), min_gain); one such block of
// each per signal (blockIdx.y)
__global__ __launch_bounds__(256) void sep_finalize_kernel(const double* __restrict__ sum, const int32_t* __restrict__ count, int ncb,
                                                           float* __restrict__ map, float* __restrict__ gain, int speech_ch, double min_gain) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)ncb * 128) return;
    const int cb = (int)(idx >> 7), band = (int)(idx & 127), sig = blockIdx.y;
    sum += (size_t)sig * 256 * ncb;
    count += (size_t)sig * ncb;
    map += (size_t)sig * 256 * ncb;
    if (gain) gain += (size_t)sig * 128 * ncb;
    const int n = count[cb];
    float y[2];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
        y[ch] = n ? (float)(sum[(size_t)(ch * 128 + band) * ncb + cb] / (double)n) : 0.f;
        map[((size_t)ch * ncb + cb) * 128 + band] = y[ch];
    }
    if (!gain) return;
    const double le = sep_log_power((double)y[1 - speech_ch]), ls = sep_log_power((double)y[speech_ch]);
    double g;
    if (le == -INFINITY && ls == -INFINITY) g = 1.0;              // no power in either: nothing to remove
    else g = 1.0 / (1.0 + exp(ls - le));                         // P_e / (P_e + P_s); 0 when only speech has power, 1 when only env
    gain[(size_t)cb * 128 + band] = (float)fmax(g, min_gain);
}

// small forward DFTs in registers, natural order in and out
template <int R> __device__ __forceinline__ void sep_dft(float2 (&v)[R]);
template <> __device__ __forceinline__ void sep_dft<2>(float2 (&v)[2]) { const float2 a = v[0]; v[0] = cadd(a, v[1]); v[1] = csub(a, v[1]); }
template <> __device__ __forceinline__ void sep_dft<4>(float2 (&v)[4]) { radix4(v[0], v[1], v[2], v[3], v[0], v[1], v[2], v[3]); }
template <> __device__ __forceinline__ void sep_dft<8>(float2 (&v)[8]) {
    constexpr float R2 = 0.70710678118654752f;
    float2 A[4], B[4];
    radix4(v[0], v[2], v[4], v[6], A[0], A[1], A[2], A[3]);
    radix4(v[1], v[3], v[5], v[7], B[0], B[1], B[2], B[3]);
    B[1] = cmul(B[1], make_float2(R2, -R2));
    B[2] = make_float2(B[2].y, -B[2].x);                          // W8^2 = -i
    B[3] = cmul(B[3], make_float2(-R2, -R2));
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = cadd(A[k], B[k]); v[k + 4] = csub(A[k], B[k]); }
}
template <> __device__ __forceinline__ void sep_dft<16>(float2 (&v)[16]) { fft16(v); }

// one FFT of N points per (256 / T) threads; T = min(256, N / 16)
template <int N> struct SepGeomT {
    static constexpr int T = N / 16 < 256 ? N / 16 : 256;
    static constexpr int ITEMS = 256 / T;
    static constexpr int PITCH = N + N / 16;                      // float2 per FFT buffer: one pad slot behind every 16
    static constexpr int LOG2 = N == 256 ? 8 : N == 512 ? 9 : N == 1024 ? 10 : N == 2048 ? 11 : N == 4096 ? 12 : 13;
    static constexpr int R0 = 1 << (LOG2 % 4);                    // the first stage's radix (1: none), then radix-16 stages
};
__device__ __forceinline__ int sep_pad(int i) { return i + (i >> 4); }   // radix-16 stride writes spread over the banks

// one Stockham stage (radix R, Ns = product of the earlier radices), in place: every thread's butterflies are read into registers,
// a barrier, then written to their autosorted places, a barrier.  Twiddles W_N^t from a host table (double -> float).
template <int N, int R>
__device__ __forceinline__ void sep_stage(float2* buf, int lt, int Ns, const float2* __restrict__ tw) {
    constexpr int T = SepGeomT<N>::T, NB = N / R / T;
    float2 v[NB][R];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = lt + b * T, jm = j & (Ns - 1);
        const int tstep = jm * (N / (Ns * R));
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float2 x = buf[sep_pad(j + r * (N / R))];
            v[b][r] = r == 0 ? x : cmul(x, tw[tstep * r]);
        }
        sep_dft<R>(v[b]);
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = lt + b * T, jm = j & (Ns - 1);
        const int d = (j - jm) * R + jm;
#pragma unroll
        for (int r = 0; r < R; ++r) buf[sep_pad(d + r * Ns)] = v[b][r];
    }
    __syncthreads();
}

template <int N>
__device__ __forceinline__ void sep_fft(float2* buf, int lt, const float2* __restrict__ tw) {
    constexpr int R0 = SepGeomT<N>::R0;
    int Ns = 1;
    if constexpr (R0 > 1) { sep_stage<N, R0>(buf, lt, 1, tw); Ns = R0; }
#pragma unroll
    for (int s = 0; s < SepGeomT<N>::LOG2 / 4; ++s) { sep_stage<N, 16>(buf, lt, Ns, tw); Ns *= 16; }
}

// The frame body every STFT kernel shares: channels c0 / c1 of the frame centred on sample k hop, decoded and windowed into the padded
// buffer -> FFT -> gains(): the kernel's own gain source scales the spectrum in place and leaves it conjugated (the inverse FFT is
// conj(FFT(conj(.))) / N) -> FFT -> synthesis window / (1.5 N) -> o[N].  Every thread of the block calls it (barriers); an item without
// a frame (!valid) transforms zeros and stores nothing.
template <int N, class Gains>
__device__ __forceinline__ void sep_frame_body(const unsigned char* pcm, int format, int channels, int64_t frames, int64_t k, bool valid, int hop,
                                               int c0, int c1, float2* buf, int lt, const float2* tw, const float* win, float2* o,
                                               Gains&& gains) {   // (no __restrict__ here: the kernels' own arguments carry it; repeated on
                                                                  // the inlined body it cost the existing forms 12 to 32 registers)
    using G = SepGeomT<N>;
    const int64_t base = k * hop - N / 2;
    for (int n = lt; n < N; n += G::T) {
        const int64_t s = base + n;
        float x0 = 0.f, x1 = 0.f;
        if (valid && s >= 0 && s < frames) {
            x0 = decode_sample(pcm, format, s * channels + c0);
            if (c1 < channels) x1 = decode_sample(pcm, format, s * channels + c1);
        }
        const float w = win[n];
        buf[sep_pad(n)] = make_float2(x0 * w, x1 * w);
    }
    __syncthreads();
    sep_fft<N>(buf, lt, tw);
    gains();
    __syncthreads();
    sep_fft<N>(buf, lt, tw);
    if (!valid) return;
    constexpr float kScale = 1.0f / (1.5f * (float)N);
    for (int n = lt; n < N; n += G::T) {
        const float2 Y = buf[sep_pad(n)];
        const float sc = win[n] * kScale;
        o[n] = make_float2(Y.x * sc, -Y.y * sc);
    }
}

// The pair (q, N - q) of Z = A + iB under the channels' own real, even gains ga / gb, in place and conjugated (q = 0 and N / 2 pair with
// themselves): Ga A + Gb iB = S Z[q] + D conj(Z[N - q]),  S = (ga + gb) / 2,  D = (ga - gb) / 2
template <int N>
__device__ __forceinline__ void sep_pair_gains(float2* buf, int q, float ga, float gb) {
    const float S = 0.5f * (ga + gb), D = 0.5f * (ga - gb);
    const int r = (N - q) & (N - 1);
    const float2 Zq = buf[sep_pad(q)], Zr = buf[sep_pad(r)];
    buf[sep_pad(q)] = make_float2(S * Zq.x + D * Zr.x, -(S * Zq.y - D * Zr.y));
    if (r != q) buf[sep_pad(r)] = make_float2(S * Zr.x + D * Zq.x, -(S * Zr.y - D * Zq.y));
}

// Block = ITEMS frames of one channel pair (blockIdx.y): channels 2p and 2p + 1 ride as the real and imaginary parts of one complex FFT
// (the gain is real and even in q, so the two stay apart).  out[rec][pair][N] = synthesis-windowed frame / (1.5 N), ready to gather.
//
// EACH (ss_separate_pcm_channels): the two channels have gains of their own, Ga and Gb, from the tables gain + c gain_cs; both are real and
// even in q, so with A, B the channels' spectra, Z = A + iB and A[q] = (Z[q] + conj(Z[N - q])) / 2, iB[q] = (Z[q] - conj(Z[N - q])) / 2:
//   Ga A + Gb iB = S Z[q] + D conj(Z[N - q]),  S = (Ga + Gb) / 2,  D = (Ga - Gb) / 2
// -- one thread per pair (q, N - q), in place (sep_pair_gains).  Ga == Gb: D = 0 adds an exact zero, S = Ga, the
// frame is the mix form's.  An unpaired last channel takes Gb := Ga.  LDS: two rows of band gains per frame in place of one.
// The two forms are launched (and recorded) as sep_stft_kernel<N> and sep_stft_each_kernel<N>; gain_cs is unused by the first.
template <int N, bool EACH>
__global__ __launch_bounds__(256) void sep_stft_form_kernel(const unsigned char* __restrict__ pcm, int format, int channels, int64_t frames,
                                                            const SepFrame* __restrict__ fr, int n_fr, int hop, const float* __restrict__ gain,
                                                            const SepBand* __restrict__ band, const float2* __restrict__ tw,
                                                            const float* __restrict__ win, float gain_hi, float2* __restrict__ out,
                                                            size_t gain_cs) {
    using G = SepGeomT<N>;
    extern __shared__ float2 sep_lds[];
    constexpr int GROWS = EACH ? 2 : 1;
    const int item = threadIdx.x / G::T, lt = threadIdx.x % G::T;
    float2* buf = sep_lds + item * G::PITCH;
    float* gt = (float*)(sep_lds + G::ITEMS * G::PITCH) + item * (128 * GROWS);
    const int64_t rec = (int64_t)blockIdx.x * G::ITEMS + item;
    const bool valid = rec < n_fr;
    const int pair = blockIdx.y, npairs = gridDim.y, c0 = 2 * pair, c1 = 2 * pair + 1;
    SepFrame f{0, 0, 0, 0.f, 0};
    if (valid) f = fr[rec];
    if constexpr (EACH) gain += (size_t)c0 * gain_cs;
    for (int m = lt; m < 128; m += G::T)                         // band gains at this frame's time: linear between two bins
        gt[m] = valid ? (1.0f - f.alpha) * gain[(size_t)f.cb0 * 128 + m] + f.alpha * gain[(size_t)f.cb1 * 128 + m] : 0.f;
    if constexpr (EACH) {
        const float* gain1 = gain + (c1 < channels ? gain_cs : 0);
        for (int m = lt; m < 128; m += G::T)
            gt[128 + m] = valid ? (1.0f - f.alpha) * gain1[(size_t)f.cb0 * 128 + m] + f.alpha * gain1[(size_t)f.cb1 * 128 + m] : 0.f;
    }
    sep_frame_body<N>(pcm, format, channels, frames, f.k, valid, hop, c0, c1, buf, lt, tw, win, out + ((size_t)rec * npairs + pair) * N, [&]() {
        if constexpr (EACH) {
            for (int q = lt; q <= N / 2; q += G::T) {            // one thread per pair (q, N - q)
                const SepBand bd = band[q];
                const float ga = bd.m0 < 0 ? gain_hi : bd.w0 * gt[bd.m0] + bd.w1 * gt[bd.m1];
                const float gb = bd.m0 < 0 ? gain_hi : bd.w0 * gt[128 + bd.m0] + bd.w1 * gt[128 + bd.m1];
                sep_pair_gains<N>(buf, q, ga, gb);
            }
        } else {
            for (int q = lt; q < N; q += G::T) {                 // X[q] g(q), conjugated
                const SepBand bd = band[q <= N / 2 ? q : N - q];
                const float g = bd.m0 < 0 ? gain_hi : bd.w0 * gt[bd.m0] + bd.w1 * gt[bd.m1];
                const float2 X = buf[sep_pad(q)];
                buf[sep_pad(q)] = make_float2(X.x * g, -X.y * g);
            }
        }
    });
}

// The band silencer's STFT (include/softspoken.h "band silencer", step 3): the frame body above with the gains of a table of boxes.
// fr[rec]: the frame and its active boxes idx[first .. first + count - 1] (rows of `rows`).  The rows are staged into LDS kBoxStage
// at a time, `rounds` times (the host's ceil(most active boxes of a frame / kBoxStage): uniform, so the barriers are); each thread
// keeps the minimum over them for its own pairs (q, N - q), q = lt + t T, in registers, for channel c0 (ga) and c1 (gb; an unpaired
// last channel takes gb := ga), then applies the channel-pair form.  omg = 1 - min_gain.
constexpr int kBoxStage = 64;

__device__ __forceinline__ float box_gain(const BoxRow& b, int q, float omg) {
    float v = 1.f;
    if (q < b.q_lo || q > b.q_hi) {
        const float d = q < b.q_lo ? (float)(b.q_lo - q) - b.lo_f : (float)(q - b.q_hi) - b.hi_f;
        const float t = d * b.inv_e;
        v = (b.inv_e > 0.f && t < 1.f) ? 0.5f + 0.5f * cospif(t) : 0.f;
    }
    return 1.f - omg * v;
}

template <int N>
__global__ __launch_bounds__(256) void box_stft_kernel(const unsigned char* __restrict__ pcm, int format, int channels, int64_t frames,
                                                       const BoxFrame* __restrict__ fr, int n_fr, int hop, const int32_t* __restrict__ idx,
                                                       const BoxRow* __restrict__ rows, int rounds, float omg, const float2* __restrict__ tw,
                                                       const float* __restrict__ win, float2* __restrict__ out) {
    using G = SepGeomT<N>;
    extern __shared__ float2 sep_lds[];
    constexpr int NQ = (N / 2) / G::T + 1;                        // pairs per thread (the last one: lt == 0 alone)
    const int item = threadIdx.x / G::T, lt = threadIdx.x % G::T;
    float2* buf = sep_lds + item * G::PITCH;
    BoxRow* stage = (BoxRow*)(sep_lds + G::ITEMS * G::PITCH) + item * kBoxStage;
    const int64_t rec = (int64_t)blockIdx.x * G::ITEMS + item;
    const bool valid = rec < n_fr;
    const int pair = blockIdx.y, npairs = gridDim.y, c0 = 2 * pair, c1 = 2 * pair + 1;
    BoxFrame f{0, 0, 0};
    if (valid) f = fr[rec];
    sep_frame_body<N>(pcm, format, channels, frames, f.k, valid, hop, c0, c1, buf, lt, tw, win, out + ((size_t)rec * npairs + pair) * N, [&]() {
        float ga[NQ], gb[NQ];
#pragma unroll
        for (int t = 0; t < NQ; ++t) ga[t] = gb[t] = 1.f;
        for (int r = 0; r < rounds; ++r) {
            const int n = min(max(f.count - r * kBoxStage, 0), kBoxStage);
            for (int j = lt; j < n; j += G::T) stage[j] = rows[idx[f.first + r * kBoxStage + j]];
            __syncthreads();
            for (int j = 0; j < n; ++j) {
                const BoxRow b = stage[j];
                const bool ona = b.channel < 0 || b.channel == c0;
                const bool onb = c1 < channels ? (b.channel < 0 || b.channel == c1) : ona;
#pragma unroll
                for (int t = 0; t < NQ; ++t) {
                    const float g = box_gain(b, lt + t * G::T, omg);
                    if (ona) ga[t] = fminf(ga[t], g);
                    if (onb) gb[t] = fminf(gb[t], g);
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            const int q = lt + t * G::T;
            if (q <= N / 2) sep_pair_gains<N>(buf, q, ga[t], gb[t]);
        }
    });
}

// Output sample `idx` (of total x channels) of the pieces in segs (out0 ascending): p = the four frames over the sample, added in
// ascending frame order; y = x + w (p - x) over the fade ramps.  at: the sample's index n channels + c in the recording.
__device__ __forceinline__ float sep_blend_sample(const unsigned char* __restrict__ pcm, int format, int channels, const SepSeg* __restrict__ segs,
                                                  int n_segs, int hop, int N, int npairs, const float2* __restrict__ fout, int64_t F, int64_t idx,
                                                  int64_t& at) {
#pragma clang fp contract(off)
    const int64_t t = idx / channels;
    const int c = (int)(idx - t * channels);
    int lo = 0, hi = n_segs - 1;                             // last piece with out0 <= t
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].out0 <= t) lo = mid; else hi = mid - 1;
    }
    const SepSeg sg = segs[lo];
    const int64_t n = sg.s0 + (t - sg.out0);
    const int64_t kb = n / hop;                              // frames kb - 1 .. kb + 2 hold sample n (N = 4 hop)
    float p = 0.f;
    for (int64_t k = kb - 1; k <= kb + 2; ++k) {
        const float2 v = fout[((size_t)(sg.rec0 + (k - sg.k0)) * npairs + (c >> 1)) * N + (n - k * hop + N / 2)];
        p += (c & 1) ? v.y : v.x;
    }
    at = n * channels + c;
    const float x = decode_sample(pcm, format, at);
    const int64_t d = std::min(n - sg.a, sg.b - 1 - n);
    const float w = d < F ? (float)(0.5 - 0.5 * cospi(((double)d + 0.5) / (double)F)) : 1.0f;
    return x + w * (p - x);
}

// The blend over `total` samples x channels, launched (and recorded) as sep_blend_kernel (Out = short): encoded as silence_encode_kernel
// encodes, lrintf(y * 32767), no clipping -- and as sep_blend_source_kernel (Out = unsigned char): the recording's own encoding (dsp.h
// encode_sample: the decode's scale, saturated) over a copy of the PCM, whose bytes outside the intervals stay the input's.
template <typename Out>
__global__ __launch_bounds__(256) void sep_blend_form_kernel(const unsigned char* __restrict__ pcm, int format, int channels,
                                                             const SepSeg* __restrict__ segs, int n_segs, int64_t total, int hop, int N,
                                                             int npairs, const float2* __restrict__ fout, int64_t F, Out* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t all = total * channels;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < all; idx += (int64_t)gridDim.x * 256) {
        int64_t at;
        const float y = sep_blend_sample(pcm, format, channels, segs, n_segs, hop, N, npairs, fout, F, idx, at);
        if constexpr (std::is_same_v<Out, short>) out[at] = (short)__float2int_rn(y * 32767.0f);
        else encode_sample(out, format, at, y);
    }
}

// =========================================================================================================
// host: device runs
// =========================================================================================================
static SepState& sep_state(ss_ctx* c) { return c->sep ? *c->sep : *(c->sep = new SepState()); }
void free_separation(ss_ctx* c) { delete c->sep; c->sep = nullptr; }      // (every buffer of SepState frees itself)

// HTK mel points of the front-end's filterbank recipe (weights.hip build_tables: torchaudio's, in float32)
static std::vector<double> mel_points() {
    std::vector<double> f(130);
    const float mmin = 0.f, mmax = (float)(2595.0 * std::log10(1.0 + 8000.0 / 700.0));
    const float step = (mmax - mmin) / 129.0f;
    for (int i = 0; i < 130; ++i) {
        const float mp = i < 65 ? mmin + step * (float)i : mmax - step * (float)(129 - i);
        f[i] = (double)(700.0f * (powf(10.0f, mp / 2595.0f) - 1.0f));
    }
    return f;
}

static int sep_tables(ss_ctx* c, int sr, SepTables** out) {
    SepTables& tb = sep_state(c).tables[sr];
    *out = &tb;
    if (tb.N) return SS_OK;                                       // (N is set behind the last upload)
    const int N = sep_fft_size(sr);
    const double PI = 3.14159265358979323846;
    std::vector<float2> tw(N);
    std::vector<float> win(N);
    for (int t = 0; t < N; ++t) {
        tw[t] = make_float2((float)std::cos(-2.0 * PI * t / N), (float)std::sin(-2.0 * PI * t / N));
        win[t] = (float)(0.5 - 0.5 * std::cos(2.0 * PI * t / N));           // periodic Hann
    }
    const std::vector<double> fp = mel_points();
    std::vector<SepBand> band(N / 2 + 1);
    for (int q = 0; q <= N / 2; ++q) {
        const double f = (double)q * sr / N;
        SepBand b{0, 0, 1.f, 0.f};
        if (f >= 8000.0) b.m0 = b.m1 = -1;
        else if (q > 0) {
            int m0 = -1; double t0 = 0, t1 = 0;
            for (int m = 0; m < 128; ++m) {
                const double T = std::max(0.0, std::min((f - fp[m]) / (fp[m + 1] - fp[m]), (fp[m + 2] - f) / (fp[m + 2] - fp[m + 1])));
                if (T > 0) { if (m0 < 0) { m0 = m; t0 = T; } else { t1 = T; break; } }
            }
            if (m0 < 0) b.m0 = b.m1 = f >= fp[128] ? 127 : 0;                // between the last point and 8 kHz: the edge band
            else { b.m0 = m0; b.m1 = t1 > 0 ? m0 + 1 : m0; b.w0 = (float)(t0 / (t0 + t1)); b.w1 = (float)(t1 / (t0 + t1)); }
        }
        band[q] = b;
    }
    int rc;
    if ((rc = tb.tw.reserve(c, N)) || (rc = tb.win.reserve(c, N)) || (rc = tb.band.reserve(c, band.size()))) return rc;
    HIPCHK(c, hipMemcpy(tb.tw.p, tw.data(), N * sizeof(float2), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(tb.win.p, win.data(), N * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(tb.band.p, band.data(), band.size() * sizeof(SepBand), hipMemcpyHostToDevice));
    tb.N = N;
    return SS_OK;
}

// Step 1 (+ 2): the spec head over the windows win_ranges (merged, ascending) of file fid, averaged over the bins bin_ranges (merged,
// ascending) -> st.map [2][ncb][128]; with gains (params non-null): st.gain [ncb][128].  Returns SS_ERR_RANGE when an f16x2 pass
// left the f16 range.  nsig > 1 (ss_separate_pcm_channels): the same for each of the files fid .. fid + nsig - 1, whose windows follow
// one another in one run list -- a pass ends where the chunk is full, not where a signal ends -- -> map [nsig][2][ncb][128],
// gain [nsig][ncb][128].
static int sep_run_maps(ss_ctx* c, int fid, int nsig, int64_t W, const Ranges& bin_ranges, const Ranges& win_ranges,
                        const ss_separation_params* params, int64_t& ncb_out) {
    SepState& st = sep_state(c);
    std::vector<int64_t> sig_off;
    for (int s = 0; s < nsig; ++s) sig_off.push_back(c->files[fid + s].off);
    MapsPlan mp;
    if (!plan_maps(bin_ranges, win_ranges, W, nsig, sig_off.data(), mp)) return fail(c, SS_ERR_ARG, "separation: too many windows");
    const int ncb = mp.ncb, nw = mp.nw, nw_all = (int)mp.off.size();
    ncb_out = ncb;
    if (ncb == 0 || nw == 0) return SS_OK;
    const size_t ns = (size_t)nsig;
    int rc;
    if ((rc = st.cbin.reserve(c, (size_t)ncb)) || (rc = st.slot.reserve(c, (size_t)W)) || (rc = st.sum.reserve(c, ns * ncb * 256)) ||
        (rc = st.count.reserve(c, ns * ncb)) || (rc = st.map.reserve(c, ns * ncb * 256)) || (params && (rc = st.gain.reserve(c, ns * ncb * 128))))
        return rc;
    HIPCHK(c, hipMemcpyAsync(st.cbin.p, mp.cbin.data(), (size_t)ncb * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(st.slot.p, mp.slot.data(), (size_t)W * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(st.sum.p, 0, ns * ncb * 256 * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(st.count.p, 0, ns * ncb * 4, c->stream));
    if ((rc = upload_winoff(c, mp.off))) return rc;               // (synchronises: the plan's vectors are free again)
    const int ch = std::min(nw_all, c->chunk);
    if ((rc = ensure_workspace(c, ch))) return rc;
    if ((rc = ensure(c, &c->d_logits, &c->logits_cap, (size_t)ch * 256))) return rc;
    if ((rc = ensure(c, &c->d_spec, &c->spec_cap, (size_t)ch * 2 * 32768))) return rc;
    c->logits_valid = false;
    if ((rc = range_clear(c, c->stream))) return rc;
    for (int p0 = 0; p0 < nw_all; p0 += ch) {
        const int m = std::min(ch, nw_all - p0);
        if ((rc = forward_chunk(c, c->ws[0], c->stream, c->d_arena, c->d_winoff + p0, m, c->d_logits, c->d_spec))) return rc;
        ScopedLaunch sl(c, c->stream, "sep_accumulate_kernel", 256.0 * ncb * 6 * nsig, (double)ncb * 256 * 16 * nsig);
        hipLaunchKernelGGL(sep_accumulate_kernel, dim3((unsigned)((ncb + 255) / 256), 256, (unsigned)nsig), dim3(256), 0, c->stream, c->d_spec, p0, m,
                           st.slot.p, (int)W, nw, st.cbin.p, ncb, st.sum.p, st.count.p);
        HIPCHK(c, hipGetLastError());
    }
    {
        const int sp = params ? params->speech_channel : 1;
        const double mg = params ? params->min_gain : 0.0;
        ScopedLaunch sl(c, c->stream, "sep_finalize_kernel", 0.0, (double)ncb * 128 * (16 + 8 + (params ? 4 : 0)) * nsig);
        hipLaunchKernelGGL(sep_finalize_kernel, dim3((unsigned)((ncb * 128 + 255) / 256), (unsigned)nsig), dim3(256), 0, c->stream, st.sum.p,
                           st.count.p, ncb, st.map.p, params ? st.gain.p : nullptr, sp, mg);
        HIPCHK(c, hipGetLastError());
    }
    if (c->d_range_flag) {
        if ((rc = range_fetch(c, c->stream))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (range_left(c))
            return fail(c, SS_ERR_RANGE, "f16x2: an activation of the spec head left the f16 range (|x| > 65504) or was not finite; run this file with the fp32 mode");
    }
    return SS_OK;
}

int separation_maps(ss_ctx* c, int fid, int64_t first_bin, int64_t n_bins, float* out) {
    const FileRec& f = c->files[fid];
    int64_t W, nb;
    file_geometry(f.duration, f.n_padded, W, nb);
    if (n_bins < 1 || first_bin < 0 || first_bin + n_bins > nb)
        return fail(c, SS_ERR_ARG, "ss_separation_maps: bins [" + std::to_string(first_bin) + ", " + std::to_string(first_bin + n_bins) +
                                       ") are not all covered by a window (covered: [0, " + std::to_string(nb) + "))");
    int64_t w0, w1, ncb;
    covering_windows(first_bin, first_bin + n_bins - 1, W, w0, w1);
    int rc = sep_run_maps(c, fid, 1, W, {{first_bin, first_bin + n_bins - 1}}, {{w0, w1}}, nullptr, ncb);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(out, sep_state(c).map.p, (size_t)n_bins * 256 * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SS_OK;
}

// The STFT launch of FFT size N = 256 << i, from a table of the twelve instantiations.  each: sep_stft_each_kernel<N> with the gain
// tables gain + c gain_cs; otherwise sep_stft_kernel<N> with the one table.
struct SepStftForm { decltype(&sep_stft_form_kernel<256, false>) kernel[2]; int items, pitch; };
template <int N> static constexpr SepStftForm sep_stft_form() { return {{sep_stft_form_kernel<N, false>, sep_stft_form_kernel<N, true>}, SepGeomT<N>::ITEMS, SepGeomT<N>::PITCH}; }
static hipError_t launch_sep_stft(int N, bool each, const void* pcm, int format, int channels, int64_t frames, const SepFrame* fr, int n_fr, int hop,
                                  const float* gain, size_t gain_cs, const SepTables& tb, float gain_hi, float2* out, hipStream_t s) {
    static const SepStftForm forms[6] = {sep_stft_form<256>(), sep_stft_form<512>(), sep_stft_form<1024>(),
                                         sep_stft_form<2048>(), sep_stft_form<4096>(), sep_stft_form<8192>()};
    static std::atomic<uint64_t> attr_done[6][2];                 // (per device: kernels.h allow_full_lds), one per kernel
    int i = 0;
    while (i < 6 && (256 << i) != N) ++i;
    if (i == 6) return hipErrorInvalidValue;
    const SepStftForm& f = forms[i];
    const size_t lds = (size_t)f.items * (f.pitch * sizeof(float2) + (each ? 256 : 128) * sizeof(float));
    const dim3 grid((unsigned)((n_fr + f.items - 1) / f.items), (unsigned)((channels + 1) / 2));
    if (hipError_t e = allow_full_lds((const void*)f.kernel[each], attr_done[i][each])) return e;
    hipLaunchKernelGGL(f.kernel[each], grid, dim3(256), lds, s, (const unsigned char*)pcm, format, channels, frames, fr, n_fr, hop, gain,
                       tb.band.p, tb.tw.p, tb.win.p, gain_hi, out, each ? gain_cs : (size_t)0);
    return hipGetLastError();
}

static constexpr size_t kSepFrameBytes = (size_t)256 << 20;      // most bytes of resynthesised frames held at once (pieces / chunks)

// Step 4 over one chunk's segments (uploaded to st.segs) and the frame buffer: sep_blend_kernel into d_sil_out, or (src)
// sep_blend_source_kernel into d_src_out.  The band silencer launches it as the separation silencer does.
static int launch_sep_blend(ss_ctx* c, bool src, int format, int ch, const SepChunk& ck, int hop, int N, int64_t F) {
    SepState& st = sep_state(c);
    const int npairs = (ch + 1) / 2;
    const int64_t all = ck.total * ch;
    const unsigned gx = (unsigned)std::min<int64_t>((all + 255) / 256, 16384);
    if (src) {
        ScopedLaunch sl(c, c->stream, "sep_blend_source_kernel", 0.0, (double)all * (16.0 + 2.0 * pcm_bytes_per_sample(format)));
        hipLaunchKernelGGL(sep_blend_form_kernel<unsigned char>, dim3(gx), dim3(256), 0, c->stream, (const unsigned char*)c->d_pcm, format, ch,
                           st.segs.p + ck.seg0, (int)ck.nseg, ck.total, hop, N, npairs, st.fout.p, F, c->d_src_out);
        HIPCHK(c, hipGetLastError());
        return SS_OK;
    }
    ScopedLaunch sl(c, c->stream, "sep_blend_kernel", 0.0, (double)all * (16.0 + pcm_bytes_per_sample(format) + 2.0));
    hipLaunchKernelGGL(sep_blend_form_kernel<short>, dim3(gx), dim3(256), 0, c->stream, (const unsigned char*)c->d_pcm, format, ch,
                       st.segs.p + ck.seg0, (int)ck.nseg, ck.total, hop, N, npairs, st.fout.p, F, c->d_sil_out);
    HIPCHK(c, hipGetLastError());
    return SS_OK;
}

// each (ss_separate_pcm_channels, ch > 1): the signals are the channels alone, every channel's STFT gets the gains of its own maps
// src: the output in the recording's own encoding (out: frames x ch x bytes-per-sample bytes) -- a device copy of the PCM in place of
// the transcode, sep_blend_source_kernel in place of sep_blend_kernel; otherwise out is int16
int separate_run(ss_ctx* c, bool each, bool src, const void* pcm, int format, int sr, int ch, int64_t frames, const ss_region* regions,
                 int64_t n_regions, const ss_separation_params* params, void* out) {
    const ss_separation_params prm = params ? *params : separation_defaults();
    SepPlan pl;
    separation_plan(sr, frames, regions, n_regions, pl);
    int rc, fid = -1;
    if ((rc = ss_reset(c))) return rc;
    if (each) rc = ss_add_pcm_channels(c, pcm, format, sr, ch, frames, &fid);  // signals in the arena, samples in c->d_pcm
    else rc = ss_add_pcm(c, pcm, format, sr, ch, frames, &fid);
    if (rc) return rc;
    if (frames == 0) return SS_OK;
    SepState& st = sep_state(c);
    const size_t total = (size_t)frames * ch, pcm_bytes = total * pcm_bytes_per_sample(format);
    if (src) {   // the recording's own bytes: what ss_silence_pcm_source writes outside its ranges
        if ((rc = ensure(c, &c->d_src_out, &c->src_out_cap, pcm_bytes + 16))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->d_src_out, c->d_pcm, pcm_bytes, hipMemcpyDeviceToDevice, c->stream));
    } else {     // the transcode of the whole file: what ss_silence_pcm writes outside its ranges
        if ((rc = ensure(c, &c->d_sil_out, &c->sil_out_cap, total + 8))) return rc;
        ScopedLaunch sl(c, c->stream, "sep_transcode/silence_encode_kernel", 0.0, (double)total * pcm_bytes_per_sample(format) + 2.0 * (double)total);
        HIPCHK(c, launch_silence_encode(c->d_pcm, format, ch, frames, nullptr, 0, c->d_sil_out, c->stream));
    }
    SynthPlan sp;                                                 // (its frames and segments are uploaded from: alive until the last synchronise)
    if (!pl.ranges.empty()) {
        const int N = pl.N, hop = pl.hop, npairs = (ch + 1) / 2;
        // steps 1 + 2 over the merged bin and window ranges
        const SepRanges rg = plan_ranges(pl);
        int64_t ncb = 0;
        if ((rc = sep_run_maps(c, fid, each ? ch : 1, pl.W, rg.br, rg.wr, &prm, ncb))) return rc;
        // step 3 + 4, chunk by chunk of the frame buffer; the frames are planned here, behind the launches of the model passes
        SepTables* tb = nullptr;
        if ((rc = sep_tables(c, sr, &tb))) return rc;
        int64_t budget = (int64_t)(kSepFrameBytes / ((size_t)npairs * N * sizeof(float2)));
#ifdef SS_DEVBUILD      // ss_debug_set_separation_budget: the tests move the piece and chunk cuts through short recordings
        if (c->sep_budget > 0) budget = c->sep_budget;
#endif
        sp = plan_synthesis(pl, rg.cbase, sr, ch, std::max<int64_t>(16, budget));
        if ((rc = st.frames.reserve(c, sp.fr.size())) || (rc = st.segs.reserve(c, sp.sg.size())) || (rc = st.fout.reserve(c, sp.fout_need))) return rc;
        HIPCHK(c, hipMemcpyAsync(st.frames.p, sp.fr.data(), sp.fr.size() * sizeof(SepFrame), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(st.segs.p, sp.sg.data(), sp.sg.size() * sizeof(SepSeg), hipMemcpyHostToDevice, c->stream));
        const float gain_hi = prm.above_fmax == SS_ABOVE_FMAX_KEEP ? 1.0f : (float)prm.min_gain;
        const int64_t F = (int64_t)std::nearbyint(prm.fade_s * sr);
        const std::string stft_name = (each ? "sep_stft_each_kernel<" : "sep_stft_kernel<") + std::to_string(N) + ">";
        for (const SepChunk& ck : sp.chunks) {
            {
                const double lg = std::log2((double)N);
                ScopedLaunch sl(c, c->stream, stft_name, 2.0 * (double)ck.nrec * npairs * (5.0 * N * lg + 8.0 * N),
                                (double)ck.nrec * npairs * N * (2.0 * pcm_bytes_per_sample(format) + 8.0));
                HIPCHK(c, launch_sep_stft(N, each, c->d_pcm, format, ch, frames, st.frames.p + ck.rec0, (int)ck.nrec, hop, st.gain.p,
                                            (size_t)ncb * 128, *tb, gain_hi, st.fout.p, c->stream));
            }
            if ((rc = launch_sep_blend(c, src, format, ch, ck, hop, N, F))) return rc;
        }
    }
    if (src) HIPCHK(c, hipMemcpyAsync(out, c->d_src_out, pcm_bytes, hipMemcpyDeviceToHost, c->stream));
    else HIPCHK(c, hipMemcpyAsync(out, c->d_sil_out, total * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                   // the plan and the caller's buffers are free again
    return SS_OK;
}

// =========================================================================================================
// band silencer (include/softspoken.h "band silencer"): separate_run without the model -- the gains come from the box table
//
//   plan   (sep_plan.h plan_boxes) merged intervals, a row per box, every frame's active boxes; plan_synthesis' pieces and chunks
//   per chunk   box_stft_kernel<N> -> the frame buffer;  sep_blend_kernel / sep_blend_source_kernel as separate_run launches them
// The recording is in c->d_pcm already (the caller staged it, as ss_silence_pcm does); the job's files and streams are not touched.
// =========================================================================================================
static hipError_t launch_box_stft(int N, const void* pcm, int format, int channels, int64_t frames, const BoxFrame* fr, int n_fr, int hop,
                                  const int32_t* idx, const BoxRow* rows, int rounds, float omg, const SepTables& tb, float2* out, hipStream_t s) {
    using Kernel = decltype(&box_stft_kernel<256>);
    static const Kernel forms[6] = {box_stft_kernel<256>, box_stft_kernel<512>, box_stft_kernel<1024>,
                                    box_stft_kernel<2048>, box_stft_kernel<4096>, box_stft_kernel<8192>};
    static const int items[6] = {SepGeomT<256>::ITEMS, SepGeomT<512>::ITEMS, SepGeomT<1024>::ITEMS, SepGeomT<2048>::ITEMS, SepGeomT<4096>::ITEMS, SepGeomT<8192>::ITEMS};
    static std::atomic<uint64_t> attr_done[6];                    // (per device: kernels.h allow_full_lds)
    int i = 0;
    while (i < 6 && (256 << i) != N) ++i;
    if (i == 6) return hipErrorInvalidValue;
    const size_t lds = (size_t)items[i] * ((size_t)(N + N / 16) * sizeof(float2) + kBoxStage * sizeof(BoxRow));
    const dim3 grid((unsigned)((n_fr + items[i] - 1) / items[i]), (unsigned)((channels + 1) / 2));
    if (hipError_t e = allow_full_lds((const void*)forms[i], attr_done[i])) return e;
    hipLaunchKernelGGL(forms[i], grid, dim3(256), lds, s, (const unsigned char*)pcm, format, channels, frames, fr, n_fr, hop, idx, rows, rounds, omg,
                       tb.tw.p, tb.win.p, out);
    return hipGetLastError();
}

int box_run(ss_ctx* c, bool src, int format, int sr, int ch, int64_t frames, const ss_box* boxes, int64_t n_boxes, const ss_box_params* params,
            void* out) {
    const ss_box_params prm = params ? *params : box_defaults();
    const int npairs = (ch + 1) / 2;
    int64_t budget = (int64_t)(kSepFrameBytes / ((size_t)npairs * sep_fft_size(sr) * sizeof(float2)));
#ifdef SS_DEVBUILD      // ss_debug_set_separation_budget moves these cuts as it moves separate_run's
    if (c->sep_budget > 0) budget = c->sep_budget;
#endif
    BoxPlan bp;                                                   // (uploaded from: alive until the last synchronise)
    if (!plan_boxes(sr, frames, ch, boxes, n_boxes, prm, std::max<int64_t>(16, budget), bp))
        return fail(c, SS_ERR_ARG, "band silencer: too many boxes lie over one another");
    SepState& st = sep_state(c);
    const size_t total = (size_t)frames * ch, pcm_bytes = total * pcm_bytes_per_sample(format);
    int rc;
    if (src) {   // the recording's own bytes: what ss_silence_pcm_source writes outside its ranges
        if ((rc = ensure(c, &c->d_src_out, &c->src_out_cap, pcm_bytes + 16))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->d_src_out, c->d_pcm, pcm_bytes, hipMemcpyDeviceToDevice, c->stream));
    } else {     // the transcode of the whole file: what ss_silence_pcm writes outside its ranges
        if ((rc = ensure(c, &c->d_sil_out, &c->sil_out_cap, total + 8))) return rc;
        ScopedLaunch sl(c, c->stream, "box_transcode/silence_encode_kernel", 0.0, (double)total * pcm_bytes_per_sample(format) + 2.0 * (double)total);
        HIPCHK(c, launch_silence_encode(c->d_pcm, format, ch, frames, nullptr, 0, c->d_sil_out, c->stream));
    }
    if (!bp.chunks.empty()) {
        const int N = bp.N, hop = bp.hop;
        SepTables* tb = nullptr;
        if ((rc = sep_tables(c, sr, &tb))) return rc;
        if ((rc = st.bframes.reserve(c, bp.fr.size())) || (rc = st.bidx.reserve(c, bp.idx.size())) || (rc = st.brows.reserve(c, bp.rows.size())) ||
            (rc = st.segs.reserve(c, bp.sg.size())) || (rc = st.fout.reserve(c, bp.fout_need)))
            return rc;
        HIPCHK(c, hipMemcpyAsync(st.bframes.p, bp.fr.data(), bp.fr.size() * sizeof(BoxFrame), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(st.bidx.p, bp.idx.data(), bp.idx.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(st.brows.p, bp.rows.data(), bp.rows.size() * sizeof(BoxRow), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(st.segs.p, bp.sg.data(), bp.sg.size() * sizeof(SepSeg), hipMemcpyHostToDevice, c->stream));
        const int64_t F = (int64_t)std::nearbyint(prm.fade_s * sr);
        const int rounds = (bp.max_count + kBoxStage - 1) / kBoxStage;
        const std::string stft_name = "box_stft_kernel<" + std::to_string(N) + ">";
        for (const SepChunk& ck : bp.chunks) {
            {
                const double lg = std::log2((double)N);
                ScopedLaunch sl(c, c->stream, stft_name, 2.0 * (double)ck.nrec * npairs * (5.0 * N * lg + 8.0 * N),
                                (double)ck.nrec * npairs * N * (2.0 * pcm_bytes_per_sample(format) + 8.0));
                HIPCHK(c, launch_box_stft(N, c->d_pcm, format, ch, frames, st.bframes.p + ck.rec0, (int)ck.nrec, hop, st.bidx.p, st.brows.p, rounds,
                                            (float)(1.0 - prm.min_gain), *tb, st.fout.p, c->stream));
            }
            if ((rc = launch_sep_blend(c, src, format, ch, ck, hop, N, F))) return rc;
        }
    }
    if (src) HIPCHK(c, hipMemcpyAsync(out, c->d_src_out, pcm_bytes, hipMemcpyDeviceToHost, c->stream));
    else HIPCHK(c, hipMemcpyAsync(out, c->d_sil_out, total * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                   // the plan and the caller's buffers are free again
    return SS_OK;
}

// =========================================================================================================
// region bands (include/softspoken.h "region bands"): the maps of step 1 reduced on the device to each region's band bounds
//
//   plan   (sep_plan.h plan_bands) rule 1 per region -> the disjoint union of the regions' bin ranges (sep_run_maps' bin_ranges), cut at
//          absolute tile boundaries into pieces of at most kBandsPieceBins bins -> segments (region, tile) over the piece that holds the tile
//   per piece   sep_run_maps -> d_map [nsig][2][ncb][128];  band_profile_kernel: one tile sum [256] per (segment, signal)
//   at the end  band_bounds_kernel: per (region, signal) the tile sums added in ascending tile order -> E, C, the bounds
// =========================================================================================================
static constexpr int64_t kBandsPieceBins = 16384;      // most bins of one sep_run_maps round: 48 MB of sums and maps per signal

// Block = one segment of one signal (blockIdx.y), thread = (spec channel, band): the sequential ascending sum of P over the segment's
// bins (at most 64: one tile's share of a region).  A bin row of a channel is 128 consecutive floats: the loads of a wave are 256 B
// runs.  part [nsig][nseg_total][256].
__global__ __launch_bounds__(256) void band_profile_kernel(const float* __restrict__ map, int ncb, const BandSeg* __restrict__ segs,
                                                           int nseg_total, double* __restrict__ part) {
    const BandSeg sg = segs[blockIdx.x];
    const int sig = blockIdx.y, ch = threadIdx.x >> 7, m = threadIdx.x & 127;
    const float* p = map + (((size_t)sig * 2 + ch) * ncb + sg.cb0) * 128 + m;
    double s = 0.0;
    for (int i = 0; i < sg.n; ++i) s += band_power(p[(size_t)i * 128]);
    part[((size_t)sig * nseg_total + sg.out) * 256 + threadIdx.x] = s;
}

// Block = one region of one signal (blockIdx.y).  Every thread adds its (channel, band)'s tile sums in ascending tile order; the bounds
// are band_bounds_block's (bands.h, shared with the streams' kernel).  out [n][nsig], profile (nullable) [n][nsig][2][128].
__global__ __launch_bounds__(256) void band_bounds_kernel(const double* __restrict__ part, int nseg_total, const BandRegion* __restrict__ regs,
                                                          int speech_ch, double q_low, double q_high, const double* __restrict__ hz,
                                                          ss_region_band* __restrict__ out, double* __restrict__ profile) {
#pragma clang fp contract(off)
    const int r = blockIdx.x, sig = blockIdx.y, nsig = gridDim.y, t = threadIdx.x;
    const BandRegion rg = regs[r];
    const double* p = part + ((size_t)sig * nseg_total + rg.seg0) * 256 + t;
    double e = 0.0;
    for (int k = 0; k < rg.nseg; ++k) e += p[(size_t)k * 256];
    if (profile) profile[((size_t)r * nsig + sig) * 256 + t] = e;
    band_bounds_block(e, rg.n_bins, speech_ch, q_low, q_high, hz, out + ((size_t)r * nsig + sig));
}

// the front-end's own table of band edges (weights.hip), not mel_points() above: the two differ by a float32 ulp at 19 edges, and a
// band's reported frequency is the edge its features were computed with
void band_edges(double* hz130) {
    const float* f = mel_edges_hz();
    for (int i = 0; i < 130; ++i) hz130[i] = (double)f[i];
}

int region_bands(ss_ctx* c, const float* maps, int fid, int nsig, int64_t first_bin, int64_t n_bins, const ss_region* regions, int64_t n,
                 const ss_band_params* params, ss_region_band* out, double* profile) {
    if (n == 0) return SS_OK;
    const ss_band_params prm = params ? *params : ss_band_params{0.05, 0.95, 1, 0};
    SepState& st = sep_state(c);
    int64_t W = 0, lo = first_bin, hi = first_bin + n_bins;
    if (!maps) {
        const FileRec& f = c->files[fid];
        for (int s = 1; s < nsig; ++s)
            if (c->files[fid + s].n_padded != f.n_padded || c->files[fid + s].duration != f.duration)
                return fail(c, SS_ERR_ARG, "ss_region_bands: the files are not the channels of one recording");
        file_geometry(f.duration, f.n_padded, W, hi);
        lo = 0;
    }
    int64_t budget = kBandsPieceBins;
#ifdef SS_DEVBUILD      // ss_debug_set_bands_budget: the tests move the cuts through a short recording
    if (c->bands_budget > 0) budget = std::max<int64_t>(64, c->bands_budget);
#endif
    BandsPlan bp;
    if (!plan_bands(regions, n, lo, hi, maps != nullptr, budget, W, bp)) return fail(c, SS_ERR_ARG, "ss_region_bands: too many region tiles");
    const size_t ns = (size_t)nsig;
    int rc;
    if ((rc = st.bseg.reserve(c, std::max<size_t>(bp.segs.size(), 1))) || (rc = st.breg.reserve(c, (size_t)n)) ||
        (rc = st.bpart.reserve(c, std::max<size_t>((size_t)bp.nseg_total * ns * 256, 1))) || (rc = st.bout.reserve(c, (size_t)n * ns)) ||
        (profile && (rc = st.bprof.reserve(c, (size_t)n * ns * 256))))
        return rc;
    if (!st.hz.p) {
        double f[130];
        band_edges(f);
        if ((rc = st.hz.reserve(c, 130))) return rc;
        HIPCHK(c, hipMemcpy(st.hz.p, f, sizeof f, hipMemcpyHostToDevice));
    }
    if (!bp.segs.empty()) HIPCHK(c, hipMemcpy(st.bseg.p, bp.segs.data(), bp.segs.size() * sizeof(BandSeg), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(st.breg.p, bp.regs.data(), (size_t)n * sizeof(BandRegion), hipMemcpyHostToDevice));
    for (const BandPiece& pc : bp.pieces) {
        if (!pc.nseg) continue;
        int64_t ncb = pc.ncb;
        if (maps) {
            if ((rc = st.map.reserve(c, ns * (size_t)n_bins * 256))) return rc;
            HIPCHK(c, hipMemcpyAsync(st.map.p, maps, ns * (size_t)n_bins * 256 * 4, hipMemcpyHostToDevice, c->stream));
        } else {
            if ((rc = sep_run_maps(c, fid, nsig, W, pc.br, pc.wr, nullptr, ncb))) return rc;
            if (ncb != pc.ncb) return fail(c, SS_ERR_HIP, "ss_region_bands: the maps do not hold the piece's bins");
        }
        ScopedLaunch sl(c, c->stream, "band_profile_kernel", 0.0, (double)pc.nseg * ns * (64.0 * 256 * 4 + 256 * 8));
        hipLaunchKernelGGL(band_profile_kernel, dim3((unsigned)pc.nseg, (unsigned)nsig), dim3(256), 0, c->stream, st.map.p, (int)ncb,
                           st.bseg.p + pc.seg0, (int)bp.nseg_total, st.bpart.p);
        HIPCHK(c, hipGetLastError());
    }
    {
        ScopedLaunch sl(c, c->stream, "band_bounds_kernel", 0.0, (double)bp.nseg_total * ns * 256 * 8 + (double)n * ns * (48 + (profile ? 2048 : 0)));
        hipLaunchKernelGGL(band_bounds_kernel, dim3((unsigned)n, (unsigned)nsig), dim3(256), 0, c->stream, st.bpart.p, (int)bp.nseg_total, st.breg.p,
                           prm.speech_channel, prm.q_low, prm.q_high, st.hz.p, st.bout.p, profile ? st.bprof.p : nullptr);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(out, st.bout.p, (size_t)n * ns * sizeof(ss_region_band), hipMemcpyDeviceToHost, c->stream));
    if (profile) HIPCHK(c, hipMemcpyAsync(profile, st.bprof.p, (size_t)n * ns * 256 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SS_OK;
}

}  // namespace ss
