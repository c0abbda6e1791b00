// Ingest kernels for gfx950: PCM decode + mixdown, the polyphase resampler in its three forms, and their per-channel twins.  The
// geometries the launchers take, the tap table and the plan of a batch call are ingest_plan.h's; abi.hip's ingest_run issues the launches.
//
// Reference: root/code/backend/voice_activity.py:32-69 (load_audio).
#include "dsp.h"
#include "kernels.h"
#include <algorithm>

namespace ss {

// =========================================================================================================
// PCM -> float32 mono.  libsndfile's float conversion (x / 2^(bits-1); unsigned 8-bit is offset by 128: dsp.h decode_sample),
// then librosa.to_mono == mean over channels in float32 (voice_activity.py:37-38, 61-62).
// =========================================================================================================
// =========================================================================================================
// Polyphase Kaiser-windowed-sinc resampler to 22 050 Hz (stands where librosa.resample -> soxr_hq stands,
// voice_activity.py:65-67).  out[m] = sum_j taps[(m M) mod L][j] * in[(m M) div L + j - half + 1].
// float32 multiply then add in tap order (no FMA contraction) so the CPU oracle can match it bit for bit.
// =========================================================================================================
// One launch covers every file of a batch (files share format / rate / channels); a single file is a batch of one.
__global__ __launch_bounds__(256) void decode_mono_batch_kernel(const unsigned char* __restrict__ pcm, int format, int channels,
                                                                const BatchFile* __restrict__ files, float* __restrict__ mono) {
    const BatchFile f = files[blockIdx.y];
    const int bps = format == 1 ? 1 : format == 2 ? 2 : format == 3 ? 3 : format == 6 ? 8 : 4;
    const unsigned char* base = pcm + f.pcm_off;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < f.frames; i += (int64_t)gridDim.x * 256) {
        float acc = decode_sample(base, format, i * channels);
        for (int c = 1; c < channels; ++c) acc = __fadd_rn(acc, decode_sample(base, format, i * channels + c));
        mono[f.mono_off + i] = channels > 1 ? __fdiv_rn(acc, (float)channels) : acc;
    }
    (void)bps;
}

__global__ __launch_bounds__(256) void resample_batch_kernel(const float* __restrict__ mono, const BatchFile* __restrict__ files, int L,
                                                             int M, int half, const float* __restrict__ taps, float* __restrict__ arena) {
#pragma clang fp contract(off)
    const BatchFile f = files[blockIdx.y];
    const float* in = mono + f.mono_off;
    float* out = arena + f.out_off;
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < f.n_out; m += (int64_t)gridDim.x * 256) {
        const int64_t pos = m * M;
        const int64_t base = pos / L;
        const int phase = (int)(pos - base * L);
        const float* tp = taps + (size_t)phase * (2 * half);
        float acc = 0.f;
        for (int j = 0; j < 2 * half; ++j) {
            const int64_t idx = base + j - half + 1;
            const float sv = (idx >= 0 && idx < f.frames) ? in[idx] : 0.f;
            { const float pr = tp[j] * sv; acc = acc + pr; }   // two roundings, as the oracle
        }
        out[m] = acc;
    }
}

// Same arithmetic with the whole polyphase table staged in LDS (rows padded to an odd pitch: lanes hold different
// phases of the same tap index, which would otherwise all hit one bank).  Used when L * (2 half + 1) floats fit.
// A block owns kResOut consecutive output samples of one file; 32-bit index math (positions relative to the block).
// (kResOut outputs, kResThreads threads: ingest_plan.h)
// Persistent: a block stages the table once and then walks (file, 4096-output chunk) items -- staging it per chunk was ~45 %
// of the kernel (4352 blocks x 115 KB for the C2 job).
__global__ __launch_bounds__(kResThreads) void resample_batch_lds_kernel(const float* __restrict__ mono, const BatchFile* __restrict__ files,
                                                                         int n_files, int chunks_per_file, int L, int M, int half, int span,
                                                                         const float* __restrict__ taps, float* __restrict__ arena) {
#pragma clang fp contract(off)
    extern __shared__ float s_taps[];
    const int nt = 2 * half, pitch = nt | 1;
    float* s_x = s_taps + L * pitch;                      // span > 0: the input samples an item touches, zero outside the file
    for (int p = threadIdx.x / 64; p < L; p += kResThreads / 64)              // one phase (row) per wave per pass: no division per element
        for (int j = threadIdx.x & 63; j < nt; j += 64) s_taps[p * pitch + j] = taps[p * nt + j];
    __syncthreads();
    const int n_items = n_files * chunks_per_file;
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int fi = item / chunks_per_file, chunk = item - fi * chunks_per_file;
        const BatchFile f = files[fi];
        const int64_t m0 = (int64_t)chunk * kResOut;
        if (m0 >= f.n_out) continue;                      // block-uniform
        const float* in = mono + f.mono_off;
        float* out = arena + f.out_off;
        const int64_t pos0 = m0 * M;
        const int64_t base0 = pos0 / L;
        const int ph0 = (int)(pos0 - base0 * L);              // position of output m0 is base0 + ph0 / L
        const int n_here = (int)((f.n_out - m0) < kResOut ? (f.n_out - m0) : kResOut);
        if (span > 0) {
            // stage x[i_lo .. i_lo + span): every tap of every output of the item reads LDS, and the file's ends need no test
            const int64_t i_lo = base0 - half + 1;
            for (int i = threadIdx.x; i < span; i += kResThreads) {
                const int64_t idx = i_lo + i;
                s_x[i] = (idx >= 0 && idx < f.frames) ? in[idx] : 0.f;
            }
            __syncthreads();
            for (int k = threadIdx.x; k < n_here; k += kResThreads) {
                const int rel = ph0 + k * M;                  // < L + 4096 * M, fits 32 bits for every audio rate
                const int db = rel / L;
                const float* tp = s_taps + (rel - db * L) * pitch;
                const float* xp = s_x + db;
                float acc = 0.f;
#pragma unroll 4
                for (int j = 0; j < nt; ++j) { const float pr = tp[j] * xp[j]; acc = acc + pr; }   // two roundings, as the oracle
                out[m0 + k] = acc;
            }
            __syncthreads();                              // s_x is rewritten by the next item
            continue;
        }
        for (int k = threadIdx.x; k < n_here; k += kResThreads) {
            const int rel = ph0 + k * M;
            const int db = rel / L;
            const int phase = rel - db * L;
            const int64_t base = base0 + db;
            const float* tp = s_taps + phase * pitch;
            float acc = 0.f;
            const int64_t i0 = base - half + 1;
            if (i0 >= 0 && i0 + nt <= f.frames) {
                for (int j = 0; j < nt; ++j) { const float pr = tp[j] * in[i0 + j]; acc = acc + pr; }
            } else {
                for (int j = 0; j < nt; ++j) {
                    const int64_t idx = i0 + j;
                    const float sv = (idx >= 0 && idx < f.frames) ? in[idx] : 0.f;
                    const float pr = tp[j] * sv; acc = acc + pr;
                }
            }
            out[m0 + k] = acc;
        }
    }
}

// Third form (round 3): decode + mixdown fused into the staging, four outputs per thread.
//   * Outputs m and m + L have the same phase (tap row) and inputs M apart, so a thread owns ONE phase p and four consecutive
//     "rows" r (outputs m0 + r L + p): a tap is read once for four multiply-adds.
//   * The input tile lies in LDS as X[u][v], u = i' mod M, v = i' div M (i' = input index from the tile's first sample): the four
//     rows' samples for tap j -- i' = r M + b(p) + j -- are FOUR CONSECUTIVE WORDS X[(b + j) mod M][(b + j) div M + r .. + 3], one
//     16-byte read.  b + j wraps past M at most once (the launch requires 2 half <= M); behind the wrap the row index is one higher,
//     which would make the read misaligned, so the rows u < 2 half exist a second time shifted by one (X1[u][v] = X[u][v + 1]).
//   * The tile is filled straight from the PCM: decode (x / 2^(bits-1)), channel mean in float32 -- decode_mono_batch_kernel's
//     arithmetic --, zero outside the file: no mono tensor is written or read (C5: 2 x 4 bytes per 48 kHz frame less HBM traffic
//     and one launch less).
// Arithmetic per output is unchanged -- float32 multiply then add, tap order, two roundings -- so both oracles still match bit for bit.
// LDS reads per multiply-add: 1/4 tap word + 1 sample word (second form: 1 + 1, and four-byte reads at half the LDS rate).
// (kRes3Threads, kRes3Stage and the geometry -- groups, pitch_v, lpg, LDS bytes: ingest_plan.h res3_geometry)
// FAST: 16-bit PCM, one or two channels (a frame is 2 or 4 bytes): the NEXT item's frames are requested as raw words before the
// current item's multiply loop and decoded behind it, so their latency hides behind the arithmetic.  Other formats decode at the
// request (all of a thread's requests go out together, but the tile waits for them).
// Which lane takes which phase (round 4).  A thread reads X[b(p) + j][4 g ..] as one 16-byte word: the 16 lanes of an LDS service group
// ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} of each half-wave: MI355X guide, LDS) are conflict-free exactly when their rows start on 16
// different banks-of-four, and with an odd number of 16-byte slots per row that is: 16 different values of b(p) mod 16.  With phases in lane
// order the lanes of a group span ~35 rows whose residues collide (2.3-way conflicts on every read, 49 % of the LDS cycles:
// profiles/r03_pmc.md).  So the phases are dealt to the service groups by residue class: phase p, the k-th of its class b(p) mod 16,
// goes to position (b(p) mod 16) of service group k.  A 4-row group then takes `lpg` = 32 ceil(max class size / 2) lanes instead of L
// (48 k -> 22.05 k: 160 for 147 phases), a few of them idle; the tap rows lie in lane order, so their reads stay conflict-free too.
// lpg = L: phases in lane order (the geometry falls back to it when the dealt form does not fit).
__device__ __forceinline__ int res3_slot(int k, int c) {  // lane (within a group's lanes) of position c in service group k
    const int a = k & 1 ? (c < 8 ? 4 + c : (c < 12 ? 8 + c : 16 + c)) : (c < 4 ? c : (c < 8 ? 8 + c : 12 + c));
    return 32 * (k >> 1) + a;
}
template <bool FAST>
__global__ __launch_bounds__(kRes3Threads) void resample_fused_kernel(const unsigned char* __restrict__ pcm, int format, int channels,
                                                                      const BatchFile* __restrict__ files, int n_files, int items_per_file,
                                                                      int L, int M, int half, int groups, int pitch_v, int lpg,
                                                                      const float* __restrict__ taps, float* __restrict__ arena) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float s_res3[];
    const int nt = 2 * half, pitch_t = nt | 1;
    const int R = 4 * groups;                             // rows per item: outputs [m0, m0 + L R), m0 a multiple of L
    float* s_x = s_res3;                                  // [M][pitch_v]
    float* s_x1 = s_x + (size_t)M * pitch_v;              // [nt][pitch_v]: rows u < nt shifted by one
    float* s_t = s_x1 + (size_t)nt * pitch_v;             // [lpg][pitch_t]: row s = the taps of the phase in lane s (taps row (p M) mod L)
    int* s_perm = (int*)(s_t + (size_t)lpg * pitch_t);    // [lpg]: phase of lane s of a group, or -1
    const int tid = threadIdx.x;
    int* s_cls = s_perm + lpg;                            // [L]: residue class of phase ph
    for (int s = tid; s < lpg; s += kRes3Threads) s_perm[s] = lpg == L ? s : -1;
    if (tid < L) s_cls[tid] = (int)(((int64_t)tid * M) / L) & 15;
    __syncthreads();
    if (lpg != L && tid < L) {                            // phase `tid`, the k-th of its class in ascending order, takes service group k
        const int c = s_cls[tid];
        int k = 0;
        for (int ph = 0; ph < tid; ++ph) k += s_cls[ph] == c;
        s_perm[res3_slot(k, c)] = tid;
    }
    __syncthreads();
    for (int s = tid / 64; s < lpg; s += kRes3Threads / 64) {
        const int ph = s_perm[s];
        if (ph < 0) continue;
        const int q = (int)(((int64_t)ph * M) % L);
        for (int j = tid & 63; j < nt; j += 64) s_t[s * pitch_t + j] = taps[(size_t)q * nt + j];
    }
    const int g = tid / lpg, slot = tid - g * lpg;
    const int p_of = g < groups ? s_perm[slot] : -1;
    const bool worker = p_of >= 0;
    const int p = worker ? p_of : 0;
    const int b = (int)(((int64_t)p * M) / L);            // input offset of phase p inside a row
    const int jx = M - b < nt ? M - b : nt;               // taps j >= jx lie behind the wrap of b + j past M
    const float* tp = s_t + (worker ? slot : 0) * pitch_t;
    const float* xa = s_x + (size_t)b * pitch_v + 4 * g;                       // + j pitch_v:  X[b + j][4 g ..]
    const float* xb = s_x1 + ((size_t)b * pitch_v + 4 * g) - (size_t)M * pitch_v;   // + j pitch_v:  X1[b + j - M][4 g ..]  (j >= jx)
    const int span = R * M + M + nt;                      // input samples an item touches (rounded up to whole rows)
    const int n_items = n_files * items_per_file;
    // this thread's places in the tile: fixed for the kernel's lifetime
    int off_x[kRes3Stage], off_x1[kRes3Stage];
#pragma unroll
    for (int k = 0; k < kRes3Stage; ++k) {
        const int ip = tid + k * kRes3Threads;
        const int vv = ip / M, u = ip - vv * M;
        off_x[k] = (ip < span && vv < pitch_v) ? u * pitch_v + vv : -1;
        off_x1[k] = (ip < span && u < nt && vv >= 1 && vv - 1 < pitch_v) ? u * pitch_v + vv - 1 : -1;
    }
    uint32_t raw[kRes3Stage];
    float val[kRes3Stage];
    auto valid_item = [&](int item, BatchFile& f, int& it) -> bool {
        if (item >= n_items) return false;
        const int fi = item / items_per_file;
        it = item - fi * items_per_file;
        f = files[fi];
        return (int64_t)it * L * R < f.n_out;
    };
    auto fetch = [&](const BatchFile& f, int it) {
        const int64_t i_lo = (int64_t)it * R * M - half + 1;                  // input index of the tile's first sample
        const unsigned char* base = pcm + f.pcm_off;
#pragma unroll
        for (int k = 0; k < kRes3Stage; ++k) {
            const int64_t idx = i_lo + tid + k * kRes3Threads;
            const bool in = off_x[k] >= 0 && idx >= 0 && idx < f.frames;
            if constexpr (FAST) {
                raw[k] = 0u;
                if (in) raw[k] = channels == 2 ? ((const uint32_t*)base)[idx] : (uint32_t)((const unsigned short*)base)[idx];
            } else {
                float v = 0.f;
                if (in) {
                    float acc = decode_sample(base, format, idx * channels);
                    for (int c = 1; c < channels; ++c) acc = __fadd_rn(acc, decode_sample(base, format, idx * channels + c));
                    v = channels > 1 ? __fdiv_rn(acc, (float)channels) : acc;
                }
                val[k] = v;
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int k = 0; k < kRes3Stage; ++k) {
            float v;
            if constexpr (FAST) {                         // decode_mono_batch_kernel's arithmetic: x / 32768, float32 channel mean
                const float s0 = (float)(short)(raw[k] & 0xffffu) / 32768.0f;
                if (channels == 2) { const float s1 = (float)(short)(raw[k] >> 16) / 32768.0f; v = __fdiv_rn(__fadd_rn(s0, s1), 2.0f); }
                else v = s0;
            } else v = val[k];
            if (off_x[k] >= 0) s_x[off_x[k]] = v;
            if (off_x1[k] >= 0) s_x1[off_x1[k]] = v;
        }
    };
    // walk this block's items; items past a file's end are skipped (block-uniform)
    int item = blockIdx.x;
    BatchFile f{}, fn{};
    int it = 0, itn = 0;
    while (item < n_items && !valid_item(item, f, it)) item += gridDim.x;
    if (item >= n_items) return;
    fetch(f, it);
    for (;;) {
        __syncthreads();                                  // the previous item's reads (and, first time, the table) are done / visible
        store_tile();
        __syncthreads();
        int next = item + gridDim.x;
        while (next < n_items && !valid_item(next, fn, itn)) next += gridDim.x;
        const bool more = next < n_items;
        if (more) fetch(fn, itn);                         // in flight during the multiply loop
        if (worker) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            auto tap = [&](const float4& x4, float t) {                        // two roundings per term, as the oracle
                { const float pr = t * x4.x; a0 = a0 + pr; }
                { const float pr = t * x4.y; a1 = a1 + pr; }
                { const float pr = t * x4.z; a2 = a2 + pr; }
                { const float pr = t * x4.w; a3 = a3 + pr; }
            };
            // (requesting a group of four taps' reads ahead of the arithmetic, ping-pong, measured slower: 1.73 against 1.55 ms on the C5
            // job -- four waves per SIMD already cover the LDS latency; what the loop waits for is the LDS array itself, 16-byte reads with
            // 2-way bank conflicts between the lanes' rows)
#pragma unroll 4
            for (int j = 0; j < nt; ++j) tap(*(const float4*)((j < jx ? xa : xb) + (size_t)j * pitch_v), tp[j]);
            float* out = arena + f.out_off;
            const int64_t m = (int64_t)it * L * R + (int64_t)(4 * g) * L + p;
            if (m < f.n_out) out[m] = a0;
            if (m + L < f.n_out) out[m + L] = a1;
            if (m + 2 * (int64_t)L < f.n_out) out[m + 2 * (int64_t)L] = a2;
            if (m + 3 * (int64_t)L < f.n_out) out[m + 3 * (int64_t)L] = a3;
        }
        if (!more) break;
        item = next; f = fn; it = itn;
    }
}

// The grid of a fused launch: a block per item up to one per CU
static unsigned res3_grid(int64_t items, int num_cus) { return (unsigned)std::min<int64_t>(items, num_cus > 0 ? num_cus : 256); }

hipError_t launch_resample_fused(const void* pcm, int format, int channels, const BatchFile* d_files, int n_files, const Res3Geom& gm, int64_t ipf,
                                 int L, int M, int half, const float* taps, float* arena, int num_cus, hipStream_t s) {
    if (n_files <= 0 || ipf <= 0) return hipSuccess;
    if (!gm.groups || ipf * n_files >= kMaxItems) return hipErrorInvalidValue;
    static std::atomic<uint64_t> attr_done{0};              // (per device: kernels.h allow_full_lds)
    if (hipError_t e = allow_full_lds((const void*)resample_fused_kernel<true>, attr_done)) return e;
    static std::atomic<uint64_t> attr_done2{0};
    if (hipError_t e = allow_full_lds((const void*)resample_fused_kernel<false>, attr_done2)) return e;
    const unsigned grid = res3_grid(ipf * n_files, num_cus);
    if (format == 2 && channels <= 2)
        hipLaunchKernelGGL(resample_fused_kernel<true>, dim3(grid), dim3(kRes3Threads), gm.lds, s, (const unsigned char*)pcm, format, channels, d_files,
                           n_files, (int)ipf, L, M, half, gm.groups, gm.pitch_v, gm.lpg, taps, arena);
    else
        hipLaunchKernelGGL(resample_fused_kernel<false>, dim3(grid), dim3(kRes3Threads), gm.lds, s, (const unsigned char*)pcm, format, channels, d_files,
                           n_files, (int)ipf, L, M, half, gm.groups, gm.pitch_v, gm.lpg, taps, arena);
    return hipGetLastError();
}

hipError_t launch_decode_mono_batch(const void* pcm, int format, int channels, const BatchFile* d_files, int n_files, int64_t max_frames,
                                    float* mono, hipStream_t s) {
    if (n_files <= 0 || max_frames <= 0) return hipSuccess;
    const unsigned gx = (unsigned)std::min<int64_t>((max_frames + 255) / 256, 4096);
    hipLaunchKernelGGL(decode_mono_batch_kernel, dim3(gx, (unsigned)n_files), dim3(256), 0, s, (const unsigned char*)pcm, format,
                       channels, d_files, mono);
    return hipGetLastError();
}

// =========================================================================================================
// Per-channel ingest (ss_add_pcm_channels*): a recording of C channels becomes C signals, no mixdown.  Signal c is bit for bit what the
// kernels above make of the one-channel PCM of channel c's samples: decode_sample(base, format, i C + c), then the same polyphase
// arithmetic (float32 multiply, then add, tap order, no contraction).
// =========================================================================================================
// 22 050 Hz input (dst = the arena) and the first half of the unfused pair (dst = the mono planes resample_batch_kernel reads): every
// interleaved frame is read once and written to C planes
__global__ __launch_bounds__(256) void decode_channels_batch_kernel(const unsigned char* __restrict__ pcm, int format, int channels,
                                                                    const ChanFile* __restrict__ files, float* __restrict__ dst) {
    const ChanFile f = files[blockIdx.y];
    const unsigned char* base = pcm + f.pcm_off;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < f.frames; i += (int64_t)gridDim.x * 256)
        for (int c = 0; c < channels; ++c) dst[f.mono_off + (int64_t)c * f.mono_stride + i] = decode_sample(base, format, i * channels + c);
}

// The fused form per channel.  Tables, tile layout, lane-to-phase dealing and the multiply loop are resample_fused_kernel's (see there);
// the table of a 48 k -> 22.05 k block already takes ~142 of the 160 KB, so there is ONE tile and the channels take turns in it: what a
// thread fetched for an item stays in registers -- FAST (16-bit stereo): the 32-bit word that holds both channels of a frame; otherwise
// CP decoded samples per frame -- and per channel the tile is staged again from them, the multiply loop runs, that channel's outputs are
// stored.  The PCM of a tile is requested once per CP channels; recordings with more channels take ceil(C / CP) passes over their items
// with the tables staged once.  The next item's request goes out behind the LAST channel's staging, so it is in flight during one multiply
// loop, as in the mixdown kernel, and needs no second set of registers.
static constexpr int kRes3CP = 2;                         // channels per pass: 2 x kRes3Stage sample registers beside the 2 x kRes3Stage tile offsets
template <bool FAST>
__global__ __launch_bounds__(kRes3Threads) void resample_fused_channels_kernel(const unsigned char* __restrict__ pcm, int format, int channels,
                                                                               const ChanFile* __restrict__ files, int n_files, int items_per_file,
                                                                               int L, int M, int half, int groups, int pitch_v, int lpg,
                                                                               const float* __restrict__ taps, float* __restrict__ arena) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float s_res3[];
    const int nt = 2 * half, pitch_t = nt | 1;
    const int R = 4 * groups;
    float* s_x = s_res3;                                  // [M][pitch_v]
    float* s_x1 = s_x + (size_t)M * pitch_v;              // [nt][pitch_v]: rows u < nt shifted by one
    float* s_t = s_x1 + (size_t)nt * pitch_v;             // [lpg][pitch_t]
    int* s_perm = (int*)(s_t + (size_t)lpg * pitch_t);    // [lpg]: phase of lane s of a group, or -1
    const int tid = threadIdx.x;
    int* s_cls = s_perm + lpg;                            // [L]
    for (int s = tid; s < lpg; s += kRes3Threads) s_perm[s] = lpg == L ? s : -1;
    if (tid < L) s_cls[tid] = (int)(((int64_t)tid * M) / L) & 15;
    __syncthreads();
    if (lpg != L && tid < L) {
        const int c = s_cls[tid];
        int k = 0;
        for (int ph = 0; ph < tid; ++ph) k += s_cls[ph] == c;
        s_perm[res3_slot(k, c)] = tid;
    }
    __syncthreads();
    for (int s = tid / 64; s < lpg; s += kRes3Threads / 64) {
        const int ph = s_perm[s];
        if (ph < 0) continue;
        const int q = (int)(((int64_t)ph * M) % L);
        for (int j = tid & 63; j < nt; j += 64) s_t[s * pitch_t + j] = taps[(size_t)q * nt + j];
    }
    const int g = tid / lpg, slot = tid - g * lpg;
    const int p_of = g < groups ? s_perm[slot] : -1;
    const bool worker = p_of >= 0;
    const int p = worker ? p_of : 0;
    const int b = (int)(((int64_t)p * M) / L);
    const int jx = M - b < nt ? M - b : nt;
    const float* tp = s_t + (worker ? slot : 0) * pitch_t;
    const float* xa = s_x + (size_t)b * pitch_v + 4 * g;
    const float* xb = s_x1 + ((size_t)b * pitch_v + 4 * g) - (size_t)M * pitch_v;
    const int span = R * M + M + nt;
    const int n_items = n_files * items_per_file;
    int off_x[kRes3Stage], off_x1[kRes3Stage];
#pragma unroll
    for (int k = 0; k < kRes3Stage; ++k) {
        const int ip = tid + k * kRes3Threads;
        const int vv = ip / M, u = ip - vv * M;
        off_x[k] = (ip < span && vv < pitch_v) ? u * pitch_v + vv : -1;
        off_x1[k] = (ip < span && u < nt && vv >= 1 && vv - 1 < pitch_v) ? u * pitch_v + vv - 1 : -1;
    }
    uint32_t raw[kRes3Stage];
    float val[kRes3CP][kRes3Stage];
    auto valid_item = [&](int item, ChanFile& f, int& it) -> bool {
        if (item >= n_items) return false;
        const int fi = item / items_per_file;
        it = item - fi * items_per_file;
        f = files[fi];
        return (int64_t)it * L * R < f.n_out;
    };
    for (int c0 = 0; c0 < channels; c0 += kRes3CP) {      // FAST: channels == 2, one pass
        const int ncp = channels - c0 < kRes3CP ? channels - c0 : kRes3CP;
        auto fetch = [&](const ChanFile& f, int it) {
            const int64_t i_lo = (int64_t)it * R * M - half + 1;
            const unsigned char* base = pcm + f.pcm_off;
#pragma unroll
            for (int k = 0; k < kRes3Stage; ++k) {
                const int64_t idx = i_lo + tid + k * kRes3Threads;
                const bool in = off_x[k] >= 0 && idx >= 0 && idx < f.frames;
                if constexpr (FAST) {
                    raw[k] = 0u;
                    if (in) raw[k] = ((const uint32_t*)base)[idx];
                } else {
#pragma unroll
                    for (int cc = 0; cc < kRes3CP; ++cc)
                        val[cc][k] = (in && cc < ncp) ? decode_sample(base, format, idx * channels + c0 + cc) : 0.f;
                }
            }
        };
        int item = blockIdx.x;
        ChanFile f{}, fn{};
        int it = 0, itn = 0;
        while (item < n_items && !valid_item(item, f, it)) item += gridDim.x;
        if (item >= n_items) return;                      // (the same items in every pass: block-uniform)
        fetch(f, it);
        bool more = true;
        while (more) {
            int next = item;
#pragma unroll
            for (int cc = 0; cc < kRes3CP; ++cc) {
                if (cc >= ncp) break;                     // block-uniform
                __syncthreads();                          // the previous multiply loop's reads (and, first time, the table) are done / visible
#pragma unroll
                for (int k = 0; k < kRes3Stage; ++k) {
                    float v;
                    if constexpr (FAST) v = (float)(short)(cc ? raw[k] >> 16 : raw[k] & 0xffffu) / 32768.0f;   // decode_sample's x / 32768
                    else v = val[cc][k];
                    if (off_x[k] >= 0) s_x[off_x[k]] = v;
                    if (off_x1[k] >= 0) s_x1[off_x1[k]] = v;
                }
                __syncthreads();
                if (cc == ncp - 1) {                      // the registers are free again: the next item's request, in flight during this multiply loop
                    next = item + gridDim.x;
                    while (next < n_items && !valid_item(next, fn, itn)) next += gridDim.x;
                    more = next < n_items;
                    if (more) fetch(fn, itn);
                }
                if (worker) {
                    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
                    auto tap = [&](const float4& x4, float t) {                    // two roundings per term, as the oracle
                        { const float pr = t * x4.x; a0 = a0 + pr; }
                        { const float pr = t * x4.y; a1 = a1 + pr; }
                        { const float pr = t * x4.z; a2 = a2 + pr; }
                        { const float pr = t * x4.w; a3 = a3 + pr; }
                    };
#pragma unroll 4
                    for (int j = 0; j < nt; ++j) tap(*(const float4*)((j < jx ? xa : xb) + (size_t)j * pitch_v), tp[j]);
                    float* out = arena + f.out_off + (int64_t)(c0 + cc) * f.out_stride;
                    const int64_t m = (int64_t)it * L * R + (int64_t)(4 * g) * L + p;
                    if (m < f.n_out) out[m] = a0;
                    if (m + L < f.n_out) out[m + L] = a1;
                    if (m + 2 * (int64_t)L < f.n_out) out[m + 2 * (int64_t)L] = a2;
                    if (m + 3 * (int64_t)L < f.n_out) out[m + 3 * (int64_t)L] = a3;
                }
            }
            item = next; f = fn; it = itn;
        }
        __syncthreads();                                  // the last multiply loop's reads, before the next pass stages its first tile
    }
}

hipError_t launch_decode_channels_batch(const void* pcm, int format, int channels, const ChanFile* d_files, int n_files, int64_t max_frames,
                                        float* dst, hipStream_t s) {
    if (n_files <= 0 || max_frames <= 0) return hipSuccess;
    const unsigned gx = (unsigned)std::min<int64_t>((max_frames + 255) / 256, 4096);
    hipLaunchKernelGGL(decode_channels_batch_kernel, dim3(gx, (unsigned)n_files), dim3(256), 0, s, (const unsigned char*)pcm, format, channels,
                       d_files, dst);
    return hipGetLastError();
}

hipError_t launch_resample_fused_channels(const void* pcm, int format, int channels, const ChanFile* d_files, int n_files, const Res3Geom& gm,
                                          int64_t ipf, int L, int M, int half, const float* taps, float* arena, int num_cus, hipStream_t s) {
    if (n_files <= 0 || ipf <= 0) return hipSuccess;
    if (!gm.groups || ipf * n_files >= kMaxItems) return hipErrorInvalidValue;
    static std::atomic<uint64_t> attr_done{0};              // (per device: kernels.h allow_full_lds)
    if (hipError_t e = allow_full_lds((const void*)resample_fused_channels_kernel<true>, attr_done)) return e;
    static std::atomic<uint64_t> attr_done2{0};
    if (hipError_t e = allow_full_lds((const void*)resample_fused_channels_kernel<false>, attr_done2)) return e;
    const unsigned grid = res3_grid(ipf * n_files, num_cus);
    if (format == 2 && channels == 2)
        hipLaunchKernelGGL(resample_fused_channels_kernel<true>, dim3(grid), dim3(kRes3Threads), gm.lds, s, (const unsigned char*)pcm, format,
                           channels, d_files, n_files, (int)ipf, L, M, half, gm.groups, gm.pitch_v, gm.lpg, taps, arena);
    else
        hipLaunchKernelGGL(resample_fused_channels_kernel<false>, dim3(grid), dim3(kRes3Threads), gm.lds, s, (const unsigned char*)pcm, format,
                           channels, d_files, n_files, (int)ipf, L, M, half, gm.groups, gm.pitch_v, gm.lpg, taps, arena);
    return hipGetLastError();
}

hipError_t launch_resample_batch(const float* mono, const BatchFile* d_files, int n_files, int64_t max_out, const ResGeom& gm, int L, int M, int half,
                                 const float* taps, float* arena, int num_cus, hipStream_t s) {
    if (n_files <= 0 || max_out <= 0) return hipSuccess;
    if (gm.lds_kernel) {
        static std::atomic<uint64_t> attr_done{0};              // (per device: kernels.h allow_full_lds)
        if (hipError_t e = allow_full_lds((const void*)resample_batch_lds_kernel, attr_done)) return e;
        const unsigned grid = (unsigned)std::min<int64_t>(gm.chunks_per_file * n_files, num_cus > 0 ? num_cus : 256);
        hipLaunchKernelGGL(resample_batch_lds_kernel, dim3(grid), dim3(kResThreads), gm.lds, s, mono, d_files, n_files, (int)gm.chunks_per_file, L, M,
                           half, gm.span, taps, arena);
        return hipGetLastError();
    }
    const unsigned gx = (unsigned)std::min<int64_t>((max_out + 255) / 256, 4096);
    hipLaunchKernelGGL(resample_batch_kernel, dim3(gx, (unsigned)n_files), dim3(256), 0, s, mono, d_files, L, M, half, taps, arena);
    return hipGetLastError();
}

}  // namespace ss
