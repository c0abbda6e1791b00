// The row-streaming core on v_mfma_f32_16x16x32_f16, shared by conv1s.hip (conv1_1), conv9a.hip (conv9_1.A) and conv9s.hip (conv9_1.B): a 3 x 3, 32 -> 32 conv at
// 128 x 256 whose operand rows a wave holds in registers while it walks down a strip of 32 columns (conv1s.hip's header tells the idea).
//   * Lane (g, c) = (lane >> 4, lane & 15).  A strip's 32 columns are two pixel tiles, interleaved: tile t holds strip columns 2 c + t.
//     A lane's B operand of a tile is channels 8 g .. 8 g + 7 of its pixel as one 16-byte run per plane (high halves, low halves);
//     result row 4 g + r of channel tile u is channel 8 g + 4 u + r.
//   * The taps of one dx accumulate into their own tile, P[dx][t][u] = sum over dy of W[dy][dx] x row[y + dy], three f16 products per
//     term; out[x] = P_-1[x - 1] + P_0[x] + P_+1[x + 1]: tile 0's column neighbours are tile 1's lanes c - 1 / c, tile 1's are tile 0's
//     lanes c / c + 1.  Strip columns 0 and 31 have no neighbour and are not stored: a strip yields 30 columns, nine strips a row
//     (conv1s.hip's form: its operand rows are made in registers and have no halo pixel to load; the form below shifts operands instead).
//   * Weight banks: weights.hip pack_conv_stream16, [plane][tap][channel tile][lane][16 B], read from the LDS one tap ahead.
#pragma once
#include "mfma_util.h"

namespace ss {

static constexpr int kH = 128, kW = 256, kC = 32;
static constexpr int kStrips = 9, kStripCols = 30;       // valid columns per strip: columns 1 .. 30 of the 32
static constexpr int kBank = 9 * 2 * 1024;               // one plane of the 3 x 3 weights: [tap][K step or channel tile][lane][16 B]
static constexpr int kS1Waves = 8;                       // two waves per SIMD (twelve at 168 registers measured the same within the noise, and sat on the edge of spilling)
static constexpr int kMaxRows = 32;                      // most rows of a work unit

struct S16Row { u32x4 f[2][2]; };                        // [pixel tile][plane: 0 = high halves, 1 = low halves]: the 3 x 3's B operands of one strip row

__device__ __forceinline__ f32x4 s16_mfma(const u32x4& a, const u32x4& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ int s16_shr1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true); }   // lane c <- lane c - 1 of its 16 (c = 0: 0)
__device__ __forceinline__ int s16_shl1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x101, 0xf, 0xf, true); }   // lane c <- lane c + 1 (c = 15: 0)
__device__ __forceinline__ float s16_shr1f(float v) { return __int_as_float(s16_shr1(__float_as_int(v))); }
__device__ __forceinline__ float s16_shl1f(float v) { return __int_as_float(s16_shl1(__float_as_int(v))); }

// a tap's weight fragments, both channel tiles and planes (four 16-byte LDS reads), in a two-slot ring
struct S16Ring {
    u32x4 wh[2][2], wl[2][2];                             // [ring slot][channel tile]
    __device__ __forceinline__ void rd(const char* wl_base, int tap) {   // wl_base: the banks + lane * 16
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            wh[tap & 1][u] = *(const u32x4*)(wl_base + (tap * 2 + u) * 1024);
            wl[tap & 1][u] = *(const u32x4*)(wl_base + kBank + (tap * 2 + u) * 1024);
        }
    }
};

// The nine taps.  ring.rd(wl_base, 0) has been issued by the caller (far enough ahead for the LDS round trip); a tap's fragments are
// requested one tap ahead (a tap's products: 192 matrix cycles).  The fences keep that order: left to itself the scheduler sinks every
// read to just in front of its products and waits there.  after_tap(tap) runs behind the products of tap 0 .. 7 (rows Ha / Hb / Hn are
// last read by taps 2 / 5 / 8).
template <typename AfterTap>
__device__ __forceinline__ void s16_taps(S16Ring& ring, const char* wl_base, const S16Row& Ha, const S16Row& Hb, const S16Row& Hn, f32x4 (&P)[3][2][2],
                                         AfterTap&& after_tap) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3, dx = tap % 3;
        const S16Row& Hr = dy == 0 ? Ha : (dy == 1 ? Hb : Hn);
        if (tap + 1 < 9) ring.rd(wl_base, tap + 1);
        __builtin_amdgcn_sched_barrier(0);
        // the four result tiles (pixel tile x channel tile) take turns: a product's accumulator was last written four products earlier
#pragma unroll
        for (int pr = 0; pr < 3; ++pr)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    P[dx][t][u] = s16_mfma(pr == 1 ? ring.wl[tap & 1][u] : ring.wh[tap & 1][u], Hr.f[t][pr == 0 ? 1 : 0], P[dx][t][u]);
        __builtin_amdgcn_sched_barrier(0);
        if (tap + 1 < 9) after_tap(tap);
    }
    __builtin_amdgcn_sched_barrier(0);
}

// out[x] = P_-1[x - 1] + P_0[x] + P_+1[x + 1], ReLU: v[pixel tile][channel tile][r]
__device__ __forceinline__ void s16_combine(const f32x4 (&P)[3][2][2], float (&v)[2][2][4]) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            v[0][u][r] = relu_i(P[1][0][u][r] + s16_shr1f(P[0][1][u][r]) + P[2][1][u][r]);
            v[1][u][r] = relu_i(P[1][1][u][r] + P[0][0][u][r] + s16_shl1f(P[2][0][u][r]));
        }
}

// ---- the core without overlap columns (conv9a.hip, conv9s.hip) -----------------------------------------------------------------------------
// The same lanes and tiles, but the OPERANDS are shifted, not the outputs: strip s holds picture columns 32 s .. 32 s + 31, tile t's
// lane c column 32 s + 2 c + t, and one accumulator set P[t][u] takes all nine taps.  For tap (dy, dx) tile t needs the pixel at column
// x + dx: for dx = -1 tile 1 reads tile 0's registers as they are and tile 0 reads tile 1's row shifted by row_shr:1, its lane 0 taking
// the pixel at column 32 s - 1; for dx = +1 tile 0 reads tile 1's registers and tile 1 reads tile 0's row shifted by row_shl:1, its
// lane 15 taking column 32 s + 32.  The two halo pixels of a row come from one more 16-byte load per plane (lanes c < 8 ask for the left
// one, the others for the right one; lanes 0 and 15 use them): a strip stores all 32 columns, eight strips cover a row exactly.
static constexpr int kStrips32 = 8;

struct S16RowH { u32x4 f[2][2]; u32x4 h[2]; };           // S16Row + the halo load, [plane]

// DPP with bound_ctrl off leaves `old` in the lane that has no source: the shifted operand and its halo lane in one move per register
__device__ __forceinline__ u32x4 s16_shr1_halo(const u32x4& v, const u32x4& halo) {      // lane c <- lane c - 1 (c = 0: its halo)
    u32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (uint32_t)__builtin_amdgcn_update_dpp((int)halo[e], (int)v[e], 0x111, 0xf, 0xf, false);
    return r;
}
__device__ __forceinline__ u32x4 s16_shl1_halo(const u32x4& v, const u32x4& halo) {      // lane c <- lane c + 1 (c = 15: its halo)
    u32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (uint32_t)__builtin_amdgcn_update_dpp((int)halo[e], (int)v[e], 0x101, 0xf, 0xf, false);
    return r;
}

// Fragment sets (both channel tiles, both planes: four 16-byte LDS reads) in a THREE-slot ring: a set of the 3 x 3 serves twelve
// products and is read one set ahead, as in S16Ring; a kernel with sets of six products (conv9a.hip's upsampled half) reads those two
// sets ahead, so that every read still lies twelve products in front of its first use.
struct S16Ring3 {
    u32x4 wh[3][2], wl[3][2];                             // [ring slot][channel tile]
    // hi / lo: the lane's address of channel tile 0's fragment of either plane; tile 1's lies `step` bytes behind
    __device__ __forceinline__ void rd(int slot, const char* hi, const char* lo, int step) {
#pragma unroll
        for (int u = 0; u < 2; ++u) { wh[slot][u] = *(const u32x4*)(hi + u * step); wl[slot][u] = *(const u32x4*)(lo + u * step); }
    }
    __device__ __forceinline__ void rd_tap(int slot, const char* wl_base, int tap) { rd(slot, wl_base + tap * 2048, wl_base + kBank + tap * 2048, 1024); }
};

// three products per term of one pixel tile and both channel tiles against the set in `slot`: B[plane]
__device__ __forceinline__ void s16_products(const S16Ring3& ring, int slot, const u32x4 (&B)[2], f32x4 (&Pt)[2]) {
#pragma unroll
    for (int pr = 0; pr < 3; ++pr)
#pragma unroll
        for (int u = 0; u < 2; ++u) Pt[u] = s16_mfma(pr == 1 ? ring.wl[slot][u] : ring.wh[slot][u], B[pr == 0 ? 1 : 0], Pt[u]);
}

// The nine taps into P[t][u].  Tap k's set is in slot k & 1; the caller has requested tap 0's.  before_last() runs in front of the
// products of tap 8, where no next tap is to be read (the caller's own next sets go there); after_tap(tap) behind the products of taps
// 0 .. 8 (rows Ha / Hb / Hn are last read by taps 2 / 5 / 8).  The shifted operand is made at the point of use.
template <typename Last, typename AfterTap>
__device__ __forceinline__ void s16_taps_shifted(S16Ring3& ring, const char* wl_base, const S16RowH& Ha, const S16RowH& Hb, const S16RowH& Hn,
                                                 f32x4 (&P)[2][2], Last&& before_last, AfterTap&& after_tap) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3, dx = tap % 3 - 1, slot = tap & 1;
        const S16RowH& Hr = dy == 0 ? Ha : (dy == 1 ? Hb : Hn);
        if (tap + 1 < 9) ring.rd_tap(slot ^ 1, wl_base, tap + 1); else before_last();
        u32x4 B[2][2];                                    // [pixel tile][plane]
#pragma unroll
        for (int pq = 0; pq < 2; ++pq) {
            B[0][pq] = dx == 0 ? Hr.f[0][pq] : (dx < 0 ? s16_shr1_halo(Hr.f[1][pq], Hr.h[pq]) : Hr.f[1][pq]);
            B[1][pq] = dx == 0 ? Hr.f[1][pq] : (dx < 0 ? Hr.f[0][pq] : s16_shl1_halo(Hr.f[0][pq], Hr.h[pq]));
        }
        __builtin_amdgcn_sched_barrier(0);
        // the four result tiles (pixel tile x channel tile) take turns: a product's accumulator was last written four products earlier
#pragma unroll
        for (int pr = 0; pr < 3; ++pr)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    P[t][u] = s16_mfma(pr == 1 ? ring.wl[slot][u] : ring.wh[slot][u], B[t][pr == 0 ? 1 : 0], P[t][u]);
        __builtin_amdgcn_sched_barrier(0);
        after_tap(tap);
    }
}

// a lane's eight values of a pixel tile are channels 8 g .. 8 g + 7 of its pixel: one 16-byte run per plane (high halves kh, low halves kl)
__device__ __forceinline__ void s16_split_px(const float (&val)[2][4], uint32_t (&kh)[4], uint32_t (&kl)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float e0 = val[i >> 1][2 * (i & 1)], e1 = val[i >> 1][2 * (i & 1) + 1];
        kh[i] = pack_f16(e0, e1);
        kl[i] = split_lo(kh[i], e0, e1);
    }
}

}  // namespace ss
