// The row-streaming core on v_mfma_f32_16x16x32_f16, shared by conv1s.hip (conv1_1), conv9a.hip (conv9_1.A) and conv9s.hip (conv9_1.B): a 3 x 3, 32 -> 32 conv at
// 128 x 256 whose operand rows a wave holds in registers while it walks down a strip of 32 columns (conv1s.hip's header tells the idea).
//   * Lane (g, c) = (lane >> 4, lane & 15).  Strip s holds picture columns 32 s .. 32 s + 31 as two pixel tiles, interleaved: tile t's
//     lane c is column 32 s + 2 c + t.  A lane's B operand of a tile is channels 8 g .. 8 g + 7 of its pixel as one 16-byte run per plane
//     (high halves, low halves); result row 4 g + r of channel tile u is channel 8 g + 4 u + r.
//   * The OPERANDS are shifted, not the outputs: one accumulator set P[t][u] takes all nine taps, three f16 products per term.  For tap
//     (dy, dx) tile t needs the pixel at column x + dx: for dx = -1 tile 1 reads tile 0's registers as they are and tile 0 reads tile 1's
//     row shifted by row_shr:1, its lane 0 taking the pixel at column 32 s - 1; for dx = +1 tile 0 reads tile 1's registers and tile 1
//     reads tile 0's row shifted by row_shl:1, its lane 15 taking column 32 s + 32.  A row carries those two halo pixels in one more
//     16-byte run per plane (lanes c < 8 hold the left one, the others the right one; lanes 0 and 15 are used) -- loaded where the row
//     lies in memory (conv9a.hip, conv9s.hip), produced by a third first-conv tile where it is made in registers (conv1s.hip).  A strip
//     stores all 32 columns, eight strips cover a row exactly.
//   * A row's two shifted operands are made at the point of use (S16RowH: 48 DPP moves per row step, no registers beyond the row's) or
//     once, with the row (S16RowS: 16 moves and 16 more registers per row).
//   * Weight banks: weights.hip pack_conv_stream16, [plane][tap][channel tile][lane][16 B], read from the LDS one tap ahead.
// (conv1s.hip's 32x32x16 form of the development build is the older idea: one accumulator tile per dx, the outputs shifted and added,
// strip columns 0 and 31 without a neighbour and not stored -- nine strips of thirty columns: kStrips, kStripCols.)
#pragma once
#include "mfma_util.h"

namespace ss {

static constexpr int kH = 128, kW = 256, kC = 32;
static constexpr int kStrips = 9, kStripCols = 30;       // conv1s.hip's 32x32x16 form: valid columns per strip are columns 1 .. 30 of the 32
static constexpr int kStrips32 = 8;                      // the 16x16x32 core: every column of a strip is stored
static constexpr int kBank = 9 * 2 * 1024;               // one plane of the 3 x 3 weights: [tap][K step or channel tile][lane][16 B]
static constexpr int kS1Waves = 8;                       // two waves per SIMD (twelve at 168 registers measured the same within the noise, and sat on the edge of spilling)
static constexpr int kMaxRows = 32;                      // most rows of a work unit

struct S16Row { u32x4 f[2][2]; };                        // [pixel tile][plane: 0 = high halves, 1 = low halves]: B operands of one strip row
struct S16RowH { u32x4 f[2][2]; u32x4 h[2]; };           // S16Row + the halo run, [plane]
// S16Row + the shifted operands, halo lane included: l = tile 0's operand for dx = -1 (tile 1 moved up a lane), r = tile 1's for dx = +1
struct S16RowS { u32x4 f[2][2]; u32x4 l[2], r[2]; };

__device__ __forceinline__ f32x4 s16_mfma(const u32x4& a, const u32x4& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

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
// pixel tile t's operand of plane pq for the taps of column offset dx
__device__ __forceinline__ u32x4 s16_operand(const S16RowH& H, int dx, int t, int pq) {
    if (dx == 0) return H.f[t][pq];
    if (dx < 0) return t == 0 ? s16_shr1_halo(H.f[1][pq], H.h[pq]) : H.f[0][pq];
    return t == 0 ? H.f[1][pq] : s16_shl1_halo(H.f[0][pq], H.h[pq]);
}
__device__ __forceinline__ u32x4 s16_operand(const S16RowS& H, int dx, int t, int pq) {
    if (dx == 0) return H.f[t][pq];
    if (dx < 0) return t == 0 ? H.l[pq] : H.f[0][pq];
    return t == 0 ? H.f[1][pq] : H.r[pq];
}
__device__ __forceinline__ void s16_make_shifted(S16RowS& H, const u32x4 (&halo)[2]) {
#pragma unroll
    for (int pq = 0; pq < 2; ++pq) { H.l[pq] = s16_shr1_halo(H.f[1][pq], halo[pq]); H.r[pq] = s16_shl1_halo(H.f[0][pq], halo[pq]); }
}

// Fragment sets (both channel tiles, both planes: four 16-byte LDS reads) in a THREE-slot ring: a set of the 3 x 3 serves twelve
// products and is read one set ahead; a kernel with sets of six products (conv9a.hip's upsampled half) reads those two
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
// 0 .. 8 (rows Ha / Hb / Hn are last read by taps 2 / 5 / 8).  Row: S16RowH (the shifted operand is made here) or S16RowS (it is there).
template <typename Row, typename Last, typename AfterTap>
__device__ __forceinline__ void s16_taps_shifted(S16Ring3& ring, const char* wl_base, const Row& Ha, const Row& Hb, const Row& Hn,
                                                 f32x4 (&P)[2][2], Last&& before_last, AfterTap&& after_tap) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3, dx = tap % 3 - 1, slot = tap & 1;
        const Row& Hr = dy == 0 ? Ha : (dy == 1 ? Hb : Hn);
        if (tap + 1 < 9) ring.rd_tap(slot ^ 1, wl_base, tap + 1); else before_last();
        u32x4 B[2][2];                                    // [pixel tile][plane]
#pragma unroll
        for (int pq = 0; pq < 2; ++pq) { B[0][pq] = s16_operand(Hr, dx, 0, pq); B[1][pq] = s16_operand(Hr, dx, 1, pq); }
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
