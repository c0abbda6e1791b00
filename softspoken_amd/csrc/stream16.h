// The row-streaming core on v_mfma_f32_16x16x32_f16, shared by conv1s.hip (conv1_1) and conv9s.hip (conv9_1.B): a 3 x 3, 32 -> 32 conv at
// 128 x 256 whose operand rows a wave holds in registers while it walks down a strip of 32 columns (conv1s.hip's header tells the idea).
//   * Lane (g, c) = (lane >> 4, lane & 15).  A strip's 32 columns are two pixel tiles, interleaved: tile t holds strip columns 2 c + t.
//     A lane's B operand of a tile is channels 8 g .. 8 g + 7 of its pixel as one 16-byte run per plane (high halves, low halves);
//     result row 4 g + r of channel tile u is channel 8 g + 4 u + r.
//   * The taps of one dx accumulate into their own tile, P[dx][t][u] = sum over dy of W[dy][dx] x row[y + dy], three f16 products per
//     term; out[x] = P_-1[x - 1] + P_0[x] + P_+1[x + 1]: tile 0's column neighbours are tile 1's lanes c - 1 / c, tile 1's are tile 0's
//     lanes c / c + 1.  Strip columns 0 and 31 have no neighbour and are not stored: a strip yields 30 columns, nine strips a row.
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
