// conv9_1.B (the second conv of ResBlock(64, 32) at 128 x 256, the block's 1 x 1 projection of cat[c1, up(c8)], the add, ReLU, and
// conv_flatten in the epilogue: pytorch_neural_nets.py:7-41, 133, 181, 188) as a ROW-STREAMING kernel, f16x2 mode.
//
// Why.  In conv4.hip this launch is bound by neither roof (matrix pipe ~35 % busy, ~3 TB/s): of a stage's 17 460 cycles the products take
// 4030, the rest is the patch image's way through the LDS, two barriers per stage and the epilogue.  Its 3 x 3 is
// the arithmetic of conv1_1's second conv, which conv1s.hip runs without a patch image and without a barrier after the prologue; and
// here the operands need not even be produced: h9 lies in memory in the order conv1s.hip's store_px writes -- lane (g, c) finds
// channels 8 g .. 8 g + 7 of its pixel as one 16-byte run per plane -- so a strip row of h9 IS the 3 x 3's B operand, four 16-byte loads
// per lane.  The core is stream16.h's form without overlap columns (shifted operands with a halo lane, one accumulator set), shared with
// conv9a.hip; the split is shared with conv1s.hip as well.
//
//   * Work unit = (window, band of `rows` rows, strip of 32 columns, all of them stored), strips fastest; a wave's units are independent.
//   * The wave holds h9 of rows y - 1, y, y + 1 in three register sets that change roles.  Row y - 1 is last read by tap 2; behind it
//     the loads of row y + 2 are issued INTO ITS REGISTERS and have the other six taps, the next row's projection and six more taps to
//     arrive (about 1.3 row steps, ~4.8 us with two waves per SIMD): no set beyond the three.  c1 and c8 of row y + 1 are requested
//     behind the projection's products of row y, a row step ahead, into the registers those products read.  In the mask-only pass
//     the loop has no stores and no request behind a branch, so vmcnt counts loads alone and every wait is for the oldest request.
//   * Rows outside the picture are zero operands; so are the two halo pixels of a row (one more 16-byte load per plane, stream16.h)
//     where they lie outside it: clamped addresses, wave-uniform masks (the 3 x 3's zero padding).
//   * P starts from the summed biases b2 + br and takes the projection: c1 at (y, x) and c8 at (y >> 1, x >> 1), each a K = 32
//     operand against fragments in 16x16x32 A-operand order (weights.hip pack_proj_stream16), three products per term.  Strip columns
//     are 32 s + 2 c + t, so both tiles' lane c sit on c8 pixel 16 s + c: one load of c8 serves both.
//   * The nine taps go into the same P; ReLU, split into f16 halves; the high halves are range-tested as in conv4.hip's form (the
//     split values feed the flatten whether c9 is stored or not).  The split row is the B operand of conv_flatten: row y's filter is an
//     A fragment whose rows 0 .. 3 are the four flatten channels (weights.hip pack_flat_rows, 256 KB, read from memory at the top of
//     the row step); three products per tile accumulate in registers over the unit's rows, and at the unit's end lanes g = 0 write
//     flat_part[window][band][4][x]: 128 / rows groups per window.
//   * store_out (a run-time flag: the spec pass) also writes both planes of c9.  One kernel for both passes: the flatten sums of the
//     mask-only pass equal those of the spec pass bit for bit.
// Per row and wave: 24 + 108 + 6 products of 16 matrix cycles.  LDS: the 3 x 3 banks (36 KB) and the projection fragments (8 KB); one
// barrier, behind their load.  Launch: one 512-thread block per CU, two waves per SIMD.
//
// Jitter test (SS_JITTER_SLEEP): nothing to cover -- the kernel has no synchronisation point after its prologue, the waves share
// nothing but read-only LDS.
#include "kernels.h"
#include "stream16.h"
#include <algorithm>

namespace ss {

static constexpr int kProjFrag = 2 * 2 * 2 * 1024;       // [source: c1, c8][channel tile][plane][lane][16 B]
static constexpr uint32_t kRowB = kW * 64, kRowB8 = (kW / 2) * 64;   // bytes per row of a plane of h9 / c1 / c9, of c8

__global__ __launch_bounds__(64 * kS1Waves) __attribute__((amdgpu_waves_per_eu(2, 2)))
void conv9_stream16_kernel(ConvArgs a, int rows_per_unit, int total_units) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sW = smem;                                      // [plane][tap][channel tile][lane][16 B]
    char* sP = smem + 2 * kBank;                          // [source][channel tile][plane][lane][16 B]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, c = lane & 15;
    for (int p = tid; p < 2 * kBank / 16; p += 64 * kS1Waves) *(u32x4*)(sW + p * 16) = *(const u32x4*)((const char*)a.wpk + (size_t)p * 16);
    for (int p = tid; p < kProjFrag / 16; p += 64 * kS1Waves) *(u32x4*)(sP + p * 16) = *(const u32x4*)((const char*)a.proj_w + (size_t)p * 16);
    // result row 4 g + r of channel tile u is channel 8 g + 4 u + r
    const f32x4 bias[2] = {*(const f32x4*)(a.bias + 8 * g), *(const f32x4*)(a.bias + 8 * g + 4)};
    __syncthreads();                                      // the only barrier

    const char* wl_base = sW + lane * 16;
    const char* pl_base = sP + lane * 16;
    const char* fw_base = (const char*)a.flat_w4 + lane * 16;           // [row][plane][lane][16 B]
    const int bands = kH / rows_per_unit;
    const int64_t lo = a.lo_delta;
    uint32_t ovf = 0;                                     // the largest high halves of the stored columns (all exponent bits set = infinity / NaN)

    for (int unit = (int)blockIdx.x * kS1Waves + wave; unit < total_units; unit += (int)gridDim.x * kS1Waves) {
        const int s = unit % kStrips32, b = (unit / kStrips32) % bands, n = unit / (kStrips32 * bands);
        const int x0 = 32 * s, y0 = b * rows_per_unit, ylast = y0 + rows_per_unit - 1;
        const int xt[2] = {x0 + 2 * c, x0 + 2 * c + 1};   // this lane's picture column in pixel tile t
        const uint32_t voff[2] = {(uint32_t)xt[0] * 64u + (uint32_t)g * 16u, (uint32_t)xt[1] * 64u + (uint32_t)g * 16u};   // its run in a row of h9 / c1 / c9
        // ... its halo pixel's (lanes c < 8: the one left of the strip, the others the one right of it; outside the picture: the edge
        // pixel, masked), and its run in a row of c8: both tiles' lane c sit on c8 pixel 16 s + c
        const uint32_t hoff = (uint32_t)(c < 8 ? max(x0 - 1, 0) : min(x0 + 32, kW - 1)) * 64u + (uint32_t)g * 16u;
        const uint32_t hkeep = (c < 8 ? s > 0 : s < kStrips32 - 1) ? 0xffffffffu : 0u;
        const uint32_t voff8 = (uint32_t)(x0 / 2 + c) * 64u + (uint32_t)g * 16u;
        const char* hw = (const char*)a.src0 + (size_t)n * kH * kRowB;   // the window's h9, c1, c8 (high planes; the low ones lie `lo` behind)
        const char* c1w = (const char*)a.xp0 + (size_t)n * kH * kRowB;
        const char* c8w = (const char*)a.xp1 + (size_t)n * (kH / 2) * kRowB8;
        char* ow = (char*)a.out + (size_t)n * kH * kRowB;

        // h9 of picture row r (any r: outside the picture the nearest row is read and mask_row clears it)
        auto load_row = [&](S16RowH& H, int r) {
            const char* p = hw + (size_t)min(max(r, 0), kH - 1) * kRowB;
#pragma unroll
            for (int t = 0; t < 2; ++t) { H.f[t][0] = *(const u32x4*)(p + voff[t]); H.f[t][1] = *(const u32x4*)(p + lo + voff[t]); }
            H.h[0] = *(const u32x4*)(p + hoff); H.h[1] = *(const u32x4*)(p + lo + hoff);
        };
        auto mask_row = [&](S16RowH& H, int r) {
            const uint32_t rk = (unsigned)r < (unsigned)kH ? 0xffffffffu : 0u;      // (wave-uniform)
#pragma unroll
            for (int pq = 0; pq < 2; ++pq)
#pragma unroll
                for (int e = 0; e < 4; ++e) { H.f[0][pq][e] &= rk; H.f[1][pq][e] &= rk; H.h[pq][e] &= hkeep & rk; }
        };
        S16RowH H0, H1, H2;                               // h9 of rows y - 1, y, y + 1 of the output row y, in rotating roles
        S16Row C1;                                        // c1 of row y
        u32x4 C8[2];                                      // c8 of row y >> 1 at the lane's pixel, [plane]
        auto load_c1 = [&](int r) {
            const char* p = c1w + (size_t)r * kRowB;
#pragma unroll
            for (int t = 0; t < 2; ++t) { C1.f[t][0] = *(const u32x4*)(p + voff[t]); C1.f[t][1] = *(const u32x4*)(p + lo + voff[t]); }
        };
        auto load_c8 = [&](int r8) {
            const char* p = c8w + (size_t)r8 * kRowB8;
            C8[0] = *(const u32x4*)(p + voff8); C8[1] = *(const u32x4*)(p + lo + voff8);
        };
        f32x4 F[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};      // conv_flatten's sums over the unit's rows, [pixel tile]
        uint32_t ovt[2] = {0u, 0u};

        // one output row: Ha = h9 of row y - 1, Hb = row y, Hn = row y + 1 (requested a row step ago; masked in front of its taps)
        auto row_step = [&](int y, S16RowH& Ha, const S16RowH& Hb, S16RowH& Hn) {
            S16Ring3 ring;                                // (two of its slots: every set here serves twelve products)
            ring.rd_tap(0, wl_base, 0);
            u32x4 pw[2][2][2];                            // the projection's fragments, [source][channel tile][plane]
#pragma unroll
            for (int q = 0; q < 8; ++q) pw[q >> 2][(q >> 1) & 1][q & 1] = *(const u32x4*)(pl_base + q * 1024);
            // row y's flatten filter: rows 0 .. 3 of the A fragment, high and low halves
            const u32x4 fwh = *(const u32x4*)(fw_base + (size_t)(2 * y) * 1024), fwl = *(const u32x4*)(fw_base + (size_t)(2 * y + 1) * 1024);
            __builtin_amdgcn_sched_barrier(0);
            // ---- P = b2 + br + projection of cat[c1, up(c8)] at (y, x) ----
            f32x4 P[2][2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int u = 0; u < 2; ++u) P[t][u] = bias[u];
#pragma unroll
            for (int src = 0; src < 2; ++src)
#pragma unroll
                for (int pr = 0; pr < 3; ++pr)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int t = 0; t < 2; ++t) {
                            const int pq = pr == 0 ? 1 : 0;
                            const u32x4& x = src == 0 ? C1.f[t][pq] : C8[pq];
                            P[t][u] = s16_mfma(pw[src][u][pr == 1 ? 1 : 0], x, P[t][u]);
                        }
            __builtin_amdgcn_sched_barrier(0);
            // the next row's c1 and c8, into the registers just read: they arrive behind this row's taps.  Every request of the loop is
            // unconditional: behind a branch that may or may not have issued loads, the compiler cannot count which of the outstanding
            // ones is the oldest and waits for all of them.  So c8's row is asked for in both rows of its pair, and the unit's last row
            // asks again for the rows it has (from the cache).
            load_c1(min(y + 1, ylast));
            load_c8(min(y + 1, ylast) >> 1);
            __builtin_amdgcn_sched_barrier(0);
            // ---- the 3 x 3 ----
            s16_taps_shifted(ring, wl_base, Ha, Hb, Hn, P, [] {}, [&](int tap) {
                if (tap == 2) load_row(Ha, min(y + 2, ylast + 1));     // row y - 1 has been read: row y + 2 takes its registers
                if (tap == 5) mask_row(Hn, y + 1);
            });
            __builtin_amdgcn_sched_barrier(0);
            // ---- ReLU, split; the range test; conv_flatten's products on the split row ----
            float v[2][2][4];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[t][u][r] = relu_i(P[t][u][r]);
            uint32_t kh[2][4], kl[2][4];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                s16_split_px(v[t], kh[t], kl[t]);
#pragma unroll
                for (int i = 0; i < 4; ++i) ovt[t] = pk_max_u16(ovt[t], kh[t][i]);
            }
#pragma unroll
            for (int pr = 0; pr < 3; ++pr)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const uint32_t (&k)[4] = pr == 0 ? kl[t] : kh[t];
                    F[t] = s16_mfma(pr == 1 ? fwl : fwh, u32x4{k[0], k[1], k[2], k[3]}, F[t]);
                }
            if (a.store_out) {                            // (wave-uniform) c9 itself: only when the spec head runs
                char* p = ow + (size_t)y * kRowB;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    *(u32x4*)(p + voff[t]) = u32x4{kh[t][0], kh[t][1], kh[t][2], kh[t][3]};
                    *(u32x4*)(p + lo + voff[t]) = u32x4{kl[t][0], kl[t][1], kl[t][2], kl[t][3]};
                }
            }
        };

        load_row(H0, y0 - 1); load_row(H1, y0); load_c1(y0); load_c8(y0 >> 1); load_row(H2, y0 + 1);
        mask_row(H0, y0 - 1); mask_row(H1, y0);
        // the three h9 rows change roles instead of places: three steps per turn
        int k = 0;
        for (; k + 3 <= rows_per_unit; k += 3) {
            row_step(y0 + k, H0, H1, H2);
            row_step(y0 + k + 1, H1, H2, H0);
            row_step(y0 + k + 2, H2, H0, H1);
        }
        if (k < rows_per_unit) {
            row_step(y0 + k, H0, H1, H2);
            if (k + 1 < rows_per_unit) row_step(y0 + k + 1, H1, H2, H0);
        }
        // the unit's flatten sums: result rows 0 .. 3 (lanes g = 0) are the four flatten channels of the lane's pixel
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (g == 0) {
                float* fp = a.flat_part + ((size_t)n * bands + b) * 4 * kW + xt[t];
#pragma unroll
                for (int r = 0; r < 4; ++r) fp[r * kW] = F[t][r];
            }
            ovf = pk_max_u16(ovf, ovt[t]);
        }
    }
    if (((ovf & 0x7fff7fffu) + 0x04000400u) & 0x80008000u) atomicOr(a.range_flag, 1);       // (rare: the engine turns it into SS_ERR_RANGE)
}

static bool px64(ActStride s) { return s.pix == 64u; }   // pixel-major, 32 channels: a pixel's plane is one 64-byte run
bool conv9_stream_supports(const ConvArgs& a) {
    return a.H == kH && a.W == kW && a.Cout == kC && a.C0 == kC && a.C1 == 0 && a.C0x == kC && a.C1x == kC && a.src0 && a.xp0 && a.xp1 && a.wpk &&
           a.proj_w && a.bias && a.flat_w4 && a.flat_part && (a.out || !a.store_out) && !a.pool_out && !a.res_in && a.lo_delta != 0 && a.range_flag &&
           a.N > 0 && px64(a.s_src0) && px64(a.s_xp0) && px64(a.s_xp1) && (px64(a.s_out) || !a.store_out);
}
const char* conv9_stream_variant() { return "conv9_stream16_kernel"; }
size_t conv9_stream_proj_bytes() { return kProjFrag; }
size_t conv9_stream_flat_bytes() { return (size_t)kH * 2 * 1024; }
bool conv9_stream_rows_ok(int rows_per_unit) { return rows_per_unit >= 2 && !(rows_per_unit & 1) && kH % rows_per_unit == 0 && rows_per_unit <= kMaxRows; }
int conv9_stream_flat_groups(int rows_per_unit) { return kH / rows_per_unit; }
// multiply-adds per term that the launch issues: a strip row is 24 + 108 + 6 products of 16 x 16 x 32,
// three products to a term (ScopedLaunch counts the three)
double conv9_stream_issued_macs(int N) { return (double)N * kH * kStrips32 * ((24 + 108 + 6) / 3) * (16.0 * 16 * 32); }

hipError_t launch_conv9_stream(const ConvArgs& a, int rows_per_unit, int grid_override, int num_cus, hipStream_t s) {
    if (!conv9_stream_supports(a) || !conv9_stream_rows_ok(rows_per_unit)) return hipErrorInvalidValue;
    const int64_t total = (int64_t)a.N * (kH / rows_per_unit) * kStrips32;
    if (total >= (int64_t)1 << 30) return hipErrorInvalidValue;
    const int cus = num_cus > 0 ? num_cus : 256;
    int grid = (int)std::min<int64_t>(cus, (total + kS1Waves - 1) / kS1Waves);
    if (grid_override > 0) grid = std::min(grid, grid_override);
    static std::atomic<uint64_t> attr_done{0};
    const size_t lds = 2 * (size_t)kBank + kProjFrag;
    if (hipError_t e = allow_full_lds((const void*)conv9_stream16_kernel, attr_done)) return e;
    hipLaunchKernelGGL(conv9_stream16_kernel, dim3(grid), dim3(64 * kS1Waves), lds, s, a, rows_per_unit, (int)total);
    return hipGetLastError();
}

}  // namespace ss
