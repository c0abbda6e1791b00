// conv9_1.A (the first conv of ResBlock(64, 32) at 128 x 256 on cat[c1, up2(c8)], BatchNorm, ReLU -> h9: pytorch_neural_nets.py:7-41,
// 180-181) as a ROW-STREAMING kernel, f16x2 mode, on stream16.h's core without overlap columns.
//
// Why.  In conv4_ups.hip this launch is conv4.hip's four-tile structure: patch images through the LDS and two barriers per stage, the
// matrix pipe busy in 56 % of its cycles and neither roof near.  Its operands are the tensors conv9s.hip already reads straight from
// memory as MFMA operands -- c1 and c8 are 32 channels, pixel-major, a pixel's plane one 64-byte run.
//
//   * Work unit = (window, band of `rows` rows, strip of 32 columns, all of them stored), strips fastest; a wave's units are independent.
//   * Skip half (c1): nine taps on rows y - 1, y, y + 1, held in three register sets that change roles; behind tap 2 the loads of row
//     y + 2 are issued into the registers of row y - 1.  A set is the two pixel tiles and the halo load (stream16.h).  108 products.
//   * Upsampled half (c8) at c8's resolution: with x = 32 s + 2 c + t both tiles' lane c sit on c8 pixel j = 16 s + c, so one 16-pixel
//     tile of c8 serves both, and nearest upsampling puts the same c8 pixel under two taps of a row or a column -- their weights are
//     summed when they are packed (weights.hip pack_ups_stream16, the sums of conv4_ups.hip's header):
//         columns   tile 0 (even x): w[-1] c8[j - 1] + (w[0] + w[+1]) c8[j]         tile 1 (odd x): (w[-1] + w[0]) c8[j] + w[+1] c8[j + 1]
//         rows      y = 2 Y:         w[-1] row Y - 1 + (w[0] + w[+1]) row Y         y = 2 Y + 1:    (w[-1] + w[0]) row Y + w[+1] row Y + 1
//     c8[j - 1] / c8[j + 1] are the row shifted with its halo lane.  2 rows x 4 column forms x 2 channel tiles x 3 = 48 products into the
//     same P[t][u] (a full-resolution form would issue 72).  c8's rows Y - 1, Y, Y + 1 are three sets that change roles per row PAIR;
//     behind the even row's last product on row Y - 1 the loads of row Y + 2 go into its registers, three row steps ahead of their use.
//     The row parity and both role cycles are compile-time: six copies of the row step, no request behind a branch.
//   * Rows and halo pixels outside the picture are zero operands (clamped addresses, wave-uniform masks: the 3 x 3's zero padding).
//   * Fragments: the c1 banks (36 KB, pack_conv_stream16 of the conv's first 32 input channels) and the c8 sets (64 KB, [row parity][row
//     tap][column form][channel tile][plane][lane][16 B]) are resident in the LDS, one barrier behind their load.  A c1 tap's set is
//     read one tap ahead; a c8 set serves six products and is read two sets ahead, so every read lies twelve products in front of its
//     first use; the next row's first set is asked for in front of this row's last twelve products.
//   * out = P + b1, ReLU, split into f16 halves, both planes of h9 stored in the order conv9s.hip reads; the high halves are range-tested
//     as in conv4_ups.hip's form.
// Per row and wave: 108 + 48 products of 16 matrix cycles.  Launch: one 512-thread block per CU, two waves per SIMD.
//
// Jitter test (SS_JITTER_SLEEP): nothing to cover -- no synchronisation point after the prologue, the waves share read-only LDS.
#include "kernels.h"
#include "stream16.h"
#include <algorithm>
#include <type_traits>

namespace ss {

static constexpr int kUpsFrag = 2 * 2 * 4 * 2 * 2 * 1024;       // [row parity][row tap][column form][channel tile][plane][lane][16 B]
static constexpr uint32_t kRowB = kW * 64, kRowB8 = (kW / 2) * 64;   // bytes per row of a plane of c1 / h9, of c8

struct A9Row8 { u32x4 f[2]; u32x4 h[2]; };               // a strip row of c8: the tile and the halo load, [plane]

__global__ __launch_bounds__(64 * kS1Waves) __attribute__((amdgpu_waves_per_eu(2, 2)))
void conv3x3_ups_stream16_kernel(ConvArgs a, int rows_per_unit, int total_units) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sW = smem;                                      // c1: [plane][tap][channel tile][lane][16 B]
    char* sU = smem + 2 * kBank;                          // c8: [row parity][row tap][column form][channel tile][plane][lane][16 B]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, c = lane & 15;
    for (int p = tid; p < 2 * kBank / 16; p += 64 * kS1Waves) *(u32x4*)(sW + p * 16) = *(const u32x4*)((const char*)a.wpk + (size_t)p * 16);
    for (int p = tid; p < kUpsFrag / 16; p += 64 * kS1Waves) *(u32x4*)(sU + p * 16) = *(const u32x4*)((const char*)a.wpk_b + (size_t)p * 16);
    // result row 4 g + r of channel tile u is channel 8 g + 4 u + r
    const f32x4 bias[2] = {*(const f32x4*)(a.bias + 8 * g), *(const f32x4*)(a.bias + 8 * g + 4)};
    __syncthreads();                                      // the only barrier

    const char* wl_base = sW + lane * 16;
    const char* ul_base = sU + lane * 16;
    const int bands = kH / rows_per_unit;
    const int64_t lo = a.lo_delta;
    uint32_t ovf = 0;                                     // the largest high halves stored (all exponent bits set = infinity / NaN)

    for (int unit = (int)blockIdx.x * kS1Waves + wave; unit < total_units; unit += (int)gridDim.x * kS1Waves) {
        const int s = unit % kStrips32, b = (unit / kStrips32) % bands, n = unit / (kStrips32 * bands);
        const int x0 = 32 * s, y0 = b * rows_per_unit, ylast = y0 + rows_per_unit - 1;
        // this lane's runs in a row of c1 / h9 (tile t: column x0 + 2 c + t), of c8 (pixel 16 s + c), and its halo pixels' (lanes c < 8:
        // the one left of the strip, the others the one right of it; outside the picture: the edge pixel, masked)
        const uint32_t voff[2] = {(uint32_t)(x0 + 2 * c) * 64u + (uint32_t)g * 16u, (uint32_t)(x0 + 2 * c + 1) * 64u + (uint32_t)g * 16u};
        const uint32_t hoff = (uint32_t)(c < 8 ? max(x0 - 1, 0) : min(x0 + 32, kW - 1)) * 64u + (uint32_t)g * 16u;
        const uint32_t voff8 = (uint32_t)(x0 / 2 + c) * 64u + (uint32_t)g * 16u;
        const uint32_t hoff8 = (uint32_t)(c < 8 ? max(x0 / 2 - 1, 0) : min(x0 / 2 + 16, kW / 2 - 1)) * 64u + (uint32_t)g * 16u;
        const uint32_t hkeep = (c < 8 ? s > 0 : s < kStrips32 - 1) ? 0xffffffffu : 0u;
        const char* c1w = (const char*)a.src0 + (size_t)n * kH * kRowB;         // the window's c1, c8 (high planes; the low ones lie `lo` behind)
        const char* c8w = (const char*)a.src1 + (size_t)n * (kH / 2) * kRowB8;
        char* ow = (char*)a.out + (size_t)n * kH * kRowB;

        // c1 of picture row r, c8 of its row r8 (any row: outside the picture the nearest row is read and the mask clears it)
        auto load_row = [&](S16RowH& H, int r) {
            const char* p = c1w + (size_t)min(max(r, 0), kH - 1) * kRowB;
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
        auto load_row8 = [&](A9Row8& K, int r8) {
            const char* p = c8w + (size_t)min(max(r8, 0), kH / 2 - 1) * kRowB8;
            K.f[0] = *(const u32x4*)(p + voff8); K.f[1] = *(const u32x4*)(p + lo + voff8);
            K.h[0] = *(const u32x4*)(p + hoff8); K.h[1] = *(const u32x4*)(p + lo + hoff8);
        };
        auto mask_row8 = [&](A9Row8& K, int r8) {
            const uint32_t rk = (unsigned)r8 < (unsigned)(kH / 2) ? 0xffffffffu : 0u;
#pragma unroll
            for (int pq = 0; pq < 2; ++pq)
#pragma unroll
                for (int e = 0; e < 4; ++e) { K.f[pq][e] &= rk; K.h[pq][e] &= hkeep & rk; }
        };
        S16RowH H0, H1, H2;                               // c1 of rows y - 1, y, y + 1 of the output row y, in rotating roles
        A9Row8 K0, K1, K2;                                // c8 of rows Y - 1, Y, Y + 1 of the output rows 2 Y, 2 Y + 1, in rotating roles
        S16Ring3 ring;
        uint32_t ovt = 0;

        // One output row y = 2 Y + par.  Ha / Hb / Hn: c1 of rows y - 1 / y / y + 1 (Hn requested a row step ago, masked in front of its
        // taps); Ka / Kb / Kc: c8 of rows Y - 1 / Y / Y + 1 (Kc masked in the odd row, in front of its only use in the pair).
        auto row_step = [&](auto parity, int y, S16RowH& Ha, const S16RowH& Hb, S16RowH& Hn, A9Row8& Ka, const A9Row8& Kb, A9Row8& Kc) {
            constexpr int par = decltype(parity)::value;
            // a c8 set: row tap ty (par 0: rows Y - 1, Y; par 1: rows Y, Y + 1), column form f = 2 t + tx; set q = 4 ty + order of f, in slot (q + 1) % 3
            auto form = [](int q) { return ((q & 1) << 1) | ((q >> 1) & 1); };      // 0, 2, 1, 3: the pixel tiles take turns
            auto rd_set8 = [&](int q) {
                const char* p = ul_base + (((par * 2 + (q >> 2)) * 4 + form(q)) * 4) * 1024;
                ring.rd((q + 1) % 3, p, p + 1024, 2048);
            };
            f32x4 P[2][2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int u = 0; u < 2; ++u) P[t][u] = bias[u];
            // ---- the skip half: nine taps on c1 ----
            s16_taps_shifted(ring, wl_base, Ha, Hb, Hn, P, [&] { rd_set8(0); rd_set8(1); }, [&](int tap) {
                if (tap == 2) load_row(Ha, min(y + 2, ylast + 1));     // row y - 1 has been read: row y + 2 takes its registers
                if (tap == 5) { mask_row(Hn, y + 1); if constexpr (par != 0) mask_row8(Kc, (y >> 1) + 1); }
            });
            // ---- the upsampled half: two rows of c8, four column forms ----
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int ty = q >> 2, f = form(q), t = f >> 1, slot = (q + 1) % 3;
                const A9Row8& K = par == 0 ? (ty == 0 ? Ka : Kb) : (ty == 0 ? Kb : Kc);
                if (q + 2 < 8) rd_set8(q + 2);
                else if (q == 6) ring.rd_tap(0, wl_base, 0);           // the next row step's first tap
                u32x4 B[2];
#pragma unroll
                for (int pq = 0; pq < 2; ++pq) B[pq] = f == 0 ? s16_shr1_halo(K.f[pq], K.h[pq]) : (f == 3 ? s16_shl1_halo(K.f[pq], K.h[pq]) : K.f[pq]);
                __builtin_amdgcn_sched_barrier(0);
                s16_products(ring, slot, B, P[t]);
                __builtin_amdgcn_sched_barrier(0);
                // row Y - 1 has been read for the last time in the even row: row Y + 2 takes its registers
                if (par == 0 && q == 3) load_row8(Ka, min((y >> 1) + 2, (ylast >> 1) + 1));
            }
            // ---- + b1 (in P from the start), ReLU, split, the range test, both planes of h9 ----
            char* p = ow + (size_t)y * kRowB;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float v[2][4];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[u][r] = relu_i(P[t][u][r]);
                uint32_t kh[4], kl[4];
                s16_split_px(v, kh, kl);
#pragma unroll
                for (int i = 0; i < 4; ++i) ovt = pk_max_u16(ovt, kh[i]);
                *(u32x4*)(p + voff[t]) = u32x4{kh[0], kh[1], kh[2], kh[3]};
                *(u32x4*)(p + lo + voff[t]) = u32x4{kl[0], kl[1], kl[2], kl[3]};
            }
        };

        load_row(H0, y0 - 1); load_row(H1, y0); load_row8(K0, (y0 >> 1) - 1); load_row8(K1, y0 >> 1); load_row(H2, y0 + 1); load_row8(K2, (y0 >> 1) + 1);
        ring.rd_tap(0, wl_base, 0);
        mask_row(H0, y0 - 1); mask_row(H1, y0); mask_row8(K0, (y0 >> 1) - 1); mask_row8(K1, y0 >> 1);
        // the c1 rows change roles every row, the c8 rows every pair of rows: six steps per turn
        const std::integral_constant<int, 0> even; const std::integral_constant<int, 1> odd;
        for (int k = 0; k < rows_per_unit; k += 6) {
            row_step(even, y0 + k, H0, H1, H2, K0, K1, K2);
            row_step(odd, y0 + k + 1, H1, H2, H0, K0, K1, K2);
            if (k + 2 >= rows_per_unit) break;
            row_step(even, y0 + k + 2, H2, H0, H1, K1, K2, K0);
            row_step(odd, y0 + k + 3, H0, H1, H2, K1, K2, K0);
            if (k + 4 >= rows_per_unit) break;
            row_step(even, y0 + k + 4, H1, H2, H0, K2, K0, K1);
            row_step(odd, y0 + k + 5, H2, H0, H1, K2, K0, K1);
        }
        ovf = pk_max_u16(ovf, ovt);
    }
    if (((ovf & 0x7fff7fffu) + 0x04000400u) & 0x80008000u) atomicOr(a.range_flag, 1);       // (rare: the engine turns it into SS_ERR_RANGE)
}

static bool px64(ActStride s) { return s.pix == 64u; }   // pixel-major, 32 channels: a pixel's plane is one 64-byte run
bool conv9a_stream_supports(const ConvArgs& a) {
    return a.plain && a.H == kH && a.W == kW && a.Cout == kC && a.C0 == kC && a.C1 == kC && a.src0 && a.src1 && a.wpk && a.wpk_b && a.bias && a.out &&
           !a.pool_out && !a.res_in && !a.res_out && a.lo_delta != 0 && a.range_flag && a.N > 0 && px64(a.s_src0) && px64(a.s_src1) && px64(a.s_out);
}
const char* conv9a_stream_variant() { return "conv3x3_ups_stream16_kernel"; }
size_t conv9a_stream_ups_bytes() { return kUpsFrag; }
bool conv9a_stream_rows_ok(int rows_per_unit) { return rows_per_unit >= 2 && !(rows_per_unit & 1) && kH % rows_per_unit == 0 && rows_per_unit <= kMaxRows; }
// multiply-adds per term that the launch issues: a strip row is 108 + 48 products of 16 x 16 x 32, three products to a term
double conv9a_stream_issued_macs(int N) { return (double)N * kH * kStrips32 * ((108 + 48) / 3) * (16.0 * 16 * 32); }

hipError_t launch_conv9a_stream(const ConvArgs& a, int rows_per_unit, int grid_override, int num_cus, hipStream_t s) {
    if (!conv9a_stream_supports(a) || !conv9a_stream_rows_ok(rows_per_unit)) return hipErrorInvalidValue;
    const int64_t total = (int64_t)a.N * (kH / rows_per_unit) * kStrips32;
    if (total >= (int64_t)1 << 30) return hipErrorInvalidValue;
    const int cus = num_cus > 0 ? num_cus : 256;
    int grid = (int)std::min<int64_t>(cus, (total + kS1Waves - 1) / kS1Waves);
    if (grid_override > 0) grid = std::min(grid, grid_override);
    static std::atomic<uint64_t> attr_done{0};
    const size_t lds = 2 * (size_t)kBank + kUpsFrag;
    if (hipError_t e = allow_full_lds((const void*)conv3x3_ups_stream16_kernel, attr_done)) return e;
    hipLaunchKernelGGL(conv3x3_ups_stream16_kernel, dim3(grid), dim3(64 * kS1Waves), lds, s, a, rows_per_unit, (int)total);
    return hipGetLastError();
}

}  // namespace ss
