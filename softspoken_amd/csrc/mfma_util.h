// Device helpers shared by the conv kernels (conv2.hip, conv2_ups.hip, conv4.hip, conv4_ups.hip, conv1s.hip): vector types, 16-bit
// pair packing, the f16x2 split, the 32x32x16 matrix product, the accumulator-tile -> 16-byte-run shuffle, LDS-only barriers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ss {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

static constexpr int kHdr = 256;         // zero bytes in front of every activation tensor (engine.hip ensure_workspace)

// LDS ops of one wave execute in issue order, so a wave's own write -> read needs no hardware wait; the asm
// statement only pins the compiler's order (and drains lgkmcnt, which is cheap).  It must NOT wait on vmcnt:
// the next stage's prefetch loads and this tile's output stores are meant to stay in flight.
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// workgroup barrier that orders LDS only (a __syncthreads() would also emit vmcnt(0))
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// ... and one that waits for the wave's loads and stores as well
__device__ __forceinline__ void vm_lds_barrier() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
}
// f16x2 mode: a value is the sum of two f16 halves.  hi = f16(v) (round to nearest), lo = f16(v - hi): v - hi is exact in fp32, so
// the pair carries ~22 significant bits; small low halves are f16 subnormals, which the matrix instruction keeps.
__device__ __forceinline__ uint32_t pack_f16(float lo, float hi) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{lo, hi}, f16x2));
}
__device__ __forceinline__ f32x2 unpack_f16(uint32_t v) { return __builtin_convertvector(__builtin_bit_cast(f16x2, v), f32x2); }
// the largest high half seen so far, per 16-bit lane (the values are >= 0 behind the ReLU: as unsigned integers they order like the
// values, infinity and NaN on top): one instruction per pair; the test for "all exponent bits set" happens once, on the maximum
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// lo = f16(x - hi) of a pair whose high halves are packed in `hi`: the mixed-precision FMA reads the f16 half and the fp32 value, subtracts in
// fp32 (exactly: hi is x rounded) and rounds to f16 into one half of the destination -- two instructions for the pair instead of two
// conversions back, two subtractions and a pack; bit for bit the same (tools/probes/fma_mix_split.hip)
__device__ __forceinline__ uint32_t split_lo(uint32_t hi, float x0, float x1) {
    uint32_t l;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l) : "v"(hi), "v"(x0));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l) : "v"(hi), "v"(x1));
    return l;
}
// ReLU as an integer max: negative floats (and -0) are negative integers -- one instruction (fmaxf: a NaN-quieting v_max first)
__device__ __forceinline__ float relu_i(float x) {
    const int b = __builtin_bit_cast(int, x);
    return __builtin_bit_cast(float, b > 0 ? b : 0);
}
// one 32x32x16 product on 16-bit operands: bf16 (throughput mode) or f16 (f16x2 mode)
template <bool F16>
__device__ __forceinline__ f32x16 mfma16(const u32x4& a, const u32x4& b, const f32x16& c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// The f16x2 multiply loops are written as software prefetch: the operand fragments of step st + depth - 1 are read from the LDS in front
// of the products of step st.  Left to itself the scheduler sinks every ds_read to just in front of the v_mfma that consumes it and waits
// there for the whole LDS round trip (~130 cycles loaded, a product is 32): the depth exists in the source only.  A fence behind a step's
// reads and one behind its products keep the order as written; the compiler still counts lgkmcnt itself (tools/frag_distance.py
// reports, per product, how many products lie between its operands' read and itself in the binary).
__device__ __forceinline__ void frag_fence() { __builtin_amdgcn_sched_barrier(0); }
// lanes 32..63 of x <-> lanes 0..31 of y
__device__ __forceinline__ void half_swap(uint32_t& x, uint32_t& y) {
    const u32x2 r = __builtin_amdgcn_permlane32_swap(x, y, false, false);
    x = r[0]; y = r[1];
}

// accumulator tile of one (M-tile, 32 output channels): rows = channels, cols = pixels.  Register r of lane (m, hh) holds
// channel (r&3) + 8*(r>>2) + 4*hh of pixel m.  P[g][h] = channels 8g + 4hh + 2h + {0,1} as a bf16 / f16 pair.
struct Packed { uint32_t p[4][2]; };

// (g, hh) pairs -> 16-byte runs: after the swaps a lane holds channels [8*hh, 8*hh+8) in lo and [16 + 8*hh, 16 + 8*hh + 8) in hi
__device__ __forceinline__ void to_runs(Packed& k, u32x4& lo, u32x4& hi) {
    half_swap(k.p[0][0], k.p[1][0]); half_swap(k.p[0][1], k.p[1][1]);
    half_swap(k.p[2][0], k.p[3][0]); half_swap(k.p[2][1], k.p[3][1]);
    lo = u32x4{k.p[0][0], k.p[0][1], k.p[1][0], k.p[1][1]};
    hi = u32x4{k.p[2][0], k.p[2][1], k.p[3][0], k.p[3][1]};
}
__device__ __forceinline__ void from_runs(const u32x4& lo, const u32x4& hi, Packed& k) {   // the swap is its own inverse
    k.p[0][0] = lo[0]; k.p[0][1] = lo[1]; k.p[1][0] = lo[2]; k.p[1][1] = lo[3];
    k.p[2][0] = hi[0]; k.p[2][1] = hi[1]; k.p[3][0] = hi[2]; k.p[3][1] = hi[3];
    half_swap(k.p[0][0], k.p[1][0]); half_swap(k.p[0][1], k.p[1][1]);
    half_swap(k.p[2][0], k.p[3][0]); half_swap(k.p[2][1], k.p[3][1]);
}

}  // namespace ss

// Timing perturbation for the tests (dev build; ConvArgs::dbg bit 10, pattern in bits 11-12): chosen waves sleep ~1 us at synchronisation
// point `site` of their n-th stage.  Results must not change; a missing barrier shows up as a changed bit.
// (A statement macro: as a function, whose arguments are evaluated ahead of the test of bit 10, it gave the dev build's kernels another
// schedule than the text in place.)
#define SS_JITTER_SLEEP(dbg, wave, site, n)                                                                                               \
    if ((dbg) & 1024) {                                                                                                                   \
        const int pat_ = ((dbg) >> 11) & 3, w_ = (wave);                                                                                  \
        const bool z_ = pat_ == 0 ? ((w_ + (site) + (n)) & 3) == 0 : pat_ == 1 ? w_ == 0 : pat_ == 2 ? w_ != 0 : (w_ & 1) != 0;           \
        if (z_) __builtin_amdgcn_s_sleep(32);                                                                                             \
    }
