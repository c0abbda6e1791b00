// Region bands, the arithmetic shared by the whole-file kernels (separate.hip) and the streams' (stream.hip): steps 3 and 4 of
// include/softspoken.h "region bands".  Both sides must produce the same values in the same order, so the two pieces live here once.
#pragma once
#include "engine.h"

namespace ss {

// P(y) = expm1(min(y^2 ln 10, 600)); NaN -> 0
__device__ __forceinline__ double band_power(float yf) {
#pragma clang fp contract(off)
    if (yf != yf) return 0.0;
    const double y = (double)yf;
    const double a = y * y * 2.302585092994045684;
    return expm1(a < 600.0 ? a : 600.0);
}

// Step 4 for one region of one signal, by a block of 256 threads = (spec channel, band): thread t brings E of its (channel, band).
// Lane 0 forms C over the speech channel and lane 128 T_env, both sequentially (that fixes the rounding); the two quantile predicates
// and the argmax are evaluated by 128 lanes and min-reduced in LDS; lane 0 writes the record with ordinary stores.  Every thread of the
// block must call it; it ends with a barrier, so a block may call it again.
__device__ __forceinline__ void band_bounds_block(double e, int n_bins, int speech_ch, double q_low, double q_high, const double* __restrict__ hz,
                                                  ss_region_band* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double E[256];
    __shared__ double Cs[128];
    __shared__ double tot[2], emax;
    __shared__ int idx[3];
    const int t = threadIdx.x;
    E[t] = e;
    if (t < 3) idx[t] = 128;
    __syncthreads();
    if (t == 0) {
        const double* Es = E + speech_ch * 128;
        double c = 0.0, mx = 0.0;
        for (int m = 0; m < 128; ++m) { c += Es[m]; Cs[m] = c; mx = Es[m] > mx ? Es[m] : mx; }
        tot[0] = c; emax = mx;
    } else if (t == 128) {
        const double* Ee = E + (1 - speech_ch) * 128;
        double c = 0.0;
        for (int m = 0; m < 128; ++m) c += Ee[m];
        tot[1] = c;
    }
    __syncthreads();
    const double T = tot[0];
    if (t < 128) {
        if (Cs[t] >= q_low * T) atomicMin(&idx[0], t);
        if (Cs[t] >= q_high * T) atomicMin(&idx[1], t);
        if (E[speech_ch * 128 + t] == emax) atomicMin(&idx[2], t);
    }
    __syncthreads();
    if (t == 0) {
        ss_region_band o;
        o.n_bins = n_bins;
        if (n_bins == 0 || !(T > 0.0)) {
            o.low_hz = o.high_hz = o.peak_hz = o.speech_share = __builtin_nan("");
            o.band_low = o.band_high = o.band_peak = -1;
        } else {
            o.band_low = idx[0]; o.band_high = idx[1]; o.band_peak = idx[2];
            o.low_hz = hz[idx[0]]; o.high_hz = hz[idx[1] + 2]; o.peak_hz = hz[idx[2] + 1];
            o.speech_share = T / (T + tot[1]);
        }
        *out = o;
    }
    __syncthreads();
}

}  // namespace ss
