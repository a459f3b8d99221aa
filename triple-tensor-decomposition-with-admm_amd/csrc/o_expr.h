// The outlier tensor of the last finished ADMM iteration, which K5 never
// stores: O_k = (D + (1/muL_{k+1}) Y_L) - T_{k+1}, stated once for the kernels
// that rebuild it (k_o_fixup, k_o_fixup32) and the one that only thresholds it
// (k_foreground.hip).  The library is compiled with -ffp-contract=off, so the
// same expression gives the same bits wherever it is inlined.
#pragma once

#include <hip/hip_runtime.h>

namespace tritd {

// fp64 session, before the mask
__device__ __forceinline__ double o_expr(double d, double yl, double t, double invL_next) {
    return (d + invL_next * yl) - t;
}
// obs: the element's bit of the mask words (true without a mask); an
// unobserved element holds L in T, and O there is 0 (k5_fused MK).
__device__ __forceinline__ double o_value(double d, double yl, double t, double invL_next,
                                          bool obs) {
    const double v = o_expr(d, yl, t, invL_next);
    return obs ? v : 0.0;
}

// fp32 session: evaluated in double, rounded to single
__device__ __forceinline__ float o_value32(float d, float yl, float t, float invL_next) {
    const double v = ((double)d + (double)invL_next * (double)yl) - (double)t;
    return (float)v;
}

}  // namespace tritd
