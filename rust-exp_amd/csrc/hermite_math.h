// hermite_math.h -- the device arithmetic that hermite.hip (K8) and hermite_block.hip (K9) must perform in ONE order: the
// corrector and the time-step ratio.  Every product and sum is rounded on its own (no contraction), so that a block step in which
// every body is due reproduces the shared step bit for bit.
#pragma once
#include "kernels.h"

namespace nbx {

// the corrector, h = dt / 2 (exact), c12 = dt^2 / 12 (rounded once, on the host); every product and sum rounded on its own:
//   v1 = (v + (a0 + a1) h) + (j0 - j1) c12        x1 = (x + (v + v1) h) + (a0 - a1) c12
__device__ __forceinline__ float correct_v(float v, float a0, float a1, float j0, float j1, float h, float c12)
{
    return __fadd_rn(__fadd_rn(v, __fmul_rn(__fadd_rn(a0, a1), h)), __fmul_rn(__fsub_rn(j0, j1), c12));
}
__device__ __forceinline__ float correct_x(float x, float v, float v1, float a0, float a1, float h, float c12)
{
    return __fadd_rn(__fadd_rn(x, __fmul_rn(__fadd_rn(v, v1), h)), __fmul_rn(__fsub_rn(a0, a1), c12));
}

// |a| / |j| = sqrt(|a|^2 / |j|^2): two sums of three squares, one IEEE division, one IEEE square root; |j| = 0: +inf (no constraint)
__device__ __forceinline__ float hermite_ratio(const HermiteAJ& k)
{
    const float a2 = __builtin_fmaf(k.a.z, k.a.z, __builtin_fmaf(k.a.y, k.a.y, __fmul_rn(k.a.x, k.a.x)));
    const float j2 = __builtin_fmaf(k.j.z, k.j.z, __builtin_fmaf(k.j.y, k.j.y, __fmul_rn(k.j.x, k.j.x)));
    return j2 > 0.f ? __fsqrt_rn(__fdiv_rn(a2, j2)) : __builtin_inff();
}

}  // namespace nbx
