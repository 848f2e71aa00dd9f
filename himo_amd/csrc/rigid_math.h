// rigid_math.h -- q = R p + t in float32, the ONE statement of the arithmetic behind himo_rigid_transform (fastnsf.hip) and the move
// of himo_accum_insert (accumulate.hip).
//
// himo_rigid_transform has always been built with the compiler's default contraction, so its sums of products were fused
// multiply-adds in an order the compiler chose.  That sequence is written out here, operation by operation, so that it no longer
// depends on a flag or on the compiler and both entry points give the same bits:
//     q0 = fma(z, T[2],  fma(y, T[1], x * T[0])) + T[3]
//     q1 = fma(z, T[6],  fma(x, T[4], y * T[5])) + T[7]
//     q2 = fma(z, T[10], fma(x, T[8], y * T[9])) + T[11]
// one rounded product, two fused multiply-adds (each rounds once) and one rounded sum per row.  A product that feeds an fma, and a
// sum that takes an fma's result, cannot be contracted any further: -ffp-contract changes nothing here.  The numpy restatement is
// tests/accumulate_ref.py (rigid_move).
#pragma once
#include <hip/hip_runtime.h>

namespace himo {

// T: the first three rows of a row-major 4x4 transform (12 floats)
__device__ inline void rigid_apply(const float* __restrict__ T, float x, float y, float z, float q[3]) {
    q[0] = __builtin_fmaf(z, T[2], __builtin_fmaf(y, T[1], x * T[0])) + T[3];
    q[1] = __builtin_fmaf(z, T[6], __builtin_fmaf(x, T[4], y * T[5])) + T[7];
    q[2] = __builtin_fmaf(z, T[10], __builtin_fmaf(x, T[8], y * T[9])) + T[11];
}

}  // namespace himo
