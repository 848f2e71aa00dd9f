// adam.h -- one Adam update (torch.optim.Adam's order), shared by adam_kernel (csrc/fastnsf.hip: himo_adam_step) and
// nsf_update_kernel (csrc/nsffused.hip: himo_nsf_update), which must give the same bits for the same inputs.
//
// Every fused multiply-add is WRITTEN here.  Left to the compiler (-ffp-contract=fast, the default of both files) the two kernels
// disagreed: nsf_update_kernel got m' = fma(1 - b1, g, b1 m) and v' = fma(b2, v, ((1 - b2) g) g), while in adam_kernel the
// vectoriser packed the products of m' and v' into v_pk_mul_f32 / v_pk_add_f32 first, which left nothing to contract -- m', v' and
// therefore p' differed in their last bits as soon as m and v were not zero (tests/test_nsf_conformance_gpu.py, step 1000).
// An explicit fmaf is never split and a product that feeds one is never contracted again, so the form below does not depend on
// what either optimiser pass does.  It is the form nsf_update_kernel had: the default FastNSF / NSFP fits keep their bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace himo {

// bc1 = 1 - b1^step, bc2_sqrt = sqrt(1 - b2^step)
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float lr, float b1, float b2, float eps, float bc1,
                                            float bc2_sqrt) {
    const float mi = fmaf(1.f - b1, g, b1 * m);
    const float vi = fmaf(b2, v, ((1.f - b2) * g) * g);
    m = mi; v = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p = fmaf(-(lr / bc1), mi / denom, p);
}

}  // namespace himo
