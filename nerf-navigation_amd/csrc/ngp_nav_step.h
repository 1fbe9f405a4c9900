// ngp_nav_step.h -- what the one-workgroup step kernels of the planner (nav_plan.hip) and of the pose filter (nav_filter.hip) share: the wave sum
// and torch.optim.Adam's step.  Kept out of ngp_device.h: no other kernel uses them, and bench.py ties the committed frame and training profiles to that file's bytes.
#pragma once
#include "ngp_device.h"

// sum over the 64 lanes of a wave by the xor butterfly: a fixed order, every lane ends with the same bits
__device__ __forceinline__ float ngp_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// torch.optim.Adam(capturable=True) on float32 tensors (adam.hip, the training optimiser, is other arithmetic).
// w1 = (float)(1 - beta1), w2 = (float)(1 - beta2) formed in float64: the lerp weight and addcmul value of a float32 tensor
struct ngp_adam_coef { float lr, beta1, beta2, w1, w2, eps; };
static inline ngp_adam_coef ngp_adam_fill(double lr, double beta1, double beta2, double eps) {
    return {(float)lr, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps};
}
// one element of the multi-tensor step (torch/optim/adam.py, _multi_tensor_adam), step = the new count
__host__ __device__ __forceinline__ float ngp_adam_step(const ngp_adam_coef& A, float param, float grad, float* m, float* v, float step) {
    *m = *m + A.w1 * (grad - *m);                                        // lerp(exp_avg, grad, 1 - beta1)
    *v = *v * A.beta2 + A.w2 * (grad * grad);                            // mul + addcmul
    float bc1 = powf(A.beta1, step), bc2 = powf(A.beta2, step);
    bc1 = bc1 - 1.0f; bc2 = -(bc2 - 1.0f);
    const float step_size = 1.0f / (bc1 / A.lr);
    const float bc2_sqrt = sqrtf(bc2);
    const float denom = (sqrtf(*v) / bc2_sqrt + A.eps) / step_size;
    return param + *m / denom;
}
