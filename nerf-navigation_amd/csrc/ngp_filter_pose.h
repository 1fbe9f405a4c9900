// ngp_filter_pose.h -- the camera pose of a filter state, float32: measurement_fn's chain (nav/estimator_helpers.py:301-309) as the filter's kernels
// evaluate it.  One copy for k_filter_rays, k_filter_step, k_filter_hessian (nav_filter.hip) and the agent's sensor rays (nav_agent.hip): the observation is
// taken along exactly the rays the filter predicts along.  Operation order is part of the contract (-ffp-contract=off).
#pragma once
#include "ngp_filter_step.h"

// rot_x(pi / 2) as the reference builds it: cos and sin of (float)(pi / 2) in float32
#define NF_C90 (-4.37113883e-08f)

// vec_to_rot_matrix (nav/math_utils.py:159-174) and what its backward needs
struct nf_rodrigues { float K[9], M[9], R[9], a, d, sn, cs; };

__device__ __forceinline__ void nf_rotation(const float* r, nf_rodrigues& Q) {
    Q.a = sqrtf((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    Q.d = 1e-10f + Q.a;
    const float k0 = r[0] / Q.d, k1 = r[1] / Q.d, k2 = r[2] / Q.d;
    const float K[9] = {0.f, -k2, k1, k2, 0.f, -k0, -k1, k0, 0.f};
    Q.sn = sinf(Q.a); Q.cs = cosf(Q.a);
    const float omc = 1.0f - Q.cs;
#pragma unroll
    for (int e = 0; e < 9; e++) { Q.K[e] = K[e]; Q.M[e] = omc * K[e]; }
    float MK[9];
    nfs_matmul3(Q.M, Q.K, MK);
#pragma unroll
    for (int e = 0; e < 9; e++) Q.R[e] = ((e % 4 == 0 ? 1.0f : 0.0f) + Q.sn * K[e]) + MK[e];
}

// measurement_fn's pose (nav/estimator_helpers.py:301-309): P = cycle (rot_x(pi/2) R) diag(1, -1, -1), T = cycle position (nerf_matrix_to_ngp_torch)
__device__ __forceinline__ void nf_pose(const float* state, nf_rodrigues& Q, float* P, float* T) {
    const float r[3] = {state[6], state[7], state[8]};
    nf_rotation(r, Q);
    nfs_camera_axes(Q.R, (double)NF_C90, P);
#pragma unroll
    for (int i = 0; i < 3; i++) T[i] = state[(i + 1) % 3];
}
