// nav_agent.hip -- the agent of the navigation loop on the device (DESIGN.md §3.5 "Native agent and the closed loop"): Agent.step
// (nav/agent_helpers.py:65-99) without its Blender subprocess.  The world is seen through a renderer; what is native here is everything around that render:
//
//   k_agent_step     drone_dynamics (ngp_filter_step.h: the functions k_filter_propagate calls, float64 from float32 inputs) + noise, rounded once; the pose
//                    the reference writes for Blender, rot_x(pi/2) R(next_state[6:9]) | next_state[:3], and the body-frame pose step() returns (:97)
//   k_agent_rays     the sensor camera's H x W rays at a state: the filter's own pose chain (ngp_filter_pose.h) and ngp_camera_ray (ngp_camera.h), so the
//                    observation is taken along exactly the rays k_filter_rays predicts along, bit for bit
//   k_agent_sensor   the camera's 8-bit round trip (:205, nav/estimator_helpers.py:192): clamp to [0, 1], (uint8)(c * 255.0f), (float)((double)u8 / 255.0)
//
// All three: one launch on the caller's stream, no host read, no atomics, no workspace.  The streaming kernels move four elements per lane with 16-byte
// stores (4-byte ones for the uint8 image) when the pointers are aligned for them, and element by element otherwise.
#include "ngp_device.h"
#include "ngp_camera.h"
#include "ngp_filter_pose.h"

static constexpr uint32_t NA_THREADS = 256, NA_PER_LANE = 4;

// rot_x(phi) M for phi = +-pi/2 as the reference builds rot_x in float32: c = cos((float)(pi/2)) = NF_C90 (cos is even), s = +-1
__device__ __forceinline__ void na_rot_x(double c, double s, const double* M, double* out) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
        out[0 + j] = M[0 + j];
        out[3 + j] = c * M[3 + j] - s * M[6 + j];
        out[6 + j] = s * M[3 + j] + c * M[6 + j];
    }
}

__device__ __forceinline__ void na_write_pose(const double* R, const double* t, float* __restrict__ pose) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) pose[4 * i + j] = (float)R[3 * i + j];
        pose[4 * i + 3] = (float)t[i];
    }
    pose[12] = pose[13] = pose[14] = 0.0f;
    pose[15] = 1.0f;
}

// one wave, one working lane: a chain of dependent float64 operations with nothing to share out
__global__ __launch_bounds__(64) void k_agent_step(nfs_dyn D, const float* __restrict__ state, const float* __restrict__ action,
                                                   const float* __restrict__ noise, float* __restrict__ next_state, float* __restrict__ blender_pose,
                                                   float* __restrict__ body_pose) {
    if (threadIdx.x != 0) return;
    nfs_d1 x[12], next[12];                                                  // the value path of k_filter_propagate's numbers: the same next state, bit for bit
    double act[4];
#pragma unroll
    for (int k = 0; k < 12; k++) x[k] = nfs_d1((double)state[k]);
#pragma unroll
    for (int k = 0; k < 4; k++) act[k] = (double)action[k];
    nfs_drone_dynamics(D, x, act, next);
    nfs_d1 noisy[12];
#pragma unroll
    for (int k = 0; k < 12; k++) {
        noisy[k] = nfs_d1(next[k].v + (noise ? (double)noise[k] : 0.0));     // no noise is zero noise
        next_state[k] = (float)noisy[k].v;
    }
    if (!blender_pose && !body_pose) return;
    nfs_d1 R1[9];
    nfs_vec_to_rot(noisy + 6, 1e-10, R1);
    double R[9], Rb[9], Rc[9];
#pragma unroll
    for (int e = 0; e < 9; e++) R[e] = R1[e].v;
    const double t[3] = {noisy[0].v, noisy[1].v, noisy[2].v};
    na_rot_x((double)NF_C90, 1.0, R, Rb);
    if (blender_pose) na_write_pose(Rb, t, blender_pose);
    na_rot_x((double)NF_C90, -1.0, Rb, Rc);
    if (body_pose) na_write_pose(Rc, t, body_pose);
}

// lane: NA_PER_LANE consecutive pixels.  The pose is formed once per workgroup.
template <bool VEC>
__global__ __launch_bounds__(NA_THREADS) void k_agent_rays(ngp_camera view, const float* __restrict__ state, uint32_t N, float* __restrict__ rays_o,
                                                           float* __restrict__ rays_d) {
    __shared__ ngp_camera cam;
    if (threadIdx.x == 0) {
        float x[12];
#pragma unroll
        for (int k = 0; k < 12; k++) x[k] = state[k];
        nf_rodrigues Q;
        ngp_camera c = view;
        nf_pose(x, Q, c.r, c.t);
        cam = c;
    }
    __syncthreads();
    const uint32_t first = (blockIdx.x * NA_THREADS + threadIdx.x) * NA_PER_LANE;
    if (first >= N) return;
    const ngp_camera c = cam;
    const uint32_t count = N - first < NA_PER_LANE ? N - first : NA_PER_LANE;
    float o[3 * NA_PER_LANE], d[3 * NA_PER_LANE];
#pragma unroll
    for (uint32_t k = 0; k < NA_PER_LANE; k++) {
        ngp_camera_ray(c, first + (k < count ? k : 0), d + 3 * k);
#pragma unroll
        for (int a = 0; a < 3; a++) o[3 * k + a] = c.t[a];
    }
    const size_t base = 3 * (size_t)first;
    if (VEC && count == NA_PER_LANE) {
        float4* po = reinterpret_cast<float4*>(rays_o + base);
        float4* pd = reinterpret_cast<float4*>(rays_d + base);
#pragma unroll
        for (int q = 0; q < 3; q++) {
            po[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
            pd[q] = make_float4(d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]);
        }
    } else {
        for (uint32_t e = 0; e < 3 * count; e++) { rays_o[base + e] = o[e]; rays_d[base + e] = d[e]; }
    }
}

__device__ __forceinline__ void na_sense(float v, uint32_t& u8, float& back) {
    const float c = fminf(fmaxf(v, 0.0f), 1.0f);                             // a NaN reads as 0
    u8 = (uint32_t)(uint8_t)(c * 255.0f);
    back = (float)((double)u8 / 255.0);
}

// lane: NA_PER_LANE consecutive channels of the flat [3 N] image
template <bool VEC>
__global__ __launch_bounds__(NA_THREADS) void k_agent_sensor(const float* __restrict__ image, uint64_t M, uint8_t* __restrict__ png, float* __restrict__ target) {
    const uint64_t first = ((uint64_t)blockIdx.x * NA_THREADS + threadIdx.x) * NA_PER_LANE;
    if (first >= M) return;
    if (VEC && M - first >= NA_PER_LANE) {
        const float4 v = *reinterpret_cast<const float4*>(image + first);
        uint32_t q[4];
        float4 t;
        na_sense(v.x, q[0], t.x); na_sense(v.y, q[1], t.y); na_sense(v.z, q[2], t.z); na_sense(v.w, q[3], t.w);
        *reinterpret_cast<uint32_t*>(png + first) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
        *reinterpret_cast<float4*>(target + first) = t;
        return;
    }
    const uint64_t last = M - first < NA_PER_LANE ? M : first + NA_PER_LANE;
    for (uint64_t e = first; e < last; e++) {
        uint32_t q;
        float t;
        na_sense(image[e], q, t);
        png[e] = (uint8_t)q;
        target[e] = t;
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

static inline bool na_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

extern "C" int ngp_agent_step(const ngp_filter_dyn_t* dyn, const float* state, const float* action, const float* noise, float* next_state,
                              float* blender_pose, float* body_pose, void* stream) {
    NGP_REQUIRE(dyn, "agent_step: null cfg");
    NGP_REQUIRE(state && action && next_state, "agent_step: null state / action / next_state");
    nfs_dyn D;
    const int bad = nfs_dyn_prepare(dyn->dt, dyn->mass, dyn->g, dyn->I, D);
    NGP_REQUIRE(bad != 1, "agent_step: dt = %g, mass = %g; both must be finite and > 0", (double)dyn->dt, (double)dyn->mass);
    NGP_REQUIRE(bad != 2, "agent_step: the inertia matrix I is singular or not finite");
    hipLaunchKernelGGL(k_agent_step, dim3(1), dim3(64), 0, (hipStream_t)stream, D, state, action, noise, next_state, blender_pose, body_pose);
    NGP_CHECK_LAUNCH("agent_step");
    return NGP_OK;
}

extern "C" int ngp_agent_rays(const ngp_filter_cfg_t* c, const float* state, float* rays_o, float* rays_d, void* stream) {
    NGP_REQUIRE(c, "agent_rays: null cfg");
    NGP_REQUIRE(c->H >= 1 && c->W >= 1 && (uint64_t)c->H * c->W <= 0x7FFFFFFFull, "agent_rays: bad image size %u x %u", c->H, c->W);
    NGP_REQUIRE(state && rays_o && rays_d, "agent_rays: null pointer");
    ngp_camera view = {};
    view.fx = c->intrinsics[0]; view.fy = c->intrinsics[1]; view.cx = c->intrinsics[2]; view.cy = c->intrinsics[3]; view.W = c->W; view.H = c->H;
    const uint32_t N = c->H * c->W, blocks = ngp_div_up(N, NA_THREADS * NA_PER_LANE);
    if (na_aligned(rays_o, 16) && na_aligned(rays_d, 16))
        hipLaunchKernelGGL(k_agent_rays<true>, dim3(blocks), dim3(NA_THREADS), 0, (hipStream_t)stream, view, state, N, rays_o, rays_d);
    else
        hipLaunchKernelGGL(k_agent_rays<false>, dim3(blocks), dim3(NA_THREADS), 0, (hipStream_t)stream, view, state, N, rays_o, rays_d);
    NGP_CHECK_LAUNCH("agent_rays");
    return NGP_OK;
}

extern "C" int ngp_agent_sensor(const float* image, uint8_t* png, float* target, uint32_t N, void* stream) {
    NGP_REQUIRE(image && png && target, "agent_sensor: null image / png / target");
    if (N == 0) return NGP_OK;
    const uint64_t M = 3 * (uint64_t)N;
    const uint32_t blocks = ngp_div_up(M, NA_THREADS * NA_PER_LANE);
    if (na_aligned(image, 16) && na_aligned(target, 16) && na_aligned(png, 4))
        hipLaunchKernelGGL(k_agent_sensor<true>, dim3(blocks), dim3(NA_THREADS), 0, (hipStream_t)stream, image, M, png, target);
    else
        hipLaunchKernelGGL(k_agent_sensor<false>, dim3(blocks), dim3(NA_THREADS), 0, (hipStream_t)stream, image, M, png, target);
    NGP_CHECK_LAUNCH("agent_sensor");
    return NGP_OK;
}
