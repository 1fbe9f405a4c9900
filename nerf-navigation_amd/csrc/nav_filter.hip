// nav_filter.hip -- the pose filter's optimisation loop on the device (DESIGN.md §3.5 "Native pose filter"): Estimator.estimate_relative_pose's
// iteration (nav/estimator_helpers.py:227-241) = measurement_fn (:293-327) -> backward -> Adam as five launches with no host synchronisation.
//
//   k_filter_rays     state [12] -> camera pose (measurement_fn's chain, :301-309) -> the batch's rays_o, rays_d (ngp_camera.h) and nears, fars
//   ngp_nav_run_forward  (nav_field.hip, unchanged) with the per-sample record kept
//   k_filter_loss     grad_image = 2 (rgb - target[row, col]) / (3 B), one partial sum of the squared error per workgroup
//   ngp_nav_run_backward (nav_field.hip, unchanged): grad_rays_o, grad_rays_d
//   k_filter_step     one workgroup: sum grad_rays_o, sum grad_rays_d (x) dir (= dL/dP, since rays_d = P dir) and the loss partials; one thread chains them
//                     back through the axis matrices and the Rodrigues formula; the Mahalanobis term; the records; torch.optim.Adam's step.
//
// Shared: the sums, the chain back to the state, the Mahalanobis row and the loss are nf_ray_sums .. nf_loss below, one copy for k_filter_step and
// k_filter_hessian; nf_begin and nf_measure are the host side the two loop entry points have in common; the Adam step and the wave sum are the
// planner's too (ngp_nav_step.h: ngp_adam_step, ngp_wave_sum); the axis matrices and the 3 x 3 product are ngp_filter_step.h's, at T = float.
//
// Multi-start (DESIGN.md §3.5 "Multi-start pose filter"): K hypotheses of B rays as ONE sequence of five launches over K B rays.  k_filter_rays_multi,
// k_filter_loss_multi and k_filter_step_multi give hypothesis k (blockIdx.y, or blockIdx.x of the step) the slice [k B, (k + 1) B) of every per-ray buffer
// and run the bodies the single kernels run (nf_ray_of, nf_squared_error, nf_step), so row k is the single run from the same start bit for bit.
//
// Occupied sampling (DESIGN.md §3.5 "Occupancy-masked pose filter"): nf_measure takes the renderer's occupancy grid as an optional argument and then renders
// and differentiates through ngp_nav_run_occ_forward / _backward (nav_field.hip); ngp_filter_iterations_occ and ngp_filter_hessian_occ are the entry points
// that pass one.  The entry points without a grid keep their code path.
//
// Resampled sampling (DESIGN.md §3.5 "Resampled run"): nf_measure takes an optional nf_res (upsample_steps and the caller's depth list) and then queues
// ngp_nav_run_resample after the rays and renders and differentiates through ngp_nav_run_at_forward / _backward over that list: six launches per iteration.
// ngp_filter_iterations_res and ngp_filter_hessian_res are the entry points that pass one; the workspace is the dense layout at num_steps + upsample_steps.
//
// The derivative conventions are torch autograd's of the formula as written (nav/math_utils.py:159-174): R = I + sin(a) K + ((1 - cos(a)) K) K,
// K = hat(r / (1e-10 + a)), a = |r|, with the denominator's dependence on a kept and a zero subgradient of the norm at r = 0.  No gradient flows through
// near / far (nerf/renderer.py:140-141).  No atomics; every sum runs in a fixed order, so two runs are bit-identical.
#include "ngp_nav_step.h"
#include "ngp_camera.h"
#include "ngp_filter_step.h"
#include "ngp_filter_pose.h"                                                 // NF_C90, nf_rodrigues, nf_rotation, nf_pose: shared with nav_agent.hip
#include "ngp_select.h"                                                      // ngp_select_best: the selection rule, shared with nav_plan.hip

static constexpr uint32_t NF_THREADS = 256, NF_WAVES = NF_THREADS / 64;
static constexpr uint32_t NF_MAX_B = 1u << 20, NF_MAX_T = 4096;             // num_steps: what ngp_nav_run_forward accepts
static constexpr uint32_t NF_SUMS = 13;                                      // grad_rays_o [3], dL/dP [9], squared error
enum : uint32_t { NF_M = 0, NF_V = 12, NF_G = 24, NF_STEP = 36 };            // adam_state (NGP_FILTER_ADAM_FLOATS)
static_assert(NGP_FILTER_ADAM_FLOATS == NF_STEP + 1, "adam_state layout");

struct nf_view { float fx, fy, cx, cy; uint32_t W, H; float aabb[6]; float min_near; };
struct nf_step_args {
    float start[12], sig_inv[144];
    ngp_adam_coef adam;                                                      // zeroed where no step is taken (ngp_filter_hessian)
};

// the backward of nf_pose's rotation part: GP = dL/dP -> dL/d state[6:9]
__device__ __forceinline__ void nf_pose_backward(const float* r, const nf_rodrigues& Q, const float* GP, float* gr) {
    float GRb[9], GR[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int m = (i + 1) % 3;
        GRb[m * 3 + 0] = GP[i * 3 + 0]; GRb[m * 3 + 1] = -GP[i * 3 + 1]; GRb[m * 3 + 2] = -GP[i * 3 + 2];
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {                                            // rot_x(pi/2)^T
        GR[0 + j] = GRb[0 + j];
        GR[3 + j] = NF_C90 * GRb[3 + j] + GRb[6 + j];
        GR[6 + j] = NF_C90 * GRb[6 + j] - GRb[3 + j];
    }
    // R = I + sn K + M K, M = (1 - cs) K
    float Kt[9], Mt[9], GM[9], GK[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { Kt[i * 3 + j] = Q.K[j * 3 + i]; Mt[i * 3 + j] = Q.M[j * 3 + i]; }
    nfs_matmul3(GR, Kt, GM);
    nfs_matmul3(Mt, GR, GK);
    const float omc = 1.0f - Q.cs;
    float g_sn = 0.0f, g_omc = 0.0f;
#pragma unroll
    for (int e = 0; e < 9; e++) {
        g_sn += GR[e] * Q.K[e];
        g_omc += GM[e] * Q.K[e];
        GK[e] = (GK[e] + Q.sn * GR[e]) + omc * GM[e];
    }
    float g_a = Q.cs * g_sn + Q.sn * g_omc;
    const float gk[3] = {GK[7] - GK[5], GK[2] - GK[6], GK[3] - GK[1]};        // hat
    // k = r / d, d = 1e-10 + a: the quotient's two branches; d depends on a
    float g_d = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        gr[i] = gk[i] / Q.d;
        g_d += -gk[i] * r[i] / (Q.d * Q.d);
    }
    g_a += g_d;
    if (Q.a > 0.0f) {                                                        // torch's subgradient of the norm at zero is zero
#pragma unroll
        for (int i = 0; i < 3; i++) gr[i] += g_a * (r[i] / Q.a);
    }
}

// the (row, col) pair of ray n, clamped into the image: the caller checks the pairs, the kernels must not read outside `target`
__device__ __forceinline__ void nf_pixel(const int32_t* __restrict__ batch, uint32_t n, uint32_t H, uint32_t W, uint32_t& row, uint32_t& col) {
    const int32_t r = batch[2 * (size_t)n], c = batch[2 * (size_t)n + 1];
    row = (uint32_t)(r < 0 ? 0 : r >= (int32_t)H ? (int32_t)H - 1 : r);
    col = (uint32_t)(c < 0 ? 0 : c >= (int32_t)W ? (int32_t)W - 1 : c);
}

// ---------------------------------------------------------------------------
// what k_filter_step and k_filter_hessian have in common: one workgroup's LDS and the passes over it.  Every sum is written once, here, so the gradient,
// the loss and dL/dP of the Hessian call are an update = 0 iteration's bit for bit
// ---------------------------------------------------------------------------

struct nf_shared { float sums[NF_WAVES][NF_SUMS], x[12], delta[12], g_image[12], quad[12], mse; };

__device__ __forceinline__ void nf_load_state(nf_shared& S, const nf_step_args& A, const float* __restrict__ state) {
    const uint32_t tid = threadIdx.x;
    if (tid < 12) {
        const float s = state[tid];
        S.x[tid] = s;
        S.delta[tid] = s - A.start[tid];
    }
}

// per-lane sums over the rays (lanes strided over them) and the loss partials, then a fixed butterfly; lane 0 of each wave stores its 13 sums
__device__ __forceinline__ void nf_ray_sums(nf_shared& S, const nf_view& V, const int32_t* __restrict__ batch, uint32_t B,
                                            const float* __restrict__ grad_rays_o, const float* __restrict__ grad_rays_d,
                                            const float* __restrict__ partials, uint32_t n_partials) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    float acc[NF_SUMS];
#pragma unroll
    for (int k = 0; k < (int)NF_SUMS; k++) acc[k] = 0.0f;
    ngp_camera unit;                                                         // identity pose: ngp_camera_ray returns the pixel's unit direction
#pragma unroll
    for (int e = 0; e < 9; e++) unit.r[e] = e % 4 == 0 ? 1.0f : 0.0f;
    unit.t[0] = unit.t[1] = unit.t[2] = 0.0f;
    unit.fx = V.fx; unit.fy = V.fy; unit.cx = V.cx; unit.cy = V.cy; unit.W = V.W; unit.H = V.H;
    for (uint32_t n = tid; n < B; n += NF_THREADS) {
        uint32_t row, col;
        nf_pixel(batch, n, V.H, V.W, row, col);
        float dir[3];
        ngp_camera_ray(unit, row * V.W + col, dir);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            acc[k] += grad_rays_o[3 * (size_t)n + k];
            const float g = grad_rays_d[3 * (size_t)n + k];
#pragma unroll
            for (int j = 0; j < 3; j++) acc[3 + 3 * k + j] += g * dir[j];
        }
    }
    for (uint32_t i = tid; i < n_partials; i += NF_THREADS) acc[12] += partials[i];
#pragma unroll
    for (int k = 0; k < (int)NF_SUMS; k++) acc[k] = ngp_wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < (int)NF_SUMS; k++) S.sums[wave][k] = acc[k];
    }
}

// sum k of the whole workgroup: the waves in order
__device__ __forceinline__ float nf_total(const nf_shared& S, int k) {
    float s = S.sums[0][k];
#pragma unroll
    for (uint32_t w = 1; w < NF_WAVES; w++) s += S.sums[w][k];
    return s;
}

// one lane, after the barrier: the totals (left in tot: grad_rays_o [3], dL/dP [9], squared error), dL/dP chained back to the state, mse
__device__ __forceinline__ void nf_image_gradient(nf_shared& S, uint32_t B, float* tot) {
#pragma unroll
    for (int k = 0; k < (int)NF_SUMS; k++) tot[k] = nf_total(S, k);
    float xs[12];
#pragma unroll
    for (int k = 0; k < 12; k++) { xs[k] = S.x[k]; S.g_image[k] = 0.0f; }
    nf_rodrigues Q;
    float P[9], T[3], gr[3];
    nf_pose(xs, Q, P, T);
    nf_pose_backward(xs + 6, Q, tot + 3, gr);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        S.g_image[(i + 1) % 3] = tot[i];                                    // T[i] = position[(i + 1) % 3]
        S.g_image[6 + i] = gr[i];
    }
    S.mse = tot[12] / (float)(3ull * B);
}

// lanes 0-11, Mahalanobis: row tid of delta^T Sinv delta into quad, and (returned) of its gradient (Sinv + Sinv^T) delta; float64 sums
__device__ __forceinline__ double nf_process_row(nf_shared& S, const nf_step_args& A) {
    const uint32_t tid = threadIdx.x;
    double mg = 0.0;
    if (tid < 12) {
        double row = 0.0;
#pragma unroll
        for (int j = 0; j < 12; j++) {
            const double dj = (double)S.delta[j];
            row += (double)A.sig_inv[tid * 12 + j] * dj;
            mg += ((double)A.sig_inv[tid * 12 + j] + (double)A.sig_inv[j * 12 + tid]) * dj;
        }
        S.quad[tid] = (float)((double)S.delta[tid] * row);
    }
    return mg;
}

__device__ __forceinline__ float nf_loss(const nf_shared& S) {
    float process = S.quad[0];
#pragma unroll
    for (int k = 1; k < 12; k++) process += S.quad[k];
    return S.mse + process;
}

// ---------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------

// ray n of the batch from `state`: the body of k_filter_rays and k_filter_rays_multi (the pointers are the hypothesis' own slices)
__device__ __forceinline__ void nf_ray_of(const nf_view& V, const float* __restrict__ state, const int32_t* __restrict__ batch, uint32_t n,
                                          float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ nears, float* __restrict__ fars) {
    float x[12];
#pragma unroll
    for (int k = 0; k < 12; k++) x[k] = state[k];
    nf_rodrigues Q;
    ngp_camera cam;
    nf_pose(x, Q, cam.r, cam.t);
    cam.fx = V.fx; cam.fy = V.fy; cam.cx = V.cx; cam.cy = V.cy; cam.W = V.W; cam.H = V.H;
    uint32_t row, col;
    nf_pixel(batch, n, V.H, V.W, row, col);
    float d[3];
    ngp_camera_ray(cam, row * V.W + col, d);
    float near, far;
    ngp_near_far_inline(cam.t, d, V.aabb, V.min_near, near, far);
#pragma unroll
    for (int k = 0; k < 3; k++) { rays_o[3 * (size_t)n + k] = cam.t[k]; rays_d[3 * (size_t)n + k] = d[k]; }
    nears[n] = near; fars[n] = far;
}

__global__ __launch_bounds__(NF_THREADS) void k_filter_rays(nf_view V, const float* __restrict__ state, const int32_t* __restrict__ batch, uint32_t B,
                                                            float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ nears,
                                                            float* __restrict__ fars) {
    const uint32_t n = blockIdx.x * NF_THREADS + threadIdx.x;
    if (n >= B) return;
    nf_ray_of(V, state, batch, n, rays_o, rays_d, nears, fars);
}

// grid (ceil(B / 256), K): hypothesis k = blockIdx.y writes rays [k B, (k + 1) B) from states[k]; the batch is shared
__global__ __launch_bounds__(NF_THREADS) void k_filter_rays_multi(nf_view V, const float* __restrict__ states, const int32_t* __restrict__ batch, uint32_t B,
                                                                  float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ nears,
                                                                  float* __restrict__ fars) {
    const uint32_t n = blockIdx.x * NF_THREADS + threadIdx.x;
    if (n >= B) return;
    const size_t first = (size_t)blockIdx.y * B;
    nf_ray_of(V, states + 12 * (size_t)blockIdx.y, batch, n, rays_o + 3 * first, rays_d + 3 * first, nears + first, fars + first);
}

// one workgroup's 256 rays of a batch of B: grad_image = 2 (rgb - target) / (3 B) and the workgroup's sum of the squared error into *partial; the body of
// k_filter_loss and k_filter_loss_multi (image and grad_image are the hypothesis' own slices, B is ITS ray count: mse_loss's mean is per hypothesis)
__device__ __forceinline__ void nf_squared_error(float* wave_sums, const float* __restrict__ image, const float* __restrict__ target,
                                                 const int32_t* __restrict__ batch, uint32_t B, uint32_t H, uint32_t W, float* __restrict__ grad_image,
                                                 float* __restrict__ partial) {
    const uint32_t n = blockIdx.x * NF_THREADS + threadIdx.x;
    float sq = 0.0f;
    if (n < B) {
        uint32_t row, col;
        nf_pixel(batch, n, H, W, row, col);
        const float* t = target + 3 * ((size_t)row * W + col);
        const float count = (float)(3ull * B);                               // mse_loss's mean over B x 3 entries
        float e[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            e[k] = image[3 * (size_t)n + k] - t[k];
            grad_image[3 * (size_t)n + k] = (2.0f * e[k]) / count;
        }
        sq = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    }
    sq = ngp_wave_sum(sq);
    if ((threadIdx.x & 63u) == 0) wave_sums[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = wave_sums[0];
#pragma unroll
        for (uint32_t w = 1; w < NF_WAVES; w++) s += wave_sums[w];
        *partial = s;
    }
}

__global__ __launch_bounds__(NF_THREADS) void k_filter_loss(const float* __restrict__ image, const float* __restrict__ target,
                                                            const int32_t* __restrict__ batch, uint32_t B, uint32_t H, uint32_t W,
                                                            float* __restrict__ grad_image, float* __restrict__ partials) {
    __shared__ float wave_sums[NF_WAVES];
    nf_squared_error(wave_sums, image, target, batch, B, H, W, grad_image, partials + blockIdx.x);
}

// grid (ceil(B / 256), K): hypothesis k = blockIdx.y takes image rows [k B, (k + 1) B) and writes partials[k gridDim.x + blockIdx.x]
__global__ __launch_bounds__(NF_THREADS) void k_filter_loss_multi(const float* __restrict__ image, const float* __restrict__ target,
                                                                  const int32_t* __restrict__ batch, uint32_t B, uint32_t H, uint32_t W,
                                                                  float* __restrict__ grad_image, float* __restrict__ partials) {
    __shared__ float wave_sums[NF_WAVES];
    const size_t first = 3 * (size_t)blockIdx.y * B;
    nf_squared_error(wave_sums, image + first, target, batch, B, H, W, grad_image + first, partials + (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// one workgroup, one hypothesis: the passes over its rays, gradients and partials, the records and the Adam step; the body of k_filter_step and
// k_filter_step_multi
__device__ __forceinline__ void nf_step(nf_shared& S, const nf_view& V, const nf_step_args& A, int update, float* __restrict__ state, float* __restrict__ adam,
                                        const int32_t* __restrict__ batch, uint32_t B, const float* __restrict__ grad_rays_o,
                                        const float* __restrict__ grad_rays_d, const float* __restrict__ partials, uint32_t n_partials,
                                        float* __restrict__ loss_out, float* __restrict__ state_out, float* __restrict__ grad_out) {
    const uint32_t tid = threadIdx.x;
    const float step = adam[NF_STEP] + 1.0f;                                 // read before any lane writes it (there are barriers in between)
    nf_load_state(S, A, state);
    nf_ray_sums(S, V, batch, B, grad_rays_o, grad_rays_d, partials, n_partials);
    __syncthreads();
    if (tid == 0) {
        float tot[NF_SUMS];
        nf_image_gradient(S, B, tot);
    }
    const double mg = nf_process_row(S, A);
    __syncthreads();
    if (tid < 12) {
        const float g = S.g_image[tid] + (float)mg;
        const float s = S.x[tid];
        adam[NF_G + tid] = g;
        if (grad_out) grad_out[tid] = g;
        if (state_out) state_out[tid] = s;
        if (update) {                                                        // bc1, bc2 = beta^step are the same for the 12 entries
            float m = adam[NF_M + tid], v = adam[NF_V + tid];
            state[tid] = ngp_adam_step(A.adam, s, g, &m, &v, step);
            adam[NF_M + tid] = m;
            adam[NF_V + tid] = v;
        }
    }
    if (tid == 0) {
        if (loss_out) *loss_out = nf_loss(S);
        if (update) adam[NF_STEP] = step;
    }
}

__global__ __launch_bounds__(NF_THREADS) void k_filter_step(nf_view V, nf_step_args A, int update, float* __restrict__ state, float* __restrict__ adam,
                                                            const int32_t* __restrict__ batch, uint32_t B, const float* __restrict__ grad_rays_o,
                                                            const float* __restrict__ grad_rays_d, const float* __restrict__ partials,
                                                            uint32_t n_partials, float* __restrict__ loss_out, float* __restrict__ state_out,
                                                            float* __restrict__ grad_out) {
    __shared__ nf_shared S;
    nf_step(S, V, A, update, state, adam, batch, B, grad_rays_o, grad_rays_d, partials, n_partials, loss_out, state_out, grad_out);
}

// K workgroups: workgroup k steps states[k] and adam_states[k] from rays [k B, (k + 1) B) and partials [k n_partials, (k + 1) n_partials); the records of
// one iteration are [K] and [K,12]
__global__ __launch_bounds__(NF_THREADS) void k_filter_step_multi(nf_view V, nf_step_args A, int update, float* __restrict__ states, float* __restrict__ adam_states,
                                                                  const int32_t* __restrict__ batch, uint32_t B, const float* __restrict__ grad_rays_o,
                                                                  const float* __restrict__ grad_rays_d, const float* __restrict__ partials,
                                                                  uint32_t n_partials, float* __restrict__ loss_out, float* __restrict__ state_out,
                                                                  float* __restrict__ grad_out) {
    __shared__ nf_shared S;
    const size_t k = blockIdx.x, first = 3 * k * B;
    nf_step(S, V, A, update, states + 12 * k, adam_states + NGP_FILTER_ADAM_FLOATS * k, batch, B, grad_rays_o + first, grad_rays_d + first,
            partials + k * n_partials, n_partials, loss_out ? loss_out + k : nullptr, state_out ? state_out + 12 * k : nullptr,
            grad_out ? grad_out + 12 * k : nullptr);
}

// one wave: every lane scans the K losses (K <= 64) by the rule of ngp_select.h, lanes 0-11 copy the winner's state, lane 0 its loss and index
__global__ __launch_bounds__(64) void k_filter_select(const float* __restrict__ losses, const float* __restrict__ states, uint32_t K,
                                                      float* __restrict__ best_state, float* __restrict__ best_loss, uint32_t* __restrict__ best_index) {
    const uint32_t best = ngp_select_best(losses, K);
    if (threadIdx.x < 12) best_state[threadIdx.x] = states[12 * (size_t)best + threadIdx.x];
    if (threadIdx.x == 0) { *best_loss = losses[best]; *best_index = best; }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------

struct nf_ws {
    float *rays_o, *rays_d, *nears, *fars, *image, *depth, *weights_sum, *grad_image;
    unsigned char* saved;
    float *grad_rays_o, *grad_rays_d, *partials;
    size_t saved_bytes, total;
};
// K hypotheses of B rays: every per-ray piece holds K B rays, hypothesis k in [k B, (k + 1) B), and the partials K slices of ceil(B / 256).  The pieces
// and their order are one statement for both entry points' workspaces; K = 1 is the single loop's
// occ: the record is the occupancy-masked run's (ngp_nav_run_occ_saved_bytes: the same records plus each ray's count and list); every other piece is unchanged
static nf_ws nf_multi_layout(uint32_t K, uint32_t B, uint32_t num_steps, void* base, bool occ = false) {
    if (K < 1 || K > NGP_FILTER_MULTI_MAX_K || B < 1 || (uint64_t)K * B > NF_MAX_B || num_steps < 1 || num_steps > NF_MAX_T) return {};   // total 0: a shape no filter call accepts
    const size_t n = (size_t)K * B, kept = occ ? ngp_nav_run_occ_saved_bytes(K * B, num_steps) : ngp_nav_run_saved_bytes(K * B, num_steps);
    ngp_carver c(base);
    return {c.take<float>(3 * n), c.take<float>(3 * n), c.take<float>(n), c.take<float>(n), c.take<float>(3 * n), c.take<float>(n), c.take<float>(n),
            c.take<float>(3 * n), c.take<unsigned char>(kept), c.take<float>(3 * n), c.take<float>(3 * n),
            c.take<float>((size_t)K * ngp_div_up(B, NF_THREADS)), kept, c.total(256)};
}
static nf_ws nf_layout(uint32_t B, uint32_t num_steps, void* base) { return nf_multi_layout(1, B, num_steps, base); }
extern "C" size_t ngp_filter_workspace(uint32_t B, uint32_t num_steps) { return nf_layout(B, num_steps, nullptr).total; }
extern "C" size_t ngp_filter_multi_workspace(uint32_t K, uint32_t B, uint32_t num_steps) { return nf_multi_layout(K, B, num_steps, nullptr).total; }
extern "C" size_t ngp_filter_occ_workspace(uint32_t K, uint32_t B, uint32_t num_steps) { return nf_multi_layout(K, B, num_steps, nullptr, true).total; }

static int nf_view_of(const char* who, const ngp_filter_cfg_t* c, nf_view& V) {
    NGP_REQUIRE(c, "%s: null cfg", who);
    NGP_REQUIRE(c->B >= 1 && c->B <= NF_MAX_B, "%s: B = %u rays per iteration; supported 1 <= B <= 2^20", who, c->B);
    NGP_REQUIRE(c->H >= 1 && c->W >= 1 && (uint64_t)c->H * c->W <= 0x7FFFFFFFull, "%s: bad image size %u x %u", who, c->H, c->W);
    V.fx = c->intrinsics[0]; V.fy = c->intrinsics[1]; V.cx = c->intrinsics[2]; V.cy = c->intrinsics[3]; V.W = c->W; V.H = c->H;
    for (int k = 0; k < 6; k++) V.aabb[k] = c->aabb[k];
    V.min_near = c->min_near;
    return NGP_OK;
}

extern "C" int ngp_filter_rays(const ngp_filter_cfg_t* c, const float* state, const int32_t* batch, float* rays_o, float* rays_d, float* nears,
                               float* fars, void* stream) {
    nf_view V;
    const int rc = nf_view_of("filter_rays", c, V);
    if (rc != NGP_OK) return rc;
    NGP_REQUIRE(state && batch && rays_o && rays_d && nears && fars, "filter_rays: null pointer");
    hipLaunchKernelGGL(k_filter_rays, dim3(ngp_div_up(c->B, NF_THREADS)), dim3(NF_THREADS), 0, (hipStream_t)stream, V, state, batch, c->B, rays_o, rays_d,
                       nears, fars);
    NGP_CHECK_LAUNCH("filter_rays");
    return NGP_OK;
}

// the resampled route (DESIGN.md §3.5 "Resampled run"): upsample_steps and the caller's depth list [rays, num_steps + Nf]
struct nf_res { uint32_t Nf; float* z; };

// what the two entry points of the loop do before they queue anything, in this order: the view, the shape, the entry point's own null-pointer refusal
// (`null_refusal`: its message, or NULL where every pointer is there), the workspace, the field (N = 0 validates and launches nothing), and the
// start state and inverse covariance the last kernel takes as arguments (A.adam is left zeroed).  K hypotheses (1: the single loop and the Hessian) size
// the workspace, whose size function `ws_fn` names.  grid: null for the dense run; else the occupancy-masked run's grid, judged with the field
// res: null, or the resampled route: its shape, z and the field are judged by ngp_nav_run_resample with no rays, and the workspace holds num_steps + Nf samples per ray
static int nf_begin(const char* who, const char* null_refusal, const ngp_nav_field_t* field, const void* prepared, const ngp_filter_cfg_t* c, uint32_t K,
                    const char* ws_fn, void* workspace, size_t workspace_bytes, void* stream, nf_view& V, nf_ws& w, nf_step_args& A,
                    const ngp_occ_grid_t* grid = nullptr, const nf_res* res = nullptr) {
    const int rc_v = nf_view_of(who, c, V);
    if (rc_v != NGP_OK) return rc_v;
    NGP_REQUIRE(c->num_steps >= 1 && c->num_steps <= NF_MAX_T, "%s: num_steps = %u; supported 1 <= num_steps <= 4096", who, c->num_steps);
    NGP_REQUIRE(!null_refusal, "%s", null_refusal);
    if (res) {                                                               // the resampled run's own refusals (shape, z, the field): N = 0 queues nothing
        const int rc_r = ngp_nav_run_resample(field, prepared, nullptr, nullptr, nullptr, nullptr, 0, c->num_steps, res->Nf, c->aabb, res->z, nullptr, stream);
        if (rc_r != NGP_OK) return rc_r;
    }
    const uint32_t T = c->num_steps + (res ? res->Nf : 0u);                  // samples per ray of the differentiated run
    w = nf_multi_layout(K, c->B, T, workspace, grid != nullptr);
    if (!workspace || workspace_bytes < w.total)
        return ngp_fail(NGP_EWORKSPACE, "%s: workspace of %zu bytes, needs %s = %zu", who, workspace_bytes, ws_fn, w.total);
    const int rc_f = grid ? ngp_nav_run_occ_forward(field, prepared, grid, w.rays_o, w.rays_d, w.nears, w.fars, 0, T, c->aabb, c->bg, w.image, w.depth,
                                                    w.weights_sum, nullptr, w.saved, w.saved_bytes, stream)
                          : ngp_nav_run_forward(field, prepared, w.rays_o, w.rays_d, w.nears, w.fars, 0, T, c->aabb, c->bg, w.image, w.depth, w.weights_sum, w.saved,
                                                w.saved_bytes, stream);
    if (rc_f != NGP_OK) return rc_f;
    A = {};
    for (int k = 0; k < 12; k++) A.start[k] = c->start_state[k];
    for (int k = 0; k < 144; k++) A.sig_inv[k] = c->sig_inv[k];
    return NGP_OK;
}

static int nf_launched(const char* who, const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? NGP_OK : ngp_fail(NGP_ELAUNCH, "%s: %s: %s", who, what, hipGetErrorString(e));
}

// the measurement pass at `state` for one batch: rays -> run forward -> loss -> run backward, queued; leaves grad_rays_o, grad_rays_d and the loss partials in w.
// K = 0: one state, the single kernels; K >= 1: `state` is [K,12] and the multi kernels fill K slices, with the run kernels launched once over K B rays.
// grid: null = the dense run; else the occupancy-masked pair renders and differentiates (w laid out with occ)
// res: null, or the resampled route: ngp_nav_run_resample fills res->z after the rays, and the run over that list renders and differentiates
static int nf_measure(const char* who, const ngp_nav_field_t* field, const void* prepared, const ngp_filter_cfg_t* c, const nf_view& V, const nf_ws& w,
                      uint32_t K, const float* state, const float* target, const int32_t* batch, void* stream, const ngp_occ_grid_t* grid = nullptr,
                      const nf_res* res = nullptr) {
    const uint32_t B = c->B, T = c->num_steps + (res ? res->Nf : 0u), blocks = ngp_div_up(B, NF_THREADS), N = (K ? K : 1u) * B;
    hipStream_t s = (hipStream_t)stream;
    if (K) hipLaunchKernelGGL(k_filter_rays_multi, dim3(blocks, K), dim3(NF_THREADS), 0, s, V, state, batch, B, w.rays_o, w.rays_d, w.nears, w.fars);
    else hipLaunchKernelGGL(k_filter_rays, dim3(blocks), dim3(NF_THREADS), 0, s, V, state, batch, B, w.rays_o, w.rays_d, w.nears, w.fars);
    int rc = nf_launched(who, "rays");
    if (rc != NGP_OK) return rc;
    if (res) {                                                               // the sixth launch: this iteration's depth lists
        rc = ngp_nav_run_resample(field, prepared, w.rays_o, w.rays_d, w.nears, w.fars, N, c->num_steps, res->Nf, c->aabb, res->z, nullptr, stream);
        if (rc != NGP_OK) return rc;
    }
    rc = res  ? ngp_nav_run_at_forward(field, prepared, w.rays_o, w.rays_d, w.nears, w.fars, N, T, c->aabb, c->bg, w.image, w.depth, w.weights_sum, w.saved,
                                       w.saved_bytes, res->z, c->num_steps, stream)
       : grid ? ngp_nav_run_occ_forward(field, prepared, grid, w.rays_o, w.rays_d, w.nears, w.fars, N, T, c->aabb, c->bg, w.image, w.depth, w.weights_sum,
                                        nullptr, w.saved, w.saved_bytes, stream)
              : ngp_nav_run_forward(field, prepared, w.rays_o, w.rays_d, w.nears, w.fars, N, T, c->aabb, c->bg, w.image, w.depth, w.weights_sum, w.saved,
                                    w.saved_bytes, stream);
    if (rc != NGP_OK) return rc;
    if (K) hipLaunchKernelGGL(k_filter_loss_multi, dim3(blocks, K), dim3(NF_THREADS), 0, s, (const float*)w.image, target, batch, B, c->H, c->W, w.grad_image, w.partials);
    else hipLaunchKernelGGL(k_filter_loss, dim3(blocks), dim3(NF_THREADS), 0, s, (const float*)w.image, target, batch, B, c->H, c->W, w.grad_image, w.partials);
    rc = nf_launched(who, "loss");
    if (rc != NGP_OK) return rc;
    if (res)
        return ngp_nav_run_at_backward(field, prepared, w.rays_o, w.rays_d, w.nears, w.fars, N, T, c->aabb, c->bg, w.grad_image, nullptr, nullptr, w.saved,
                                       w.saved_bytes, w.grad_rays_o, w.grad_rays_d, res->z, c->num_steps, stream);
    if (grid)
        return ngp_nav_run_occ_backward(field, prepared, grid, w.rays_o, w.rays_d, w.nears, w.fars, N, T, c->aabb, c->bg, w.grad_image, nullptr, nullptr,
                                        w.saved, w.saved_bytes, w.grad_rays_o, w.grad_rays_d, stream);
    return ngp_nav_run_backward(field, prepared, w.rays_o, w.rays_d, w.nears, w.fars, N, T, c->aabb, c->bg, w.grad_image, nullptr, nullptr, w.saved,
                                w.saved_bytes, w.grad_rays_o, w.grad_rays_d, stream);
}

extern "C" int ngp_filter_iterations(const ngp_nav_field_t* field, const void* prepared, const ngp_filter_cfg_t* c, float* state, float* adam_state,
                                     const float* target, const int32_t* batches, uint32_t first_iter, uint32_t n_iter, int update, float* losses,
                                     float* states_out, float* grads_out, void* workspace, size_t workspace_bytes, void* stream) {
    nf_view V;
    nf_ws w;
    nf_step_args A;
    int rc = nf_begin("filter_iterations", state && adam_state && target && batches ? nullptr : "filter_iterations: null state / adam_state / target / batches",
                      field, prepared, c, 1, "ngp_filter_workspace(B, num_steps)", workspace, workspace_bytes, stream, V, w, A);
    if (rc != NGP_OK) return rc;
    A.adam = ngp_adam_fill(c->lr, c->beta1, c->beta2, c->eps);
    const uint32_t B = c->B, blocks = ngp_div_up(B, NF_THREADS);
    for (uint32_t k = 0; k < n_iter; k++) {
        const int32_t* batch = batches + 2 * (size_t)B * ((size_t)first_iter + k);
        rc = nf_measure("filter_iterations", field, prepared, c, V, w, 0, state, target, batch, stream);
        if (rc != NGP_OK) return rc;
        hipLaunchKernelGGL(k_filter_step, dim3(1), dim3(NF_THREADS), 0, (hipStream_t)stream, V, A, update, state, adam_state, batch, B,
                           (const float*)w.grad_rays_o, (const float*)w.grad_rays_d, (const float*)w.partials, blocks, losses ? losses + k : (float*)nullptr,
                           states_out ? states_out + 12 * (size_t)k : (float*)nullptr, grads_out ? grads_out + 12 * (size_t)k : (float*)nullptr);
        NGP_CHECK_LAUNCH("filter_iterations: step");
    }
    return NGP_OK;
}

// the K-hypothesis loop: ngp_filter_iterations_multi (grid null) and ngp_filter_iterations_occ (the grid given); `who` names the entry point in every
// refusal, `null_refusal` and `ws_fn` are its own words
static int nf_iterations_multi(const char* who, const char* null_refusal, const char* ws_fn, const ngp_nav_field_t* field, const void* prepared,
                               const ngp_filter_cfg_t* c, const ngp_occ_grid_t* grid, uint32_t K, float* states, float* adam_states, const float* target,
                               const int32_t* batches, uint32_t first_iter, uint32_t n_iter, int update, float* losses, float* states_out, float* grads_out,
                               void* workspace, size_t workspace_bytes, void* stream, const nf_res* res = nullptr) {
    NGP_REQUIRE(K >= 1 && K <= NGP_FILTER_MULTI_MAX_K, "%s: K = %u hypotheses; supported 1 <= K <= %u", who, K, NGP_FILTER_MULTI_MAX_K);
    NGP_REQUIRE(!c || c->B > NF_MAX_B || (uint64_t)K * c->B <= NF_MAX_B, "%s: K * B = %u * %u rays per iteration; supported K * B <= 2^20", who,
                K, c ? c->B : 0u);
    nf_view V;
    nf_ws w;
    nf_step_args A;
    int rc = nf_begin(who, states && adam_states && target && batches ? nullptr : null_refusal, field, prepared, c, K, ws_fn, workspace, workspace_bytes,
                      stream, V, w, A, grid, res);
    if (rc != NGP_OK) return rc;
    A.adam = ngp_adam_fill(c->lr, c->beta1, c->beta2, c->eps);
    const uint32_t B = c->B, blocks = ngp_div_up(B, NF_THREADS);
    for (uint32_t k = 0; k < n_iter; k++) {
        const int32_t* batch = batches + 2 * (size_t)B * ((size_t)first_iter + k);
        rc = nf_measure(who, field, prepared, c, V, w, K, states, target, batch, stream, grid, res);
        if (rc != NGP_OK) return rc;
        const size_t row = (size_t)k * K;
        hipLaunchKernelGGL(k_filter_step_multi, dim3(K), dim3(NF_THREADS), 0, (hipStream_t)stream, V, A, update, states, adam_states, batch, B,
                           (const float*)w.grad_rays_o, (const float*)w.grad_rays_d, (const float*)w.partials, blocks, losses ? losses + row : (float*)nullptr,
                           states_out ? states_out + 12 * row : (float*)nullptr, grads_out ? grads_out + 12 * row : (float*)nullptr);
        { const int rc_s = nf_launched(who, "step"); if (rc_s != NGP_OK) return rc_s; }
    }
    return NGP_OK;
}

extern "C" int ngp_filter_iterations_multi(const ngp_nav_field_t* field, const void* prepared, const ngp_filter_cfg_t* c, uint32_t K, float* states,
                                           float* adam_states, const float* target, const int32_t* batches, uint32_t first_iter, uint32_t n_iter, int update,
                                           float* losses, float* states_out, float* grads_out, void* workspace, size_t workspace_bytes, void* stream) {
    return nf_iterations_multi("filter_iterations_multi", "filter_iterations_multi: null states / adam_states / target / batches",
                               "ngp_filter_multi_workspace(K, B, num_steps)", field, prepared, c, nullptr, K, states, adam_states, target, batches, first_iter,
                               n_iter, update, losses, states_out, grads_out, workspace, workspace_bytes, stream);
}

extern "C" int ngp_filter_iterations_occ(const ngp_nav_field_t* field, const void* prepared, const ngp_filter_cfg_t* c, const ngp_occ_grid_t* grid, uint32_t K,
                                         float* states, float* adam_states, const float* target, const int32_t* batches, uint32_t first_iter, uint32_t n_iter,
                                         int update, float* losses, float* states_out, float* grads_out, void* workspace, size_t workspace_bytes, void* stream) {
    NGP_REQUIRE(grid, "filter_iterations_occ: null occupancy grid");
    return nf_iterations_multi("filter_iterations_occ", "filter_iterations_occ: null states / adam_states / target / batches",
                               "ngp_filter_occ_workspace(K, B, num_steps)", field, prepared, c, grid, K, states, adam_states, target, batches, first_iter,
                               n_iter, update, losses, states_out, grads_out, workspace, workspace_bytes, stream);
}

static int nf_select_args(const char* who, const float* losses, const float* states, uint32_t K, float* best_state, float* best_loss, uint32_t* best_index) {
    NGP_REQUIRE(K >= 1 && K <= NGP_FILTER_MULTI_MAX_K, "%s: K = %u hypotheses; supported 1 <= K <= %u", who, K, NGP_FILTER_MULTI_MAX_K);
    NGP_REQUIRE(losses && states && best_state && best_loss && best_index, "%s: null pointer", who);
    return NGP_OK;
}

extern "C" int ngp_filter_select(const float* losses, const float* states, uint32_t K, float* best_state, float* best_loss, uint32_t* best_index,
                                 void* stream) {
    const int rc = nf_select_args("filter_select", losses, states, K, best_state, best_loss, best_index);
    if (rc != NGP_OK) return rc;
    hipLaunchKernelGGL(k_filter_select, dim3(1), dim3(64), 0, (hipStream_t)stream, losses, states, K, best_state, best_loss, best_index);
    NGP_CHECK_LAUNCH("filter_select");
    return NGP_OK;
}

extern "C" int ngp_filter_select_host(const float* losses, const float* states, uint32_t K, float* best_state, float* best_loss, uint32_t* best_index) {
    const int rc = nf_select_args("filter_select_host", losses, states, K, best_state, best_loss, best_index);
    if (rc != NGP_OK) return rc;
    const uint32_t best = ngp_select_best(losses, K);
    for (int e = 0; e < 12; e++) best_state[e] = states[12 * (size_t)best + e];
    *best_loss = losses[best];
    *best_index = best;
    return NGP_OK;
}

// ---------------------------------------------------------------------------
// the rest of the estimator's time step (Estimator.estimate_state, nav/estimator_helpers.py:347-406; DESIGN.md §3.5 "Native time step"):
//
//   k_filter_propagate   Agent.drone_dynamics, its 12 x 12 Jacobian A (lane j carries the forward-mode tangent along state[j]) and (A sig) A^T + Q
//   k_filter_hessian     measurement_fn's 12 x 12 Hessian under the reference's differentiation rule: k_filter_step's passes (nf_ray_sums .. nf_loss: the
//                        gradient, the loss and dL/dP come out bit for bit as an update = 0 iteration writes them), then sum_ab (dL/dP)_ab d2 P_ab / dr_i dr_j
//                        into H[6:9, 6:9] (one lane per (i, j), second-order forward mode) and Sinv + Sinv^T everywhere
//
// Both evaluate the formulas as written in float64 from the float32 inputs and round every output once (ngp_filter_step.h); one workgroup each.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(NF_THREADS) void k_filter_propagate(nfs_dyn D, const float* __restrict__ state, const float* __restrict__ action,
                                                                 const float* __restrict__ sig, const float* __restrict__ Q,
                                                                 float* __restrict__ next_state, float* __restrict__ A_out, float* __restrict__ sig_prop) {
    __shared__ double A[144], AS[144];
    const uint32_t tid = threadIdx.x;
    if (tid < 12) {
        nfs_d1 x[12], next[12];
        double act[4];
#pragma unroll
        for (int k = 0; k < 12; k++) x[k] = nfs_d1((double)state[k], k == (int)tid ? 1.0 : 0.0);
#pragma unroll
        for (int k = 0; k < 4; k++) act[k] = (double)action[k];
        nfs_drone_dynamics(D, x, act, next);
#pragma unroll
        for (int i = 0; i < 12; i++) {
            A[i * 12 + tid] = next[i].d;
            if (A_out) A_out[i * 12 + tid] = (float)next[i].d;
            if (tid == 0) next_state[i] = (float)next[i].v;
        }
    }
    if (!sig_prop) return;
    __syncthreads();
    const uint32_t i = tid / 12, j = tid % 12;
    if (tid < 144) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 12; k++) s += A[i * 12 + k] * (double)sig[k * 12 + j];
        AS[tid] = s;
    }
    __syncthreads();
    if (tid < 144) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 12; k++) s += AS[i * 12 + k] * A[j * 12 + k];
        sig_prop[tid] = (float)(s + (double)Q[tid]);
    }
}

__global__ __launch_bounds__(NF_THREADS) void k_filter_hessian(nf_view V, nf_step_args A, const float* __restrict__ state, const int32_t* __restrict__ batch,
                                                               uint32_t B, const float* __restrict__ grad_rays_o, const float* __restrict__ grad_rays_d,
                                                               const float* __restrict__ partials, uint32_t n_partials, float* __restrict__ hessian,
                                                               float* __restrict__ grad_out, float* __restrict__ loss_out, float* __restrict__ dLdP_out) {
    __shared__ nf_shared S;
    __shared__ double h_image[9];
    const uint32_t tid = threadIdx.x;
    nf_load_state(S, A, state);
    nf_ray_sums(S, V, batch, B, grad_rays_o, grad_rays_d, partials, n_partials);
    __syncthreads();
    if (tid == 0) {
        float tot[NF_SUMS];
        nf_image_gradient(S, B, tot);
        if (dLdP_out) {
#pragma unroll
            for (int e = 0; e < 9; e++) dLdP_out[e] = tot[3 + e];
        }
    }
    // the second wave meanwhile: lane 3 i + j takes d2 / dr_i dr_j of the camera rotation and contracts it with dL/dP (the same totals, nf_total's order)
    if (tid >= 64 && tid < 73) {
        const int ij = (int)tid - 64, i = ij / 3, j = ij % 3;
        nfs_d2 r[3], P[9];
#pragma unroll
        for (int k = 0; k < 3; k++) r[k] = nfs_d2((double)S.x[6 + k], k == i ? 1.0 : 0.0, k == j ? 1.0 : 0.0, 0.0);
        nfs_measurement_rotation(r, (double)1e-10f, (double)NF_C90, P);
        double h = 0.0;
#pragma unroll
        for (int e = 0; e < 9; e++) h += (double)nf_total(S, 3 + e) * P[e].ab;
        h_image[ij] = h;
    }
    const double mg = nf_process_row(S, A);
    __syncthreads();
    if (tid < 12 && grad_out) grad_out[tid] = S.g_image[tid] + (float)mg;
    if (tid == 0 && loss_out) *loss_out = nf_loss(S);
    if (tid < 144) {
        const uint32_t i = tid / 12, j = tid % 12;
        double h = (double)A.sig_inv[i * 12 + j] + (double)A.sig_inv[j * 12 + i];
        if (i >= 6 && i < 9 && j >= 6 && j < 9) h += h_image[(i - 6) * 3 + (j - 6)];
        hessian[tid] = (float)h;
    }
}

extern "C" int ngp_filter_propagate(const ngp_filter_dyn_t* dyn, const float* state, const float* action, const float* sig, const float* Q,
                                    float* next_state, float* A, float* sig_prop, void* stream) {
    NGP_REQUIRE(dyn, "filter_propagate: null cfg");
    NGP_REQUIRE(state && action && next_state, "filter_propagate: null state / action / next_state");
    NGP_REQUIRE(!sig_prop || (sig && Q), "filter_propagate: sig_prop needs sig and Q");
    nfs_dyn D;
    const int bad = nfs_dyn_prepare(dyn->dt, dyn->mass, dyn->g, dyn->I, D);
    NGP_REQUIRE(bad != 1, "filter_propagate: dt = %g, mass = %g; both must be finite and > 0", (double)dyn->dt, (double)dyn->mass);
    NGP_REQUIRE(bad != 2, "filter_propagate: the inertia matrix I is singular or not finite");
    hipLaunchKernelGGL(k_filter_propagate, dim3(1), dim3(NF_THREADS), 0, (hipStream_t)stream, D, state, action, sig, Q, next_state, A, sig_prop);
    NGP_CHECK_LAUNCH("filter_propagate");
    return NGP_OK;
}

static int nf_hessian(const char* who, const char* null_refusal, const char* ws_fn, const ngp_nav_field_t* field, const void* prepared,
                      const ngp_filter_cfg_t* c, const ngp_occ_grid_t* grid, const float* state, const float* target, const int32_t* batch, float* hessian,
                      float* grad, float* loss, float* dLdP, void* workspace, size_t workspace_bytes, void* stream, const nf_res* res = nullptr) {
    nf_view V;
    nf_ws w;
    nf_step_args A;
    int rc = nf_begin(who, state && target && batch && hessian ? nullptr : null_refusal, field, prepared, c, 1, ws_fn, workspace, workspace_bytes, stream, V, w,
                      A, grid, res);
    if (rc != NGP_OK) return rc;
    rc = nf_measure(who, field, prepared, c, V, w, 0, state, target, batch, stream, grid, res);
    if (rc != NGP_OK) return rc;
    hipLaunchKernelGGL(k_filter_hessian, dim3(1), dim3(NF_THREADS), 0, (hipStream_t)stream, V, A, state, batch, c->B, (const float*)w.grad_rays_o,
                       (const float*)w.grad_rays_d, (const float*)w.partials, ngp_div_up(c->B, NF_THREADS), hessian, grad, loss, dLdP);
    return nf_launched(who, "hessian");
}

extern "C" int ngp_filter_hessian(const ngp_nav_field_t* field, const void* prepared, const ngp_filter_cfg_t* c, const float* state, const float* target,
                                  const int32_t* batch, float* hessian, float* grad, float* loss, float* dLdP, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    return nf_hessian("filter_hessian", "filter_hessian: null state / target / batch / hessian", "ngp_filter_workspace(B, num_steps)", field, prepared, c,
                      nullptr, state, target, batch, hessian, grad, loss, dLdP, workspace, workspace_bytes, stream);
}

extern "C" int ngp_filter_hessian_occ(const ngp_nav_field_t* field, const void* prepared, const ngp_filter_cfg_t* c, const ngp_occ_grid_t* grid,
                                      const float* state, const float* target, const int32_t* batch, float* hessian, float* grad, float* loss, float* dLdP,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    NGP_REQUIRE(grid, "filter_hessian_occ: null occupancy grid");
    return nf_hessian("filter_hessian_occ", "filter_hessian_occ: null state / target / batch / hessian", "ngp_filter_occ_workspace(1, B, num_steps)", field,
                      prepared, c, grid, state, target, batch, hessian, grad, loss, dLdP, workspace, workspace_bytes, stream);
}

// ---- the resampled route: the same loop and Hessian with ngp_nav_run_resample + the run over its depth list in the measurement pass ----

extern "C" int ngp_filter_iterations_res(const ngp_nav_field_t* field, const void* prepared, const ngp_filter_cfg_t* c, uint32_t K, float* states,
                                         float* adam_states, const float* target, const int32_t* batches, uint32_t first_iter, uint32_t n_iter, int update,
                                         float* losses, float* states_out, float* grads_out, void* workspace, size_t workspace_bytes, uint32_t upsample_steps,
                                         float* z, void* stream) {
    const nf_res res = {upsample_steps, z};
    return nf_iterations_multi("filter_iterations_res", "filter_iterations_res: null states / adam_states / target / batches",
                               "ngp_filter_multi_workspace(K, B, num_steps + upsample_steps)", field, prepared, c, nullptr, K, states, adam_states, target,
                               batches, first_iter, n_iter, update, losses, states_out, grads_out, workspace, workspace_bytes, stream, &res);
}

extern "C" int ngp_filter_hessian_res(const ngp_nav_field_t* field, const void* prepared, const ngp_filter_cfg_t* c, const float* state, const float* target,
                                      const int32_t* batch, float* hessian, float* grad, float* loss, float* dLdP, void* workspace, size_t workspace_bytes,
                                      uint32_t upsample_steps, float* z, void* stream) {
    const nf_res res = {upsample_steps, z};
    return nf_hessian("filter_hessian_res", "filter_hessian_res: null state / target / batch / hessian", "ngp_filter_workspace(B, num_steps + upsample_steps)",
                      field, prepared, c, nullptr, state, target, batch, hessian, grad, loss, dLdP, workspace, workspace_bytes, stream, &res);
}
