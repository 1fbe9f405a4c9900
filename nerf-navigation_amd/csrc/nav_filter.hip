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
// The derivative conventions are torch autograd's of the formula as written (nav/math_utils.py:159-174): R = I + sin(a) K + ((1 - cos(a)) K) K,
// K = hat(r / (1e-10 + a)), a = |r|, with the denominator's dependence on a kept and a zero subgradient of the norm at r = 0.  No gradient flows through
// near / far (nerf/renderer.py:140-141).  No atomics; every sum runs in a fixed order, so two runs are bit-identical.
#include "ngp_device.h"
#include "ngp_camera.h"

static constexpr uint32_t NF_THREADS = 256, NF_WAVES = NF_THREADS / 64;
static constexpr uint32_t NF_MAX_B = 1u << 20, NF_MAX_T = 4096;             // num_steps: what ngp_nav_run_forward accepts
static constexpr uint32_t NF_SUMS = 13;                                      // grad_rays_o [3], dL/dP [9], squared error
enum : uint32_t { NF_M = 0, NF_V = 12, NF_G = 24, NF_STEP = 36 };            // adam_state (NGP_FILTER_ADAM_FLOATS)
static_assert(NGP_FILTER_ADAM_FLOATS == NF_STEP + 1, "adam_state layout");

// rot_x(pi / 2) as the reference builds it: cos and sin of (float)(pi / 2) in float32
#define NF_C90 (-4.37113883e-08f)

struct nf_view { float fx, fy, cx, cy; uint32_t W, H; float aabb[6]; float min_near; };
struct nf_step_args {
    float start[12], sig_inv[144];
    float lr, beta1, beta2, w1, w2, eps;                                     // Adam: w1 = (float)(1 - beta1), w2 = (float)(1 - beta2) formed in float64
};

// vec_to_rot_matrix (nav/math_utils.py:159-174) and what its backward needs
struct nf_rodrigues { float K[9], M[9], R[9], a, d, sn, cs; };

__device__ __forceinline__ void nf_matmul3(const float* A, const float* B, float* C) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[i * 3 + j] = (A[i * 3 + 0] * B[0 * 3 + j] + A[i * 3 + 1] * B[1 * 3 + j]) + A[i * 3 + 2] * B[2 * 3 + j];
}

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
    nf_matmul3(Q.M, Q.K, MK);
#pragma unroll
    for (int e = 0; e < 9; e++) Q.R[e] = ((e % 4 == 0 ? 1.0f : 0.0f) + Q.sn * K[e]) + MK[e];
}

// measurement_fn's pose (nav/estimator_helpers.py:301-309): P = cycle (rot_x(pi/2) R) diag(1, -1, -1), T = cycle position (nerf_matrix_to_ngp_torch)
__device__ __forceinline__ void nf_pose(const float* state, nf_rodrigues& Q, float* P, float* T) {
    const float r[3] = {state[6], state[7], state[8]};
    nf_rotation(r, Q);
    float Rb[9];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        Rb[0 + j] = Q.R[0 + j];
        Rb[3 + j] = NF_C90 * Q.R[3 + j] - Q.R[6 + j];
        Rb[6 + j] = Q.R[3 + j] + NF_C90 * Q.R[6 + j];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int m = (i + 1) % 3;
        P[i * 3 + 0] = Rb[m * 3 + 0]; P[i * 3 + 1] = -Rb[m * 3 + 1]; P[i * 3 + 2] = -Rb[m * 3 + 2];
        T[i] = state[m];
    }
}

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
    nf_matmul3(GR, Kt, GM);
    nf_matmul3(Mt, GR, GK);
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

__device__ __forceinline__ float nf_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ---------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(NF_THREADS) void k_filter_rays(nf_view V, const float* __restrict__ state, const int32_t* __restrict__ batch, uint32_t B,
                                                            float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ nears,
                                                            float* __restrict__ fars) {
    const uint32_t n = blockIdx.x * NF_THREADS + threadIdx.x;
    if (n >= B) return;
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

__global__ __launch_bounds__(NF_THREADS) void k_filter_loss(const float* __restrict__ image, const float* __restrict__ target,
                                                            const int32_t* __restrict__ batch, uint32_t B, uint32_t H, uint32_t W,
                                                            float* __restrict__ grad_image, float* __restrict__ partials) {
    __shared__ float wave_sums[NF_WAVES];
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
    sq = nf_wave_sum(sq);
    if ((threadIdx.x & 63u) == 0) wave_sums[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = wave_sums[0];
#pragma unroll
        for (uint32_t w = 1; w < NF_WAVES; w++) s += wave_sums[w];
        partials[blockIdx.x] = s;
    }
}

// one element of torch.optim.Adam(capturable=True)'s step: k_plan_cost_step's arithmetic (nav_plan.hip np_adam), restated here so that
// that kernel's code is not touched; bc1, bc2 = beta^step are the same for the 12 entries
__device__ __forceinline__ float nf_adam(const nf_step_args& A, float param, float grad, float* m, float* v, float step) {
    *m = *m + A.w1 * (grad - *m);
    *v = *v * A.beta2 + A.w2 * (grad * grad);
    float bc1 = powf(A.beta1, step), bc2 = powf(A.beta2, step);
    bc1 = bc1 - 1.0f; bc2 = -(bc2 - 1.0f);
    const float step_size = 1.0f / (bc1 / A.lr);
    const float bc2_sqrt = sqrtf(bc2);
    const float denom = (sqrtf(*v) / bc2_sqrt + A.eps) / step_size;
    return param + *m / denom;
}

__global__ __launch_bounds__(NF_THREADS) void k_filter_step(nf_view V, nf_step_args A, int update, float* __restrict__ state, float* __restrict__ adam,
                                                            const int32_t* __restrict__ batch, uint32_t B, const float* __restrict__ grad_rays_o,
                                                            const float* __restrict__ grad_rays_d, const float* __restrict__ partials,
                                                            uint32_t n_partials, float* __restrict__ loss_out, float* __restrict__ state_out,
                                                            float* __restrict__ grad_out) {
    __shared__ float sums[NF_WAVES][NF_SUMS];
    __shared__ float x[12], delta[12], g_image[12], quad[12], mse;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const float step = adam[NF_STEP] + 1.0f;                                 // read before any lane writes it (there are barriers in between)
    if (tid < 12) {
        const float s = state[tid];
        x[tid] = s;
        delta[tid] = s - A.start[tid];
    }
    // per-lane sums over the rays (lanes strided over them), then a fixed butterfly and the waves in order
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
    for (int k = 0; k < (int)NF_SUMS; k++) acc[k] = nf_wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < (int)NF_SUMS; k++) sums[wave][k] = acc[k];
    }
    __syncthreads();
    if (tid == 0) {
        float tot[NF_SUMS];
#pragma unroll
        for (int k = 0; k < (int)NF_SUMS; k++) {
            float s = sums[0][k];
#pragma unroll
            for (uint32_t w = 1; w < NF_WAVES; w++) s += sums[w][k];
            tot[k] = s;
        }
        float xs[12];
#pragma unroll
        for (int k = 0; k < 12; k++) { xs[k] = x[k]; g_image[k] = 0.0f; }
        nf_rodrigues Q;
        float P[9], T[3], gr[3];
        nf_pose(xs, Q, P, T);
        nf_pose_backward(xs + 6, Q, tot + 3, gr);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            g_image[(i + 1) % 3] = tot[i];                                  // T[i] = position[(i + 1) % 3]
            g_image[6 + i] = gr[i];
        }
        mse = tot[12] / (float)(3ull * B);
    }
    double mg = 0.0;
    if (tid < 12) {                                                          // Mahalanobis: delta^T Sinv delta and its gradient (Sinv + Sinv^T) delta
        double row = 0.0;
#pragma unroll
        for (int j = 0; j < 12; j++) {
            const double dj = (double)delta[j];
            row += (double)A.sig_inv[tid * 12 + j] * dj;
            mg += ((double)A.sig_inv[tid * 12 + j] + (double)A.sig_inv[j * 12 + tid]) * dj;
        }
        quad[tid] = (float)((double)delta[tid] * row);
    }
    __syncthreads();
    if (tid < 12) {
        const float g = g_image[tid] + (float)mg;
        const float s = x[tid];
        adam[NF_G + tid] = g;
        if (grad_out) grad_out[tid] = g;
        if (state_out) state_out[tid] = s;
        if (update) {
            float m = adam[NF_M + tid], v = adam[NF_V + tid];
            state[tid] = nf_adam(A, s, g, &m, &v, step);
            adam[NF_M + tid] = m;
            adam[NF_V + tid] = v;
        }
    }
    if (tid == 0) {
        if (loss_out) {
            float process = quad[0];
#pragma unroll
            for (int k = 1; k < 12; k++) process += quad[k];
            *loss_out = mse + process;
        }
        if (update) adam[NF_STEP] = step;
    }
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
static nf_ws nf_layout(uint32_t B, uint32_t num_steps, void* base) {
    if (B < 1 || B > NF_MAX_B || num_steps < 1 || num_steps > NF_MAX_T) return {};   // total 0: a shape no filter call accepts
    const size_t n = B, kept = ngp_nav_run_saved_bytes(B, num_steps);
    ngp_carver c(base);
    return {c.take<float>(3 * n), c.take<float>(3 * n), c.take<float>(n), c.take<float>(n), c.take<float>(3 * n), c.take<float>(n), c.take<float>(n),
            c.take<float>(3 * n), c.take<unsigned char>(kept), c.take<float>(3 * n), c.take<float>(3 * n), c.take<float>(ngp_div_up(B, NF_THREADS)),
            kept, c.total(256)};
}
extern "C" size_t ngp_filter_workspace(uint32_t B, uint32_t num_steps) { return nf_layout(B, num_steps, nullptr).total; }

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

extern "C" int ngp_filter_iterations(const ngp_nav_field_t* field, const void* prepared, const ngp_filter_cfg_t* c, float* state, float* adam_state,
                                     const float* target, const int32_t* batches, uint32_t first_iter, uint32_t n_iter, int update, float* losses,
                                     float* states_out, float* grads_out, void* workspace, size_t workspace_bytes, void* stream) {
    nf_view V;
    const int rc_v = nf_view_of("filter_iterations", c, V);
    if (rc_v != NGP_OK) return rc_v;
    const uint32_t B = c->B, T = c->num_steps;
    NGP_REQUIRE(T >= 1 && T <= NF_MAX_T, "filter_iterations: num_steps = %u; supported 1 <= num_steps <= 4096", T);
    NGP_REQUIRE(state && adam_state && target && batches, "filter_iterations: null state / adam_state / target / batches");
    const nf_ws w = nf_layout(B, T, workspace);
    if (!workspace || workspace_bytes < w.total)
        return ngp_fail(NGP_EWORKSPACE, "filter_iterations: workspace of %zu bytes, needs ngp_filter_workspace(B, num_steps) = %zu", workspace_bytes, w.total);
    {   // the field is checked here, before anything is queued (N = 0 validates and launches nothing)
        const int rc_f = ngp_nav_run_forward(field, prepared, w.rays_o, w.rays_d, w.nears, w.fars, 0, T, c->aabb, c->bg, w.image, w.depth, w.weights_sum,
                                             w.saved, w.saved_bytes, stream);
        if (rc_f != NGP_OK) return rc_f;
    }
    if (n_iter == 0) return NGP_OK;
    nf_step_args A;
    for (int k = 0; k < 12; k++) A.start[k] = c->start_state[k];
    for (int k = 0; k < 144; k++) A.sig_inv[k] = c->sig_inv[k];
    A.lr = (float)c->lr; A.beta1 = (float)c->beta1; A.beta2 = (float)c->beta2;
    A.w1 = (float)(1.0 - c->beta1); A.w2 = (float)(1.0 - c->beta2); A.eps = (float)c->eps;
    const uint32_t blocks = ngp_div_up(B, NF_THREADS);
    hipStream_t s = (hipStream_t)stream;
    for (uint32_t k = 0; k < n_iter; k++) {
        const int32_t* batch = batches + 2 * (size_t)B * ((size_t)first_iter + k);
        hipLaunchKernelGGL(k_filter_rays, dim3(blocks), dim3(NF_THREADS), 0, s, V, (const float*)state, batch, B, w.rays_o, w.rays_d, w.nears, w.fars);
        NGP_CHECK_LAUNCH("filter_iterations: rays");
        int rc = ngp_nav_run_forward(field, prepared, w.rays_o, w.rays_d, w.nears, w.fars, B, T, c->aabb, c->bg, w.image, w.depth, w.weights_sum, w.saved,
                                     w.saved_bytes, stream);
        if (rc != NGP_OK) return rc;
        hipLaunchKernelGGL(k_filter_loss, dim3(blocks), dim3(NF_THREADS), 0, s, (const float*)w.image, target, batch, B, c->H, c->W, w.grad_image, w.partials);
        NGP_CHECK_LAUNCH("filter_iterations: loss");
        rc = ngp_nav_run_backward(field, prepared, w.rays_o, w.rays_d, w.nears, w.fars, B, T, c->aabb, c->bg, w.grad_image, nullptr, nullptr, w.saved,
                                  w.saved_bytes, w.grad_rays_o, w.grad_rays_d, stream);
        if (rc != NGP_OK) return rc;
        hipLaunchKernelGGL(k_filter_step, dim3(1), dim3(NF_THREADS), 0, s, V, A, update, state, adam_state, batch, B, (const float*)w.grad_rays_o,
                           (const float*)w.grad_rays_d, (const float*)w.partials, blocks, losses ? losses + k : (float*)nullptr,
                           states_out ? states_out + 12 * (size_t)k : (float*)nullptr, grads_out ? grads_out + 12 * (size_t)k : (float*)nullptr);
        NGP_CHECK_LAUNCH("filter_iterations: step");
    }
    return NGP_OK;
}

// ---------------------------------------------------------------------------
// the rest of the estimator's time step (Estimator.estimate_state, nav/estimator_helpers.py:347-406; DESIGN.md §3.5 "Native time step"):
//
//   k_filter_propagate   Agent.drone_dynamics, its 12 x 12 Jacobian A (lane j carries the forward-mode tangent along state[j]) and (A sig) A^T + Q
//   k_filter_hessian     measurement_fn's 12 x 12 Hessian under the reference's differentiation rule: the sums of k_filter_step in its order (the
//                        gradient, the loss and dL/dP come out bit for bit as an update = 0 iteration writes them), then sum_ab (dL/dP)_ab d2 P_ab / dr_i dr_j
//                        into H[6:9, 6:9] (one lane per (i, j), second-order forward mode) and Sinv + Sinv^T everywhere
//
// Both evaluate the formulas as written in float64 from the float32 inputs and round every output once (ngp_filter_step.h); one workgroup each.
// ---------------------------------------------------------------------------
#include "ngp_filter_step.h"

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
    __shared__ float sums[NF_WAVES][NF_SUMS];
    __shared__ float x[12], delta[12], g_image[12], quad[12], mse;
    __shared__ double h_image[9];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid < 12) {
        const float s = state[tid];
        x[tid] = s;
        delta[tid] = s - A.start[tid];
    }
    // k_filter_step's sums, in its order
    float acc[NF_SUMS];
#pragma unroll
    for (int k = 0; k < (int)NF_SUMS; k++) acc[k] = 0.0f;
    ngp_camera unit;
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
    for (int k = 0; k < (int)NF_SUMS; k++) acc[k] = nf_wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < (int)NF_SUMS; k++) sums[wave][k] = acc[k];
    }
    __syncthreads();
    if (tid == 0) {
        float tot[NF_SUMS];
#pragma unroll
        for (int k = 0; k < (int)NF_SUMS; k++) {
            float s = sums[0][k];
#pragma unroll
            for (uint32_t w = 1; w < NF_WAVES; w++) s += sums[w][k];
            tot[k] = s;
        }
        float xs[12];
#pragma unroll
        for (int k = 0; k < 12; k++) { xs[k] = x[k]; g_image[k] = 0.0f; }
        nf_rodrigues Q;
        float P[9], T[3], gr[3];
        nf_pose(xs, Q, P, T);
        nf_pose_backward(xs + 6, Q, tot + 3, gr);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            g_image[(i + 1) % 3] = tot[i];
            g_image[6 + i] = gr[i];
        }
        mse = tot[12] / (float)(3ull * B);
        if (dLdP_out) {
#pragma unroll
            for (int e = 0; e < 9; e++) dLdP_out[e] = tot[3 + e];
        }
    }
    // the second wave meanwhile: lane 3 i + j takes d2 / dr_i dr_j of the camera rotation and contracts it with dL/dP (the same sums, added in the same order)
    if (tid >= 64 && tid < 73) {
        const int ij = (int)tid - 64, i = ij / 3, j = ij % 3;
        nfs_d2 r[3], P[9];
#pragma unroll
        for (int k = 0; k < 3; k++) r[k] = nfs_d2((double)x[6 + k], k == i ? 1.0 : 0.0, k == j ? 1.0 : 0.0, 0.0);
        nfs_measurement_rotation(r, (double)1e-10f, (double)NF_C90, P);
        double h = 0.0;
#pragma unroll
        for (int e = 0; e < 9; e++) {
            float s = sums[0][3 + e];
#pragma unroll
            for (uint32_t w = 1; w < NF_WAVES; w++) s += sums[w][3 + e];
            h += (double)s * P[e].ab;
        }
        h_image[ij] = h;
    }
    double mg = 0.0;
    if (tid < 12) {
        double row = 0.0;
#pragma unroll
        for (int j = 0; j < 12; j++) {
            const double dj = (double)delta[j];
            row += (double)A.sig_inv[tid * 12 + j] * dj;
            mg += ((double)A.sig_inv[tid * 12 + j] + (double)A.sig_inv[j * 12 + tid]) * dj;
        }
        quad[tid] = (float)((double)delta[tid] * row);
    }
    __syncthreads();
    if (tid < 12 && grad_out) grad_out[tid] = g_image[tid] + (float)mg;
    if (tid == 0 && loss_out) {
        float process = quad[0];
#pragma unroll
        for (int k = 1; k < 12; k++) process += quad[k];
        *loss_out = mse + process;
    }
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

extern "C" int ngp_filter_hessian(const ngp_nav_field_t* field, const void* prepared, const ngp_filter_cfg_t* c, const float* state, const float* target,
                                  const int32_t* batch, float* hessian, float* grad, float* loss, float* dLdP, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    nf_view V;
    const int rc_v = nf_view_of("filter_hessian", c, V);
    if (rc_v != NGP_OK) return rc_v;
    const uint32_t B = c->B, T = c->num_steps;
    NGP_REQUIRE(T >= 1 && T <= NF_MAX_T, "filter_hessian: num_steps = %u; supported 1 <= num_steps <= 4096", T);
    NGP_REQUIRE(state && target && batch && hessian, "filter_hessian: null state / target / batch / hessian");
    const nf_ws w = nf_layout(B, T, workspace);
    if (!workspace || workspace_bytes < w.total)
        return ngp_fail(NGP_EWORKSPACE, "filter_hessian: workspace of %zu bytes, needs ngp_filter_workspace(B, num_steps) = %zu", workspace_bytes, w.total);
    {   // the field is checked here, before anything is queued (N = 0 validates and launches nothing)
        const int rc_f = ngp_nav_run_forward(field, prepared, w.rays_o, w.rays_d, w.nears, w.fars, 0, T, c->aabb, c->bg, w.image, w.depth, w.weights_sum,
                                             w.saved, w.saved_bytes, stream);
        if (rc_f != NGP_OK) return rc_f;
    }
    nf_step_args A = {};
    for (int k = 0; k < 12; k++) A.start[k] = c->start_state[k];
    for (int k = 0; k < 144; k++) A.sig_inv[k] = c->sig_inv[k];
    const uint32_t blocks = ngp_div_up(B, NF_THREADS);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_filter_rays, dim3(blocks), dim3(NF_THREADS), 0, s, V, state, batch, B, w.rays_o, w.rays_d, w.nears, w.fars);
    NGP_CHECK_LAUNCH("filter_hessian: rays");
    int rc = ngp_nav_run_forward(field, prepared, w.rays_o, w.rays_d, w.nears, w.fars, B, T, c->aabb, c->bg, w.image, w.depth, w.weights_sum, w.saved,
                                 w.saved_bytes, stream);
    if (rc != NGP_OK) return rc;
    hipLaunchKernelGGL(k_filter_loss, dim3(blocks), dim3(NF_THREADS), 0, s, (const float*)w.image, target, batch, B, c->H, c->W, w.grad_image, w.partials);
    NGP_CHECK_LAUNCH("filter_hessian: loss");
    rc = ngp_nav_run_backward(field, prepared, w.rays_o, w.rays_d, w.nears, w.fars, B, T, c->aabb, c->bg, w.grad_image, nullptr, nullptr, w.saved,
                              w.saved_bytes, w.grad_rays_o, w.grad_rays_d, stream);
    if (rc != NGP_OK) return rc;
    hipLaunchKernelGGL(k_filter_hessian, dim3(1), dim3(NF_THREADS), 0, s, V, A, state, batch, B, (const float*)w.grad_rays_o, (const float*)w.grad_rays_d,
                       (const float*)w.partials, blocks, hessian, grad, loss, dLdP);
    NGP_CHECK_LAUNCH("filter_hessian: hessian");
    return NGP_OK;
}
