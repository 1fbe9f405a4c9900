// nav_field.hip -- the navigation loop's queries (BASELINE config 4) as fused float32 gfx950 kernels.
//
// The reference's planner and pose filter (simulate.py:340-347, nav/quad_plot.py:224-250, nav/estimator_helpers.py:293-327) call the
// DEFAULT field (nerf/network.py: hash grid -> Linear(32,64) -> Linear(64,16) ; SH(16) ++ geo(15) -> Linear(31,64) -> Linear(64,64) ->
// Linear(64,3), no biases) in float32, without autocast, through torch autograd:
//     density_fn(x)          = exp(h0(x))                                   with d sigma / d x
//     render_fn(rays)        = NeRFRenderer.run(num_steps = 512, upsample_steps = 0)      with d image / d rays_o, d rays_d
// Per filter iteration that is ~130 launches (encoder, 5 rocBLAS GEMMs and their 8 backward GEMMs, ~60 elementwise kernels over
// [1024, 512] tensors).  Here: one launch forward, one launch backward.
//
//   k_nav_density_fwd / _bwd   one lane per point: 16 x 8 float2 gathers, the 32-64-16 MLP on the VALU with the weights read through
//                              the scalar cache (every lane of a wave multiplies by the same weight: an SGPR operand, no LDS, no VGPR)
//   k_nav_run_fwd / _bwd       one 256-thread workgroup per ray, samples in chunks of 256: positions, density, the alpha / cumprod
//                              weights of nerf/renderer.py:206-210 by a block scan, colour only where weights > 1e-4 (:217), the
//                              image / depth / weights_sum reductions; the backward recomputes the forward, derives d L / d sigma_i
//                              analytically (prefix product + suffix sum), and runs colour-net and density-net backward per sample down
//                              to d L / d xyz, reduced into d L / d rays_o and d L / d rays_d.
//   k_nav_run_occ_fwd / _bwd   the same run with the occupancy grid consulted (sigma = 0 where the bit is clear), one WAVE per ray over the compacted
//                              list of its occupied samples: the pose filter's opt-in route (the section before "host side" below)
//   k_nav_resample, k_sample_pdf, k_nav_run_fwd<true> / _bwd<true>   the run with upsample_steps > 0: the coarse pass, sample_pdf's inverse CDF and the depth-ordered
//                              merge in one launch, then the run kernels over that explicit depth list ("The resampled run" below)
// The run exists ONCE: nv_run_sample_fwd<W, COLOUR> and nv_run_sample_bwd<W> are one sample's forward and backward on one of the W lanes that share its
// ray (W = NV_BLOCK: the dense / depth-list kernels and the resample kernel's coarse pass; W = 64: the occupied kernels), over the team primitives
// nv_team_excl_product / _sum / _excl_suffix_sum<W>, with nv_ray_load, nv_run_write and nv_run_write_grads around them.  A kernel states which sample
// a lane handles and where its record lies, its LDS carve-up, and what is its own (the lattice walk and compaction; the pdf, inverse CDF and merge).
// float32 FMA throughput is the same on the VALU and on the f32 MFMA of this chip, and the batch is small (10 k - 524 k points), so
// the matrix cores would buy nothing here; what the fusion removes is launches and the [M, 64] round trips through HBM.
//
// Arithmetic: float32 like the reference path, but sums are fused multiply-adds in a fixed order of their own (rocBLAS has its own):
// results agree with the torch path to float32 rounding (tests/test_gpu_nav_native.py states the tolerances against the CPU oracle).
#include "ngp_nav_field.h"
#include "ngp_march.h"                                                       // ngp_point::at: the cell of a position (the occupancy-masked run)

// ---------------------------------------------------------------------------
// density queries on explicit points (planner: nav/quad_plot.py:224-250)
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(NV_BLOCK) void k_nav_density_fwd(nav_params P, const float* __restrict__ xyz, uint32_t M, float* __restrict__ sigma,
                                                              float* __restrict__ geo) {
    extern __shared__ float nv_smem[];
    float* col = nv_smem + 16 + threadIdx.x;
    const uint32_t i = blockIdx.x * NV_BLOCK + threadIdx.x;
    const uint32_t ic = i < M ? i : M - 1;
    float x0, x1, x2;
    const bool inside = nv_normalise(P, xyz[3ull * ic], xyz[3ull * ic + 1], xyz[3ull * ic + 2], x0, x1, x2);
    float out[16];
    nv_density_forward<4>(P, inside, x0, x1, x2, col, out);
    if (i >= M) return;
    if (geo) {
        #pragma unroll
        for (int m = 0; m < NV_GEO; m++) geo[(uint64_t)i * NV_GEO + m] = out[1 + m];
    }
    sigma[i] = expf(out[0]);                                           // trunc_exp forward (activation.py:9-10)
}

__global__ __launch_bounds__(NV_BLOCK) void k_nav_density_bwd(nav_params P, const float* __restrict__ xyz, uint32_t M, const float* __restrict__ gsigma,
                                                              const float* __restrict__ ggeo, float* __restrict__ gxyz) {
    extern __shared__ float nv_smem[];
    float* col = nv_smem + 16 + threadIdx.x;
    const uint32_t i = blockIdx.x * NV_BLOCK + threadIdx.x;
    const uint32_t ic = i < M ? i : M - 1;
    float x0, x1, x2;
    const bool inside = nv_normalise(P, xyz[3ull * ic], xyz[3ull * ic + 1], xyz[3ull * ic + 2], x0, x1, x2);
    float out[16], gout[16];
    const uint64_t relu = nv_density_forward<4>(P, inside, x0, x1, x2, col, out);
    gout[0] = gsigma[ic] * nv_exp_clamped(out[0]);
    #pragma unroll
    for (int m = 0; m < NV_GEO; m++) gout[1 + m] = ggeo ? ggeo[(uint64_t)ic * NV_GEO + m] : 0.0f;
    float gx, gy, gz;
    nv_density_backward<4>(P, inside, x0, x1, x2, relu, gout, col, gx, gy, gz);
    if (i >= M) return;
    gxyz[3ull * i] = gx; gxyz[3ull * i + 1] = gy; gxyz[3ull * i + 2] = gz;
}

// ---------------------------------------------------------------------------
// The planner's query (nav/quad_plot.py:224-250 through simulate.py:340-343): sigma AND d sigma / d x for a FEW THOUSAND points, in one launch.
//
// k_nav_density_fwd / _bwd walk a point's 16 levels in one lane: for 10,000 body points that is 40 workgroups on 256 CUs, each waiting for 16 dependent
// gather round trips and a 6,000-FMA matrix-vector chain on one wave -- slower than the level-parallel op chain (0.21 against 0.15 ms).  Here a
// point's levels are split over the FOUR WAVES of its workgroup (64 points per workgroup, lane = point, wave w = levels 4w..4w+3): all 32 gathers of a
// lane are issued before the first use (one round trip), each wave accumulates its share of the first layer, the shares meet in LDS, and since only
// sigma = exp(out[0]) is asked for, the second layer is ONE row: out0 = W2[0] . relu(h) and d out0 / d h = W2[0] masked by the ReLU -- no matrix-vector
// product on the way back.  The Jacobian reuses the corner values the forward gathered (nv_level_grad would fetch them again).
// `rot`: simulate.py:340's axis change x @ rot folded in (a 3x3 row-major matrix or null): p = x rot on the way in, d sigma / d x = rot (d sigma / d p) on the
// way out.  jac already contains trunc_exp's backward factor exp(clamp(out0, -15, 15)) (activation.py:16-18): grad_x = grad_sigma * jac.
// ---------------------------------------------------------------------------
struct nav_rot { float m[9]; uint32_t on; };
static constexpr uint32_t NV_VJ_POINTS = 64;
static constexpr size_t NV_VJ_LDS = sizeof(float) * (4 * NV_H * 64 + NV_H * 64 + 4 * 64 + 4 * 3 * 64);      // h shares | d out0 / d h | out0 shares | gradient shares

__global__ __launch_bounds__(256) void k_nav_density_vj(nav_params P, nav_rot R, const float* __restrict__ xyz, uint32_t M, float* __restrict__ sigma,
                                                        float* __restrict__ jac) {
    extern __shared__ float nv_smem[];
    float* lds_h = nv_smem;                                              // [4 waves][64 j][64 lanes]
    float* lds_gh = lds_h + 4 * NV_H * 64;                               // [64 j][64 lanes]
    float* lds_o = lds_gh + NV_H * 64;                                   // [4][64]
    float* lds_a = lds_o + 4 * 64;                                       // [4][3][64]
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t i = blockIdx.x * NV_VJ_POINTS + lane;
    const uint32_t ic = i < M ? i : M - 1;
    const float wx = xyz[3ull * ic], wy = xyz[3ull * ic + 1], wz = xyz[3ull * ic + 2];
    float px = wx, py = wy, pz = wz;
    if (R.on) {                                                          // p = x @ rot (row vector times matrix)
        px = (wx * R.m[0] + wy * R.m[3]) + wz * R.m[6];
        py = (wx * R.m[1] + wy * R.m[4]) + wz * R.m[7];
        pz = (wx * R.m[2] + wy * R.m[5]) + wz * R.m[8];
    }
    float x0, x1, x2;
    const bool inside = nv_normalise(P, px, py, pz, x0, x1, x2);

    // ---- this wave's four levels: cells, all 32 corner rows in flight at once ----
    nv_cell c[4];
    float2 v[4][8];
    #pragma unroll
    for (int k = 0; k < 4; k++) {
        const int l = (int)(4u * wave) + k;
        c[k] = nv_locate(P.lv.scale[l], x0, x1, x2);
        #pragma unroll
        for (int q = 0; q < 8; q++) v[k][q] = P.table[nv_row(P, l, c[k].gx + (q & 1), c[k].gy + ((q >> 1) & 1), c[k].gz + (q >> 2))];
    }
    // ---- its share of the hidden pre-activations: h += W1t[2l] e0 + W1t[2l+1] e1 (nv_hidden's order inside a level) ----
    {
        float h[NV_H];
        #pragma unroll
        for (int j = 0; j < NV_H; j++) h[j] = 0.0f;
        #pragma unroll
        for (int k = 0; k < 4; k++) {
            float e0 = 0.0f, e1 = 0.0f;
            #pragma unroll
            for (int q = 0; q < 8; q++) {
                const float w = (((q & 1) ? c[k].fx : 1.0f - c[k].fx) * ((q & 2) ? c[k].fy : 1.0f - c[k].fy)) * ((q & 4) ? c[k].fz : 1.0f - c[k].fz);
                e0 = __builtin_fmaf(w, v[k][q].x, e0);
                e1 = __builtin_fmaf(w, v[k][q].y, e1);
            }
            if (!inside) { e0 = 0.0f; e1 = 0.0f; }
            const nv_wptr wa = nv_hide(P.w1t) + (2 * (4 * wave + k)) * NV_H;
            const nv_wptr wb = wa + NV_H;
            #pragma unroll
            for (int j = 0; j < NV_H; j++) h[j] = __builtin_fmaf(wa[j], e0, h[j]);
            #pragma unroll
            for (int j = 0; j < NV_H; j++) h[j] = __builtin_fmaf(wb[j], e1, h[j]);
        }
        #pragma unroll
        for (int j = 0; j < NV_H; j++) lds_h[(wave * NV_H + j) * 64 + lane] = h[j];
    }
    __syncthreads();
    // ---- wave w owns hidden units 16w .. 16w+15: sum the four shares (fixed order), ReLU, its part of out0 = W2[0] . relu(h) and of d out0 / d h ----
    {
        const nv_wptr w2 = nv_hide(P.w2);                                // row 0 of sigma_net.1.weight [16][64]
        float o = 0.0f;
        #pragma unroll
        for (int jj = 0; jj < 16; jj++) {
            const int j = (int)(16u * wave) + jj;
            const float hj = ((lds_h[(0 * NV_H + j) * 64 + lane] + lds_h[(1 * NV_H + j) * 64 + lane]) + lds_h[(2 * NV_H + j) * 64 + lane]) + lds_h[(3 * NV_H + j) * 64 + lane];
            const float wj = w2[j];
            o = __builtin_fmaf(wj, fmaxf(hj, 0.0f), o);
            lds_gh[j * 64 + lane] = hj > 0.0f ? wj : 0.0f;
        }
        lds_o[wave * 64 + lane] = o;
    }
    __syncthreads();
    const float out0 = ((lds_o[lane] + lds_o[64 + lane]) + lds_o[128 + lane]) + lds_o[192 + lane];
    // ---- back through the first layer for this wave's levels, contracted with the trilinear Jacobian of the corners it still holds ----
    {
        float ax = 0.0f, ay = 0.0f, az = 0.0f;
        #pragma unroll
        for (int k = 0; k < 4; k++) {
            const nv_wptr wa = nv_hide(P.w1t) + (2 * (4 * wave + k)) * NV_H;
            const nv_wptr wb = wa + NV_H;
            float g0 = 0.0f, g1 = 0.0f;
            #pragma unroll
            for (int j = 0; j < NV_H; j++) { const float gj = lds_gh[j * 64 + lane]; g0 = __builtin_fmaf(wa[j], gj, g0); g1 = __builtin_fmaf(wb[j], gj, g1); }
            float sv[8];
            #pragma unroll
            for (int q = 0; q < 8; q++) sv[q] = __builtin_fmaf(g0, v[k][q].x, g1 * v[k][q].y);
            const float fx = c[k].fx, fy = c[k].fy, fz = c[k].fz, wx0 = 1.0f - fx, wy0 = 1.0f - fy, wz0 = 1.0f - fz;
            const float dx = (wy0 * wz0) * (sv[1] - sv[0]) + (fy * wz0) * (sv[3] - sv[2]) + (wy0 * fz) * (sv[5] - sv[4]) + (fy * fz) * (sv[7] - sv[6]);
            const float dy = (wx0 * wz0) * (sv[2] - sv[0]) + (fx * wz0) * (sv[3] - sv[1]) + (wx0 * fz) * (sv[6] - sv[4]) + (fx * fz) * (sv[7] - sv[5]);
            const float dz = (wx0 * wy0) * (sv[4] - sv[0]) + (fx * wy0) * (sv[5] - sv[1]) + (wx0 * fy) * (sv[6] - sv[2]) + (fx * fy) * (sv[7] - sv[3]);
            const float scale = P.lv.scale[4 * wave + k];
            ax = __builtin_fmaf(scale, dx, ax); ay = __builtin_fmaf(scale, dy, ay); az = __builtin_fmaf(scale, dz, az);
        }
        lds_a[(wave * 3 + 0) * 64 + lane] = ax; lds_a[(wave * 3 + 1) * 64 + lane] = ay; lds_a[(wave * 3 + 2) * 64 + lane] = az;
    }
    __syncthreads();
    if (wave != 0 || i >= M) return;
    float a[3];
    #pragma unroll
    for (int d = 0; d < 3; d++) a[d] = ((lds_a[(0 * 3 + d) * 64 + lane] + lds_a[(1 * 3 + d) * 64 + lane]) + lds_a[(2 * 3 + d) * 64 + lane]) + lds_a[(3 * 3 + d) * 64 + lane];
    const float k = (inside ? P.r2b : 0.0f) * nv_exp_clamped(out0);      // d x01 / d p, times trunc_exp's backward factor
    const float gpx = a[0] * k, gpy = a[1] * k, gpz = a[2] * k;
    float gx = gpx, gy = gpy, gz = gpz;
    if (R.on) {                                                          // d sigma / d x = rot . (d sigma / d p)
        gx = (R.m[0] * gpx + R.m[1] * gpy) + R.m[2] * gpz;
        gy = (R.m[3] * gpx + R.m[4] * gpy) + R.m[5] * gpz;
        gz = (R.m[6] * gpx + R.m[7] * gpy) + R.m[8] * gpz;
    }
    sigma[i] = expf(out0);                                               // trunc_exp forward (activation.py:9-10)
    jac[3ull * i] = gx; jac[3ull * i + 1] = gy; jac[3ull * i + 2] = gz;
}

// ---------------------------------------------------------------------------
// NeRFRenderer.run (nerf/renderer.py:125-254) with upsample_steps = 0, perturb = False
// ---------------------------------------------------------------------------

struct nav_run {
    const float* rays_o; const float* rays_d; const float* nears; const float* fars;
    uint32_t N, T;
    float aabb[6];
    float bg[3];
};
// the explicit depth list [N, T] of the AT instantiations of the run kernels and their sample_dist = (far - near) / dist.  The LAST kernel argument, so that
// the linspace instantiations, which never read it, keep the argument offsets and the code they had
struct nav_at { const float* z; uint32_t dist; };

// torch.linspace(0, 1, T)[i] in float32 as ATen's GPU kernel produces it (RangeFactories.cu: start + step * i for the first half,
// end - step * (T - 1 - i) for the second, compiled with contraction: ONE rounding).  Matching its bits matters more than it looks: a
// sample one ulp away can sit in the neighbouring cell of a fine level, where the derivative of the trilinear interpolation differs.
__device__ __forceinline__ float nv_lin(uint32_t i, uint32_t T) {
    if (T < 2) return 0.0f;
    const float step = 1.0f / (float)(T - 1);
    return i < T / 2 ? step * (float)i : __builtin_fmaf(-step, (float)(T - 1 - i), 1.0f);
}

struct nv_sample { float z, znext_minus_z, px, py, pz, lin, bx, by, bz; };       // b*: how much of the gradient the clip of that coordinate passes

// d min(max(x, lo), hi) / d x as torch.max / torch.min differentiate it (:159): 1 inside, 0 outside, and HALF on a tie -- which is the
// common case for the first sample of a ray, whose position is the point where the ray enters the box
__device__ __forceinline__ float nv_clip_pass(float x, float lo, float hi) {
    const float a = x > lo ? 1.0f : (x == lo ? 0.5f : 0.0f);
    const float m = fmaxf(x, lo);
    const float b = m < hi ? 1.0f : (m == hi ? 0.5f : 0.0f);
    return a * b;
}

struct nv_ray { float ox, oy, oz, dx, dy, dz, near, far, span; };

__device__ __forceinline__ nv_ray nv_ray_load(const nav_run& R, uint32_t n) {
    nv_ray r;
    r.ox = R.rays_o[3ull * n]; r.oy = R.rays_o[3ull * n + 1]; r.oz = R.rays_o[3ull * n + 2];
    r.dx = R.rays_d[3ull * n]; r.dy = R.rays_d[3ull * n + 1]; r.dz = R.rays_d[3ull * n + 2];
    r.near = R.nears[n]; r.far = R.fars[n]; r.span = r.far - r.near;
    return r;
}

// AT: the depths come from the ray's row of the depth list (`zrow`, T entries) instead of the linspace lattice, and the last delta is (far - near) / dist
template <bool AT = false>
__device__ __forceinline__ nv_sample nv_sample_at(const nav_run& R, uint32_t i, const nv_ray& ray, const float* __restrict__ zrow = nullptr, uint32_t dist = 0) {
    nv_sample s;
    if (AT) {
        s.lin = 0.0f;
        s.z = zrow[i];                                                   // the merged list (:196-197)
        s.znext_minus_z = (i + 1 < R.T) ? zrow[i + 1] - s.z : ray.span / (float)dist;    // :206-207 with :153's sample_dist
    } else {
        s.lin = nv_lin(i, R.T);
        s.z = ray.near + ray.span * s.lin;                               // :147-148
        const float zn = (i + 1 < R.T) ? ray.near + ray.span * nv_lin(i + 1, R.T) : 0.0f;
        s.znext_minus_z = (i + 1 < R.T) ? zn - s.z : ray.span / (float)R.T;              // deltas, last = sample_dist (:206-207, :151)
    }
    const float x = ray.ox + ray.dx * s.z, y = ray.oy + ray.dy * s.z, z = ray.oz + ray.dz * s.z;     // :158
    s.px = fminf(fmaxf(x, R.aabb[0]), R.aabb[3]);                        // :159
    s.py = fminf(fmaxf(y, R.aabb[1]), R.aabb[4]);
    s.pz = fminf(fmaxf(z, R.aabb[2]), R.aabb[5]);
    s.bx = nv_clip_pass(x, R.aabb[0], R.aabb[3]);
    s.by = nv_clip_pass(y, R.aabb[1], R.aabb[4]);
    s.bz = nv_clip_pass(z, R.aabb[2], R.aabb[5]);
    return s;
}

// ---- team primitives: one value per lane over the W lanes that share a ray.  W = NV_BLOCK: the four waves of a workgroup meet through `lds4` (two
// barriers per call); W = 64: one wave, shuffles only, no barrier, `lds4` untouched.  Two specialisations of one name, chosen at compile time. ----

__device__ __forceinline__ float nro_wave_sum(float v) {                // lane 0 holds the sum
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ float nv_wave_incl_product(float v) {
    const int lane = threadIdx.x & 63;
    #pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const float up = __shfl_up(v, off, 64); if (lane >= off) v = up * v; }
    return v;
}

// EXCLUSIVE by construction (scan of the sequence shifted by one lane): an inclusive scan minus the own term would cancel --
// an opaque sample's own A w is many orders of magnitude above the sum of everything behind it, and that small sum, divided
// by the sample's equally small (1 - alpha), is a first-order term of d L / d alpha
__device__ __forceinline__ float nv_wave_excl_suffix_sum(float v) {
    const int lane = threadIdx.x & 63;
    float rs = __shfl_down(v, 1, 64);
    if (lane == 63) rs = 0.0f;
    #pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const float dn = __shfl_down(rs, off, 64); if (lane + off < 64) rs += dn; }
    return rs;
}

// exclusive prefix product of one value per lane; `total` = the product of all of them
template <uint32_t W> __device__ __forceinline__ float nv_team_excl_product(float v, float* __restrict__ lds4, float& total);
// the sum of one value per lane (W = 64: in lane 0)
template <uint32_t W> __device__ __forceinline__ float nv_team_sum(float v, float* __restrict__ lds4);
// `behind` + the sum of the lanes after this one; `total` = the sum of all lanes
template <uint32_t W> __device__ __forceinline__ float nv_team_excl_suffix_sum(float v, float behind, float* __restrict__ lds4, float& total);

template <> __device__ __forceinline__ float nv_team_excl_product<NV_BLOCK>(float v, float* __restrict__ lds4, float& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float incl = nv_wave_incl_product(v);
    __syncthreads();
    if (lane == 63) lds4[wave] = incl;
    __syncthreads();
    float before = __shfl_up(incl, 1, 64);
    if (lane == 0) before = 1.0f;
    float base = 1.0f, tot = 1.0f;
    #pragma unroll
    for (int w = 0; w < (int)(NV_BLOCK / 64); w++) { const float t = lds4[w]; if (w < wave) base *= t; tot *= t; }
    total = tot;
    return base * before;
}

template <> __device__ __forceinline__ float nv_team_excl_product<64>(float v, float* __restrict__, float& total) {
    const float incl = nv_wave_incl_product(v);
    float before = __shfl_up(incl, 1, 64);
    if ((threadIdx.x & 63) == 0) before = 1.0f;
    total = __shfl(incl, 63, 64);
    return before;
}

template <> __device__ __forceinline__ float nv_team_sum<NV_BLOCK>(float v, float* __restrict__ lds4) {
    v = nro_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
}

template <> __device__ __forceinline__ float nv_team_sum<64>(float v, float* __restrict__) { return nro_wave_sum(v); }

template <> __device__ __forceinline__ float nv_team_excl_suffix_sum<NV_BLOCK>(float v, float behind, float* __restrict__ lds4, float& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float rs = nv_wave_excl_suffix_sum(v);
    __syncthreads();
    if (lane == 0) lds4[wave] = rs + v;                                  // the wave's total
    __syncthreads();
    float tot = 0.0f;
    #pragma unroll
    for (int wv = (int)(NV_BLOCK / 64) - 1; wv >= 0; wv--) { const float t = lds4[wv]; if (wv > wave) behind += t; tot += t; }
    total = tot;
    return behind + rs;
}

template <> __device__ __forceinline__ float nv_team_excl_suffix_sum<64>(float v, float behind, float* __restrict__, float& total) {
    const float rs = nv_wave_excl_suffix_sum(v);
    total = __shfl(rs + v, 0, 64);
    return behind + rs;
}

// alpha and the transmittance factor of one sample (:208-209); ex = exp(-delta scale sigma), the number alpha was rounded from
__device__ __forceinline__ void nv_alpha(float delta, float scale, float sigma, float& ex, float& alpha, float& keep) {
    ex = expf(-delta * scale * sigma);
    alpha = 1.0f - ex;
    keep = 1.0f - alpha + 1e-15f;
}

// What the forward leaves for the backward, one record per sample, stored word-major ([word][N*T]: the lanes of a wave are consecutive
// samples, so every word is a coalesced 256-byte store): the density net's 16 outputs, its ReLU mask, exp(-delta scale sigma) and the
// transmittance in front of the sample, the colour and the colour net's two ReLU masks.  108 bytes per sample (57 MB for 1,024 rays x 512 steps)
// instead of recomputing two encoder passes and both networks in the backward.
static constexpr uint32_t NV_REC_WORDS = 27;
// NV_R_EX and not alpha: alpha = 1 - ex is recomputed from it bit for bit, but ex cannot be recovered from alpha -- 1 - alpha has an ABSOLUTE error of
// 2^-25, which for an opaque sample (ex = 1e-4) is 3e-4 of d alpha / d sigma = delta scale ex, and that sample is the one the ray's gradient hangs on
enum { NV_R_OUT = 0, NV_R_RELU = 16, NV_R_EX = 18, NV_R_TR = 19, NV_R_RGB = 20, NV_R_MA = 23, NV_R_MB = 25 };

// a 64-bit mask in two words of the record `q` (word stride NT)
__device__ __forceinline__ void nv_rec_put64(uint32_t* __restrict__ q, uint32_t word, size_t NT, uint64_t m) {
    q[word * NT] = (uint32_t)m; q[(word + 1) * NT] = (uint32_t)(m >> 32);
}
__device__ __forceinline__ uint64_t nv_rec_get64(const uint32_t* __restrict__ q, uint32_t word, size_t NT) {
    return (uint64_t)q[word * NT] | ((uint64_t)q[(word + 1) * NT] << 32);
}

struct nv_run_sums { float w, d, r, g, b; };                            // a lane's share of weights_sum, depth and the colour

// One sample of the run, forward, on one of the W lanes of its ray: density, alpha, the weight w = alpha T (returned) with the transmittance T = `carry` x
// the exclusive product over the lanes in front (nerf/renderer.py:206-210); `carry` moves on to the next chunk.  COLOUR: the record into word-major
// `save` at `at` (save null: nothing is kept), the colour net where the weight matters, and the lane's sums; without it the function ends at the weight.
// A lane that is not `live` computes along (the scans need every lane) and contributes alpha = 0, keep = 1: exact no-ops.
template <uint32_t W, bool COLOUR>
__device__ __forceinline__ float nv_run_sample_fwd(const nav_params& P, const nv_ray& ray, const nv_sample& s, bool live, float& carry, float* __restrict__ col,
                                                   float* __restrict__ lds4, uint32_t* __restrict__ save, size_t at, size_t NT, nv_run_sums& acc) {
    float x0, x1, x2;
    const bool inside = nv_normalise(P, s.px, s.py, s.pz, x0, x1, x2);
    float out[16];
    const uint64_t relu = nv_density_forward<NV_RUN_U, W>(P, inside, x0, x1, x2, col, out);
    float ex, alpha, keep;
    nv_alpha(s.znext_minus_z, P.density_scale, expf(out[0]), ex, alpha, keep);
    if (!live) { alpha = 0.0f; keep = 1.0f; }
    float total;
    const float Tr = carry * nv_team_excl_product<W>(keep, lds4, total);
    const float w = alpha * Tr;
    if (COLOUR) {
        uint32_t* q = save + at;
        if (save && live) {                                              // before the colour net, so that out[] dies here
            #pragma unroll
            for (int m = 0; m < 16; m++) q[(NV_R_OUT + m) * NT] = __float_as_uint(out[m]);
            nv_rec_put64(q, NV_R_RELU, NT, relu);
            q[NV_R_EX * NT] = __float_as_uint(ex); q[NV_R_TR * NT] = __float_as_uint(Tr);
        }
        float rgb[3] = {0.0f, 0.0f, 0.0f};
        uint64_t ma = 0, mb = 0;
        if (live && w > 1e-4f) {                                         // :217 colour only where the weight matters
            float geo[NV_GEO];
            #pragma unroll
            for (int m = 0; m < NV_GEO; m++) geo[m] = out[1 + m];
            nv_color_forward<W>(P, ray.dx, ray.dy, ray.dz, geo, col, rgb, ma, mb);
        }
        if (save && live) {
            q[NV_R_RGB * NT] = __float_as_uint(rgb[0]); q[(NV_R_RGB + 1) * NT] = __float_as_uint(rgb[1]); q[(NV_R_RGB + 2) * NT] = __float_as_uint(rgb[2]);
            nv_rec_put64(q, NV_R_MA, NT, ma);
            nv_rec_put64(q, NV_R_MB, NT, mb);
        }
        const float oz01 = fminf(fmaxf((s.z - ray.near) / ray.span, 0.0f), 1.0f);        // :225
        acc.w += w; acc.d += w * oz01; acc.r += w * rgb[0]; acc.g += w * rgb[1]; acc.b += w * rgb[2];
    }
    carry *= total;
    return w;
}

// the ray's weights_sum, depth and image from its lanes' sums (:241)
template <uint32_t W>
__device__ __forceinline__ void nv_run_write(const nav_run& R, uint32_t n, const nv_run_sums& acc, float* __restrict__ lds4, float* __restrict__ image,
                                             float* __restrict__ depth, float* __restrict__ weights_sum) {
    const float ws = nv_team_sum<W>(acc.w, lds4), dsum = nv_team_sum<W>(acc.d, lds4);
    const float r = nv_team_sum<W>(acc.r, lds4), g = nv_team_sum<W>(acc.g, lds4), b = nv_team_sum<W>(acc.b, lds4);
    if (threadIdx.x == 0) {                                              // a ray without a sample: ws = 0, so the image is bg bit for bit
        weights_sum[n] = ws;
        depth[n] = dsum;
        image[3ull * n] = r + (1.0f - ws) * R.bg[0];
        image[3ull * n + 1] = g + (1.0f - ws) * R.bg[1];
        image[3ull * n + 2] = b + (1.0f - ws) * R.bg[2];
    }
}

// colour net backward from the saved forward: grgb[3] = d L / d rgb  ->  ggeo[15], d L / d dir (added)
template <uint32_t S = NV_BLOCK>
__device__ __forceinline__ void nv_color_backward_saved(const nav_params& P, float dxr, float dyr, float dzr, const float (&rgb)[3], uint64_t mask_a,
                                                        uint64_t mask_b, const float (&grgb)[3], float* __restrict__ col, float (&ggeo)[NV_GEO],
                                                        float& gdx, float& gdy, float& gdz) {
    float go[3];
    #pragma unroll
    for (int c = 0; c < 3; c++) go[c] = grgb[c] * rgb[c] * (1.0f - rgb[c]);
    float g[NV_H];
    nv_park<S>(go, col);
    nv_matvec<3, NV_H, S>(P.v2, col, g);                                 // d L / d hb
    #pragma unroll
    for (int j = 0; j < NV_H; j++) col[j * S] = ((mask_b >> j) & 1ull) ? g[j] : 0.0f;
    nv_matvec<NV_H, NV_H, S>(P.v1, col, g);                              // d L / d ha
    #pragma unroll
    for (int k = 0; k < NV_H; k++) col[k * S] = ((mask_a >> k) & 1ull) ? g[k] : 0.0f;
    float gin[NV_CIN];
    nv_matvec<NV_H, NV_CIN, S>(P.v0, col, gin);                            // d L / d cat(SH, geo)
    float gsh[16];
    #pragma unroll
    for (int i = 0; i < 16; i++) gsh[i] = gin[i];
    #pragma unroll
    for (int i = 0; i < NV_GEO; i++) ggeo[i] = gin[16 + i];
    float sx, sy, sz;
    nv_sh_backward(P, dxr, dyr, dzr, gsh, sx, sy, sz);
    gdx += sx; gdy += sy; gdz += sz;
}

struct nv_run_gout { float i0, i1, i2, d, w; };                         // d L / d image, depth, weights_sum of the ray
struct nv_ray_grads { float o0, o1, o2, dx, dy, dz; };                  // a lane's share of d L / d rays_o, d L / d rays_d

__device__ __forceinline__ nv_run_gout nv_run_gout_load(uint32_t n, const float* __restrict__ gimage, const float* __restrict__ gdepth,
                                                        const float* __restrict__ gws) {
    return {gimage[3ull * n], gimage[3ull * n + 1], gimage[3ull * n + 2], gdepth ? gdepth[n] : 0.0f, gws ? gws[n] : 0.0f};
}

// One sample of the run, backward, from its record `q` (that of any sample of the ray for a lane that is not `live`).  The chunks run back to front:
// d L / d sigma_i needs the sum over the samples BEHIND i, which `suffix` carries from chunk to chunk.
template <uint32_t W>
__device__ __forceinline__ void nv_run_sample_bwd(const nav_params& P, const nav_run& R, const nv_ray& ray, const nv_run_gout& g, const nv_sample& s, bool live,
                                                  float& suffix, float* __restrict__ col, float* __restrict__ lds4, const uint32_t* __restrict__ q, size_t NT,
                                                  nv_ray_grads& acc) {
    const float ex = live ? __uint_as_float(q[NV_R_EX * NT]) : 1.0f, Tr = live ? __uint_as_float(q[NV_R_TR * NT]) : 0.0f;
    const float alpha = 1.0f - ex;                                       // the forward's own alpha
    const float rgb[3] = {__uint_as_float(q[NV_R_RGB * NT]), __uint_as_float(q[(NV_R_RGB + 1) * NT]), __uint_as_float(q[(NV_R_RGB + 2) * NT])};
    const float w = alpha * Tr;
    const bool masked = live && w > 1e-4f;
    const float oz01 = fminf(fmaxf((s.z - ray.near) / ray.span, 0.0f), 1.0f);
    // A_i = d L / d w_i : image (colour minus background), depth, weights_sum
    const float A = live ? (g.i0 * (rgb[0] - R.bg[0]) + g.i1 * (rgb[1] - R.bg[1]) + g.i2 * (rgb[2] - R.bg[2]) + g.d * oz01 + g.w) : 0.0f;
    float chunk_total;
    const float S = nv_team_excl_suffix_sum<W>(A * w, suffix, lds4, chunk_total);        // sum over k > i of A_k w_k
    suffix += chunk_total;
    // w_i = alpha_i T_i, T_k (k > i) carries the factor (1 - alpha_i + eps):
    //   d L / d alpha_i = A_i T_i - S_i / (1 - alpha_i + eps);   d alpha_i / d sigma_i = delta_i scale exp(-delta_i scale sigma_i)
    // S_i / keep_i with the forward's own (rounded) keep: every T behind i carries that factor, so the quotient does not see its rounding
    const float keep = 1.0f - alpha + 1e-15f;
    const float gsigma = live ? s.znext_minus_z * P.density_scale * ex * (A * Tr - S / keep) : 0.0f;

    float gout[16];
    #pragma unroll
    for (int m = 0; m < 16; m++) gout[m] = 0.0f;
    if (masked) {
        float ggeo[NV_GEO];
        const uint64_t ma = nv_rec_get64(q, NV_R_MA, NT), mb = nv_rec_get64(q, NV_R_MB, NT);
        const float grgb[3] = {g.i0 * w, g.i1 * w, g.i2 * w};
        nv_color_backward_saved<W>(P, ray.dx, ray.dy, ray.dz, rgb, ma, mb, grgb, col, ggeo, acc.dx, acc.dy, acc.dz);
        #pragma unroll
        for (int m = 0; m < NV_GEO; m++) gout[1 + m] = ggeo[m];
    }
    gout[0] = gsigma * nv_exp_clamped(__uint_as_float(q[NV_R_OUT * NT]));
    const uint64_t relu = nv_rec_get64(q, NV_R_RELU, NT);
    float x0, x1, x2;
    const bool inside = nv_normalise(P, s.px, s.py, s.pz, x0, x1, x2);
    float gx, gy, gz;
    nv_density_backward<NV_RUN_U, W>(P, inside, x0, x1, x2, relu, gout, col, gx, gy, gz);
    if (!live) { gx = 0.0f; gy = 0.0f; gz = 0.0f; }
    gx *= s.bx; gy *= s.by; gz *= s.bz;                                  // clipped coordinates pass no (or half the) gradient (:159)
    acc.o0 += gx; acc.o1 += gy; acc.o2 += gz;
    acc.dx = __builtin_fmaf(s.z, gx, acc.dx); acc.dy = __builtin_fmaf(s.z, gy, acc.dy); acc.dz = __builtin_fmaf(s.z, gz, acc.dz);
}

template <uint32_t W>
__device__ __forceinline__ void nv_run_write_grads(uint32_t n, const nv_ray_grads& acc, float* __restrict__ lds4, float* __restrict__ grays_o,
                                                   float* __restrict__ grays_d) {
    const float a0 = nv_team_sum<W>(acc.o0, lds4), a1 = nv_team_sum<W>(acc.o1, lds4), a2 = nv_team_sum<W>(acc.o2, lds4);
    const float b0 = nv_team_sum<W>(acc.dx, lds4), b1 = nv_team_sum<W>(acc.dy, lds4), b2 = nv_team_sum<W>(acc.dz, lds4);
    if (threadIdx.x == 0) {                                              // a ray without a sample: exact zeros
        grays_o[3ull * n] = a0; grays_o[3ull * n + 1] = a1; grays_o[3ull * n + 2] = a2;
        grays_d[3ull * n] = b0; grays_d[3ull * n + 1] = b1; grays_d[3ull * n + 2] = b2;
    }
}

// ---- the dense run and the run over a depth list: one 256-thread workgroup per ray, a lane's sample = its place in the lattice chunk ----

template <bool AT>
__global__ __launch_bounds__(NV_BLOCK) void k_nav_run_fwd(nav_params P, nav_run R, float* __restrict__ image, float* __restrict__ depth,
                                                          float* __restrict__ weights_sum, uint32_t* __restrict__ save, nav_at Z) {
    extern __shared__ float nv_smem[];
    float* lds4 = nv_smem;                                              // 16 floats of scan scratch
    float* col = nv_smem + 16 + threadIdx.x;                            // this lane's column of the [64][256] scratch
    const uint32_t n = blockIdx.x;
    const size_t NT = (size_t)R.N * R.T;
    const nv_ray ray = nv_ray_load(R, n);
    const float* zrow = AT ? Z.z + (size_t)n * R.T : nullptr;
    float carry = 1.0f;
    nv_run_sums acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t c0 = 0; c0 < R.T; c0 += NV_BLOCK) {
        const uint32_t i = c0 + threadIdx.x;
        const bool live = i < R.T;
        const nv_sample s = nv_sample_at<AT>(R, live ? i : R.T - 1, ray, zrow, Z.dist);
        nv_run_sample_fwd<NV_BLOCK, true>(P, ray, s, live, carry, col, lds4, save, (size_t)n * R.T + i, NT, acc);
    }
    nv_run_write<NV_BLOCK>(R, n, acc, lds4, image, depth, weights_sum);
}

template <bool AT>
__global__ __launch_bounds__(NV_BLOCK) void k_nav_run_bwd(nav_params P, nav_run R, const float* __restrict__ gimage, const float* __restrict__ gdepth,
                                                          const float* __restrict__ gws, const uint32_t* __restrict__ save,
                                                          float* __restrict__ grays_o, float* __restrict__ grays_d, nav_at Z) {
    extern __shared__ float nv_smem[];
    float* lds4 = nv_smem;
    float* col = nv_smem + 16 + threadIdx.x;
    const uint32_t n = blockIdx.x;
    const size_t NT = (size_t)R.N * R.T;
    const nv_ray ray = nv_ray_load(R, n);
    const float* zrow = AT ? Z.z + (size_t)n * R.T : nullptr;
    const nv_run_gout g = nv_run_gout_load(n, gimage, gdepth, gws);
    const uint32_t nchunks = (R.T + NV_BLOCK - 1) / NV_BLOCK;
    float suffix = 0.0f;
    nv_ray_grads acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t cc = nchunks; cc-- > 0;) {
        const uint32_t i = cc * NV_BLOCK + threadIdx.x;
        const bool live = i < R.T;
        const uint32_t ic = live ? i : R.T - 1;
        const nv_sample s = nv_sample_at<AT>(R, ic, ray, zrow, Z.dist);
        nv_run_sample_bwd<NV_BLOCK>(P, R, ray, g, s, live, suffix, col, lds4, save + (size_t)n * R.T + ic, NT, acc);
    }
    nv_run_write_grads<NV_BLOCK>(n, acc, lds4, grays_o, grays_d);
}

// ---------------------------------------------------------------------------
// The same run with the occupancy grid consulted (DESIGN.md §3.5 "Occupancy-masked pose filter"): the sigma of every lattice sample whose occupancy bit
// is clear is zero.  Such a sample has alpha = 0 and keep = 1 - 0 + 1e-15f = 1.0f exactly, so it drops out of every sum and of the transmittance product
// without a rounding, and the kernels below never evaluate the field there: per ray they walk the T lattice positions (one bitfield byte each), compact
// the indices of the occupied ones in lattice order, and run nv_run_sample_fwd / _bwd over that list only.  Everything else is the dense
// run's: nears, fars, nv_lin, the clipped positions, the deltas of the LATTICE (not merged over the gaps), the colour mask, depth and background.
//
// The bit of a sample is that of its clipped float32 position under the march's own cell arithmetic, ngp_point::at (ngp_march.h), through a view whose
// "ray" is the position itself (origin = position, direction 0, parameter 0) and whose step is 0, which leaves the step's cascade out: level = mip of
// the position alone.  The mask is a constant of the float32 position: no gradient flows through it.
//
// Shape: ONE WAVE PER RAY (workgroup = 64 lanes, the W = 64 team).  With ~45 live samples per ray three of k_nav_run_*'s four waves would idle; here the
// activation scratch is [64][64] floats = 16 KB plus the list (T x 2 B <= 8 KB), and the single barrier (list written, list read) is a wave barrier.
// No atomics; a ray's outputs depend on nothing but the ray; two runs give the same bits.
// ---------------------------------------------------------------------------
static constexpr uint32_t NO_W = 64;                                     // lanes per ray = the chunk width of the compacted list

struct nav_occ { const uint8_t* bits; uint32_t H3; int Cm1; float rbound, hHf, Hm1; };

struct nro_view {                                                        // what ngp_point<V>::at reads (ngp_march.h)
    static constexpr bool pow2_grid = true;
    float ox, oy, oz, dx, dy, dz, bound, rbound, dt_gamma, dt_min, dt_max, hHf, Hm1;
    int Cm1;
    __device__ __forceinline__ int mip(int e) const { return e < 0 ? 0 : (e > Cm1 ? Cm1 : e); }
};

__device__ __forceinline__ bool nro_occupied(const nav_occ& G, float bound, float px, float py, float pz) {
    nro_view m;
    m.ox = px; m.oy = py; m.oz = pz; m.dx = 0.0f; m.dy = 0.0f; m.dz = 0.0f;
    m.bound = bound; m.rbound = G.rbound; m.dt_gamma = 0.0f; m.dt_min = 0.0f; m.dt_max = 0.0f;      // step 0: frexp exponent 0, cascade 0
    m.hHf = G.hHf; m.Hm1 = G.Hm1; m.Cm1 = G.Cm1;
    ngp_point<nro_view> p;
    p.at(m, 0.0f);
    const uint32_t bit = (uint32_t)p.level * G.H3 + ngp_morton3((uint32_t)p.nx, (uint32_t)p.ny, (uint32_t)p.nz);   // < C H^3 <= 2^32 (host check)
    return (G.bits[bit >> 3] >> (bit & 7u)) & 1u;
}

// what the forward leaves besides the records: the ray's count and its list, so that the backward walks the same samples.  Record j of ray n (the j-th
// occupied sample) sits where the dense run keeps sample j: word-major at n T + j
struct nro_kept { uint32_t* save; uint32_t* counts; uint16_t* lists; };

__global__ __launch_bounds__(NO_W) void k_nav_run_occ_fwd(nav_params P, nav_run R, nav_occ G, float* __restrict__ image, float* __restrict__ depth,
                                                          float* __restrict__ weights_sum, uint32_t* __restrict__ counts_out, nro_kept K) {
    extern __shared__ float nv_smem[];
    const uint32_t lane = threadIdx.x;
    float* col = nv_smem + lane;                                         // this lane's column of the [64][64] scratch
    uint16_t* list = reinterpret_cast<uint16_t*>(nv_smem + NV_H * NO_W); // [T]
    const uint32_t n = blockIdx.x;
    const size_t NT = (size_t)R.N * R.T;
    const nv_ray ray = nv_ray_load(R, n);

    // ---- the lattice walk: position and one bitfield byte per sample; the occupied indices, in lattice order, by ballot and prefix count ----
    uint32_t count = 0;
    for (uint32_t c0 = 0; c0 < R.T; c0 += NO_W) {
        const uint32_t i = c0 + lane;
        const bool live = i < R.T;
        const nv_sample s = nv_sample_at(R, live ? i : R.T - 1, ray);
        const bool occ = live && nro_occupied(G, P.bound, s.px, s.py, s.pz);
        const unsigned long long m = __ballot(occ);
        if (occ) list[count + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)i;       // < count + popc(m) <= T
        count += (uint32_t)__popcll(m);                                  // wave-uniform
    }
    __syncthreads();                                                     // one wave: the list is written before it is read

    float carry = 1.0f;
    nv_run_sums acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t j0 = 0; j0 < count; j0 += NO_W) {                      // a lane's sample = entry j of the list
        const uint32_t j = j0 + lane;
        const bool live = j < count;
        const uint32_t i = list[live ? j : count - 1];
        const nv_sample s = nv_sample_at(R, i, ray);
        if (K.save && live) K.lists[(size_t)n * R.T + j] = (uint16_t)i;
        nv_run_sample_fwd<NO_W, true>(P, ray, s, live, carry, col, nullptr, K.save, (size_t)n * R.T + j, NT, acc);
    }
    nv_run_write<NO_W>(R, n, acc, nullptr, image, depth, weights_sum);
    if (lane == 0) {
        if (K.save) K.counts[n] = count;
        if (counts_out) counts_out[n] = count;
    }
}

__global__ __launch_bounds__(NO_W) void k_nav_run_occ_bwd(nav_params P, nav_run R, const float* __restrict__ gimage, const float* __restrict__ gdepth,
                                                          const float* __restrict__ gws, nro_kept K, float* __restrict__ grays_o,
                                                          float* __restrict__ grays_d) {
    extern __shared__ float nv_smem[];
    const uint32_t lane = threadIdx.x;
    float* col = nv_smem + lane;
    const uint32_t n = blockIdx.x;
    const size_t NT = (size_t)R.N * R.T;
    const nv_ray ray = nv_ray_load(R, n);
    const nv_run_gout g = nv_run_gout_load(n, gimage, gdepth, gws);
    const uint32_t stored = K.counts[n];
    const uint32_t count = stored < R.T ? stored : R.T;                  // the forward's own number; the clamp keeps a foreign buffer inside the ray's slice
    const uint32_t nchunks = (count + NO_W - 1) / NO_W;
    const uint16_t* list = K.lists + (size_t)n * R.T;

    float suffix = 0.0f;                                                 // over the occupied samples behind; the others' w is zero
    nv_ray_grads acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t cc = nchunks; cc-- > 0;) {
        const uint32_t j = cc * NO_W + lane;
        const bool live = j < count;
        const uint32_t jc = live ? j : count - 1;
        const uint32_t listed = list[jc];
        const uint32_t i = listed < R.T ? listed : R.T - 1;
        const nv_sample s = nv_sample_at(R, i, ray);
        nv_run_sample_bwd<NO_W>(P, R, ray, g, s, live, suffix, col, nullptr, K.save + (size_t)n * R.T + jc, NT, acc);
    }
    nv_run_write_grads<NO_W>(n, acc, nullptr, grays_o, grays_d);
}

// ---------------------------------------------------------------------------
// The resampled run (DESIGN.md §3.5 "Resampled run"; include/ngp_hip.h states the contract): NeRFRenderer.run's upsample_steps > 0 branch
// (nerf/renderer.py:172-204) with sample_pdf's deterministic branch (:12-46).
//
//   k_nav_resample   one 256-thread workgroup per ray: the coarse pass = nv_run_sample_fwd without the colour net (the weights stay in LDS), the cdf of
//                    w[1 : Nc - 1], one binary search per new sample, two rank searches for the merge; writes the merged depth list z [N, T]
//   k_sample_pdf     the same device functions on caller-given bins / weights (and uniforms): the piece a host restatement reproduces bit for bit
//   k_nav_run_fwd<true> / _bwd<true> then run over z (nv_sample_at<true>).
//
// The two sums of sample_pdf (the normaliser and the cumulative sum) are taken in 64-bit FIXED POINT, 2^-40 per unit: w + 1e-5 >= 2^-17 is a multiple
// of 2^-40 in float32, so the conversion is exact, integer addition is associative, and any scan order gives the same cdf -- which a numpy restatement
// reproduces from the same float32 weights.  cdf_k = (float)((double) P_k / (double) S): cdf_0 = 0 and the last entry is 1 exactly.
// No atomics; the ray's outputs depend on nothing but the ray.
// ---------------------------------------------------------------------------
struct nv_pdf_u { float s, e, step; };                                   // linspace(0.5 / n, 1 - 0.5 / n, n): start, end, step (float32, ATen's rule)
static constexpr size_t NV_PDF_SCAN_BYTES = 32;                          // one 64-bit total per wave

static nv_pdf_u nv_pdf_u_of(uint32_t n) {
    nv_pdf_u U;
    U.s = (float)(0.5 / (double)n);
    U.e = (float)(1.0 - 0.5 / (double)n);
    U.step = n > 1 ? (U.e - U.s) / (float)(n - 1) : 0.0f;
    return U;
}

__device__ __forceinline__ float nv_pdf_u_at(const nv_pdf_u& U, uint32_t j, uint32_t n) {
    if (n < 2) return U.s;
    return j < n / 2 ? __builtin_fmaf(U.step, (float)j, U.s) : __builtin_fmaf(-U.step, (float)(n - 1 - j), U.e);
}

__device__ __forceinline__ long long nv_pdf_fixed(float w) {
    const float v = w + 1e-5f;                                           // :19
    if (!(v >= 0.0f)) return 0;                                          // negative or NaN
    return __float2ll_rn(fminf(v, 1024.0f) * 1099511627776.0f);          // 2^40: the product is exact
}

// cdf [Tb] (LDS) from the Tb - 1 weights w[] (LDS or global); `scan`: NV_PDF_SCAN_BYTES of LDS.  Every thread of the 256 calls it; thread t owns a
// contiguous run of weights, the runs' totals are scanned by shuffles and the four wave totals through LDS.  Ends with a barrier: cdf is readable.
__device__ __forceinline__ void nv_pdf_cdf(const float* __restrict__ w, uint32_t Tb, float* __restrict__ cdf, long long* __restrict__ scan) {
    const uint32_t nb = Tb - 1, per = (nb + NV_BLOCK - 1) / NV_BLOCK;
    const uint32_t k0 = min(threadIdx.x * per, nb), k1 = min(k0 + per, nb);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long own = 0;
    for (uint32_t k = k0; k < k1; k++) own += nv_pdf_fixed(w[k]);
    long long incl = own;
    #pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const long long up = __shfl_up(incl, off, 64); if (lane >= off) incl += up; }
    __syncthreads();
    if (lane == 63) scan[wave] = incl;
    __syncthreads();
    long long base = 0, S = 0;
    #pragma unroll
    for (int v = 0; v < (int)(NV_BLOCK / 64); v++) { const long long t = scan[v]; if (v < wave) base += t; S += t; }
    long long Pk = base + (incl - own);
    if (threadIdx.x == 0) cdf[0] = 0.0f;
    for (uint32_t k = k0; k < k1; k++) {
        Pk += nv_pdf_fixed(w[k]);
        cdf[k + 1] = S > 0 ? (float)((double)Pk / (double)S) : 0.0f;
    }
    __syncthreads();
}

// one new depth: searchsorted(cdf, u, right = True), the two clamps, the guarded quotient and the interpolation (:32-44); bins(k) = the k-th bin edge
template <class Bins>
__device__ __forceinline__ float nv_pdf_invert(const float* __restrict__ cdf, uint32_t Tb, float u, Bins bins) {
    uint32_t a = 0, b = Tb;                                              // cdf[k] <= u below a, > u from b on
    while (a < b) { const uint32_t m = (a + b) >> 1; if (cdf[m] <= u) a = m + 1; else b = m; }
    const uint32_t lo = a > 0 ? a - 1 : 0, hi = a < Tb - 1 ? a : Tb - 1;
    const float c0 = cdf[lo];
    float denom = cdf[hi] - c0;
    if (denom < 1e-5f) denom = 1.0f;
    const float t = (u - c0) / denom;
    const float b0 = bins(lo), b1 = bins(hi);
    return fminf(b0 + t * (b1 - b0), b1);                                // the min: see the contract (one ulp past the bin's edge at most)
}

__global__ __launch_bounds__(NV_BLOCK) void k_sample_pdf(const float* __restrict__ bins, const float* __restrict__ weights, uint32_t Tb,
                                                         const float* __restrict__ u, uint32_t n, nv_pdf_u U, float* __restrict__ out) {
    extern __shared__ float nv_smem[];
    long long* scan = reinterpret_cast<long long*>(nv_smem);
    float* cdf = nv_smem + NV_PDF_SCAN_BYTES / sizeof(float);           // [Tb]
    const size_t row = blockIdx.x;
    const float* b = bins + row * Tb;
    nv_pdf_cdf(weights + row * (Tb - 1), Tb, cdf, scan);
    for (uint32_t j = threadIdx.x; j < n; j += NV_BLOCK) {
        const float uj = u ? u[row * n + j] : nv_pdf_u_at(U, j, n);
        out[row * n + j] = nv_pdf_invert(cdf, Tb, uj, [b](uint32_t k) { return b[k]; });
    }
}

// dynamic LDS of k_nav_resample: k_nav_run_fwd's scratch, then the Nc coarse weights.  The cdf [Nc - 1] and the new depths [Nf] reuse the column scratch,
// which is free once the coarse pass is over (8 + 4096 + 4096 floats of its 16384)
static size_t nv_resample_lds(uint32_t Nc) { return sizeof(float) * (16 + NV_H * NV_BLOCK + (size_t)Nc); }

__global__ __launch_bounds__(NV_BLOCK) void k_nav_resample(nav_params P, nav_run R, uint32_t Nf, nv_pdf_u U, float* __restrict__ zout,
                                                           float* __restrict__ wout) {
    extern __shared__ float nv_smem[];
    float* lds4 = nv_smem;
    float* col = nv_smem + 16 + threadIdx.x;
    float* wts = nv_smem + 16 + NV_H * NV_BLOCK;                         // [Nc]
    long long* scan = reinterpret_cast<long long*>(nv_smem + 16);
    float* cdf = nv_smem + 16 + NV_PDF_SCAN_BYTES / sizeof(float);      // [Nc - 1]
    float* znew = cdf + 4096;                                            // [Nf]
    const uint32_t n = blockIdx.x, Nc = R.T, T = Nc + Nf;
    const nv_ray ray = nv_ray_load(R, n);
    const float near = ray.near, span = ray.span;

    // ---- the coarse pass: the run's forward down to the weight ----
    float carry = 1.0f;
    nv_run_sums unused = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t c0 = 0; c0 < Nc; c0 += NV_BLOCK) {
        const uint32_t i = c0 + threadIdx.x;
        const bool live = i < Nc;
        const nv_sample s = nv_sample_at(R, live ? i : Nc - 1, ray);
        const float w = nv_run_sample_fwd<NV_BLOCK, false>(P, ray, s, live, carry, col, lds4, nullptr, 0, 0, unused);
        if (live) {
            wts[i] = w;
            if (wout) wout[(size_t)n * Nc + i] = w;
        }
    }
    __syncthreads();                                                     // the weights are written; the column scratch is free

    // ---- sample_pdf over w[1 : Nc - 1] and the mid points ----
    nv_pdf_cdf(wts + 1, Nc - 1, cdf, scan);
    const auto zc = [near, span, Nc](uint32_t i) { return near + span * nv_lin(i, Nc); };       // nv_sample_at's z, the same bits
    const auto bin = [&zc](uint32_t k) { const float z0 = zc(k); return z0 + 0.5f * (zc(k + 1) - z0); };      // :183
    for (uint32_t j = threadIdx.x; j < Nf; j += NV_BLOCK) znew[j] = nv_pdf_invert(cdf, Nc - 1, nv_pdf_u_at(U, j, Nf), bin);
    __syncthreads();

    // ---- the merge: the stable sort of cat(z, z_new) by ranks; both lists are non-decreasing ----
    float* zr = zout + (size_t)n * T;
    for (uint32_t i = threadIdx.x; i < Nc; i += NV_BLOCK) {
        const float zi = zc(i);
        uint32_t a = 0, b = Nf;                                          // #{j : z_new_j < z_i}
        while (a < b) { const uint32_t m = (a + b) >> 1; if (znew[m] < zi) a = m + 1; else b = m; }
        zr[i + a] = zi;                                                  // i + a <= Nc - 1 + Nf
    }
    for (uint32_t j = threadIdx.x; j < Nf; j += NV_BLOCK) {
        const float v = znew[j];
        uint32_t a = 0, b = Nc;                                          // #{i : z_i <= z_new_j}
        while (a < b) { const uint32_t m = (a + b) >> 1; if (zc(m) <= v) a = m + 1; else b = m; }
        zr[j + a] = v;                                                   // j + a <= Nf - 1 + Nc
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_nav_transpose(const float* __restrict__ src, uint32_t rows, uint32_t cols, float* __restrict__ dst) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * cols) return;
    const uint32_t r = t / cols, c = t - r * cols;
    dst[c * rows + r] = src[t];
}

extern "C" size_t ngp_nav_field_workspace(void) { return nav_prep_layout(nullptr).total; }

// transposed copies of the five weight matrices into `workspace`; call again whenever the weights change
extern "C" int ngp_nav_field_prepare(const ngp_nav_field_t* f, void* workspace, size_t workspace_bytes, void* stream) {
    nav_params P;                                  // the queries' own checks: a field they would refuse is refused when it is set up
    { const int rc = nav_fill("nav_field_prepare", f, workspace, P); if (rc != NGP_OK) return rc; }
    NGP_REQUIRE(workspace_bytes >= ngp_nav_field_workspace(), "nav_field_prepare: bad argument");
    const nav_prep_ws w = nav_prep_layout(workspace);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_nav_transpose, dim3(8), dim3(256), 0, st, f->sigma_w0, 64u, 32u, w.w1t);
    hipLaunchKernelGGL(k_nav_transpose, dim3(4), dim3(256), 0, st, f->sigma_w1, 16u, 64u, w.w2t);
    hipLaunchKernelGGL(k_nav_transpose, dim3(8), dim3(256), 0, st, f->color_w0, 64u, 31u, w.v0t);
    hipLaunchKernelGGL(k_nav_transpose, dim3(16), dim3(256), 0, st, f->color_w1, 64u, 64u, w.v1t);
    hipLaunchKernelGGL(k_nav_transpose, dim3(1), dim3(256), 0, st, f->color_w2, 3u, 64u, w.v2t);
    NGP_CHECK_LAUNCH("nav_field_prepare");
    return NGP_OK;
}

// the kernels use slightly more than the default 64 KiB of dynamic LDS; the raised limit is a per-device function attribute
static int nav_allow_big_lds() {
    static std::atomic<unsigned long long> devices{0};
    const int rc = ngp_allow_dynamic_lds(devices, {(const void*)k_nav_density_fwd, (const void*)k_nav_density_bwd, (const void*)k_nav_run_fwd<false>,
                                                   (const void*)k_nav_run_bwd<false>, (const void*)k_nav_density_vj,
                                                   (const void*)k_nav_run_fwd<true>, (const void*)k_nav_run_bwd<true>, (const void*)k_nav_resample}, 160 * 1024);
    if (rc == NGP_LDS_NO_DEVICE) return ngp_fail(NGP_ELAUNCH, "nav: no current device");
    if (rc != NGP_LDS_OK) return ngp_fail(NGP_ELAUNCH, "nav: cannot raise the dynamic LDS limit");
    return NGP_OK;
}

extern "C" int ngp_nav_density_forward(const ngp_nav_field_t* f, const void* prepared, const float* xyz, uint32_t M, float* sigma, float* geo,
                                       void* stream) {
    nav_params P;
    const int rc = nav_fill("nav_density_forward", f, prepared, P);
    if (rc != NGP_OK) return rc;
    if (M == 0) return NGP_OK;
    NGP_REQUIRE(xyz && sigma, "nav_density_forward: null pointer");
    { const int rc_lds = nav_allow_big_lds(); if (rc_lds != NGP_OK) return rc_lds; }
    hipLaunchKernelGGL(k_nav_density_fwd, dim3(ngp_div_up(M, NV_BLOCK)), dim3(NV_BLOCK), sizeof(float) * (16 + NV_H * NV_BLOCK), (hipStream_t)stream, P, xyz, M, sigma, geo);
    NGP_CHECK_LAUNCH("nav_density_forward");
    return NGP_OK;
}

extern "C" int ngp_nav_density_backward(const ngp_nav_field_t* f, const void* prepared, const float* xyz, uint32_t M, const float* grad_sigma,
                                        const float* grad_geo, float* grad_xyz, void* stream) {
    nav_params P;
    const int rc = nav_fill("nav_density_backward", f, prepared, P);
    if (rc != NGP_OK) return rc;
    if (M == 0) return NGP_OK;
    NGP_REQUIRE(xyz && grad_sigma && grad_xyz, "nav_density_backward: null pointer");
    { const int rc_lds = nav_allow_big_lds(); if (rc_lds != NGP_OK) return rc_lds; }
    hipLaunchKernelGGL(k_nav_density_bwd, dim3(ngp_div_up(M, NV_BLOCK)), dim3(NV_BLOCK), sizeof(float) * (16 + NV_H * NV_BLOCK), (hipStream_t)stream, P, xyz, M, grad_sigma, grad_geo, grad_xyz);
    NGP_CHECK_LAUNCH("nav_density_backward");
    return NGP_OK;
}

extern "C" int ngp_nav_density_value_jac(const ngp_nav_field_t* f, const void* prepared, const float* xyz, uint32_t M, const float* rot9_host, float* sigma,
                                         float* jac, void* stream) {
    nav_params P;
    const int rc = nav_fill("nav_density_value_jac", f, prepared, P);
    if (rc != NGP_OK) return rc;
    if (M == 0) return NGP_OK;
    NGP_REQUIRE(xyz && sigma && jac, "nav_density_value_jac: null pointer");
    nav_rot R;
    R.on = rot9_host ? 1u : 0u;
    for (int k = 0; k < 9; k++) R.m[k] = rot9_host ? rot9_host[k] : (k % 4 == 0 ? 1.0f : 0.0f);
    { const int rc_lds = nav_allow_big_lds(); if (rc_lds != NGP_OK) return rc_lds; }
    hipLaunchKernelGGL(k_nav_density_vj, dim3(ngp_div_up(M, NV_VJ_POINTS)), dim3(256), NV_VJ_LDS, (hipStream_t)stream, P, R, xyz, M, sigma, jac);
    NGP_CHECK_LAUNCH("nav_density_value_jac");
    return NGP_OK;
}

static ngp_array_ws<uint32_t> nav_saved_layout(uint32_t N, uint32_t num_steps, void* base) { return ngp_array_layout<uint32_t>(NV_REC_WORDS * (size_t)N * num_steps, base); }
extern "C" size_t ngp_nav_run_saved_bytes(uint32_t N, uint32_t num_steps) { return nav_saved_layout(N, num_steps, nullptr).total; }

static int nav_run_args(const char* who, const float* rays_o, const float* rays_d, const float* nears, const float* fars, uint32_t N, uint32_t T,
                        const float* aabb_host, const float* bg_host, nav_run& R) {
    NGP_REQUIRE(rays_o && rays_d && nears && fars && aabb_host, "%s: null pointer", who);
    NGP_REQUIRE(T >= 1 && T <= 4096, "%s: num_steps must be in [1, 4096]", who);
    R.rays_o = rays_o; R.rays_d = rays_d; R.nears = nears; R.fars = fars; R.N = N; R.T = T;
    for (int i = 0; i < 6; i++) R.aabb[i] = aabb_host[i];
    for (int i = 0; i < 3; i++) R.bg[i] = bg_host ? bg_host[i] : 1.0f;
    return NGP_OK;
}

// the dense run and the run over an explicit depth list share everything on the host but the kernel instantiation: z null = the linspace lattice
static int nav_run_forward_impl(const char* who, const ngp_nav_field_t* f, const void* prepared, const float* rays_o, const float* rays_d, const float* nears,
                                const float* fars, uint32_t N, uint32_t T, const float* aabb_host, const float* bg_color3_host, float* image, float* depth,
                                float* weights_sum, void* saved, size_t saved_bytes, const float* z, uint32_t dist_steps, void* stream) {
    nav_params P;
    int rc = nav_fill(who, f, prepared, P);
    if (rc != NGP_OK) return rc;
    if (N == 0) return NGP_OK;
    nav_run R;
    rc = nav_run_args(who, rays_o, rays_d, nears, fars, N, T, aabb_host, bg_color3_host, R);
    if (rc != NGP_OK) return rc;
    NGP_REQUIRE(image && depth && weights_sum, "%s: null output", who);
    const auto kept = nav_saved_layout(N, T, saved);
    NGP_REQUIRE(!saved || saved_bytes >= kept.total, "%s: `saved` is smaller than ngp_nav_run_saved_bytes(N, num_steps)", who);
    const size_t lds = sizeof(float) * (16 + NV_H * NV_BLOCK);
    { const int rc_lds = nav_allow_big_lds(); if (rc_lds != NGP_OK) return rc_lds; }
    const nav_at Z = {z, dist_steps};
    if (z) hipLaunchKernelGGL(k_nav_run_fwd<true>, dim3(N), dim3(NV_BLOCK), lds, (hipStream_t)stream, P, R, image, depth, weights_sum, kept.p, Z);
    else hipLaunchKernelGGL(k_nav_run_fwd<false>, dim3(N), dim3(NV_BLOCK), lds, (hipStream_t)stream, P, R, image, depth, weights_sum, kept.p, Z);
    NGP_CHECK_LAUNCH(who);
    return NGP_OK;
}

static int nav_run_backward_impl(const char* who, const ngp_nav_field_t* f, const void* prepared, const float* rays_o, const float* rays_d,
                                 const float* nears, const float* fars, uint32_t N, uint32_t T, const float* aabb_host, const float* bg_color3_host,
                                 const float* grad_image, const float* grad_depth, const float* grad_weights_sum, const void* saved, size_t saved_bytes,
                                 float* grad_rays_o, float* grad_rays_d, const float* z, uint32_t dist_steps, void* stream) {
    nav_params P;
    int rc = nav_fill(who, f, prepared, P);
    if (rc != NGP_OK) return rc;
    if (N == 0) return NGP_OK;
    nav_run R;
    rc = nav_run_args(who, rays_o, rays_d, nears, fars, N, T, aabb_host, bg_color3_host, R);
    if (rc != NGP_OK) return rc;
    NGP_REQUIRE(grad_image && grad_rays_o && grad_rays_d, "%s: null pointer", who);
    const auto kept = nav_saved_layout(N, T, const_cast<void*>(saved));
    NGP_REQUIRE(saved && saved_bytes >= kept.total, "%s: needs the `saved` buffer its forward filled", who);
    const size_t lds = sizeof(float) * (16 + NV_H * NV_BLOCK);
    { const int rc_lds = nav_allow_big_lds(); if (rc_lds != NGP_OK) return rc_lds; }
    const nav_at Z = {z, dist_steps};
    if (z) hipLaunchKernelGGL(k_nav_run_bwd<true>, dim3(N), dim3(NV_BLOCK), lds, (hipStream_t)stream, P, R, grad_image, grad_depth, grad_weights_sum,
                              (const uint32_t*)kept.p, grad_rays_o, grad_rays_d, Z);
    else hipLaunchKernelGGL(k_nav_run_bwd<false>, dim3(N), dim3(NV_BLOCK), lds, (hipStream_t)stream, P, R, grad_image, grad_depth, grad_weights_sum,
                            (const uint32_t*)kept.p, grad_rays_o, grad_rays_d, Z);
    NGP_CHECK_LAUNCH(who);
    return NGP_OK;
}

extern "C" int ngp_nav_run_forward(const ngp_nav_field_t* f, const void* prepared, const float* rays_o, const float* rays_d, const float* nears,
                                   const float* fars, uint32_t N, uint32_t num_steps, const float* aabb_host, const float* bg_color3_host,
                                   float* image, float* depth, float* weights_sum, void* saved, size_t saved_bytes, void* stream) {
    return nav_run_forward_impl("nav_run_forward", f, prepared, rays_o, rays_d, nears, fars, N, num_steps, aabb_host, bg_color3_host, image, depth,
                                weights_sum, saved, saved_bytes, nullptr, num_steps, stream);
}

extern "C" int ngp_nav_run_backward(const ngp_nav_field_t* f, const void* prepared, const float* rays_o, const float* rays_d, const float* nears,
                                    const float* fars, uint32_t N, uint32_t num_steps, const float* aabb_host, const float* bg_color3_host,
                                    const float* grad_image, const float* grad_depth, const float* grad_weights_sum, const void* saved,
                                    size_t saved_bytes, float* grad_rays_o, float* grad_rays_d, void* stream) {
    return nav_run_backward_impl("nav_run_backward", f, prepared, rays_o, rays_d, nears, fars, N, num_steps, aabb_host, bg_color3_host, grad_image,
                                 grad_depth, grad_weights_sum, saved, saved_bytes, grad_rays_o, grad_rays_d, nullptr, num_steps, stream);
}

// ---- the resampled run (DESIGN.md §3.5 "Resampled run") ----

extern "C" int ngp_nav_run_at_forward(const ngp_nav_field_t* f, const void* prepared, const float* rays_o, const float* rays_d, const float* nears,
                                      const float* fars, uint32_t N, uint32_t T, const float* aabb_host, const float* bg_color3_host, float* image,
                                      float* depth, float* weights_sum, void* saved, size_t saved_bytes, const float* z, uint32_t dist_steps, void* stream) {
    NGP_REQUIRE(z, "nav_run_at_forward: null depth list z");
    NGP_REQUIRE(dist_steps >= 1, "nav_run_at_forward: dist_steps must be >= 1");
    return nav_run_forward_impl("nav_run_at_forward", f, prepared, rays_o, rays_d, nears, fars, N, T, aabb_host, bg_color3_host, image, depth, weights_sum,
                                saved, saved_bytes, z, dist_steps, stream);
}

extern "C" int ngp_nav_run_at_backward(const ngp_nav_field_t* f, const void* prepared, const float* rays_o, const float* rays_d, const float* nears,
                                       const float* fars, uint32_t N, uint32_t T, const float* aabb_host, const float* bg_color3_host,
                                       const float* grad_image, const float* grad_depth, const float* grad_weights_sum, const void* saved,
                                       size_t saved_bytes, float* grad_rays_o, float* grad_rays_d, const float* z, uint32_t dist_steps, void* stream) {
    NGP_REQUIRE(z, "nav_run_at_backward: null depth list z");
    NGP_REQUIRE(dist_steps >= 1, "nav_run_at_backward: dist_steps must be >= 1");
    return nav_run_backward_impl("nav_run_at_backward", f, prepared, rays_o, rays_d, nears, fars, N, T, aabb_host, bg_color3_host, grad_image, grad_depth,
                                 grad_weights_sum, saved, saved_bytes, grad_rays_o, grad_rays_d, z, dist_steps, stream);
}

// the shape of a resampled run; with N = 0 ngp_nav_run_resample judges field, shape and z and queues nothing (nav_filter.hip asks that way)
static int nav_resample_shape(const char* who, uint32_t num_steps, uint32_t upsample_steps) {
    NGP_REQUIRE(num_steps >= 3, "%s: num_steps = %u; the resampled run needs num_steps >= 3", who, num_steps);
    NGP_REQUIRE(upsample_steps >= 1, "%s: upsample_steps = 0; use the dense entry point", who);
    NGP_REQUIRE((uint64_t)num_steps + upsample_steps <= 4096, "%s: num_steps + upsample_steps = %u + %u; supported <= 4096", who, num_steps, upsample_steps);
    return NGP_OK;
}

extern "C" int ngp_nav_run_resample(const ngp_nav_field_t* f, const void* prepared, const float* rays_o, const float* rays_d, const float* nears,
                                    const float* fars, uint32_t N, uint32_t num_steps, uint32_t upsample_steps, const float* aabb_host, float* z,
                                    float* coarse_weights, void* stream) {
    nav_params P;
    int rc = nav_fill("nav_run_resample", f, prepared, P);
    if (rc != NGP_OK) return rc;
    rc = nav_resample_shape("nav_run_resample", num_steps, upsample_steps);
    if (rc != NGP_OK) return rc;
    NGP_REQUIRE(z, "nav_run_resample: null depth list z");
    if (N == 0) return NGP_OK;
    nav_run R;
    rc = nav_run_args("nav_run_resample", rays_o, rays_d, nears, fars, N, num_steps, aabb_host, nullptr, R);
    if (rc != NGP_OK) return rc;
    { const int rc_lds = nav_allow_big_lds(); if (rc_lds != NGP_OK) return rc_lds; }
    const nv_pdf_u U = nv_pdf_u_of(upsample_steps);
    hipLaunchKernelGGL(k_nav_resample, dim3(N), dim3(NV_BLOCK), nv_resample_lds(num_steps), (hipStream_t)stream, P, R, upsample_steps, U, z, coarse_weights);
    NGP_CHECK_LAUNCH("nav_run_resample");
    return NGP_OK;
}

extern "C" int ngp_sample_pdf(const float* bins, const float* weights, uint32_t N, uint32_t Tb, const float* u, uint32_t n, float* out, void* stream) {
    NGP_REQUIRE(Tb >= 2 && Tb <= 4096, "sample_pdf: Tb = %u bins; supported 2 <= Tb <= 4096", Tb);
    NGP_REQUIRE(n >= 1, "sample_pdf: n = 0 samples");
    if (N == 0) return NGP_OK;
    NGP_REQUIRE(bins && weights && out, "sample_pdf: null pointer");
    const nv_pdf_u U = nv_pdf_u_of(n);
    hipLaunchKernelGGL(k_sample_pdf, dim3(N), dim3(NV_BLOCK), sizeof(float) * Tb + NV_PDF_SCAN_BYTES, (hipStream_t)stream, bins, weights, Tb, u, n, U, out);
    NGP_CHECK_LAUNCH("sample_pdf");
    return NGP_OK;
}

// ---- the occupancy-masked run ----

// records as the dense run keeps them (worst case: every sample occupied), then the counts [N] and the lists [N][T]; nothing needs clearing
static nro_kept nro_layout(uint32_t N, uint32_t num_steps, void* base, size_t* total) {
    const size_t nt = (size_t)N * num_steps;
    ngp_carver c(base);
    const nro_kept k = {c.take<uint32_t>(NV_REC_WORDS * nt, 1), c.take<uint32_t>(N), c.take<uint16_t>(nt)};
    *total = nt ? c.total(256) : 0;
    return k;
}
extern "C" size_t ngp_nav_run_occ_saved_bytes(uint32_t N, uint32_t num_steps) {
    size_t total;
    nro_layout(N, num_steps, nullptr, &total);
    return total;
}

// Hgrid a power of two (the one-multiply cell coordinate, ngp_cell_coord), at most 1024 (ngp_morton3's 10 bits per axis), C H^3 bits indexed in 32 bits
static int nro_grid(const char* who, const ngp_occ_grid_t* g, float bound, nav_occ& G) {
    NGP_REQUIRE(g && g->bitfield, "%s: null occupancy grid", who);
    NGP_REQUIRE(g->C >= 1 && g->C <= 32, "%s: C = %u cascades; supported 1 <= C <= 32", who, g->C);
    NGP_REQUIRE(g->Hgrid >= 2 && g->Hgrid <= 1024 && (g->Hgrid & (g->Hgrid - 1u)) == 0u, "%s: Hgrid = %u; the grid size must be a power of two in [2, 1024]", who, g->Hgrid);
    const uint64_t h3 = (uint64_t)g->Hgrid * g->Hgrid * g->Hgrid;
    NGP_REQUIRE(h3 * g->C <= (1ull << 32), "%s: C * Hgrid^3 = %u * %u^3 bits do not fit a 32-bit index", who, g->C, g->Hgrid);
    G.bits = g->bitfield; G.H3 = (uint32_t)h3; G.Cm1 = (int)g->C - 1;
    G.rbound = 1.0f / bound; G.hHf = 0.5f * (float)g->Hgrid; G.Hm1 = (float)(g->Hgrid - 1u);
    return NGP_OK;
}

extern "C" int ngp_nav_run_occ_forward(const ngp_nav_field_t* f, const void* prepared, const ngp_occ_grid_t* grid_host, const float* rays_o,
                                       const float* rays_d, const float* nears, const float* fars, uint32_t N, uint32_t num_steps, const float* aabb_host,
                                       const float* bg_color3_host, float* image, float* depth, float* weights_sum, uint32_t* counts, void* saved,
                                       size_t saved_bytes, void* stream) {
    nav_params P;
    int rc = nav_fill("nav_run_occ_forward", f, prepared, P);
    if (rc != NGP_OK) return rc;
    nav_occ G;
    rc = nro_grid("nav_run_occ_forward", grid_host, P.bound, G);
    if (rc != NGP_OK) return rc;
    if (N == 0) return NGP_OK;
    nav_run R;
    rc = nav_run_args("nav_run_occ_forward", rays_o, rays_d, nears, fars, N, num_steps, aabb_host, bg_color3_host, R);
    if (rc != NGP_OK) return rc;
    NGP_REQUIRE(image && depth && weights_sum, "nav_run_occ_forward: null output");
    size_t total;
    const nro_kept kept = nro_layout(N, num_steps, saved, &total);
    NGP_REQUIRE(!saved || saved_bytes >= total, "nav_run_occ_forward: `saved` is smaller than ngp_nav_run_occ_saved_bytes(N, num_steps)");
    const size_t lds = sizeof(float) * NV_H * NO_W + ((sizeof(uint16_t) * num_steps + 3) & ~(size_t)3);          // 16 KB + the list: below the default limit
    hipLaunchKernelGGL(k_nav_run_occ_fwd, dim3(N), dim3(NO_W), lds, (hipStream_t)stream, P, R, G, image, depth, weights_sum, counts, kept);
    NGP_CHECK_LAUNCH("nav_run_occ_forward");
    return NGP_OK;
}

extern "C" int ngp_nav_run_occ_backward(const ngp_nav_field_t* f, const void* prepared, const ngp_occ_grid_t* grid_host, const float* rays_o,
                                        const float* rays_d, const float* nears, const float* fars, uint32_t N, uint32_t num_steps, const float* aabb_host,
                                        const float* bg_color3_host, const float* grad_image, const float* grad_depth, const float* grad_weights_sum,
                                        const void* saved, size_t saved_bytes, float* grad_rays_o, float* grad_rays_d, void* stream) {
    nav_params P;
    int rc = nav_fill("nav_run_occ_backward", f, prepared, P);
    if (rc != NGP_OK) return rc;
    nav_occ G;                                                           // the samples come from the forward's lists; the grid is only judged here
    rc = nro_grid("nav_run_occ_backward", grid_host, P.bound, G);
    if (rc != NGP_OK) return rc;
    if (N == 0) return NGP_OK;
    nav_run R;
    rc = nav_run_args("nav_run_occ_backward", rays_o, rays_d, nears, fars, N, num_steps, aabb_host, bg_color3_host, R);
    if (rc != NGP_OK) return rc;
    NGP_REQUIRE(grad_image && grad_rays_o && grad_rays_d, "nav_run_occ_backward: null pointer");
    size_t total;
    const nro_kept kept = nro_layout(N, num_steps, const_cast<void*>(saved), &total);
    NGP_REQUIRE(saved && saved_bytes >= total, "nav_run_occ_backward: needs the `saved` buffer its forward filled");
    hipLaunchKernelGGL(k_nav_run_occ_bwd, dim3(N), dim3(NO_W), sizeof(float) * NV_H * NO_W, (hipStream_t)stream, P, R, grad_image, grad_depth,
                       grad_weights_sum, kept, grad_rays_o, grad_rays_d);
    NGP_CHECK_LAUNCH("nav_run_occ_backward");
    return NGP_OK;
}
