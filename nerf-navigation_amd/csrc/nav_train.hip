// nav_train.hip -- training forward and backward of the DEFAULT float32 field (nerf/network.py; ngp.field.NGPField) in native launches:
// what csrc/field_train.hip is for NGPFieldFF, for the model the nav kernels (nav_field.hip, nav_frame.hip, nav_plan.hip, nav_filter.hip) run.
//
//   k_nt_forward    one lane per sample, the text of k_nav_density_fwd + nv_color_forward: 16 x 8 float2 gathers, both nets on the VALU with the
//                   weights through the scalar cache.  Keeps the 32 encoded features per sample (128 B, word-major [32][M]) and nothing else.
//   k_nt_backward   a FIXED number of workgroups (at most NT_MAX_GROUPS), each walking its share of 256-sample chunks.  Per chunk, lane = sample:
//                   both nets recomputed from the kept features (no gather), the activation gradients on the VALU down to d L / d enc
//                   ([16][M][2], the `grad` of ngp_grid_encode_backward); the five weight gradients dW[out][in] = sum_s g[out][s] a[in][s] on the
//                   matrix cores (v_mfma_f32_32x32x2_f32: exact float32, samples = the reduction dimension), accumulated in registers over ALL the
//                   chunks of the workgroup and written once as raw tiles into the workspace.
//   k_nt_reduce     adds the workgroups' tiles in a fixed order into grad_weights [9344] (nn.Linear's [out, in] layouts, back to back).  No atomics:
//                   two runs give the same bits.
//
// LDS of the backward: two [64][NT_S] float images X, Y and three rows for d L / d (pre-sigmoid colour).  Row = feature, column = sample, row stride
// NT_S = 257 words: a lane walking its own column (the matrix-vector products) and 32 lanes reading 32 rows of one column (the MFMA operands: lane l
// supplies A[row l & 31][k = l >> 5] and B[k = l >> 5][col l & 31]) both touch 32 different banks.
//
// Numerics: float32 FMA chains in a fixed order, like the nav kernels; tests/test_gpu_default_train.py holds every output to the pinned float64
// oracle by the rule of tests/_nav_pinned_cases.py.
#include "ngp_nav_field.h"

static constexpr int NT_S = 257;                       // row stride of the backward's LDS images, in words
static constexpr uint32_t NT_CHUNK = 256;              // samples per chunk = threads per workgroup
static constexpr uint32_t NT_MAX_GROUPS = 256;         // workgroups of the backward = partial sums to add: one per CU (its LDS admits one workgroup per CU)
static constexpr uint32_t NT_SLOTS = 5;                // accumulator tiles per wave: dV2, dV1, dV0, dW2, dW1
static constexpr uint32_t NT_GROUP_FLOATS = 4 * NT_SLOTS * 1024;       // [wave][slot][16 registers][64 lanes]
static constexpr uint32_t NT_NW = 64 * 32 + 16 * 64 + 64 * 31 + 64 * 64 + 3 * 64;      // 9344
static constexpr size_t NT_LDS_BWD = sizeof(float) * (size_t)(2 * NV_H + 3) * NT_S;
static constexpr size_t NT_LDS_FWD = sizeof(float) * (16 + NV_H * NV_BLOCK);

typedef float nt_f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(NV_BLOCK) void k_nt_forward(nav_params P, const float* __restrict__ xyz, const float* __restrict__ dirs, uint32_t M,
                                                         float* __restrict__ sigma, float* __restrict__ rgbs, float* __restrict__ enc) {
    extern __shared__ float nv_smem[];
    float* col = nv_smem + 16 + threadIdx.x;
    const uint32_t i = blockIdx.x * NV_BLOCK + threadIdx.x;
    const bool live = i < M;
    const uint32_t ic = live ? i : M - 1;
    float x0, x1, x2;
    const bool inside = nv_normalise(P, xyz[3ull * ic], xyz[3ull * ic + 1], xyz[3ull * ic + 2], x0, x1, x2);
    float out[16];
    {
        float h[NV_H];                                                   // nv_hidden, with the features written out on the way
        #pragma unroll
        for (int j = 0; j < NV_H; j++) h[j] = 0.0f;
        #pragma unroll 4
        for (int l = 0; l < NV_L; l++) {
            float e0, e1;
            nv_level(P, l, x0, x1, x2, e0, e1);
            if (!inside) { e0 = 0.0f; e1 = 0.0f; }
            if (live) { enc[(size_t)(2 * l) * M + i] = e0; enc[(size_t)(2 * l + 1) * M + i] = e1; }
            const nv_wptr wa = nv_hide(P.w1t) + (2 * l) * NV_H;           // pinned here: two rows of weights in flight, not thirty-two
            const nv_wptr wb = wa + NV_H;
            #pragma unroll
            for (int j = 0; j < NV_H; j++) h[j] = __builtin_fmaf(wa[j], e0, h[j]);
            #pragma unroll
            for (int j = 0; j < NV_H; j++) h[j] = __builtin_fmaf(wb[j], e1, h[j]);
        }
        nv_park_relu(h, col);
    }
    nv_matvec<NV_H, 16>(nv_hide(P.w2t), col, out);
    if (live) sigma[i] = expf(out[0]);                                   // trunc_exp forward (activation.py:9-10); density_scale is the renderer's
    float geo[NV_GEO], rgb[3];
    #pragma unroll
    for (int m = 0; m < NV_GEO; m++) geo[m] = out[1 + m];
    uint64_t ma, mb;
    nv_color_forward(P, dirs[3ull * ic], dirs[3ull * ic + 1], dirs[3ull * ic + 2], geo, col, rgb, ma, mb);
    if (live) { rgbs[3ull * i] = rgb[0]; rgbs[3ull * i + 1] = rgb[1]; rgbs[3ull * i + 2] = rgb[2]; }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------

// nv_matvec on an image of row stride NT_S
template <int NIN, int NOUT>
__device__ __forceinline__ void nt_matvec(nv_wptr W, const float* __restrict__ col, float (&y)[NOUT]) {
    W = nv_hide(W);
    #pragma unroll
    for (int j = 0; j < NOUT; j++) y[j] = 0.0f;
    #pragma unroll 1
    for (int k = 0; k < NIN; k++) {
        const float a = col[k * NT_S];
        const nv_wptr w = W + k * NOUT;
        #pragma unroll
        for (int j = 0; j < NOUT; j++) y[j] = __builtin_fmaf(w[j], a, y[j]);
    }
}

template <int N>
__device__ __forceinline__ void nt_park(const float (&v)[N], float* __restrict__ col) {
    #pragma unroll
    for (int k = 0; k < N; k++) col[k * NT_S] = v[k];
}

template <int N>
__device__ __forceinline__ uint64_t nt_relu_mask(float (&v)[N]) {        // v <- relu(v); returns which entries were positive
    uint64_t m = 0;
    #pragma unroll
    for (int k = 0; k < N; k++) { m |= (uint64_t)(v[k] > 0.0f) << k; v[k] = fmaxf(v[k], 0.0f); }
    return m;
}

template <int N>
__device__ __forceinline__ void nt_apply_mask(float (&v)[N], uint64_t m) {
    #pragma unroll
    for (int k = 0; k < N; k++) v[k] = ((m >> k) & 1ull) ? v[k] : 0.0f;
}

// acc[out][in] += sum over samples s in [s0, s1) of A[a_row0 + out][s] B[b_row0 + in][s] for one 32 x 32 tile; rows from a_rows / b_rows on count as zero
__device__ __forceinline__ nt_f32x16 nt_tile(const float* __restrict__ A, int a_row0, int a_rows, const float* __restrict__ B, int b_row0, int b_rows,
                                             int s0, int s1, nt_f32x16 acc) {
    const int lane = (int)(threadIdx.x & 63u), r = lane & 31, kk = lane >> 5;
    const bool a_on = r < a_rows, b_on = r < b_rows;
    const float* pa = A + (a_row0 + (a_on ? r : 0)) * NT_S + kk;
    const float* pb = B + (b_row0 + (b_on ? r : 0)) * NT_S + kk;
    #pragma unroll 4
    for (int s = s0; s < s1; s += 2) {
        const float a = a_on ? pa[s] : 0.0f;
        const float b = b_on ? pb[s] : 0.0f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    return acc;
}

struct nt_weights { nv_wptr w1; };                     // sigma_net.0.weight [64][32] as it lies in the module: the one layout nav_params does not carry

template <bool WEIGHTS>
__global__ __launch_bounds__(NT_CHUNK) void k_nt_backward(nav_params P, nt_weights Q, const float* __restrict__ enc, const float* __restrict__ dirs, uint32_t M,
                                                          const float* __restrict__ gsigma, const float* __restrict__ grgb, float* __restrict__ genc,
                                                          float* __restrict__ partial) {
    extern __shared__ float nt_smem[];
    float* X = nt_smem;                                                  // [64][NT_S]
    float* Y = X + NV_H * NT_S;                                          // [64][NT_S]
    float* G3 = Y + NV_H * NT_S;                                         // [3][NT_S]
    const uint32_t tid = threadIdx.x;
    float* xc = X + tid;
    float* yc = Y + tid;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int th = wave & 1, kh = wave >> 1;                             // the 2-tile products: tile th, sample half kh; the 4-tile product: tile (kh, th)
    const int sa = kh * (int)(NT_CHUNK / 2), sb = sa + (int)(NT_CHUNK / 2);
    nt_f32x16 a_v2, a_v1, a_v0, a_w2, a_w1;
    #pragma unroll
    for (int q = 0; q < 16; q++) { a_v2[q] = 0.0f; a_v1[q] = 0.0f; a_v0[q] = 0.0f; a_w2[q] = 0.0f; a_w1[q] = 0.0f; }

    const uint32_t nchunks = (M + NT_CHUNK - 1) / NT_CHUNK;
    for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const uint32_t i = c * NT_CHUNK + tid;
        const bool live = i < M;
        const uint32_t ic = live ? i : M - 1;
        const float dxr = dirs[3ull * ic], dyr = dirs[3ull * ic + 1], dzr = dirs[3ull * ic + 2];
        // a sample behind the end of the batch carries zero gradients: every A operand of the products below is then zero in its column
        const float gs = live ? gsigma[ic] : 0.0f;
        const float gr0 = live ? grgb[3ull * ic] : 0.0f, gr1 = live ? grgb[3ull * ic + 1] : 0.0f, gr2 = live ? grgb[3ull * ic + 2] : 0.0f;

        // ---- density net again: enc -> X[32..63], relu(h) -> Y, out[16] ----
        #pragma unroll
        for (int k = 0; k < 32; k++) xc[(32 + k) * NT_S] = enc[(size_t)k * M + ic];
        float out[16];
        uint64_t mask_h;
        {
            float h[NV_H];
            nt_matvec<32, NV_H>(P.w1t, xc + 32 * NT_S, h);
            mask_h = nt_relu_mask(h);
            nt_park(h, yc);
        }
        nt_matvec<NV_H, 16>(P.w2t, yc, out);
        // ---- colour net again: cin -> X[0..30], relu(ha) -> Y, relu(hb) in registers, the three outputs straight from them ----
        {
            float sh[16];
            nv_sh(P, dxr, dyr, dzr, sh);
            nt_park(sh, xc);
            #pragma unroll
            for (int m = 0; m < NV_GEO; m++) xc[(16 + m) * NT_S] = out[1 + m];
        }
        uint64_t mask_a, mask_b;
        {
            float ha[NV_H];
            nt_matvec<NV_CIN, NV_H>(P.v0t, xc, ha);
            mask_a = nt_relu_mask(ha);
            nt_park(ha, yc);
        }
        float go[3];
        {
            float hb[NV_H];
            nt_matvec<NV_H, NV_H>(P.v1t, yc, hb);
            mask_b = nt_relu_mask(hb);
            const nv_wptr v2 = nv_hide(P.v2);
            float o[3] = {0.0f, 0.0f, 0.0f};
            #pragma unroll
            for (int cc = 0; cc < 3; cc++) {
                #pragma unroll
                for (int k = 0; k < NV_H; k++) o[cc] = __builtin_fmaf(v2[cc * NV_H + k], hb[k], o[cc]);
            }
            const float g3[3] = {gr0, gr1, gr2};
            #pragma unroll
            for (int cc = 0; cc < 3; cc++) {
                const float s = 1.0f / (1.0f + expf(-o[cc]));
                go[cc] = g3[cc] * s * (1.0f - s);                        // sigmoid's derivative
                G3[cc * NT_S + tid] = go[cc];
            }
            nt_park(hb, xc);                                             // relu(hb) -> X (a lane has only read its own column so far)
        }
        __syncthreads();
        if (WEIGHTS) a_v2 = nt_tile(G3, 0, 3, X, 32 * th, 32, sa, sb, a_v2);             // d V2 [3][64] = go x relu(hb)
        float g[NV_H];
        {
            const nv_wptr v2 = nv_hide(P.v2);
            #pragma unroll
            for (int k = 0; k < NV_H; k++) g[k] = __builtin_fmaf(v2[2 * NV_H + k], go[2], __builtin_fmaf(v2[NV_H + k], go[1], v2[k] * go[0]));
            nt_apply_mask(g, mask_b);                                    // d L / d hb
        }
        __syncthreads();                                                 // the product above has read X
        nt_park(g, xc);
        __syncthreads();
        if (WEIGHTS) a_v1 = nt_tile(X, 32 * kh, 32, Y, 32 * th, 32, 0, (int)NT_CHUNK, a_v1);   // d V1 [64][64] = d hb x relu(ha)
        nt_matvec<NV_H, NV_H>(P.v1, xc, g);
        nt_apply_mask(g, mask_a);                                        // d L / d ha
        __syncthreads();                                                 // the product above has read X and Y
        nt_park(g, yc);
        {
            float sh[16];
            nv_sh(P, dxr, dyr, dzr, sh);
            nt_park(sh, xc);
            #pragma unroll
            for (int m = 0; m < NV_GEO; m++) xc[(16 + m) * NT_S] = out[1 + m];
        }
        __syncthreads();
        if (WEIGHTS) a_v0 = nt_tile(Y, 32 * th, 32, X, 0, NV_CIN, sa, sb, a_v0);            // d V0 [64][31] = d ha x cat(SH, geo)
        float gout[16];
        {
            float gin[NV_CIN];
            nt_matvec<NV_H, NV_CIN>(P.v0, yc, gin);
            gout[0] = gs * nv_exp_clamped(out[0]);                       // trunc_exp's clamped derivative (activation.py:16-18)
            #pragma unroll
            for (int m = 0; m < NV_GEO; m++) gout[1 + m] = gin[16 + m];
        }
        __syncthreads();                                                 // the product above has read X and Y
        // ---- density net backward: d out -> X[0..15], enc -> X[32..63], relu(h) -> Y ----
        nt_park(gout, xc);
        #pragma unroll
        for (int k = 0; k < 32; k++) xc[(32 + k) * NT_S] = enc[(size_t)k * M + ic];
        {
            float h[NV_H];
            nt_matvec<32, NV_H>(P.w1t, xc + 32 * NT_S, h);               // the same chain as above: the same mask
            nt_relu_mask(h);
            nt_park(h, yc);
        }
        nt_matvec<16, NV_H>(P.w2, xc, g);
        nt_apply_mask(g, mask_h);                                        // d L / d h
        __syncthreads();
        if (WEIGHTS) a_w2 = nt_tile(X, 0, 16, Y, 32 * th, 32, sa, sb, a_w2);                // d W2 [16][64] = d out x relu(h)
        __syncthreads();                                                 // the product above has read Y
        nt_park(g, yc);
        __syncthreads();
        if (WEIGHTS) a_w1 = nt_tile(Y, 32 * th, 32, X, 32, 32, sa, sb, a_w1);               // d W1 [64][32] = d h x enc
        if (genc) {
            float ge[32];
            nt_matvec<NV_H, 32>(Q.w1, yc, ge);
            if (live) {
                #pragma unroll
                for (int l = 0; l < NV_L; l++) *(float2*)(genc + ((size_t)l * M + i) * 2) = make_float2(ge[2 * l], ge[2 * l + 1]);
            }
        }
        __syncthreads();                                                 // the product above has read X and Y
    }
    if (WEIGHTS) {
        float* out_w = partial + ((size_t)blockIdx.x * 4 + (size_t)wave) * (NT_SLOTS * 1024) + (tid & 63u);
        #pragma unroll
        for (int q = 0; q < 16; q++) {
            out_w[0 * 1024 + q * 64] = a_v2[q];
            out_w[1 * 1024 + q * 64] = a_v1[q];
            out_w[2 * 1024 + q * 64] = a_v0[q];
            out_w[3 * 1024 + q * 64] = a_w2[q];
            out_w[4 * 1024 + q * 64] = a_w1[q];
        }
    }
}

// where entry (row, col) of a 32 x 32 result tile lies in a wave's 16 registers x 64 lanes: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
__device__ __forceinline__ uint32_t nt_tile_word(uint32_t row, uint32_t col) {
    const uint32_t reg = (row & 3u) + 4u * (row >> 3), lane = col + 32u * ((row >> 2) & 1u);
    return reg * 64u + lane;
}

// grad_weights[e] = sum over the workgroups (ascending, in eight runs that are then added in order) of the one or two tiles that hold entry e
__global__ __launch_bounds__(256) void k_nt_reduce(const float* __restrict__ partial, uint32_t groups, float* __restrict__ gw) {
    __shared__ float part[8][32];
    const uint32_t e = blockIdx.x * 32u + (threadIdx.x & 31u), p = threadIdx.x >> 5;
    float sum = 0.0f;
    if (e < NT_NW) {
        uint32_t slot, row, col, w0, w1;                                 // w0, w1: the waves that hold the entry (w1 == w0: one wave)
        if (e < 2048u)      { slot = 4; row = e >> 5; col = e & 31u; w0 = row >> 5; w1 = w0 + 2; row &= 31u; }                                  // sigma_net.0 [64][32]
        else if (e < 3072u) { const uint32_t t = e - 2048u; slot = 3; row = t >> 6; col = t & 63u; w0 = col >> 5; w1 = w0 + 2; col &= 31u; }   // sigma_net.1 [16][64]
        else if (e < 5056u) { const uint32_t t = e - 3072u; slot = 2; row = t / 31u; col = t - row * 31u; w0 = row >> 5; w1 = w0 + 2; row &= 31u; }   // color_net.0 [64][31]
        else if (e < 9152u) { const uint32_t t = e - 5056u; slot = 1; row = t >> 6; col = t & 63u; w0 = (row >> 5) * 2 + (col >> 5); w1 = w0; row &= 31u; col &= 31u; }   // color_net.1 [64][64]
        else                { const uint32_t t = e - 9152u; slot = 0; row = t >> 6; col = t & 63u; w0 = col >> 5; w1 = w0 + 2; col &= 31u; }   // color_net.2 [3][64]
        const uint32_t word = slot * 1024u + nt_tile_word(row, col);
        const uint32_t per = (groups + 7u) / 8u, g0 = p * per, g1 = (g0 + per < groups) ? g0 + per : groups;
        for (uint32_t g = g0; g < g1; g++) {
            const float* base = partial + (size_t)g * NT_GROUP_FLOATS + word;
            float v = base[(size_t)w0 * (NT_SLOTS * 1024)];
            if (w1 != w0) v += base[(size_t)w1 * (NT_SLOTS * 1024)];
            sum += v;
        }
    }
    part[p][threadIdx.x & 31u] = sum;
    __syncthreads();
    if (p == 0 && e < NT_NW) {
        float s = part[0][threadIdx.x];
        #pragma unroll
        for (int q = 1; q < 8; q++) s += part[q][threadIdx.x];
        gw[e] = s;
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

struct nt_saved_ws { float* enc; size_t total; };                      // the 32 encoded features of every sample, word-major [32][M]
static nt_saved_ws nt_saved_layout(uint32_t M, void* base) {
    ngp_carver c(base);
    return {c.take<float>(32 * (size_t)M), c.total(256)};
}
static uint32_t nt_groups(uint32_t M) {
    const uint32_t chunks = ngp_div_up(M, NT_CHUNK);
    return chunks < NT_MAX_GROUPS ? chunks : NT_MAX_GROUPS;
}
struct nt_work_ws { float* partial; size_t total; };                    // [groups][4 waves][5 tiles][16][64]: the workgroups' weight-gradient tiles
static nt_work_ws nt_work_layout(uint32_t M, void* base) {
    ngp_carver c(base);
    return {c.take<float>((size_t)nt_groups(M) * NT_GROUP_FLOATS), c.total(256)};
}

extern "C" size_t ngp_nav_field_train_saved_bytes(uint32_t M) { return M ? nt_saved_layout(M, nullptr).total : 0; }
extern "C" size_t ngp_nav_field_train_workspace(uint32_t M) { return M ? nt_work_layout(M, nullptr).total : 0; }

static int nt_allow_big_lds() {
    static std::atomic<unsigned long long> devices{0};
    const int rc = ngp_allow_dynamic_lds(devices, {(const void*)k_nt_forward, (const void*)k_nt_backward<true>, (const void*)k_nt_backward<false>}, 160 * 1024);
    if (rc == NGP_LDS_NO_DEVICE) return ngp_fail(NGP_ELAUNCH, "nav_field_train: no current device");
    if (rc != NGP_LDS_OK) return ngp_fail(NGP_ELAUNCH, "nav_field_train: cannot raise the dynamic LDS limit");
    return NGP_OK;
}

extern "C" int ngp_nav_field_train_forward(const ngp_nav_field_t* f, const void* prepared, const float* xyzs, const float* dirs, uint32_t M,
                                           float* sigmas, float* rgbs, void* saved, size_t saved_bytes, void* stream) {
    nav_params P;
    const int rc = nav_fill("nav_field_train_forward", f, prepared, P);
    if (rc != NGP_OK) return rc;
    if (M == 0) return NGP_OK;
    NGP_REQUIRE(xyzs && dirs && sigmas && rgbs, "nav_field_train_forward: null pointer");
    const nt_saved_ws kept = nt_saved_layout(M, saved);
    if (!saved || saved_bytes < kept.total)
        return ngp_fail(NGP_EWORKSPACE, "nav_field_train_forward: `saved` of %zu bytes, needs ngp_nav_field_train_saved_bytes(M) = %zu", saved ? saved_bytes : (size_t)0, kept.total);
    { const int rc_lds = nt_allow_big_lds(); if (rc_lds != NGP_OK) return rc_lds; }
    hipLaunchKernelGGL(k_nt_forward, dim3(ngp_div_up(M, NV_BLOCK)), dim3(NV_BLOCK), NT_LDS_FWD, (hipStream_t)stream, P, xyzs, dirs, M, sigmas, rgbs, kept.enc);
    NGP_CHECK_LAUNCH("nav_field_train_forward");
    return NGP_OK;
}

extern "C" int ngp_nav_field_train_backward(const ngp_nav_field_t* f, const void* prepared, const void* saved, const float* xyzs, const float* dirs,
                                            uint32_t M, const float* grad_sigmas, const float* grad_rgbs, float* grad_enc, float* grad_weights,
                                            void* workspace, size_t workspace_bytes, void* stream) {
    nav_params P;
    const int rc = nav_fill("nav_field_train_backward", f, prepared, P);
    if (rc != NGP_OK) return rc;
    if (M == 0) return NGP_OK;
    NGP_REQUIRE(saved && xyzs && dirs && grad_sigmas && grad_rgbs, "nav_field_train_backward: null pointer");
    NGP_REQUIRE(grad_enc || grad_weights, "nav_field_train_backward: null pointer (grad_enc and grad_weights: at least one)");
    const nt_work_ws w = nt_work_layout(M, workspace);
    if (grad_weights && (!workspace || workspace_bytes < w.total))
        return ngp_fail(NGP_EWORKSPACE, "nav_field_train_backward: workspace of %zu bytes, needs ngp_nav_field_train_workspace(M) = %zu", workspace ? workspace_bytes : (size_t)0, w.total);
    const nt_saved_ws kept = nt_saved_layout(M, const_cast<void*>(saved));
    { const int rc_lds = nt_allow_big_lds(); if (rc_lds != NGP_OK) return rc_lds; }
    nt_weights Q;
    Q.w1 = (nv_wptr)(uintptr_t)f->sigma_w0;
    const uint32_t groups = nt_groups(M);
    hipStream_t st = (hipStream_t)stream;
    if (grad_weights) {
        hipLaunchKernelGGL(k_nt_backward<true>, dim3(groups), dim3(NT_CHUNK), NT_LDS_BWD, st, P, Q, kept.enc, dirs, M, grad_sigmas, grad_rgbs, grad_enc, w.partial);
        hipLaunchKernelGGL(k_nt_reduce, dim3(ngp_div_up(NT_NW, 32)), dim3(256), 0, st, w.partial, groups, grad_weights);
    } else {
        hipLaunchKernelGGL(k_nt_backward<false>, dim3(groups), dim3(NT_CHUNK), NT_LDS_BWD, st, P, Q, kept.enc, dirs, M, grad_sigmas, grad_rgbs, grad_enc, (float*)nullptr);
    }
    NGP_CHECK_LAUNCH("nav_field_train_backward");
    return NGP_OK;
}
