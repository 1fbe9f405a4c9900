// ngp_nav_field.h -- the default float32 field (nerf/network.py) as device functions, and its host-side descriptor: shared by the nav queries
// (nav_field.hip) and the frame kernel of the default model (nav_frame.hip).  The text is nav_field.hip's own, moved here unchanged.
#pragma once
#include "ngp_sh.h"

#ifndef NV_RUN_U
#define NV_RUN_U 1                         // levels of the hash grid the run kernels may overlap (gathers in flight per lane: 8 x U); A/B: profiles/HISTORY.md 4.5
#endif
static constexpr int NV_L = 16;            // levels
static constexpr int NV_H = 64;            // hidden width
static constexpr int NV_GEO = 15;
static constexpr int NV_CIN = 31;          // 16 SH + 15 geo
static constexpr uint32_t NV_BLOCK = 256;
#define NV_FENCE() __builtin_amdgcn_sched_barrier(0)

struct nav_levels {
    float scale[NV_L];
    uint32_t base[NV_L], size[NV_L], mask[NV_L], s1[NV_L], s2[NV_L];     // rows; mask = size - 1 when size is 2^k else 0; s1 == 0: hashed
};

// Weights are read through the CONSTANT address space: a load from it is invariant by definition, so a wave-uniform address always
// becomes a scalar load (s_load_dwordx8/x16 into SGPRs) -- also behind the barriers of the run kernels, where the compiler must assume
// that ordinary global memory may have changed and would otherwise fetch every weight per lane into a VGPR.
typedef const float __attribute__((address_space(4)))* nv_wptr;

// Constant-space loads are speculatable, so left alone the optimiser hoists EVERY weight load of a kernel to its entry (out of the
// `weights > 1e-4` branch, out of the chunk loops): ~9,000 live SGPRs, spilled lane by lane into VGPRs (15,000 v_readlane in
// k_nav_run_bwd).  Passing the pointer through an empty volatile asm where a layer starts pins that layer's loads inside it.
__device__ __forceinline__ nv_wptr nv_hide(nv_wptr p) {
    unsigned long long v = (unsigned long long)p;
    asm volatile("" : "+s"(v));
    return (nv_wptr)v;
}

struct nav_params {
    const float2* table;                   // [sO] rows of 2 float32 features
    nv_wptr w1t;                           // [32][64]  sigma_net.0.weight transposed
    nv_wptr w2, w2t;                       // [16][64]  sigma_net.1.weight, [64][16] its transpose
    nv_wptr v0, v0t;                       // [64][31]  color_net.0.weight, [31][64]
    nv_wptr v1, v1t;                       // [64][64]  color_net.1.weight and its transpose
    nv_wptr v2, v2t;                       // [3][64]   color_net.2.weight, [64][3]
    nav_levels lv;
    sh_norm shn;
    float bound, r2b, density_scale;
};

// ---------------------------------------------------------------------------
// hash-grid encoding of one level (gridencoder.cu:125-170, float32), optionally with the Jacobian contraction
// ---------------------------------------------------------------------------

__device__ __forceinline__ uint32_t nv_row(const nav_params& P, int l, uint32_t x, uint32_t y, uint32_t z) {
    if (P.lv.s1[l]) return P.lv.base[l] + x + y * P.lv.s1[l] + z * P.lv.s2[l];                    // dense level: always < size
    const uint32_t h = x ^ (y * NGP_HASH_P1) ^ (z * NGP_HASH_P2);                                  // fast_hash (gridencoder.cu:35-51)
    return P.lv.base[l] + (P.lv.mask[l] ? (h & P.lv.mask[l]) : (h % P.lv.size[l]));
}

struct nv_cell { uint32_t gx, gy, gz; float fx, fy, fz; };

__device__ __forceinline__ nv_cell nv_locate(float scale, float x0, float x1, float x2) {
    nv_cell c;
    const float px = x0 * scale + 0.5f, py = x1 * scale + 0.5f, pz = x2 * scale + 0.5f;
    const float flx = floorf(px), fly = floorf(py), flz = floorf(pz);
    c.gx = (uint32_t)flx; c.gy = (uint32_t)fly; c.gz = (uint32_t)flz;
    c.fx = px - flx; c.fy = py - fly; c.fz = pz - flz;
    return c;
}

// the two features of level l at a normalised position in [0,1]^3: corners in the reference's order, w = ((wx) wy) wz
__device__ __forceinline__ void nv_level(const nav_params& P, int l, float x0, float x1, float x2, float& e0, float& e1) {
    const nv_cell c = nv_locate(P.lv.scale[l], x0, x1, x2);
    float2 v[8];
    #pragma unroll
    for (int k = 0; k < 8; k++) v[k] = P.table[nv_row(P, l, c.gx + (k & 1), c.gy + ((k >> 1) & 1), c.gz + (k >> 2))];
    e0 = 0.0f; e1 = 0.0f;
    #pragma unroll
    for (int k = 0; k < 8; k++) {
        const float w = (((k & 1) ? c.fx : 1.0f - c.fx) * ((k & 2) ? c.fy : 1.0f - c.fy)) * ((k & 4) ? c.fz : 1.0f - c.fz);
        e0 = __builtin_fmaf(w, v[k].x, e0);
        e1 = __builtin_fmaf(w, v[k].y, e1);
    }
}

// g0 * d e0 / d x01 + g1 * d e1 / d x01 for level l (the dy_dx of gridencoder.cu:173-222 contracted with the gradient)
__device__ __forceinline__ void nv_level_grad(const nav_params& P, int l, float x0, float x1, float x2, float g0, float g1,
                                              float& ax, float& ay, float& az) {
    const float scale = P.lv.scale[l];
    const nv_cell c = nv_locate(scale, x0, x1, x2);
    float s[8];                                                          // g . value at each corner
    #pragma unroll
    for (int k = 0; k < 8; k++) {
        const float2 v = P.table[nv_row(P, l, c.gx + (k & 1), c.gy + ((k >> 1) & 1), c.gz + (k >> 2))];
        s[k] = __builtin_fmaf(g0, v.x, g1 * v.y);
    }
    const float wx0 = 1.0f - c.fx, wy0 = 1.0f - c.fy, wz0 = 1.0f - c.fz;
    // d/dx: sum over (y,z) of wy wz (right - left), etc.
    const float dx = (wy0 * wz0) * (s[1] - s[0]) + (c.fy * wz0) * (s[3] - s[2]) + (wy0 * c.fz) * (s[5] - s[4]) + (c.fy * c.fz) * (s[7] - s[6]);
    const float dy = (wx0 * wz0) * (s[2] - s[0]) + (c.fx * wz0) * (s[3] - s[1]) + (wx0 * c.fz) * (s[6] - s[4]) + (c.fx * c.fz) * (s[7] - s[5]);
    const float dz = (wx0 * wy0) * (s[4] - s[0]) + (c.fx * wy0) * (s[5] - s[1]) + (wx0 * c.fy) * (s[6] - s[2]) + (c.fx * c.fy) * (s[7] - s[3]);
    ax = __builtin_fmaf(scale, dx, ax);
    ay = __builtin_fmaf(scale, dy, ay);
    az = __builtin_fmaf(scale, dz, az);
}

// ---------------------------------------------------------------------------
// density net: hash grid -> Linear(32,64) -> ReLU -> Linear(64,16)      (nerf/network.py:95-111)
// ---------------------------------------------------------------------------

// world position -> normalised position (grid.py:144); `inside` false = outside [0,1]^3 (or NaN): the encoder returns zeros (gridencoder.cu:99-123)
__device__ __forceinline__ bool nv_normalise(const nav_params& P, float wx, float wy, float wz, float& x0, float& x1, float& x2) {
    // torch on the GPU divides by a host scalar by multiplying with its binary32 reciprocal (ATen BinaryDivTrueKernel.cu): r2b = fl(1 / (2 bound))
    x0 = (wx + P.bound) * P.r2b; x1 = (wy + P.bound) * P.r2b; x2 = (wz + P.bound) * P.r2b;
    const bool inside = (x0 >= 0.0f && x0 <= 1.0f) && (x1 >= 0.0f && x1 <= 1.0f) && (x2 >= 0.0f && x2 <= 1.0f);
    if (!inside) { x0 = 0.0f; x1 = 0.0f; x2 = 0.0f; }                     // gather somewhere valid; the features are discarded
    return inside;
}

// y[j] = sum_k W[k][j] x[k] for j < NOUT: a rolled loop over the reduction index k, x[k] read from this lane's LDS column, the NOUT
// accumulators in registers with compile-time indices, row k of W (NOUT contiguous floats) through the scalar cache.  One row is at
// most 64 SGPRs, so nothing spills; the loop stays rolled so that no more than one row is ever in flight.
// S: the stride between a column's entries, i.e. the lanes that share the scratch -- NV_BLOCK for the one-workgroup-per-ray and per-point kernels, 64 for
// the one-wave-per-ray kernels (k_nav_run_occ_*); the same parameter on every helper below that touches the column.
template <int NIN, int NOUT, uint32_t S = NV_BLOCK>
__device__ __forceinline__ void nv_matvec(nv_wptr W, const float* __restrict__ col, float (&y)[NOUT]) {
    #pragma unroll
    for (int j = 0; j < NOUT; j++) y[j] = 0.0f;
    #pragma unroll 1
    for (int k = 0; k < NIN; k++) {
        const float a = col[k * S];
        const nv_wptr w = W + k * NOUT;
        #pragma unroll
        for (int j = 0; j < NOUT; j++) y[j] = __builtin_fmaf(w[j], a, y[j]);
    }
}

template <uint32_t S = NV_BLOCK, int N>
__device__ __forceinline__ void nv_park(const float (&v)[N], float* __restrict__ col, int at = 0) {
    #pragma unroll
    for (int k = 0; k < N; k++) col[(at + k) * S] = v[k];
}

template <uint32_t S = NV_BLOCK, int N>
__device__ __forceinline__ uint64_t nv_park_relu(const float (&v)[N], float* __restrict__ col) {       // relu(v) into the column; returns the mask
    uint64_t m = 0;
    #pragma unroll
    for (int k = 0; k < N; k++) { col[k * S] = fmaxf(v[k], 0.0f); m |= (uint64_t)(v[k] > 0.0f) << k; }
    return m;
}

// hidden pre-activations h[64] = W1 . enc(x): the first layer is accumulated level by level, so the 32 features never exist together
// (U = how many levels the compiler may overlap: 1 inside the run kernels, whose eight waves per CU hide the gather latency by themselves;
//  4 in the point kernels, where a planner-sized batch is 40 workgroups on 256 CUs and the 16 dependent round trips are the run time)
template <int U>
__device__ __forceinline__ void nv_hidden(const nav_params& P, bool inside, float x0, float x1, float x2, float (&h)[NV_H]) {
    #pragma unroll
    for (int j = 0; j < NV_H; j++) h[j] = 0.0f;
    #pragma unroll U
    for (int l = 0; l < NV_L; l++) {
        float e0, e1;
        nv_level(P, l, x0, x1, x2, e0, e1);
        if (!inside) { e0 = 0.0f; e1 = 0.0f; }
        const nv_wptr wa = P.w1t + (2 * l) * NV_H;                       // wave-uniform addresses: scalar loads
        const nv_wptr wb = wa + NV_H;
        #pragma unroll
        for (int j = 0; j < NV_H; j++) h[j] = __builtin_fmaf(wa[j], e0, h[j]);
        #pragma unroll
        for (int j = 0; j < NV_H; j++) h[j] = __builtin_fmaf(wb[j], e1, h[j]);
    }
}

// density net forward for one point: out[16] = W2 . relu(W1 . enc(x)); returns the ReLU mask of the hidden layer
template <int U = 1, uint32_t S = NV_BLOCK>
__device__ __forceinline__ uint64_t nv_density_forward(const nav_params& P, bool inside, float x0, float x1, float x2, float* __restrict__ col,
                                                       float (&out)[16]) {
    float h[NV_H];
    nv_hidden<U>(P, inside, x0, x1, x2, h);
    const uint64_t relu = nv_park_relu<S>(h, col);
    nv_matvec<NV_H, 16, S>(P.w2t, col, out);
    return relu;
}

// backward of the density net for one point: gout[16] = d L / d out, `relu` = which hidden units were active  ->  d L / d (world position)
template <int U = 1, uint32_t S = NV_BLOCK>
__device__ __forceinline__ void nv_density_backward(const nav_params& P, bool inside, float x0, float x1, float x2, uint64_t relu,
                                                    const float (&gout)[16], float* __restrict__ col, float& gx, float& gy, float& gz) {
    float gh[NV_H];                                                      // d L / d h (ReLU mask applied)
    nv_park<S>(gout, col);
    nv_matvec<16, NV_H, S>(P.w2, col, gh);
    #pragma unroll
    for (int j = 0; j < NV_H; j++) gh[j] = ((relu >> j) & 1ull) ? gh[j] : 0.0f;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    #pragma unroll U
    for (int l = 0; l < NV_L; l++) {
        const nv_wptr wa = P.w1t + (2 * l) * NV_H;
        const nv_wptr wb = wa + NV_H;
        float g0 = 0.0f, g1 = 0.0f;                                      // d L / d enc[2l], enc[2l+1]
        #pragma unroll
        for (int j = 0; j < NV_H; j++) g0 = __builtin_fmaf(wa[j], gh[j], g0);
        #pragma unroll
        for (int j = 0; j < NV_H; j++) g1 = __builtin_fmaf(wb[j], gh[j], g1);
        nv_level_grad(P, l, x0, x1, x2, g0, g1, ax, ay, az);
    }
    const float k = inside ? P.r2b : 0.0f;                                                 // d x01 / d world; zero outside the box
    gx = ax * k; gy = ay * k; gz = az * k;
}

__device__ __forceinline__ float nv_exp_clamped(float x) { return expf(fminf(fmaxf(x, -15.0f), 15.0f)); }   // trunc_exp backward (activation.py:16-18)

// ---------------------------------------------------------------------------
// colour net: cat(SH16(dir), geo15) -> Linear(31,64) -> ReLU -> Linear(64,64) -> ReLU -> Linear(64,3) -> sigmoid   (network.py:113-123)
// ---------------------------------------------------------------------------

// SH(4) of a direction and, on request, the contraction of its Jacobian with a gradient vector (shencoder.cu:50-355 through the
// recurrences of ngp_sh.h)
__device__ __forceinline__ void nv_sh(const nav_params& P, float x, float y, float z, float (&sh)[16]) { sh_eval<4>(x, y, z, P.shn, sh); }

__device__ __forceinline__ void nv_sh_backward(const nav_params& P, float x, float y, float z, const float (&g)[16], float& dx, float& dy, float& dz) {
    sh_tables<4> t;
    t.build(x, y, z);
    dx = 0.0f; dy = 0.0f; dz = 0.0f;
    #pragma unroll
    for (uint32_t l = 0; l < 4; l++) {
        #pragma unroll
        for (uint32_t m = 0; m <= l; m++) {
            const float nq = P.shn.n[l][m] * t.Q[l][m], nqz = P.shn.n[l][m] * t.Q[l][m + 1];
            const uint32_t ip = l * l + l + m, in = l * l + l - m;
            dz = __builtin_fmaf(g[ip], nqz * t.A[m], dz);
            if (m > 0) {
                const float fm = (float)m;
                dz = __builtin_fmaf(g[in], nqz * t.B[m], dz);
                dx = __builtin_fmaf(g[ip], nq * (fm * t.A[m - 1]), dx);
                dy = __builtin_fmaf(g[ip], nq * (-fm * t.B[m - 1]), dy);
                dx = __builtin_fmaf(g[in], nq * (fm * t.B[m - 1]), dx);
                dy = __builtin_fmaf(g[in], nq * (fm * t.A[m - 1]), dy);
            }
        }
    }
}

// colour forward for one sample; returns the ReLU masks of the two hidden layers and the pre-sigmoid... no: rgb after the sigmoid
template <uint32_t S = NV_BLOCK>
__device__ __forceinline__ void nv_color_forward(const nav_params& P, float dxr, float dyr, float dzr, const float (&geo)[NV_GEO],
                                                 float* __restrict__ col, float (&rgb)[3], uint64_t& mask_a, uint64_t& mask_b) {
    {
        float sh[16];
        nv_sh(P, dxr, dyr, dzr, sh);
        nv_park<S>(sh, col);
        nv_park<S>(geo, col, 16);
    }
    float hid[NV_H];
    nv_matvec<NV_CIN, NV_H, S>(P.v0t, col, hid);
    mask_a = nv_park_relu<S>(hid, col);
    nv_matvec<NV_H, NV_H, S>(P.v1t, col, hid);
    mask_b = nv_park_relu<S>(hid, col);
    float o[3];
    nv_matvec<NV_H, 3, S>(P.v2t, col, o);
    #pragma unroll
    for (int c = 0; c < 3; c++) rgb[c] = 1.0f / (1.0f + expf(-o[c]));
}

// ---------------------------------------------------------------------------
// host side: the prepared weights and the descriptor -> kernel parameters
// ---------------------------------------------------------------------------

// the prepared workspace: transposed copies of the five weight matrices, back to back
struct nav_prep_ws { float* w1t; float* w2t; float* v0t; float* v1t; float* v2t; size_t total; };
static nav_prep_ws nav_prep_layout(void* base) {
    ngp_carver c(base);
    return {c.take<float>(32 * 64, 1), c.take<float>(64 * 16, 1), c.take<float>(31 * 64, 1), c.take<float>(64 * 64, 1), c.take<float>(64 * 3, 1), c.total()};
}

static int nav_fill(const char* who, const ngp_nav_field_t* f, const void* prepared, nav_params& P) {
    NGP_REQUIRE(f && f->embeddings && f->offsets_host && f->sigma_w0 && f->sigma_w1 && f->color_w0 && f->color_w1 && f->color_w2 && prepared,
                "%s: null field pointer", who);
    NGP_REQUIRE(f->L == NV_L && f->bound > 0.0f, "%s: the fused nav queries are built for the default field (16 levels x 2 features, 32-64-16 | 31-64-64-3)", who);
    P.table = (const float2*)f->embeddings;
    const nav_prep_ws prep = nav_prep_layout(const_cast<void*>(prepared));
    P.w1t = (nv_wptr)(uintptr_t)prep.w1t; P.w2t = (nv_wptr)(uintptr_t)prep.w2t;
    P.v0t = (nv_wptr)(uintptr_t)prep.v0t; P.v1t = (nv_wptr)(uintptr_t)prep.v1t; P.v2t = (nv_wptr)(uintptr_t)prep.v2t;
    P.w2 = (nv_wptr)(uintptr_t)f->sigma_w1; P.v0 = (nv_wptr)(uintptr_t)f->color_w0;
    P.v1 = (nv_wptr)(uintptr_t)f->color_w1; P.v2 = (nv_wptr)(uintptr_t)f->color_w2;
    for (int l = 0; l < NV_L; l++) {
        const float sc = ngp_level_scale((uint32_t)l, f->S, f->H);
        const uint32_t side = ngp_level_resolution(sc) + 1u;
        const uint32_t o0 = (uint32_t)f->offsets_host[l], size = (uint32_t)f->offsets_host[l + 1] - o0;
        NGP_REQUIRE(size > 0, "%s: empty level %d", who, l);
        const ngp_level_index ix = ngp_classify_level(size, side);          // (ngp_device.h)
        // nv_row adds a dense level's strides without a modulo, which is only right for exact strides
        NGP_REQUIRE(!ix.dense || ix.exact, "%s: level %d (side %u, %u rows) is indexed with wrapped 32-bit strides, which the fused nav kernels do not implement; "
                    "query this field through NavQueries' op chain instead", who, l, side, size);
        P.lv.scale[l] = sc; P.lv.base[l] = o0; P.lv.size[l] = size;
        P.lv.mask[l] = (size & (size - 1)) == 0 ? size - 1 : 0u;
        P.lv.s1[l] = ix.dense ? ix.s1 : 0u; P.lv.s2[l] = ix.dense ? ix.s2 : 0u;
    }
    sh_fill_norm(P.shn);
    P.bound = f->bound;
    P.r2b = 1.0f / (2.0f * f->bound);
    P.density_scale = f->density_scale;
    return NGP_OK;
}
