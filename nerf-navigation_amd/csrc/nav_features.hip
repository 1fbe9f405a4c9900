// nav_features.hip -- the pose filter's interest regions (Estimator.find_POI, the dilation, coords[mask] and the batch draw: nav/estimator_helpers.py:181-204,
// 229-230) on the device.  The contract and every per-pixel function live in ngp_features.h; DESIGN.md 3.5 "Native interest regions".
//
//   k_feat_blur<1>        gray, aligned 2x upsample and the base blur in one launch: the tile with its halo is computed into LDS from the image
//   k_feat_blur<0>        one Gaussian level from the one before it: tile + halo (folded at the image's ends) into LDS, the row pass into LDS, the
//                         column pass out of it.  Halo rows are blurred again per tile by the same taps in the same order, so the result does not
//                         depend on the tiling.  The level the next octave starts from also writes its even rows and columns there.
//   k_feat_extrema        one lane per pixel of an octave: the difference of Gaussians is formed on the fly from the levels (one rounding either way),
//                         tested against its 26 neighbours, refined, and stamped into the mask (plain stores of the same value)
//   k_feat_stamp          one lane per pixel of the mask: a set pixel stores its clipped square of ones into the cleared dilated mask (one value: no atomics)
//   k_feat_count          one lane per pixel of the dilated mask in (column, row) order: the wave's ballot to a bitmap, the workgroup's count
//   k_feat_list_write     workgroup c adds up the counts before it and writes its (row, col) pairs behind them; the last one leaves M in the count word
//   k_feat_draw           one lane per (iteration, entry): the keyed permutation, a gather of one pair
// No atomics, no scratch, nothing to clear but the two masks.
#include "ngp_device.h"
#include "ngp_features.h"

static constexpr int FEAT_TW = 64, FEAT_TH = 16, FEAT_BLOCK = 256;          // 32-row tiles (34 KB of LDS) were slower: 0.95 against 0.79 ms on an 800 x 800 image
static constexpr int FEAT_PW = FEAT_TW + 2 * NGP_FEAT_MAX_RADIUS, FEAT_PH = FEAT_TH + 2 * NGP_FEAT_MAX_RADIUS;
static constexpr uint32_t FEAT_CHUNK = 1024;

// SRC = 0: src is a level [h,w].  SRC = 1: src is the image [sh,sw,3] and the source pixel is its upsample's (h = 2 sh, w = 2 sw).
template <int SRC>
__global__ __launch_bounds__(FEAT_BLOCK) void k_feat_blur(const float* __restrict__ src, int sh, int sw, float* __restrict__ dst, int h, int w, ngp_feat_blur b,
                                                         float* __restrict__ sub, int subw) {
    __shared__ float s_src[FEAT_PH * FEAT_PW];
    __shared__ float s_row[FEAT_PH * FEAT_TW];
    const int r = b.r, tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * FEAT_TW, y0 = (int)blockIdx.y * FEAT_TH;
    const int pw = FEAT_TW + 2 * r, ph = FEAT_TH + 2 * r;
    for (int i = tid; i < ph * pw; i += FEAT_BLOCK) {
        const int ly = i / pw, lx = i - ly * pw;
        const int gy = ngp_feat_fold(y0 - r + ly, h), gx = ngp_feat_fold(x0 - r + lx, w);     // any index folds to a pixel of the image: tiles past its end stay inside
        s_src[i] = SRC ? ngp_feat_up(src, sh, sw, gy, gx) : src[(size_t)gy * (size_t)w + (size_t)gx];
    }
    __syncthreads();
    for (int i = tid; i < ph * FEAT_TW; i += FEAT_BLOCK) {
        const int ly = i / FEAT_TW, lx = i % FEAT_TW;
        s_row[i] = ngp_feat_taps(b.w, r, &s_src[ly * pw + lx + r], 1);
    }
    __syncthreads();
    for (int i = tid; i < FEAT_TH * FEAT_TW; i += FEAT_BLOCK) {
        const int ly = i / FEAT_TW, lx = i % FEAT_TW;
        const int y = y0 + ly, x = x0 + lx;
        if (y < h && x < w) {
            const float v = ngp_feat_taps(b.w, r, &s_row[(ly + r) * FEAT_TW + lx], FEAT_TW);
            dst[(size_t)y * (size_t)w + (size_t)x] = v;
            if (sub && !(y & 1) && !(x & 1)) sub[(size_t)(y >> 1) * (size_t)subw + (size_t)(x >> 1)] = v;
        }
    }
}

__global__ __launch_bounds__(FEAT_BLOCK) void k_feat_extrema(ngp_feat_oct o, ngp_feat_params P, float scale, uint8_t* __restrict__ mask, int H, int W) {
    const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u)), y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (x < o.w && y < o.h) ngp_feat_pixel(o, P, scale, y, x, mask, H, W);
}

__global__ __launch_bounds__(FEAT_BLOCK) void k_feat_stamp(const uint8_t* __restrict__ mask, int H, int W, int radius, uint8_t* __restrict__ dilated) {
    const uint32_t i = blockIdx.x * FEAT_BLOCK + threadIdx.x;
    if (i < (uint32_t)H * (uint32_t)W && mask[i]) ngp_feat_stamp(dilated, H, W, radius, (int)(i / (uint32_t)W), (int)(i % (uint32_t)W));
}

// lane t of the image in (column, row) order: pixel (t % H, t / H)
__global__ __launch_bounds__(FEAT_CHUNK) void k_feat_count(const uint8_t* __restrict__ dilated, int H, int W, uint32_t* __restrict__ counts,
                                                          unsigned long long* __restrict__ bitmap) {
    __shared__ uint32_t s_cnt[FEAT_CHUNK / 64];
    const uint32_t tid = threadIdx.x, t = blockIdx.x * FEAT_CHUNK + tid, wave = tid >> 6;
    bool on = false;
    if (t < (uint32_t)H * (uint32_t)W) on = dilated[(size_t)(t % (uint32_t)H) * (size_t)W + (size_t)(t / (uint32_t)H)] != 0;
    const unsigned long long word = __ballot(on);
    if ((tid & 63u) == 0u) { bitmap[(size_t)blockIdx.x * (FEAT_CHUNK / 64) + wave] = word; s_cnt[wave] = (uint32_t)__popcll(word); }
    __syncthreads();
    if (tid == 0) {
        uint32_t c = 0;
        #pragma unroll
        for (uint32_t k = 0; k < FEAT_CHUNK / 64; k++) c += s_cnt[k];
        counts[blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(FEAT_CHUNK) void k_feat_list_write(const uint32_t* __restrict__ counts, const unsigned long long* __restrict__ bitmap, uint32_t nchunks,
                                                               uint32_t H, int32_t* __restrict__ regions, uint32_t* __restrict__ count) {
    __shared__ uint32_t s_part[FEAT_CHUNK / 64], s_cnt[FEAT_CHUNK / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, chunk = blockIdx.x;
    uint32_t before = 0;
    for (uint32_t c = tid; c < chunk; c += FEAT_CHUNK) before += counts[c];
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_down(before, off, 64);
    const unsigned long long word = bitmap[(size_t)chunk * (FEAT_CHUNK / 64) + wave];
    if (lane == 0) { s_part[wave] = before; s_cnt[wave] = (uint32_t)__popcll(word); }
    __syncthreads();
    uint32_t base = 0, own = 0;
    #pragma unroll
    for (uint32_t k = 0; k < FEAT_CHUNK / 64; k++) { base += s_part[k]; if (k < wave) base += s_cnt[k]; own += s_cnt[k]; }
    if ((word >> lane) & 1ull) {                                           // a set bit is a pixel inside the image: k_feat_count sets none past it
        const uint32_t t = chunk * FEAT_CHUNK + tid, at = base + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
        regions[2 * (size_t)at] = (int32_t)(t % H);
        regions[2 * (size_t)at + 1] = (int32_t)(t / H);
    }
    if (chunk == nchunks - 1 && tid == 0) {
        uint32_t total = own;
        #pragma unroll
        for (uint32_t k = 0; k < FEAT_CHUNK / 64; k++) total += s_part[k];
        count[0] = total;
    }
}

__global__ __launch_bounds__(FEAT_BLOCK) void k_feat_draw(const int32_t* __restrict__ regions, uint32_t M, uint32_t B, uint32_t total, uint32_t half, uint32_t seed,
                                                         int32_t* __restrict__ batches) {
    const uint32_t i = blockIdx.x * FEAT_BLOCK + threadIdx.x;
    if (i >= total) return;
    const uint32_t k = i / B, j = i - k * B;
    const uint32_t p = ngp_feat_permute(j, M, half, ngp_feat_key(seed, k));
    batches[2 * (size_t)i] = regions[2 * (size_t)p];
    batches[2 * (size_t)i + 1] = regions[2 * (size_t)p + 1];
}

// ---------------------------------------------------------------------------
// workspace: [pyramid: per octave 6 levels of float32 [h,w] | dilated mask [H,W] u8 (cleared by the call) | per-chunk counts | bitmap]
// ---------------------------------------------------------------------------
struct feat_ws { float* pyramid; uint8_t* dilated; uint32_t* counts; unsigned long long* bitmap; size_t total; };
static bool feat_shape_ok(uint32_t H, uint32_t W) { return H >= NGP_FEAT_MIN_SIDE && W >= NGP_FEAT_MIN_SIDE && H <= NGP_FEAT_MAX_SIDE && W <= NGP_FEAT_MAX_SIDE; }
static feat_ws feat_layout(uint32_t H, uint32_t W, void* base) {
    const size_t nch = ngp_div_up((uint64_t)H * W, FEAT_CHUNK);
    ngp_carver c(base);
    return {c.take<float>(ngp_feat_shape_of(H, W).floats), c.take<uint8_t>((size_t)H * W), c.take<uint32_t>(nch), c.take<unsigned long long>(nch * (FEAT_CHUNK / 64)),
            c.total(256)};
}

extern "C" size_t ngp_features_workspace(uint32_t H, uint32_t W) { return feat_shape_ok(H, W) ? feat_layout(H, W, nullptr).total : 0; }

extern "C" int ngp_features_layout(uint32_t H, uint32_t W, uint64_t* out_host) {
    NGP_REQUIRE(out_host, "features_layout: null pointer");
    NGP_REQUIRE(feat_shape_ok(H, W), "features_layout: image %u x %u; supported from %u to %u pixels a side", H, W, NGP_FEAT_MIN_SIDE, NGP_FEAT_MAX_SIDE);
    unsigned char* block = reinterpret_cast<unsigned char*>((uintptr_t)4096);       // the carver never touches the block: only offsets are taken
    const feat_ws w = feat_layout(H, W, block);
    const ngp_feat_shape S = ngp_feat_shape_of(H, W);
    out_host[0] = (uint64_t)S.n_oct;
    out_host[1] = (uint64_t)((unsigned char*)w.dilated - block);
    out_host[2] = (uint64_t)((unsigned char*)w.counts - block);
    out_host[3] = (uint64_t)((unsigned char*)w.bitmap - block);
    for (int o = 0; o < NGP_FEAT_MAX_OCTAVES; o++) {
        out_host[4 + 3 * o] = o < S.n_oct ? (uint64_t)S.h[o] : 0;
        out_host[5 + 3 * o] = o < S.n_oct ? (uint64_t)S.w[o] : 0;
        out_host[6 + 3 * o] = o < S.n_oct ? (uint64_t)((unsigned char*)w.pyramid - block) + S.off[o] * sizeof(float) : 0;
    }
    return NGP_OK;
}

extern "C" void ngp_features_default_cfg(ngp_features_cfg_t* cfg) {
    if (!cfg) return;
    cfg->contrast = 0.04f; cfg->edge = 10.0f; cfg->sigma = 1.6f; cfg->layers = 3; cfg->border = 5;
}

static int feat_detect_args(const char* who, const float* image, uint32_t H, uint32_t W, const ngp_features_cfg_t* c, const uint8_t* mask, void* ws, size_t ws_bytes,
                            feat_ws& w) {
    NGP_REQUIRE(image && c && mask, "%s: null pointer", who);
    NGP_REQUIRE(feat_shape_ok(H, W), "%s: image %u x %u; supported from %u to %u pixels a side", who, H, W, NGP_FEAT_MIN_SIDE, NGP_FEAT_MAX_SIDE);
    NGP_REQUIRE(c->layers >= 1 && c->layers <= (uint32_t)NGP_FEAT_MAX_LAYERS, "%s: layers = %u; supported 1..%d", who, c->layers, NGP_FEAT_MAX_LAYERS);
    NGP_REQUIRE(c->border >= 1 && c->border <= 64, "%s: border = %u; supported 1..64 (a candidate needs its 26 neighbours)", who, c->border);
    NGP_REQUIRE(c->sigma > 1.0f && c->sigma <= 4.0f, "%s: sigma = %g; supported above 1 (the upsampled image counts as blurred by 1) up to 4", who, (double)c->sigma);
    NGP_REQUIRE(c->contrast >= 0.0f && c->edge > 0.0f, "%s: contrast = %g, edge = %g; contrast must not be negative, edge must be positive", who, (double)c->contrast,
                (double)c->edge);
    w = feat_layout(H, W, ws);
    if (!ws || ws_bytes < w.total)
        return ngp_fail(NGP_EWORKSPACE, "%s: workspace of %zu bytes, needs ngp_features_workspace(H, W) = %zu", who, ws_bytes, w.total);
    return NGP_OK;
}

extern "C" int ngp_features_detect(const float* image, uint32_t H, uint32_t W, const ngp_features_cfg_t* cfg_host, uint8_t* mask, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    feat_ws w;
    const int rc = feat_detect_args("features_detect", image, H, W, cfg_host, mask, workspace, workspace_bytes, w);
    if (rc != NGP_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const ngp_feat_shape S = ngp_feat_shape_of(H, W);
    const int layers = (int)cfg_host->layers;
    const ngp_feat_params P = ngp_feat_params_of(cfg_host->contrast, cfg_host->edge, layers, (int)cfg_host->border);
    ngp_feat_blur blur[NGP_FEAT_LEVELS];
    ngp_feat_blurs_of(cfg_host->sigma, layers, blur);
    if (hipMemsetAsync(mask, 0, (size_t)H * W, st) != hipSuccess) return ngp_fail(NGP_ELAUNCH, "features_detect: cannot clear the mask");
    auto tiles = [](int h, int w) { return dim3(ngp_div_up((uint64_t)w, FEAT_TW), ngp_div_up((uint64_t)h, FEAT_TH)); };
    hipLaunchKernelGGL(k_feat_blur<1>, tiles(S.h[0], S.w[0]), dim3(FEAT_BLOCK), 0, st, image, (int)H, (int)W, w.pyramid, S.h[0], S.w[0], blur[0], (float*)nullptr, 0);
    NGP_CHECK_LAUNCH("features_detect (base)");
    for (int o = 0; o < S.n_oct; o++) {
        const int h = S.h[o], wd = S.w[o];
        const size_t hw = (size_t)h * (size_t)wd;
        float* g = w.pyramid + S.off[o];
        for (int i = 1; i < layers + 3; i++) {
            const bool feeds = i == layers && o + 1 < S.n_oct;
            hipLaunchKernelGGL(k_feat_blur<0>, tiles(h, wd), dim3(FEAT_BLOCK), 0, st, (const float*)(g + (size_t)(i - 1) * hw), 0, 0, g + (size_t)i * hw, h, wd, blur[i],
                               feeds ? w.pyramid + S.off[o + 1] : (float*)nullptr, feeds ? S.w[o + 1] : 0);
        }
        NGP_CHECK_LAUNCH("features_detect (levels)");
        const ngp_feat_oct oct = {g, h, wd, hw};
        hipLaunchKernelGGL(k_feat_extrema, dim3(ngp_div_up((uint64_t)wd, 64), ngp_div_up((uint64_t)h, 4)), dim3(FEAT_BLOCK), 0, st, oct, P, ldexpf(0.5f, o), mask, (int)H,
                           (int)W);
        NGP_CHECK_LAUNCH("features_detect (extrema)");
    }
    return NGP_OK;
}

extern "C" int ngp_features_detect_host(const float* image, uint32_t H, uint32_t W, const ngp_features_cfg_t* cfg_host, uint8_t* mask, void* workspace,
                                        size_t workspace_bytes) {
    feat_ws w;
    const int rc = feat_detect_args("features_detect_host", image, H, W, cfg_host, mask, workspace, workspace_bytes, w);
    if (rc != NGP_OK) return rc;
    ngp_feat_detect_host(image, H, W, cfg_host->contrast, cfg_host->edge, cfg_host->sigma, (int)cfg_host->layers, (int)cfg_host->border, w.pyramid, mask);
    return NGP_OK;
}

static int feat_regions_args(const char* who, const uint8_t* mask, uint32_t H, uint32_t W, uint32_t kernel_size, uint32_t dil_iter, const int32_t* regions,
                             const uint32_t* count, void* ws, size_t ws_bytes, feat_ws& w, int& radius) {
    NGP_REQUIRE(mask && regions && count, "%s: null pointer", who);
    NGP_REQUIRE(feat_shape_ok(H, W), "%s: image %u x %u; supported from %u to %u pixels a side", who, H, W, NGP_FEAT_MIN_SIDE, NGP_FEAT_MAX_SIDE);
    NGP_REQUIRE(kernel_size >= 1 && (kernel_size & 1u), "%s: kernel_size = %u must be odd (the kernel has a centre)", who, kernel_size);
    NGP_REQUIRE(dil_iter >= 1, "%s: dil_iter = 0 (no dilation to run)", who);
    NGP_REQUIRE((uint64_t)dil_iter * (kernel_size - 1u) / 2u <= NGP_FEAT_MAX_SIDE, "%s: kernel_size = %u, dil_iter = %u reach further than any image", who, kernel_size,
                dil_iter);
    radius = (int)(dil_iter * (kernel_size - 1u) / 2u);
    w = feat_layout(H, W, ws);
    if (!ws || ws_bytes < w.total)
        return ngp_fail(NGP_EWORKSPACE, "%s: workspace of %zu bytes, needs ngp_features_workspace(H, W) = %zu", who, ws_bytes, w.total);
    return NGP_OK;
}

extern "C" int ngp_features_regions(const uint8_t* mask, uint32_t H, uint32_t W, uint32_t kernel_size, uint32_t dil_iter, int32_t* regions, uint32_t* count_dev,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    feat_ws w;
    int radius;
    const int rc = feat_regions_args("features_regions", mask, H, W, kernel_size, dil_iter, regions, count_dev, workspace, workspace_bytes, w, radius);
    if (rc != NGP_OK) return rc;
    const uint32_t nch = ngp_div_up((uint64_t)H * W, FEAT_CHUNK);
    if (hipMemsetAsync(w.dilated, 0, (size_t)H * W, (hipStream_t)stream) != hipSuccess) return ngp_fail(NGP_ELAUNCH, "features_regions: cannot clear the dilated mask");
    hipLaunchKernelGGL(k_feat_stamp, dim3(ngp_div_up((uint64_t)H * W, FEAT_BLOCK)), dim3(FEAT_BLOCK), 0, (hipStream_t)stream, mask, (int)H, (int)W, radius, w.dilated);
    hipLaunchKernelGGL(k_feat_count, dim3(nch), dim3(FEAT_CHUNK), 0, (hipStream_t)stream, (const uint8_t*)w.dilated, (int)H, (int)W, w.counts, w.bitmap);
    hipLaunchKernelGGL(k_feat_list_write, dim3(nch), dim3(FEAT_CHUNK), 0, (hipStream_t)stream, (const uint32_t*)w.counts, (const unsigned long long*)w.bitmap, nch, H,
                       regions, count_dev);
    NGP_CHECK_LAUNCH("features_regions");
    return NGP_OK;
}

extern "C" int ngp_features_regions_host(const uint8_t* mask, uint32_t H, uint32_t W, uint32_t kernel_size, uint32_t dil_iter, int32_t* regions, uint32_t* count_host,
                                         void* workspace, size_t workspace_bytes) {
    feat_ws w;
    int radius;
    const int rc = feat_regions_args("features_regions_host", mask, H, W, kernel_size, dil_iter, regions, count_host, workspace, workspace_bytes, w, radius);
    if (rc != NGP_OK) return rc;
    count_host[0] = ngp_feat_regions_host(mask, H, W, radius, w.dilated, regions);
    return NGP_OK;
}

static int feat_draw_args(const char* who, const int32_t* regions, uint32_t M, uint32_t B, uint32_t n_iter, const int32_t* batches) {
    NGP_REQUIRE(regions && batches, "%s: null pointer", who);
    NGP_REQUIRE(B >= 1, "%s: B = 0 (an empty batch)", who);
    NGP_REQUIRE(M >= 1, "%s: M = 0 (no interest points to draw from)", who);
    NGP_REQUIRE(M >= B, "%s: %u interest points cannot fill a batch of %u without replacement", who, M, B);
    NGP_REQUIRE(M <= NGP_FEAT_MAX_SIDE * NGP_FEAT_MAX_SIDE, "%s: M = %u; an image holds at most %u pixels", who, M, NGP_FEAT_MAX_SIDE * NGP_FEAT_MAX_SIDE);
    NGP_REQUIRE((uint64_t)B * n_iter < (1ull << 31), "%s: %u batches of %u entries; supported below 2^31 entries in all", who, n_iter, B);
    return NGP_OK;
}

extern "C" int ngp_features_draw(const int32_t* regions, uint32_t M, uint32_t B, uint32_t n_iter, uint32_t seed, int32_t* batches, void* stream) {
    const int rc = feat_draw_args("features_draw", regions, M, B, n_iter, batches);
    if (rc != NGP_OK) return rc;
    if (n_iter == 0) return NGP_OK;
    const uint32_t total = B * n_iter;
    hipLaunchKernelGGL(k_feat_draw, dim3(ngp_div_up(total, FEAT_BLOCK)), dim3(FEAT_BLOCK), 0, (hipStream_t)stream, regions, M, B, total, ngp_feat_half_bits(M), seed, batches);
    NGP_CHECK_LAUNCH("features_draw");
    return NGP_OK;
}

extern "C" int ngp_features_draw_host(const int32_t* regions, uint32_t M, uint32_t B, uint32_t n_iter, uint32_t seed, int32_t* batches) {
    const int rc = feat_draw_args("features_draw_host", regions, M, B, n_iter, batches);
    if (rc != NGP_OK) return rc;
    ngp_feat_draw_host(regions, M, B, n_iter, seed, batches);
    return NGP_OK;
}
