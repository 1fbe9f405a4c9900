// The pose filter's interest regions (nav_features.hip), written once for the kernels and for the host exports ngp_features_*_host, which the CPU tests
// drive; compiles with a plain C++ compiler too (tests/helpers/features_check.cpp).  DESIGN.md 3.5 "Native interest regions" holds the contract:
// Lowe's difference-of-Gaussians detector with OpenCV's default parameters on an aligned 2x upsample, keypoint positions only; a square dilation; the
// pixel list in (column, row) order; batches by a keyed Feistel permutation.  All image arithmetic is float32, one rounding per written operation (the
// library is built with -ffp-contract=off), so the kernels, the host route below and tests/_features_restated.py agree bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NGP_FEAT_HD __host__ __device__ __forceinline__
#else
#define NGP_FEAT_HD inline
#endif

static constexpr int NGP_FEAT_MAX_RADIUS = 12;                 // a blur's taps reach at most 12 pixels to either side
static constexpr int NGP_FEAT_MAX_LAYERS = 3;                  // S; an octave holds S + 3 Gaussian levels, the workspace is laid out for 6
static constexpr int NGP_FEAT_LEVELS = NGP_FEAT_MAX_LAYERS + 3;
static constexpr int NGP_FEAT_MAX_OCTAVES = 12;                // 4096 x 4096 has 11
static constexpr int NGP_FEAT_ATTEMPTS = 5;
static constexpr int NGP_FEAT_ROUNDS = 4;                      // Feistel rounds of the batch draw
static constexpr uint32_t NGP_FEAT_MIN_SIDE = 16, NGP_FEAT_MAX_SIDE = 4096;

struct ngp_feat_blur { float w[NGP_FEAT_MAX_RADIUS + 1]; int r; };          // w[0] the centre weight, w[i] that of both pixels at distance i
struct ngp_feat_params {                                                     // the detector's thresholds as the per-pixel code reads them
    float threshold;                                                         // 0.5f * contrast / layers: a candidate has |d| above it
    float contrast, edge, layers_f;
    int layers, border;
};
struct ngp_feat_oct { const float* g; int h, w; size_t hw; };               // one octave: layers + 3 levels of [h,w] back to back, NGP_FEAT_LEVELS * hw apart per octave

// ---------------------------------------------------------------------------
// per pixel
// ---------------------------------------------------------------------------
// reflect-101 for any index: folded with period 2(n - 1); n >= 2
NGP_FEAT_HD int ngp_feat_fold(int i, int n) {
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

NGP_FEAT_HD float ngp_feat_gray(const float* img, int W, int r, int c) {
    const float* p = img + 3 * ((size_t)r * (size_t)W + (size_t)c);
    return (0.299f * p[0] + 0.587f * p[1]) + 0.114f * p[2];
}

// pixel (y, x) of the aligned 2x upsample of the gray image: u[2r,2c] IS g[r,c]; the index past the edge is reflected (n -> n - 2)
NGP_FEAT_HD float ngp_feat_up(const float* img, int H, int W, int y, int x) {
    const int r = y >> 1, c = x >> 1;
    const int r1 = r + 1 < H ? r + 1 : H - 2, c1 = c + 1 < W ? c + 1 : W - 2;
    const float g00 = ngp_feat_gray(img, W, r, c);
    if (!(y & 1) && !(x & 1)) return g00;
    if (!(y & 1)) return (g00 + ngp_feat_gray(img, W, r, c1)) * 0.5f;
    if (!(x & 1)) return (g00 + ngp_feat_gray(img, W, r1, c)) * 0.5f;
    return ((g00 + ngp_feat_gray(img, W, r, c1)) + (ngp_feat_gray(img, W, r1, c) + ngp_feat_gray(img, W, r1, c1))) * 0.25f;
}

// one pass of a blur at one pixel: `centre` points into a line that is already folded at its ends, neighbours `stride` apart
NGP_FEAT_HD float ngp_feat_taps(const float* w, int r, const float* centre, ptrdiff_t stride) {
    float acc = w[0] * centre[0];
    for (int i = 1; i <= r; i++) acc = acc + w[i] * (centre[-i * stride] + centre[i * stride]);
    return acc;
}

NGP_FEAT_HD float ngp_feat_dog(const ngp_feat_oct& o, int s, int y, int x) {
    const size_t i = (size_t)y * (size_t)o.w + (size_t)x;
    return o.g[(size_t)(s + 1) * o.hw + i] - o.g[(size_t)s * o.hw + i];
}

// |d| above the threshold and d not below (d > 0) / not above (d < 0) any of its 26 neighbours; ties pass
NGP_FEAT_HD bool ngp_feat_is_extremum(const ngp_feat_oct& o, float threshold, int s, int y, int x) {
    const float d = ngp_feat_dog(o, s, y, x);
    if (!(fabsf(d) > threshold)) return false;
    for (int ds = -1; ds <= 1; ds++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const float v = ngp_feat_dog(o, s + ds, y + dy, x + dx);
                if (d > 0.0f ? v > d : v < d) return false;
            }
    return true;
}

// Lowe 4 / OpenCV's adjustLocalExtrema from the candidate (s, y, x); true when it survives, with the sub-pixel column and row in (px, py)
NGP_FEAT_HD bool ngp_feat_refine(const ngp_feat_oct& o, const ngp_feat_params& P, int s, int y, int x, float& px, float& py) {
    for (int attempt = 0; attempt < NGP_FEAT_ATTEMPTS; attempt++) {
        const float v = ngp_feat_dog(o, s, y, x), v2 = v * 2.0f;
        const float xm = ngp_feat_dog(o, s, y, x - 1), xp = ngp_feat_dog(o, s, y, x + 1);
        const float ym = ngp_feat_dog(o, s, y - 1, x), yp = ngp_feat_dog(o, s, y + 1, x);
        const float sm = ngp_feat_dog(o, s - 1, y, x), sp = ngp_feat_dog(o, s + 1, y, x);
        const float gx = (xp - xm) * 0.5f, gy = (yp - ym) * 0.5f, gs = (sp - sm) * 0.5f;
        const float a = (xp + xm) - v2, d = (yp + ym) - v2, f = (sp + sm) - v2;                                  // dxx, dyy, dss
        const float b = (((ngp_feat_dog(o, s, y + 1, x + 1) - ngp_feat_dog(o, s, y + 1, x - 1)) - ngp_feat_dog(o, s, y - 1, x + 1)) +
                         ngp_feat_dog(o, s, y - 1, x - 1)) * 0.25f;                                               // dxy
        const float c = (((ngp_feat_dog(o, s + 1, y, x + 1) - ngp_feat_dog(o, s + 1, y, x - 1)) - ngp_feat_dog(o, s - 1, y, x + 1)) +
                         ngp_feat_dog(o, s - 1, y, x - 1)) * 0.25f;                                               // dxs
        const float e = (((ngp_feat_dog(o, s + 1, y + 1, x) - ngp_feat_dog(o, s + 1, y - 1, x)) - ngp_feat_dog(o, s - 1, y + 1, x)) +
                         ngp_feat_dog(o, s - 1, y - 1, x)) * 0.25f;                                               // dys
        // x = -H^-1 g through the adjugate of the symmetric H = [a b c; b d e; c e f]
        const float A00 = d * f - e * e, A01 = c * e - b * f, A02 = b * e - c * d;
        const float A11 = a * f - c * c, A12 = b * c - a * e, A22 = a * d - b * b;
        const float det = (a * A00 + b * A01) + c * A02;
        if (det == 0.0f) return false;
        const float xc = -(((A00 * gx + A01 * gy) + A02 * gs) / det);
        const float xr = -(((A01 * gx + A11 * gy) + A12 * gs) / det);
        const float xs = -(((A02 * gx + A12 * gy) + A22 * gs) / det);
        if (fabsf(xc) < 0.5f && fabsf(xr) < 0.5f && fabsf(xs) < 0.5f) {
            const float contr = v + 0.5f * ((gx * xc + gy * xr) + gs * xs);
            if (!(fabsf(contr) * P.layers_f >= P.contrast)) return false;
            const float tr = a + d, det2 = a * d - b * b;
            if (!(det2 > 0.0f)) return false;
            if (!((tr * tr) * P.edge < ((P.edge + 1.0f) * (P.edge + 1.0f)) * det2)) return false;
            px = (float)x + xc;
            py = (float)y + xr;
            return true;
        }
        if (!(fabsf(xc) <= 1.0e6f && fabsf(xr) <= 1.0e6f && fabsf(xs) <= 1.0e6f)) return false;                  // (also an infinite or NaN offset)
        x += (int)rintf(xc);
        y += (int)rintf(xr);
        s += (int)rintf(xs);
        if (s < 1 || s > P.layers || x < P.border || x >= o.w - P.border || y < P.border || y >= o.h - P.border) return false;
    }
    return false;
}

// everything one pixel (y, x) of an octave does: test its layers, refine, stamp the [H,W] mask.  scale = 2^octave / 2 maps back to the image.
NGP_FEAT_HD void ngp_feat_pixel(const ngp_feat_oct& o, const ngp_feat_params& P, float scale, int y, int x, uint8_t* mask, int H, int W) {
    if (x < P.border || x >= o.w - P.border || y < P.border || y >= o.h - P.border) return;
    for (int s = 1; s <= P.layers; s++) {
        if (!ngp_feat_is_extremum(o, P.threshold, s, y, x)) continue;
        float px, py;
        if (!ngp_feat_refine(o, P, s, y, x, px, py)) continue;
        const int ix = (int)(px * scale), iy = (int)(py * scale);
        if ((uint32_t)ix < (uint32_t)W && (uint32_t)iy < (uint32_t)H) mask[(size_t)iy * (size_t)W + (size_t)ix] = 1;
    }
}

// cv2.dilate with a k x k kernel of ones, I iterations: one square of radius R = I (k - 1) / 2 around every set pixel, clipped at the image edge.  What a
// set pixel (row, col) of the mask does to the cleared `dilated`: plain stores of one value, so pixels whose squares overlap may run in any order, or at once.
NGP_FEAT_HD void ngp_feat_stamp(uint8_t* dilated, int H, int W, int R, int row, int col) {
    const int r0 = row - R > 0 ? row - R : 0, r1 = row + R < H - 1 ? row + R : H - 1;
    const int c0 = col - R > 0 ? col - R : 0, c1 = col + R < W - 1 ? col + R : W - 1;
    for (int r = r0; r <= r1; r++)
        for (int c = c0; c <= c1; c++) dilated[(size_t)r * (size_t)W + (size_t)c] = 1;
}

// ---------------------------------------------------------------------------
// the batch draw: a keyed bijection of [0, M)
// ---------------------------------------------------------------------------
NGP_FEAT_HD uint32_t ngp_feat_mix(uint32_t h) {                             // murmur3's finaliser
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
NGP_FEAT_HD uint32_t ngp_feat_key(uint32_t seed, uint32_t k) { return ngp_feat_mix(seed ^ ngp_feat_mix(k + 0x9E3779B9u)); }
// half the bits of the next even power of two >= M (at least 1)
NGP_FEAT_HD uint32_t ngp_feat_half_bits(uint32_t M) {
    uint32_t bits = 0;
    while (bits < 32u && ((uint64_t)1 << bits) < (uint64_t)M) bits++;
    const uint32_t half = (bits + 1u) >> 1;
    return half ? half : 1u;
}
// A balanced Feistel network of NGP_FEAT_ROUNDS rounds over 2 * half bits, walked until it lands below M.  v < M, and v's cycle leads back to v,
// so the walk ends; the domain is below 4 M, so it takes 4 trips on average at the most.
NGP_FEAT_HD uint32_t ngp_feat_permute(uint32_t v, uint32_t M, uint32_t half, uint32_t key) {
    const uint32_t low = (1u << half) - 1u;
    do {
        uint32_t L = v >> half, R = v & low;
        for (uint32_t r = 0; r < (uint32_t)NGP_FEAT_ROUNDS; r++) {
            const uint32_t t = L ^ (ngp_feat_mix((R + key) + r * 0x9E3779B9u) & low);
            L = R;
            R = t;
        }
        v = (L << half) | R;
    } while (v >= M);
    return v;
}

// ---------------------------------------------------------------------------
// host: the pyramid's shape and weights, and the whole pipeline level by level
// ---------------------------------------------------------------------------
struct ngp_feat_shape {
    int n_oct;
    int h[NGP_FEAT_MAX_OCTAVES], w[NGP_FEAT_MAX_OCTAVES];
    size_t off[NGP_FEAT_MAX_OCTAVES];                          // where octave o's level 0 begins, in floats
    size_t floats;                                             // NGP_FEAT_LEVELS levels per octave
};
inline ngp_feat_shape ngp_feat_shape_of(uint32_t H, uint32_t W) {
    ngp_feat_shape s;
    const uint32_t least = 2u * (H < W ? H : W);
    s.n_oct = (int)lround(log2((double)least)) - 2;
    if (s.n_oct < 1) s.n_oct = 1;
    if (s.n_oct > NGP_FEAT_MAX_OCTAVES) s.n_oct = NGP_FEAT_MAX_OCTAVES;
    int h = (int)(2u * H), w = (int)(2u * W);
    s.floats = 0;
    for (int o = 0; o < s.n_oct; o++) {
        s.h[o] = h; s.w[o] = w; s.off[o] = s.floats;
        s.floats += (size_t)NGP_FEAT_LEVELS * (size_t)h * (size_t)w;
        h = (h + 1) / 2; w = (w + 1) / 2;                      // every second row and column from 0
    }
    return s;
}

// weights exp(-i^2 / 2 sigma^2) over their sum, in double, rounded once
inline ngp_feat_blur ngp_feat_blur_of(double sigma) {
    ngp_feat_blur b;
    int r = (int)(4.0 * sigma + 0.5);
    b.r = r > NGP_FEAT_MAX_RADIUS ? NGP_FEAT_MAX_RADIUS : r;
    double e[NGP_FEAT_MAX_RADIUS + 1], sum = 1.0;
    e[0] = 1.0;
    for (int i = 1; i <= b.r; i++) { e[i] = exp(-(double)(i * i) / (2.0 * sigma * sigma)); sum += 2.0 * e[i]; }
    for (int i = 0; i <= NGP_FEAT_MAX_RADIUS; i++) b.w[i] = i <= b.r ? (float)(e[i] / sum) : 0.0f;
    return b;
}
// blur[0]: the base image's (the upsample counts as sigma 1.0); blur[i], i >= 1: from level i - 1 to level i
inline void ngp_feat_blurs_of(float sigma_f, int layers, ngp_feat_blur* blur) {
    const double sigma = (double)sigma_f, k = pow(2.0, 1.0 / (double)layers);
    blur[0] = ngp_feat_blur_of(sqrt(sigma * sigma - 1.0));
    for (int i = 1; i < layers + 3; i++) {
        const double prev = sigma * pow(k, (double)(i - 1)), total = prev * k;
        blur[i] = ngp_feat_blur_of(sqrt(total * total - prev * prev));
    }
}
inline ngp_feat_params ngp_feat_params_of(float contrast, float edge, int layers, int border) {
    ngp_feat_params P;
    P.layers_f = (float)layers;
    P.threshold = (0.5f * contrast) / P.layers_f;
    P.contrast = contrast; P.edge = edge; P.layers = layers; P.border = border;
    return P;
}

// rows first, then columns, each line folded at its ends into a padded copy
inline void ngp_feat_blur_host(const float* src, float* dst, int h, int w, const ngp_feat_blur& b) {
    const int r = b.r;
    std::vector<float> rowed((size_t)h * (size_t)w), line((size_t)(h > w ? h : w) + 2 * (size_t)r);
    for (int y = 0; y < h; y++) {
        for (int i = -r; i < w + r; i++) line[(size_t)(i + r)] = src[(size_t)y * (size_t)w + (size_t)ngp_feat_fold(i, w)];
        for (int x = 0; x < w; x++) rowed[(size_t)y * (size_t)w + (size_t)x] = ngp_feat_taps(b.w, r, &line[(size_t)(x + r)], 1);
    }
    for (int x = 0; x < w; x++) {
        for (int i = -r; i < h + r; i++) line[(size_t)(i + r)] = rowed[(size_t)ngp_feat_fold(i, h) * (size_t)w + (size_t)x];
        for (int y = 0; y < h; y++) dst[(size_t)y * (size_t)w + (size_t)x] = ngp_feat_taps(b.w, r, &line[(size_t)(y + r)], 1);
    }
}

// image [H,W,3] -> pyramid (ngp_feat_shape_of(H, W).floats floats) and mask [H,W]
inline void ngp_feat_detect_host(const float* image, uint32_t H, uint32_t W, float contrast, float edge, float sigma, int layers, int border,
                                 float* pyramid, uint8_t* mask) {
    const ngp_feat_shape S = ngp_feat_shape_of(H, W);
    const ngp_feat_params P = ngp_feat_params_of(contrast, edge, layers, border);
    ngp_feat_blur blur[NGP_FEAT_LEVELS];
    ngp_feat_blurs_of(sigma, layers, blur);
    for (size_t i = 0; i < (size_t)H * (size_t)W; i++) mask[i] = 0;
    {
        std::vector<float> up((size_t)S.h[0] * (size_t)S.w[0]);
        for (int y = 0; y < S.h[0]; y++)
            for (int x = 0; x < S.w[0]; x++) up[(size_t)y * (size_t)S.w[0] + (size_t)x] = ngp_feat_up(image, (int)H, (int)W, y, x);
        ngp_feat_blur_host(up.data(), pyramid, S.h[0], S.w[0], blur[0]);
    }
    for (int o = 0; o < S.n_oct; o++) {
        const int h = S.h[o], w = S.w[o];
        const size_t hw = (size_t)h * (size_t)w;
        float* g = pyramid + S.off[o];
        for (int i = 1; i < layers + 3; i++) ngp_feat_blur_host(g + (size_t)(i - 1) * hw, g + (size_t)i * hw, h, w, blur[i]);
        if (o + 1 < S.n_oct) {
            float* next = pyramid + S.off[o + 1];
            for (int y = 0; y < S.h[o + 1]; y++)
                for (int x = 0; x < S.w[o + 1]; x++) next[(size_t)y * (size_t)S.w[o + 1] + (size_t)x] = g[(size_t)layers * hw + (size_t)(2 * y) * (size_t)w + (size_t)(2 * x)];
        }
        const ngp_feat_oct oct = {g, h, w, hw};
        const float scale = ldexpf(0.5f, o);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) ngp_feat_pixel(oct, P, scale, y, x, mask, (int)H, (int)W);
    }
}

// mask [H,W] -> dilated [H,W] and the list of its pixels as (row, col) pairs in ascending column, then row; returns their number
inline uint32_t ngp_feat_regions_host(const uint8_t* mask, uint32_t H, uint32_t W, int radius, uint8_t* dilated, int32_t* regions) {
    for (size_t i = 0; i < (size_t)H * W; i++) dilated[i] = 0;
    for (uint32_t row = 0; row < H; row++)
        for (uint32_t col = 0; col < W; col++)
            if (mask[(size_t)row * W + col]) ngp_feat_stamp(dilated, (int)H, (int)W, radius, (int)row, (int)col);
    uint32_t n = 0;
    for (uint32_t col = 0; col < W; col++)
        for (uint32_t row = 0; row < H; row++)
            if (dilated[(size_t)row * W + col]) { regions[2 * (size_t)n] = (int32_t)row; regions[2 * (size_t)n + 1] = (int32_t)col; n++; }
    return n;
}

// batches [n_iter,B,2]: batch k's entry j is regions[permute_{seed,k}(j)]
inline void ngp_feat_draw_host(const int32_t* regions, uint32_t M, uint32_t B, uint32_t n_iter, uint32_t seed, int32_t* batches) {
    const uint32_t half = ngp_feat_half_bits(M);
    for (uint32_t k = 0; k < n_iter; k++) {
        const uint32_t key = ngp_feat_key(seed, k);
        for (uint32_t j = 0; j < B; j++) {
            const uint32_t p = ngp_feat_permute(j, M, half, key);
            batches[2 * ((size_t)k * B + j)] = regions[2 * (size_t)p];
            batches[2 * ((size_t)k * B + j) + 1] = regions[2 * (size_t)p + 1];
        }
    }
}
