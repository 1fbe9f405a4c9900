// Stand-alone check of csrc/ngp_features.h, built with -fsanitize=address,undefined by tests/test_features_host.py.
// Runs the host pipeline (image -> pyramid -> mask -> dilated mask -> list -> batches) at 16 x 16 and 37 x 53 in buffers of exactly the sizes the
// layout asks for, so a fold that leaves its line or a stamp outside the mask is caught.  Exit status 0 and "features ok ..." on success.
#include "ngp_features.h"

#include <stdio.h>
#include <stdlib.h>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "features_check.cpp:%d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int run(uint32_t H, uint32_t W, uint32_t* keypoints, uint32_t* listed) {
    float* image = (float*)malloc(sizeof(float) * 3 * H * W);
    CHECK(image);
    uint32_t state = 12345u + H * 7919u + W;
    for (uint32_t i = 0; i < H * W; i++) {                                   // blocks of 3 x 3 pixels of one random gray, so that some structure survives the blurs
        const uint32_t r = i / W, c = i % W, cell = (r / 3) * 64 + c / 3;
        state = ngp_feat_mix(cell + 977u * H);
        const float v = (float)(state >> 8) / 16777216.0f;
        image[3 * i] = v; image[3 * i + 1] = v * 0.9f; image[3 * i + 2] = 1.0f - v;
    }
    const ngp_feat_shape S = ngp_feat_shape_of(H, W);
    CHECK(S.n_oct >= 1 && S.n_oct <= NGP_FEAT_MAX_OCTAVES);
    float* pyramid = (float*)malloc(sizeof(float) * S.floats);
    uint8_t* mask = (uint8_t*)malloc((size_t)H * W);
    uint8_t* dilated = (uint8_t*)malloc((size_t)H * W);
    int32_t* regions = (int32_t*)malloc(sizeof(int32_t) * 2 * H * W);
    CHECK(pyramid && mask && dilated && regions);
    ngp_feat_detect_host(image, H, W, 0.04f, 10.0f, 1.6f, 3, 5, pyramid, mask);
    uint32_t n = 0;
    for (uint32_t i = 0; i < H * W; i++) { CHECK(mask[i] <= 1); n += mask[i]; }
    for (int o = 0; o < S.n_oct; o++)
        for (size_t i = 0; i < (size_t)NGP_FEAT_LEVELS * S.h[o] * S.w[o]; i++) CHECK(pyramid[S.off[o] + i] >= 0.0f && pyramid[S.off[o] + i] <= 1.0001f);
    mask[0] = mask[(size_t)H * W - 1] = mask[W - 1] = 1;                     // corners: the dilation's square is clipped on two sides
    const uint32_t M = ngp_feat_regions_host(mask, H, W, 6, dilated, regions);
    CHECK(M >= 3 * 49 && M <= H * W);
    for (uint32_t i = 1; i < M; i++)
        CHECK(regions[2 * i + 1] > regions[2 * i - 1] || (regions[2 * i + 1] == regions[2 * i - 1] && regions[2 * i] > regions[2 * i - 2]));
    const uint32_t B = M < 64 ? M : 64, n_iter = 5;
    int32_t* batches = (int32_t*)malloc(sizeof(int32_t) * 2 * B * n_iter);
    CHECK(batches);
    ngp_feat_draw_host(regions, M, B, n_iter, 99u, batches);
    for (uint32_t i = 0; i < B * n_iter; i++) CHECK((uint32_t)batches[2 * i] < H && (uint32_t)batches[2 * i + 1] < W && dilated[(size_t)batches[2 * i] * W + batches[2 * i + 1]]);
    for (uint32_t v = 0; v < 64; v++) CHECK(ngp_feat_permute(v % 1u, 1u, ngp_feat_half_bits(1u), v) == 0u);      // M = 1: the smallest domain
    CHECK(ngp_feat_fold(-25, 8) == 3 && ngp_feat_fold(7, 8) == 7 && ngp_feat_fold(8, 8) == 6 && ngp_feat_fold(14, 8) == 0 && ngp_feat_fold(-1, 2) == 1);
    *keypoints = n; *listed = M;
    free(batches); free(regions); free(dilated); free(mask); free(pyramid); free(image);
    return 0;
}

int main() {
    uint32_t k0, m0, k1, m1;
    if (run(16, 16, &k0, &m0)) return 1;
    if (run(37, 53, &k1, &m1)) return 1;
    printf("features ok: 16x16 %u keypoint pixels, %u listed; 37x53 %u keypoint pixels, %u listed\n", k0, m0, k1, m1);
    return 0;
}
