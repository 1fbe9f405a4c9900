// ngp_select.h -- the one rule by which the multi-start routes of the pose filter (nav_filter.hip) and of the planner (nav_plan.hip) pick the best of K
// hypotheses: compiled for the selection kernels and for their host twins (ngp_filter_select_host, ngp_plan_select_host).
#pragma once
#include <stdint.h>

// the best of K final losses, indices in ascending order: a candidate replaces the best when its loss is smaller, or when the best is NaN and the
// candidate is not; so ties keep the lowest index and K NaNs give index 0
__host__ __device__ inline uint32_t ngp_select_best(const float* losses, uint32_t K) {
    uint32_t best = 0;
    for (uint32_t i = 1; i < K; i++) {
        const float l = losses[i], b = losses[best];
        if (l < b || (b != b && l == l)) best = i;
    }
    return best;
}
