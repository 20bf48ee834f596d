// Helpers shared by the per-jet observable kernels (jet_obs.hip, jet_efp.hip): the pair distance and the fixed-order
// workgroup reductions that make two launches on the same input give the same bits.
#pragma once
#include "common.h"

namespace {

MPG_DEV float theta(float e1, float p1, float e2, float p2) {
    const float de = e1 - e2, dp = p1 - p2;
    return sqrtf(de * de + dp * dp);
}

MPG_DEV float wave_sum_xor(float x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// sum of v[k] over the workgroup, fixed order; every thread gets the totals.  `red` holds NW * 8 floats.
template <int NW, int K>
MPG_DEV void block_sums(float (&v)[K], float* red) {
    static_assert(K <= 8, "red holds 8 values per wave");
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float s = wave_sum_xor(v[k]);
        if (lane == 0) red[wv * 8 + k] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) s += red[w * 8 + k];
        v[k] = s;
    }
    __syncthreads();
}

}  // namespace
