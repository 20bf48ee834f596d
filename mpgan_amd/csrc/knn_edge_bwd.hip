// mpg_knn_edge_bwd: data gradients of the edge network on the rows of the k-nearest-neighbour graph -- the backward of
// mpgan/model.py:256-267 and of the gather of :319-381 (knn_edge_impl.h has the row and tile plan).
//
// Two kernels on one stream:
//   knn_edge_bwd_kernel   per tile of 32 rows, one wave: dZ3 = dagg_i * agg_scale * mask_j * (dropout, LeakyReLU') from the parked
//                         sign words; dZ2 = gate2 * W3^T dZ3; dZ1 = gate1 * W2^T dZ2 with the gates from the parked E2 / E1
//                         (E > 0 <=> Z > 0 where the element was kept) and the regenerated keep words.  Nothing of the forward is
//                         recomputed.  The gradient rows are the B operands: each is split hi + lo in fp16 in a power-of-two unit
//                         of ITS OWN row (a column of the product scales with its column of B), three terms against the W3T / W2T
//                         images.  dZ1 (always), dZ2 and dZ3 (for the weight-gradient GEMMs) leave row-major in fp32.
//   knn_dadc_kernel       one workgroup per node: da_i = its k rows of dZ1 in ascending row order; dc_j = the rows that list
//                         sender j, found by walking column j of the bit words in ascending receiver index.  No atomics.
#include "knn_edge_impl.h"

namespace {

template <int DROP, bool NEEDW>
__global__ __launch_bounds__(256) void knn_edge_bwd_kernel(const MpgKnnEdgeBwd p) {
    typedef f16x8 V;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5, nwaves = (int)blockDim.x >> 6;
    const int NB = (p.N + p.RW - 1) / p.RW;
    const int b = blockIdx.x / NB, rb = blockIdx.x % NB;
    const int i0 = rb * p.RW, nrec = min(p.RW, p.N - i0), nrows = nrec * p.k, ntiles = (nrows + 31) >> 5;
    const size_t g0 = (size_t)(b * p.N + i0) * p.k;
    uint32_t seed_lo = 0, seed_hi = 0;
    if (DROP) { const uint64_t sd = *p.seed; seed_lo = (uint32_t)sd; seed_hi = (uint32_t)(sd >> 32); }
    const KnnImg W3T = knn_img(p.W3Timg, NF3T, lane);
    const KnnImg W2T = knn_img(p.W2Timg, NF2T, lane);
    const bool dvec = p.ld_dagg % 4 == 0 && ((uintptr_t)p.dagg & 15) == 0;

    for (int tl = w; tl < ntiles; tl += nwaves) {
        const int lrow = tl * 32 + r;
        const KnnRow R = knn_row(p.nbr, b, p.N, p.k, i0, lrow, nrows);
        const float mj = R.live ? (p.mask != nullptr ? p.mask[b * p.N + R.j] : 1.f) : 0.f;
        const bool on = mj != 0.f;
        const size_t grow = g0 + (R.in_range ? lrow : 0);
        if (!__any(on)) {   // (wave-uniform) the rows of zero-masked senders carry no gradient
            if (R.in_range) {
#pragma unroll
                for (int f = 0; f < H1; f += 8) st4(p.dZ1 + grow * H1 + f + 4 * h, 0.f, 0.f, 0.f, 0.f);
                if constexpr (NEEDW) {
#pragma unroll
                    for (int f = 0; f < H2; f += 8) st4(p.dZ2 + grow * H2 + f + 4 * h, 0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int f = 0; f < H3; f += 8) st4(p.dZ3 + grow * H3 + f + 4 * h, 0.f, 0.f, 0.f, 0.f);
                }
            }
            continue;
        }
        const uint32_t erow = (uint32_t)((b * p.N + R.i) * p.N + R.j);
        const float gf = on ? mj * p.dscale * p.agg_scale : 0.f;   // d(agg_i) / d(X3 row), with the third dropout's scale
        const float* dg = p.dagg + (size_t)(b * p.N + R.i) * p.ld_dagg;

        // ---- dZ3 (accumulator order: register 4g + t of tile m <-> feature 32m + 8g + 4h + t; halves 8s .. 8s + 7 are B fragments)
        float z3[T3][16], mx3 = 0.f;
        static_for<0, T3>([&](auto mc) {
            MPG_CI(m, mc);
            KnnKeep<DROP> kp;
            kp.load(seed_lo, seed_hi, p.tag_base + TAG_E2, erow, m, h);
            const uint32_t sg = p.sign3[(grow * T3 + m) * 2 + h];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float dv[4];
                knn_ld4(dg + 32 * m + 8 * g + 4 * h, dvec, dv);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float gt = ((sg >> (4 * g + t)) & 1u) ? p.alpha : 1.f;
                    z3[m][4 * g + t] = kp.apply(on ? dv[t] * gf * gt : 0.f, g, t, p.thr);
                    mx3 = fmaxf(mx3, fabsf(z3[m][4 * g + t]));
                }
                if constexpr (NEEDW) {
                    if (R.in_range) st4(p.dZ3 + grow * H3 + 32 * m + 8 * g + 4 * h, z3[m][4 * g], z3[m][4 * g + 1], z3[m][4 * g + 2], z3[m][4 * g + 3]);
                }
            }
        });
        float u3, i3;
        knn_unit(knn_row_max(mx3), u3, i3);
        V g3h[T3 * 2], g3l[T3 * 2];
        static_for<0, T3 * 2>([&](auto kc) {
            MPG_CI(kk, kc);
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = z3[kk >> 1][8 * (kk & 1) + e] * u3;
            split8(v, g3h[kk], g3l[kk]);
        });

        // ---- dZ2 = gate2 * (W3^T dZ3): the W3T image carries dscale * SC_W3 (the second dropout's scale is in it)
        const float s2 = i3 * (1.f / SC_W3);
        float z2[T2][16], mx2 = 0.f;
        knn_layer<T2, T3 * 2>(W3T, NF3T, g3h, g3l, [&](auto, f32x16& acc) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        }, [&](auto mc, const f32x16& acc) {
            MPG_CI(mm, mc);
            KnnKeep<DROP> kp;
            kp.load(seed_lo, seed_hi, p.tag_base + TAG_E1, erow, mm, h);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 e4 = ld4(p.E2 + grow * H2 + 32 * mm + 8 * g + 4 * h);
                const float ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    z2[mm][4 * g + t] = kp.apply(on ? acc[4 * g + t] * s2 * (ev[t] > 0.f ? 1.f : p.alpha) : 0.f, g, t, p.thr);
                    mx2 = fmaxf(mx2, fabsf(z2[mm][4 * g + t]));
                }
                if constexpr (NEEDW) {
                    if (R.in_range) st4(p.dZ2 + grow * H2 + 32 * mm + 8 * g + 4 * h, z2[mm][4 * g], z2[mm][4 * g + 1], z2[mm][4 * g + 2], z2[mm][4 * g + 3]);
                }
            }
        });
        float u2, i2;
        knn_unit(knn_row_max(mx2), u2, i2);
        V g2h[T2 * 2], g2l[T2 * 2];
        static_for<0, T2 * 2>([&](auto kc) {
            MPG_CI(kk, kc);
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = z2[kk >> 1][8 * (kk & 1) + e] * u2;
            split8(v, g2h[kk], g2l[kk]);
        });

        // ---- dZ1 = gate1 * (W2^T dZ2): the W2T image carries dscale * SC_W2
        const float s1 = i2 * (1.f / SC_W2);
        knn_layer<T1, T2 * 2>(W2T, NF2T, g2h, g2l, [&](auto, f32x16& acc) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        }, [&](auto mc, const f32x16& acc) {
            MPG_CI(m1, mc);
            KnnKeep<DROP> kp;
            kp.load(seed_lo, seed_hi, p.tag_base + TAG_E0, erow, m1, h);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 e4 = ld4(p.E1 + grow * H1 + 32 * m1 + 8 * g + 4 * h);
                const float ev[4] = {e4.x, e4.y, e4.z, e4.w};
                float o[4];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    o[t] = kp.apply(on ? acc[4 * g + t] * s1 * (ev[t] > 0.f ? 1.f : p.alpha) : 0.f, g, t, p.thr);
                if (R.in_range) st4(p.dZ1 + grow * H1 + 32 * m1 + 8 * g + 4 * h, o[0], o[1], o[2], o[3]);
            }
        });
    }
}

// da | dc of node (b, v): threads 0..95 da, 96..191 dc, one feature each.  The rows that list v as a sender are found once per
// workgroup -- thread i looks at receiver i's words -- and left in LDS in ascending receiver order; the feature threads then
// add those rows (about k of them) instead of walking all N receivers each.
__global__ __launch_bounds__(192) void knn_dadc_kernel(const MpgKnnEdgeBwd p) {
    __shared__ int rows[32 * KNN_NW_MAX];    // the hit rows, ascending receiver
    __shared__ int wcount[3];
    const int node = blockIdx.x, b = node / p.N, v = node - b * p.N;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int NW = (p.N + 31) >> 5;
    int row = -1;
    if (tid < p.N) {
        const unsigned int* wd = p.nbr + (size_t)(b * p.N + tid) * NW;
        const int wj = v >> 5;
        const unsigned int bit = 1u << (v & 31), own = wd[wj];
        if (own & bit) {
            int rk = __popc(own & (bit - 1u));   // rank of sender v among receiver tid's neighbours = its row
            for (int q = 0; q < wj; ++q) rk += __popc(wd[q]);
            if (rk < p.k) row = (b * p.N + tid) * p.k + rk;
        }
    }
    const unsigned long long hits = __ballot(row >= 0);
    if (lane == 0) wcount[wv] = __popcll(hits);
    __syncthreads();
    int pos = __popcll(hits & ((1ull << lane) - 1ull));
    for (int q = 0; q < wv; ++q) pos += wcount[q];
    if (row >= 0) rows[pos] = row;
    __syncthreads();
    const int nhit = wcount[0] + wcount[1] + wcount[2];
    const int f = tid % H1, part = tid / H1;
    float sum = 0.f;
    if (part == 0) {
        const float* z = p.dZ1 + (size_t)node * p.k * H1 + f;
        for (int q = 0; q < p.k; ++q) sum += z[(size_t)q * H1];
    } else {
        for (int q = 0; q < nhit; ++q) sum += p.dZ1[(size_t)rows[q] * H1 + f];
    }
    p.dadc[(size_t)node * (2 * H1) + part * H1 + f] = sum;
}

template <int D>
int knn_bwd_launch(const MpgKnnEdgeBwd* p, hipStream_t st) {
    const int NB = (p->N + p->RW - 1) / p->RW;
    if (p->dZ2 != nullptr) hipLaunchKernelGGL((knn_edge_bwd_kernel<D, true>), dim3(p->B * NB), dim3(knn_block_threads(p->RW, p->k)), 0, st, *p);
    else hipLaunchKernelGGL((knn_edge_bwd_kernel<D, false>), dim3(p->B * NB), dim3(knn_block_threads(p->RW, p->k)), 0, st, *p);
    HIP_CHECK_RET(hipGetLastError());
    hipLaunchKernelGGL(knn_dadc_kernel, dim3(p->B * p->N), dim3(192), 0, st, *p);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int mpg_knn_edge_bwd(const MpgKnnEdgeBwd* p, void* stream) {
    if (p->B <= 0 || p->N <= 0 || p->k <= 0 || p->RW <= 0 || p->k > p->N || p->N > 32 * KNN_NW_MAX) return -1;
    if (p->nbr == nullptr || p->dagg == nullptr || p->W3Timg == nullptr || p->W2Timg == nullptr || p->E1 == nullptr || p->E2 == nullptr ||
        p->sign3 == nullptr || p->dZ1 == nullptr || p->dadc == nullptr)
        return -2;
    if ((p->dZ2 != nullptr) != (p->dZ3 != nullptr)) return -3;
    if (!(p->alpha >= 0.f && p->alpha <= 1.f)) return -4;
    if (p->ld_dagg < H3) return -5;
    if (p->thr != 0 && p->seed == nullptr) return -2;
    if ((long long)p->B * p->N * p->N > 0x7fffffffLL) return -7;
    hipStream_t st = (hipStream_t)stream;
    switch (edge_drop_mode(p->thr)) {
        case 0: return knn_bwd_launch<0>(p, st);
        case 1: return knn_bwd_launch<1>(p, st);
        default: return knn_bwd_launch<2>(p, st);
    }
}
