// mpg_knn_edge_fwd: the edge network's forward on the B * N * k rows of the k-nearest-neighbour graph (knn_edge_impl.h has the
// row and tile plan).  Replaces, for fully_connected=False, the reference's
//   _getA_knn            mpgan/model.py:319-381  (distances, topk, gather -> [B*N*k, 2F] edge tensor)
//   self.fe(A)           mpgan/model.py:256 -> LinearNet.forward :70-85
//   A * mask ; sum/mean  mpgan/model.py:257-267
// Arithmetic per row is that of the dense forward (edge_fwd2_impl.h): Z1 = a_i + c_j in the SC_A scale, layers 2 and 3 as
// three fp16 terms against the W2 / W3 images, bias first, k-steps ascending; the same dropout words.  What differs is the sum:
// a wave leaves its tile's masked layer-3 rows in LDS, and after a barrier one thread per (receiver, feature) adds that
// receiver's k rows in ascending row order.
#include "knn_edge_impl.h"

namespace {

template <int DROP, bool SAVE>
__global__ __launch_bounds__(256) void knn_edge_fwd_kernel(const MpgKnnEdgeFwd p) {
    typedef f16x8 V;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* stage = reinterpret_cast<float*>(smem);   // [RW * k rows][KNN_STAGE_LD]: mask_j * dscale * X3 of every row
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5, nwaves = (int)blockDim.x >> 6;
    const int NB = (p.N + p.RW - 1) / p.RW;
    const int b = blockIdx.x / NB, rb = blockIdx.x % NB;
    const int i0 = rb * p.RW, nrec = min(p.RW, p.N - i0), nrows = nrec * p.k, ntiles = (nrows + 31) >> 5;
    const size_t g0 = (size_t)(b * p.N + i0) * p.k;
    const int ldac = p.ld_ac ? p.ld_ac : H1;
    uint32_t seed_lo = 0, seed_hi = 0;
    if (DROP) { const uint64_t sd = *p.seed; seed_lo = (uint32_t)sd; seed_hi = (uint32_t)(sd >> 32); }
    const KnnImg W2 = knn_img(p.W2img, NF2, lane);
    const KnnImg W3 = knn_img(p.W3img, NF3, lane);
    const float e1s = p.dscale * (1.f / SC_A), e2s = p.dscale * (1.f / SC_E2);   // operand scale -> the reference's layer inputs

    for (int tl = w; tl < ntiles; tl += nwaves) {
        const int lrow = tl * 32 + r;
        const KnnRow R = knn_row(p.nbr, b, p.N, p.k, i0, lrow, nrows);
        const float mj = R.live ? (p.mask != nullptr ? p.mask[b * p.N + R.j] : 1.f) : 0.f;
        const bool on = mj != 0.f;                       // (a zero-masked sender's row adds exactly 0)
        const float mjf = mj * p.dscale * (1.f / SC_E3); // (the layer-3 output carries SC_E3)
        float* srow = stage + (size_t)(R.in_range ? lrow : 0) * KNN_STAGE_LD;
        const size_t grow = g0 + (R.in_range ? lrow : 0);
        if (!__any(on)) {   // wave-uniform: a tile of zero-masked senders is not computed, its rows are zero everywhere
            if (R.in_range) {
#pragma unroll
                for (int f = 0; f < H3; f += 8) st4(srow + f + 4 * h, 0.f, 0.f, 0.f, 0.f);
                if constexpr (SAVE) {
#pragma unroll
                    for (int f = 0; f < H1; f += 8) st4(p.E1 + grow * H1 + f + 4 * h, 0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int f = 0; f < H2; f += 8) st4(p.E2 + grow * H2 + f + 4 * h, 0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int m = 0; m < T3; ++m) p.sign3[(grow * T3 + m) * 2 + h] = 0;
                }
            }
            continue;
        }
        const float* ai = p.a + (size_t)(b * p.N + R.i) * ldac;
        const float* cj = p.c + (size_t)(b * p.N + R.j) * ldac;
        const uint32_t erow = (uint32_t)((b * p.N + R.i) * p.N + R.j);   // the DENSE edge row: the dropout key

        // ---- layer 1: E1 = drop(lrelu(a_i + c_j)) straight into B fragments (k-step kk = (q, s): features 32q + rho(s, h, .))
        V e1h[T1 * 2], e1l[T1 * 2];
        static_for<0, T1 * 2>([&](auto kc) {
            MPG_CI(kk, kc);
            constexpr int q = kk >> 1, s = kk & 1;
            float v[8];
#pragma unroll
            for (int uh = 0; uh < 2; ++uh) {
                const int f0 = 32 * q + 16 * s + 8 * uh + 4 * h;
                const float4 a4 = ld4(ai + f0), c4 = ld4(cj + f0);
                const float av[4] = {a4.x, a4.y, a4.z, a4.w}, cv[4] = {c4.x, c4.y, c4.z, c4.w};
                const uint32_t wd = drop_tile_word<DROP>(seed_lo, seed_hi, p.tag_base + TAG_E0, erow, q, 4 * s + 2 * uh + h, h);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float cc = cv[t] * SC_A + av[t] * SC_A;
                    v[4 * uh + t] = drop_apply<DROP>(lrelu(cc, p.alpha), wd, 16 * s + 8 * uh + t, t, p.thr);
                }
                if constexpr (SAVE) {
                    if (R.in_range) {
                        const float z = on ? e1s : 0.f;
                        st4(p.E1 + grow * H1 + f0, v[4 * uh] * z, v[4 * uh + 1] * z, v[4 * uh + 2] * z, v[4 * uh + 3] * z);
                    }
                }
            }
            split8(v, e1h[kk], e1l[kk]);
        });

        // ---- layer 2: Z2 = W2' E1 + b2, then E2 = drop(lrelu(Z2)) as B fragments (tile mm, half s -> fragment 2 mm + s)
        V e2h[T2 * 2], e2l[T2 * 2];
        knn_layer<T2, T1 * 2>(W2, NF2, e1h, e1l, [&](auto mc, f32x16& acc) {
            MPG_CI(mm, mc);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 b4 = ld4(p.b2 + 32 * mm + 8 * g + 4 * h);
                acc[4 * g + 0] = b4.x * SC_E2; acc[4 * g + 1] = b4.y * SC_E2;
                acc[4 * g + 2] = b4.z * SC_E2; acc[4 * g + 3] = b4.w * SC_E2;
            }
        }, [&](auto mc, const f32x16& acc) {
            MPG_CI(mm, mc);
            KnnKeep<DROP> kp;
            kp.load(seed_lo, seed_hi, p.tag_base + TAG_E1, erow, mm, h);
            float x2[16];
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int t = 0; t < 4; ++t) x2[4 * g + t] = kp.apply(lrelu(acc[4 * g + t], p.alpha), g, t, p.thr);
            split8(x2, e2h[2 * mm], e2l[2 * mm]);
            split8(x2 + 8, e2h[2 * mm + 1], e2l[2 * mm + 1]);
            if constexpr (SAVE) {
                if (R.in_range) {
                    const float z = on ? e2s : 0.f;
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        st4(p.E2 + grow * H2 + 32 * mm + 8 * g + 4 * h, x2[4 * g] * z, x2[4 * g + 1] * z, x2[4 * g + 2] * z, x2[4 * g + 3] * z);
                }
            }
        });

        // ---- layer 3: Z3 = W3' E2 + b3 tile by tile; LeakyReLU, dropout, sign bits, the row's mask factor; into the staging rows
        knn_layer<T3, T2 * 2>(W3, NF3, e2h, e2l, [&](auto mc, f32x16& acc) {
            MPG_CI(m, mc);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 b4 = ld4(p.b3 + 32 * m + 8 * g + 4 * h);
                acc[4 * g + 0] = b4.x * SC_E3; acc[4 * g + 1] = b4.y * SC_E3;
                acc[4 * g + 2] = b4.z * SC_E3; acc[4 * g + 3] = b4.w * SC_E3;
            }
        }, [&](auto mc, const f32x16& acc) {
            MPG_CI(m, mc);
            KnnKeep<DROP> kp;
            kp.load(seed_lo, seed_hi, p.tag_base + TAG_E2, erow, m, h);
            uint32_t sg = 0u;
            float x3[16];
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float z = acc[4 * g + t];
                    sg |= (z > 0.f ? 0u : 1u) << (4 * g + t);
                    const float x = kp.apply(lrelu(z, p.alpha), g, t, p.thr);
                    x3[4 * g + t] = on ? mjf * x : 0.f;
                }
            if (R.in_range) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    st4(srow + 32 * m + 8 * g + 4 * h, x3[4 * g], x3[4 * g + 1], x3[4 * g + 2], x3[4 * g + 3]);
                if constexpr (SAVE) p.sign3[(grow * T3 + m) * 2 + h] = (unsigned short)(on ? sg : 0u);
            }
        });
    }

    // ---- the segmented sum: receiver li owns rows li k .. li k + k - 1, added in that order
    __syncthreads();
    float* out = p.agg + (size_t)(b * p.N + i0) * H3;
    for (int e = tid; e < nrec * H3; e += (int)blockDim.x) {
        const int li = e / H3, f = e - li * H3;
        const float* s0 = stage + (size_t)li * p.k * KNN_STAGE_LD + f;
        float sum = 0.f;
        for (int q = 0; q < p.k; ++q) sum += s0[(size_t)q * KNN_STAGE_LD];
        out[e] = sum * p.agg_scale;
    }
}

template <int D>
int knn_fwd_launch(const MpgKnnEdgeFwd* p, hipStream_t st) {
    using Go = int (*)(dim3, dim3, int, hipStream_t, const MpgKnnEdgeFwd&);
    static constexpr Go GO[2] = {mpg_go<knn_edge_fwd_kernel<D, false>, MpgKnnEdgeFwd>, mpg_go<knn_edge_fwd_kernel<D, true>, MpgKnnEdgeFwd>};
    const int NB = (p->N + p->RW - 1) / p->RW;
    return GO[p->E1 != nullptr](dim3(p->B * NB), dim3(knn_block_threads(p->RW, p->k)), p->RW * p->k * KNN_STAGE_LD * 4, st, *p);
}

}  // namespace

extern "C" int mpg_knn_edge_fwd(const MpgKnnEdgeFwd* p, void* stream) {
    if (p->B <= 0 || p->N <= 0 || p->k <= 0 || p->RW <= 0 || p->k > p->N || p->N > 32 * KNN_NW_MAX) return -1;
    if (p->a == nullptr || p->c == nullptr || p->nbr == nullptr || p->agg == nullptr || p->W2img == nullptr || p->W3img == nullptr) return -2;
    if ((p->E1 != nullptr) != (p->E2 != nullptr) || (p->E1 != nullptr) != (p->sign3 != nullptr)) return -3;
    if (!(p->alpha >= 0.f && p->alpha <= 1.f)) return -4;  // lrelu() is max(v, alpha v)
    if ((long long)p->RW * p->k * KNN_STAGE_LD * 4 > 160 * 1024) return -6;
    if (p->thr != 0 && p->seed == nullptr) return -2;
    if ((long long)p->B * p->N * p->N > 0x7fffffffLL) return -7;   // the dropout key (b N + i) N + j is a 32-bit word
    hipStream_t st = (hipStream_t)stream;
    switch (edge_drop_mode(p->thr)) {
        case 0: return knn_fwd_launch<0>(p, st);
        case 1: return knn_fwd_launch<1>(p, st);
        default: return knn_fwd_launch<2>(p, st);
    }
}
