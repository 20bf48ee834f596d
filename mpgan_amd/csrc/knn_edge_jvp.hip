// mpg_knn_edge_jvp: the second-order half of the edge network on explicit edge rows -- what a twice-differentiable aggregation (the
// gradient penalty, train.py:286-324; ops.EdgeRowsFn / EdgeRowsVJPFn) needs beside mpg_knn_edge_fwd and mpg_knn_edge_bwd.
// knn_edge_impl.h has the row and tile plan; the gates are taken exactly as knn_edge_bwd_kernel takes them: the sign of the parked
// E1 / E2 where the element was kept, the parked sign words for layer 3, the keep words regenerated under the same seed, tag and
// dense edge-row key.  Nothing of layers 1 and 2 of the forward is recomputed.
//
// Two kernels on one stream:
//   knn_edge_jvp_kernel<., JVP>   per tile of 32 rows, one wave.
//        dot (JVP = false)   Z3 = W3 E2 + b3 from the parked E2 as the forward's layer 3 forms it, gate 3, and per row
//                            <E3_row, dagg_i>: lane partials, then the row's other lane half.
//        jvp (JVP = true)    T1 = gate1 (ta_i + tc_j) straight from the tangent projections, T2 = gate2 W2 T1, T3 = gate3 W3 T2
//                            through knn_layer<>; a tangent row has no fixed scale, so it is split hi + lo in fp16 in a
//                            power-of-two unit of ITS OWN row (knn_unit), three terms, as the backward splits gradient rows.
//                            With mu the primal layer 3 runs alongside (E2 keeps SC_E2) for the mu_j E3 term.  mask_j T3 +
//                            mu_j E3 is staged in LDS and summed per receiver in ascending row order, as the forward sums.
//   knn_dmask_kernel              one workgroup per node: dmask[b,j] = agg_scale * the row dots of the rows that list sender j,
//                                 found and added in ascending receiver order as knn_dadc_kernel finds them.  No atomics.
#include "knn_edge_impl.h"

namespace {

template <int DROP, bool JVP>
__global__ __launch_bounds__(256) void knn_edge_jvp_kernel(const MpgKnnEdgeJvp p) {
    typedef f16x8 V;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* stage = reinterpret_cast<float*>(smem);   // (jvp with aggt) [RW * k rows][KNN_STAGE_LD]: mask_j T3 + mu_j E3 of every row
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5, nwaves = (int)blockDim.x >> 6;
    const int NB = (p.N + p.RW - 1) / p.RW;
    const int b = blockIdx.x / NB, rb = blockIdx.x % NB;
    const int i0 = rb * p.RW, nrec = min(p.RW, p.N - i0), nrows = nrec * p.k, ntiles = (nrows + 31) >> 5;
    const size_t g0 = (size_t)(b * p.N + i0) * p.k;
    uint32_t seed_lo = 0, seed_hi = 0;
    if (DROP) { const uint64_t sd = *p.seed; seed_lo = (uint32_t)sd; seed_hi = (uint32_t)(sd >> 32); }
    const KnnImg W3 = knn_img(p.W3img, NF3, lane);
    const bool dvec = p.ld_dagg % 4 == 0 && ((uintptr_t)p.dagg & 15) == 0;
    const bool want_agg = JVP && p.aggt != nullptr, want_dot = p.rowdot != nullptr;   // (kernel arguments: wave-uniform)
    const bool primal = !JVP || p.mu != nullptr;
    const float e2op = SC_E2 / p.dscale;             // parked E2 (dropout scale included) -> the forward's layer-3 operand
    const float e3s = p.dscale * (1.f / SC_E3);      // layer-3 accumulator -> E3 as the reference has it

    for (int tl = w; tl < ntiles; tl += nwaves) {
        const int lrow = tl * 32 + r;
        const KnnRow R = knn_row(p.nbr, b, p.N, p.k, i0, lrow, nrows);
        const float mj = R.live ? (p.mask != nullptr ? p.mask[b * p.N + R.j] : 1.f) : 0.f;
        const float muj = (R.live && JVP && p.mu != nullptr) ? p.mu[b * p.N + R.j] : 0.f;
        const bool on = mj != 0.f || muj != 0.f;
        float* srow = stage + (size_t)(R.in_range ? lrow : 0) * KNN_STAGE_LD;
        const size_t grow = g0 + (R.in_range ? lrow : 0);
        if (!__any(on)) {   // (wave-uniform) neither the senders' masks nor their mu reach these rows
            if (R.in_range) {
                if constexpr (JVP) {
                    if (p.T1 != nullptr) {
#pragma unroll
                        for (int f = 0; f < H1; f += 8) st4(p.T1 + grow * H1 + f + 4 * h, 0.f, 0.f, 0.f, 0.f);
                    }
                    if (p.T2 != nullptr) {
#pragma unroll
                        for (int f = 0; f < H2; f += 8) st4(p.T2 + grow * H2 + f + 4 * h, 0.f, 0.f, 0.f, 0.f);
                    }
                    if (want_agg) {
#pragma unroll
                        for (int f = 0; f < H3; f += 8) st4(srow + f + 4 * h, 0.f, 0.f, 0.f, 0.f);
                    }
                }
                if (want_dot && h == 0) p.rowdot[grow] = 0.f;
            }
            continue;
        }
        const uint32_t erow = (uint32_t)((b * p.N + R.i) * p.N + R.j);
        const float* dg = p.dagg + (size_t)(b * p.N + R.i) * p.ld_dagg;
        float dot = 0.f;

        if constexpr (JVP) {
            const KnnImg W2 = knn_img(p.W2img, NF2, lane);
            const float* ta = p.ta + (size_t)(b * p.N + R.i) * p.ld_t;
            const float* tc = p.tc + (size_t)(b * p.N + R.j) * p.ld_t;

            // ---- T1 = gate1 * (ta_i + tc_j)  (accumulator order: register 4g + t of tile m <-> feature 32m + 8g + 4h + t)
            float t1[T1][16], mx1 = 0.f;
            static_for<0, T1>([&](auto mc) {
                MPG_CI(m1, mc);
                KnnKeep<DROP> kp;
                kp.load(seed_lo, seed_hi, p.tag_base + TAG_E0, erow, m1, h);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int f0 = 32 * m1 + 8 * g + 4 * h;
                    const float4 e4 = ld4(p.E1 + grow * H1 + f0), a4 = ld4(ta + f0), c4 = ld4(tc + f0);
                    const float ev[4] = {e4.x, e4.y, e4.z, e4.w}, av[4] = {a4.x, a4.y, a4.z, a4.w}, cv[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        t1[m1][4 * g + t] = kp.apply(on ? (av[t] + cv[t]) * (ev[t] > 0.f ? 1.f : p.alpha) : 0.f, g, t, p.thr);
                        mx1 = fmaxf(mx1, fabsf(t1[m1][4 * g + t]));
                    }
                    if (p.T1 != nullptr && R.in_range)
                        st4(p.T1 + grow * H1 + f0, t1[m1][4 * g] * p.dscale, t1[m1][4 * g + 1] * p.dscale, t1[m1][4 * g + 2] * p.dscale,
                            t1[m1][4 * g + 3] * p.dscale);
                }
            });
            float u1, i1;
            knn_unit(knn_row_max(mx1), u1, i1);
            V t1h[T1 * 2], t1l[T1 * 2];
            static_for<0, T1 * 2>([&](auto kc) {
                MPG_CI(kk, kc);
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = t1[kk >> 1][8 * (kk & 1) + e] * u1;
                split8(v, t1h[kk], t1l[kk]);
            });

            // ---- T2 = gate2 * (W2 T1): the W2 image carries dscale * SC_W2 (the first dropout's scale is in it); no bias
            const float s2 = i1 * (1.f / SC_W2);
            float t2[T2][16], mx2 = 0.f;
            knn_layer<T2, T1 * 2>(W2, NF2, t1h, t1l, [&](auto, f32x16& acc) {
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[e] = 0.f;
            }, [&](auto mc, const f32x16& acc) {
                MPG_CI(mm, mc);
                KnnKeep<DROP> kp;
                kp.load(seed_lo, seed_hi, p.tag_base + TAG_E1, erow, mm, h);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int f0 = 32 * mm + 8 * g + 4 * h;
                    const float4 e4 = ld4(p.E2 + grow * H2 + f0);
                    const float ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        t2[mm][4 * g + t] = kp.apply(on ? acc[4 * g + t] * s2 * (ev[t] > 0.f ? 1.f : p.alpha) : 0.f, g, t, p.thr);
                        mx2 = fmaxf(mx2, fabsf(t2[mm][4 * g + t]));
                    }
                    if (p.T2 != nullptr && R.in_range)
                        st4(p.T2 + grow * H2 + f0, t2[mm][4 * g] * p.dscale, t2[mm][4 * g + 1] * p.dscale, t2[mm][4 * g + 2] * p.dscale,
                            t2[mm][4 * g + 3] * p.dscale);
                }
            });
            float u2, i2;
            knn_unit(knn_row_max(mx2), u2, i2);
            V t2h[T2 * 2], t2l[T2 * 2];
            static_for<0, T2 * 2>([&](auto kc) {
                MPG_CI(kk, kc);
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = t2[kk >> 1][8 * (kk & 1) + e] * u2;
                split8(v, t2h[kk], t2l[kk]);
            });

            // ---- T3 = gate3 * (W3 T2): the W3 image carries dscale * SC_W3; the third dropout's scale joins here
            if (want_agg || want_dot) {
                const float s3 = i2 * (1.f / SC_W3) * p.dscale;
                knn_layer<T3, T2 * 2>(W3, NF3, t2h, t2l, [&](auto, f32x16& acc) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
                }, [&](auto mc, const f32x16& acc) {
                    MPG_CI(m, mc);
                    KnnKeep<DROP> kp;
                    kp.load(seed_lo, seed_hi, p.tag_base + TAG_E2, erow, m, h);
                    const uint32_t sg = p.sign3[(grow * T3 + m) * 2 + h];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        float dv[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
                        if (want_dot) knn_ld4(dg + 32 * m + 8 * g + 4 * h, dvec, dv);
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const float gt = ((sg >> (4 * g + t)) & 1u) ? p.alpha : 1.f;
                            const float x = kp.apply(on ? acc[4 * g + t] * s3 * gt : 0.f, g, t, p.thr);
                            dot += x * dv[t];
                            o[t] = mj * x;
                        }
                        if (want_agg && R.in_range) st4(srow + 32 * m + 8 * g + 4 * h, o[0], o[1], o[2], o[3]);
                    }
                });
            }
        }

        // ---- the primal layer 3 from the parked E2: Z3 = W3 E2 + b3 as the forward forms it, gate 3 from the parked sign words
        if (primal && (!JVP || want_agg)) {
            V e2h[T2 * 2], e2l[T2 * 2];
            static_for<0, T2>([&](auto mc) {
                MPG_CI(mm, mc);
                float x2[16];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 e4 = ld4(p.E2 + grow * H2 + 32 * mm + 8 * g + 4 * h);
                    x2[4 * g] = e4.x * e2op; x2[4 * g + 1] = e4.y * e2op; x2[4 * g + 2] = e4.z * e2op; x2[4 * g + 3] = e4.w * e2op;
                }
                split8(x2, e2h[2 * mm], e2l[2 * mm]);
                split8(x2 + 8, e2h[2 * mm + 1], e2l[2 * mm + 1]);
            });
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
                const uint32_t sg = p.sign3[(grow * T3 + m) * 2 + h];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float x[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const float gt = ((sg >> (4 * g + t)) & 1u) ? p.alpha : 1.f;
                        x[t] = kp.apply(on ? acc[4 * g + t] * e3s * gt : 0.f, g, t, p.thr);
                    }
                    if constexpr (JVP) {   // (the same lane wrote these four floats of its row above: no barrier between the two)
                        if (R.in_range) {
                            float* q = srow + 32 * m + 8 * g + 4 * h;
                            const float4 s4 = ld4(q);
                            st4(q, s4.x + muj * x[0], s4.y + muj * x[1], s4.z + muj * x[2], s4.w + muj * x[3]);
                        }
                    } else {
                        float dv[4];
                        knn_ld4(dg + 32 * m + 8 * g + 4 * h, dvec, dv);
#pragma unroll
                        for (int t = 0; t < 4; ++t) dot += x[t] * dv[t];
                    }
                }
            });
        }
        if (want_dot) {
            dot += __shfl_xor(dot, 32);   // (the row's other lane half: features 4h .. 4h + 3 of every group of 8)
            if (R.in_range && h == 0) p.rowdot[grow] = dot;
        }
    }

    // ---- the segmented sum: receiver li owns rows li k .. li k + k - 1, added in that order
    if (want_agg) {
        __syncthreads();
        float* out = p.aggt + (size_t)(b * p.N + i0) * H3;
        for (int e = tid; e < nrec * H3; e += (int)blockDim.x) {
            const int li = e / H3, f = e - li * H3;
            const float* s0 = stage + (size_t)li * p.k * KNN_STAGE_LD + f;
            float sum = 0.f;
            for (int q = 0; q < p.k; ++q) sum += s0[(size_t)q * KNN_STAGE_LD];
            out[e] = sum * p.agg_scale;
        }
    }
}

// dmask of node (b, v): thread i looks at receiver i's words for sender v, the hit rows land in LDS in ascending receiver order
// (as knn_dadc_kernel orders them), and one thread adds their row dots in that order.
__global__ __launch_bounds__(192) void knn_dmask_kernel(const MpgKnnEdgeJvp p) {
    __shared__ int rows[32 * KNN_NW_MAX];
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
    if (tid == 0) {
        const int nhit = wcount[0] + wcount[1] + wcount[2];
        float sum = 0.f;
        for (int q = 0; q < nhit; ++q) sum += p.rowdot[rows[q]];
        p.dmask[node] = sum * p.agg_scale;
    }
}

template <int D>
int knn_jvp_launch(const MpgKnnEdgeJvp* p, hipStream_t st) {
    using Go = int (*)(dim3, dim3, int, hipStream_t, const MpgKnnEdgeJvp&);
    static constexpr Go GO[2] = {mpg_go<knn_edge_jvp_kernel<D, false>, MpgKnnEdgeJvp>, mpg_go<knn_edge_jvp_kernel<D, true>, MpgKnnEdgeJvp>};
    const int NB = (p->N + p->RW - 1) / p->RW;
    const bool jvp = p->ta != nullptr;
    const int lds = jvp && p->aggt != nullptr ? p->RW * p->k * KNN_STAGE_LD * 4 : 0;
    const int rc = GO[jvp](dim3(p->B * NB), dim3(knn_block_threads(p->RW, p->k)), lds, st, *p);
    if (rc != 0 || p->dmask == nullptr) return rc;
    hipLaunchKernelGGL(knn_dmask_kernel, dim3(p->B * p->N), dim3(192), 0, st, *p);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int mpg_knn_edge_jvp(const MpgKnnEdgeJvp* p, void* stream) {
    if (p->B <= 0 || p->N <= 0 || p->k <= 0 || p->RW <= 0 || p->k > p->N || p->N > 32 * KNN_NW_MAX) return -1;
    const bool jvp = p->ta != nullptr;
    if ((p->ta != nullptr) != (p->tc != nullptr) || (p->rowdot != nullptr) != (p->dmask != nullptr)) return -3;
    {   // the parked rows: all three or none -- and none is no call
        const int n = (p->E1 != nullptr) + (p->E2 != nullptr) + (p->sign3 != nullptr);
        if (n != 0 && n != 3) return -3;
        if (n == 0) return -2;
    }
    if (p->nbr == nullptr || p->dagg == nullptr || p->W3img == nullptr || p->b3 == nullptr) return -2;
    if (jvp && p->W2img == nullptr) return -2;
    if (!jvp && p->dmask == nullptr) return -2;
    if (jvp && p->T1 == nullptr && p->T2 == nullptr && p->aggt == nullptr && p->dmask == nullptr) return -2;
    if (!(p->alpha >= 0.f && p->alpha <= 1.f)) return -4;
    if (p->ld_dagg < H3 || (jvp && (p->ld_t < H1 || p->ld_t % 4 != 0))) return -5;
    if (jvp && (((uintptr_t)p->ta | (uintptr_t)p->tc) & 15) != 0) return -5;
    if ((long long)p->RW * p->k * KNN_STAGE_LD * 4 > 160 * 1024) return -6;
    if (p->thr != 0 && p->seed == nullptr) return -2;
    if (!(p->dscale > 0.f)) return -1;
    if ((long long)p->B * p->N * p->N > 0x7fffffffLL) return -7;   // the dropout key (b N + i) N + j is a 32-bit word
    hipStream_t st = (hipStream_t)stream;
    switch (edge_drop_mode(p->thr)) {
        case 0: return knn_jvp_launch<0>(p, st);
        case 1: return knn_jvp_launch<1>(p, st);
        default: return knn_jvp_launch<2>(p, st);
    }
}
