// Shared pieces of the SPARSE k-nearest-neighbour edge kernels (forward: knn_edge_fwd.hip, data gradients: knn_edge_bwd.hip).
//
// The dense kernels walk all N senders of every receiver and take the neighbour bit as a 0/1 factor; these kernels work on the
// B * N * k edge ROWS of the neighbour sets themselves (mpgan/model.py:319-381: the reference gathers exactly those rows).
//   row (b, i, r)   = receiver i of jet b with its r-th neighbour: the r-th set bit, in ascending sender index, of the words
//                     nbr[(b N + i) NW ..] that mpg_knn_sets writes.  Global row index  g = (b N + i) k + r.
//   workgroup       = RW consecutive receivers of one jet: RW * k rows, cut into tiles of 32; a wave per tile, four waves at the most
//                     (wave w then takes tiles w, w + 4, ...)
//   tile            = 32 rows on the MFMA columns (lane & 31), features in accumulator registers: the "chain" layout of
//                     common.h, so the weight images of PackedMPLayer (W2, W3, W3T, W2T) are the A operands as they are.
// A tile straddles receivers whenever k does not divide 32; every sum over a receiver's rows (agg, da) and over the receivers
// that list a sender (dc) is therefore taken AFTER the tiles, by one thread per output element in ascending row order: no
// float atomics, and no dependence on which wave finished first.
#pragma once
#include "edge_common.h"

#ifndef MPG_KNN_PF
#define MPG_KNN_PF 8   // k-steps of weight-fragment prefetch (a workgroup's LDS allows one wave per SIMD: the registers are there)
#endif

namespace {

constexpr int KNN_NW_MAX = 6;            // words per receiver: mpg_knn_sets takes N <= 192
constexpr int KNN_STAGE_LD = H3 + 4;     // floats per staged row of X3 (the 16-byte pad spreads the rows over the LDS banks)

// The lane's row: which receiver, which sender.  `lrow` = row within the workgroup; rows at or beyond `nrows` belong to nobody.
struct KnnRow {
    int i, j;         // receiver, sender (clamped to 0 where the row does not exist: addresses stay inside the jet)
    bool in_range;    // the row exists in the parked buffers (lrow < nrows)
    bool live;        // ... and has a sender (its receiver has more than r set bits: always, with mpg_knn_sets' words)
};

MPG_DEV KnnRow knn_row(const unsigned int* __restrict__ nbr, int b, int N, int k, int i0, int lrow, int nrows) {
    KnnRow R;
    R.in_range = lrow < nrows;
    const int li = R.in_range ? lrow / k : 0;
    int r = R.in_range ? lrow - li * k : 0;
    R.i = i0 + li;
    const int NW = (N + 31) >> 5;
    const unsigned int* wd = nbr + (size_t)(b * N + R.i) * NW;
    int j = -1;
    for (int w = 0; w < NW; ++w) {
        unsigned int bits = wd[w];
        if (w == NW - 1 && (N & 31)) bits &= (1u << (N & 31)) - 1u;   // (bits beyond the jet are nobody's)
        const int c = __popc(bits);
        if (j < 0) {
            if (r < c) {
                for (int q = 0; q < r; ++q) bits &= bits - 1u;
                j = 32 * w + (__ffs((int)bits) - 1);
            } else {
                r -= c;
            }
        }
    }
    R.live = R.in_range && j >= 0;
    R.j = j >= 0 ? j : 0;
    return R;
}

// keep words of one 32-feature tile m in ACCUMULATOR order (register 4g + t <-> feature 32m + 8g + 4h + t), for drop_apply:
// bit mode one word per tile (already shifted by 4h), byte mode one word per group g
template <int DM>
struct KnnKeep {
    uint32_t w[DM == 1 ? 4 : 1];
    MPG_DEV void load(uint32_t seed_lo, uint32_t seed_hi, uint32_t tag, uint32_t erow, int m, int h) {
        if constexpr (DM == 2) w[0] = drop_tile_word<2>(seed_lo, seed_hi, tag, erow, m, 0, h);
        else if constexpr (DM == 1) {
#pragma unroll
            for (int g = 0; g < 4; ++g) w[g] = drop_tile_word<1>(seed_lo, seed_hi, tag, erow, m, 2 * g + h, h);
        } else w[0] = 0u;
    }
    MPG_DEV float apply(float x, int g, int t, uint32_t thr) const {
        return drop_apply<DM>(x, w[DM == 1 ? g : 0], 8 * g + t, t, thr);
    }
};

// threads of a workgroup: a wave per tile of its RW * k rows, four at the most (the waves then loop over the tiles)
inline int knn_block_threads(int RW, int k) { return 64 * max(1, min(4, (RW * k + 31) / 32)); }

MPG_DEV void st4(float* p, float x, float y, float z, float w) { *reinterpret_cast<float4*>(p) = make_float4(x, y, z, w); }

// A weight image (hi | lo halves of `nfrag` fragments each) behind a buffer descriptor: a fragment is one load with a per-lane
// offset (lane * 16) and a constant fragment offset -- no 64-bit address per fragment (edge_common.h: img_frag)
struct KnnImg {
    __amdgpu_buffer_rsrc_t rs;
    int lane16;
};
MPG_DEV KnnImg knn_img(const void* img, int nfrag, int lane) { return KnnImg{img_rsrc(img, 2 * nfrag), lane * 16}; }

// One layer of a row tile: MT output tiles of KS k-steps each, acc = init(m), then += image fragments m KS .. m KS + KS - 1 (hi and
// lo) times the B fragments bh / bl -- three terms per k-step, k ascending --, then epi(m, acc).  The fragments stream from the
// L2-resident image PF k-steps ahead of their MFMAs in ONE ring over the whole layer, so the loads of output tile m + 1 are in
// flight while tile m's epilogue runs (a ring per output tile left an L2 round trip exposed in front of each); sched_barrier pins
// that order (left alone the compiler hoists every load of the layer to its top: some 700 registers, and spills).
template <int MT, int KS, typename V, typename Init, typename Epi>
MPG_DEV void knn_layer(const KnnImg& img, int nfrag, const V* bh, const V* bl, Init init, Epi epi) {
    constexpr int PF = MPG_KNN_PF, TOT = MT * KS;
    V ah[PF + 1], al[PF + 1];
    static_for<0, (PF < TOT ? PF : TOT)>([&](auto sc) {
        MPG_CI(s, sc);
        ah[s] = img_frag<V>(img.rs, img.lane16, s);
        al[s] = img_frag<V>(img.rs, img.lane16, nfrag + s);
    });
    __builtin_amdgcn_sched_barrier(0);
    f32x16 acc;
    static_for<0, TOT>([&](auto sc) {
        MPG_CI(s, sc);
        constexpr int m = s / KS, k = s % KS;
        if constexpr (s + PF < TOT) {
            ah[(s + PF) % (PF + 1)] = img_frag<V>(img.rs, img.lane16, s + PF);
            al[(s + PF) % (PF + 1)] = img_frag<V>(img.rs, img.lane16, nfrag + s + PF);
        }
        if constexpr (k == 0) init(std::integral_constant<int, m>{}, acc);
        acc = mfma3(ah[s % (PF + 1)], al[s % (PF + 1)], bh[k], bl[k], acc);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (k == KS - 1) {
            epi(std::integral_constant<int, m>{}, acc);
            __builtin_amdgcn_sched_barrier(0);
        }
    });
}

// ---- what the kernels that take a GRADIENT or TANGENT row as the B operand share (knn_edge_bwd.hip, knn_edge_jvp.hip)
// power-of-two unit of a row whose largest magnitude is `mx`: mx * unit in [2^10, 2^11) -- inside fp16's range with 22
// significand bits for the hi + lo pair --, 1 for a row of zeros; `inv` = 1 / unit, exact
MPG_DEV void knn_unit(float mx, float& unit, float& inv) {
    const int ex = (int)((__builtin_bit_cast(uint32_t, mx) >> 23) & 0xffu);
    int f = ex == 0 ? 127 : 264 - ex;
    f = max(30, min(224, f));
    unit = __builtin_bit_cast(float, (uint32_t)f << 23);
    inv = __builtin_bit_cast(float, (uint32_t)(254 - f) << 23);
}

MPG_DEV float knn_row_max(float mx) { return fmaxf(mx, __shfl_xor(mx, 32)); }   // (with the row's other lane half)

// four consecutive floats of a dagg row: one 16-byte load where the rows are 16-byte aligned (`vec`, uniform), else four loads
MPG_DEV void knn_ld4(const float* q, bool vec, float* o) {
    if (vec) { const float4 d4 = ld4(q); o[0] = d4.x; o[1] = d4.y; o[2] = d4.z; o[3] = d4.w; }
    else { o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3]; }
}

}  // namespace
