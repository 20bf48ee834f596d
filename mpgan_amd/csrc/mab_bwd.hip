// The backward kernels of the one-launch attention blocks for sets of up to 32 tokens (one and two waves per jet), their launch
// tables and mpg_mab_bwd; the large-set backward is mab_bwds.hip.
#include "mab_bwd_impl.h"

namespace {
template <int NT, bool CROSS, bool LN = false>
__global__ __launch_bounds__(256) void mab_bwd_kernel(const MpgMab p) {
    typedef f16x8 VF;
    typedef bf16x8 VB;
    constexpr int KS = 2 * NT;
    MAB_STAMPS_DECL;
    MAB_WAVE(p, MAB_STAMP(0), mab_st);
    const float sc2 = 1.44269504088896341f / (sa * sa);   // (scores in the base-2 domain)
    constexpr int nfIn = 3 * NT * KS, nfE = NT * KS, nfInT = NT * 3 * KS;
    MAB_BWD_CARVE(NT);
    // ONE jet per wave (the launcher sizes the grid for it).  Its dout and z rows -- all the feed-forward half needs --
    // are requested BEFORE the 144 KiB weight fill (loads return in issue order: behind the fill they arrived ~8,000 clk
    // late); x and y follow the fill and land while that half runs.
    const int nw = blockDim.x >> 6;
    const long jet_raw = (long)blockIdx.x * nw + w;
    const long jet = min(jet_raw, (long)p.B - 1);
    const long xrow = jet * p.L + min(r, p.L - 1), yrow = jet * p.S + min(r, p.S - 1);
    f32x16 dzf[NT], zt[NT], zat[LN ? NT : 1];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        dzf[t] = rows_to_tile(p.dout, p.lddout, xrow, t, h);
        zt[t] = rows_to_tile(p.save_z, p.E, xrow, t, h);
        if constexpr (LN) zat[t] = rows_to_tile(p.save_za, p.E, xrow, t, h);
    }
    MAB_BWD_FILL(p);
    MAB_BWD_CARVE_BIASES;                 // biases: in_proj [3E] | ff [E]
    MAB_BWD_STAGE_BIASES(p);
    __syncthreads();
    const WImg rIn = sIn, rF = sF, rInT = sInT, rOT = sOT, rFT = sFT;
    MAB_STAMP(1);
    if (jet_raw >= p.B) return;           // (a wave without a jet: it has helped with the fill)
    {
    const bool xvalid = r < p.L, yvalid = r < p.S;
    const float xlive = xvalid ? 1.f : 0.f;
    const f32x16 kneg = key_mask_regs(p.ignore, p.x, jet, p.S, h);
    // this lane as a KEY (transposed tiles); no branch on the pointer, as in key_mask_load
    const float ign_r = (p.ignore != nullptr ? p.ignore + jet * p.S : p.x)[min(r, p.S - 1)];
    const bool key_off = !yvalid || (p.ignore != nullptr && ign_r != 0.f);
    f32x16 xt[NT], yt[CROSS ? NT : 1];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        xt[t] = rows_to_tile(p.x, p.ldx, xrow, t, h);
        if constexpr (CROSS) yt[t] = rows_to_tile(p.y, p.ldy, yrow, t, h);
    }
    VF xh[KS], xl[KS], yh_[CROSS ? KS : 1], yl_[CROSS ? KS : 1];
    tiles_to_frags<NT>(xt, sa, xh, xl);
    if constexpr (CROSS) tiles_to_frags<NT>(yt, sa, yh_, yl_);
    const VF* yh = CROSS ? yh_ : xh;
    const VF* yl = CROSS ? yl_ : xl;

    MAB_STAMP(2);
    // ---- feed-forward half: dzf = dropout'(dout) ; du = dzf drop_ff' act'(u) ; dz = dzf + du Wf ; dza = dropout'(dz)
    VB dzah[KS], dzal[KS];
    f32x16 dxa[NT];                       // gradient with respect to x: starts as the residual path
    mab_bwd_ff<NT, LN>(p, dzf, zt, zat, xlive, rF, rFT, sBf, xrow, xvalid, wv, dzah, dzal, dxa);
    MAB_STAMP(3);
    f32x16 dya[CROSS ? NT : 1];
    if constexpr (CROSS) {
#pragma unroll
        for (int t = 0; t < NT; ++t) dya[t] = zero16();
    }
    f32x16* dkv_acc = CROSS ? dya : dxa;

    static_for<0, NT>([&](auto tc) {
        MPG_CI(t, tc);
        // gradient of the attention output of this tile's two heads, both orientations
        const f32x16 dOn = proj_n<KS>(rOT, nfE, t, dzah, dzal, zero16(), lane16);
        const f32x16 dOp = proj_t<KS>(rOT, nfE, t, dzah, dzal, zero16(), lane16);
        const f32x16 Qn = proj_n<KS>(rIn, nfIn, t, xh, xl, bias_regs(sBin, t, h), lane16);
        const f32x16 Kn = proj_n<KS>(rIn, nfIn, NT + t, yh, yl, bias_regs(sBin, NT + t, h), lane16);
        const f32x16 Vn = proj_n<KS>(rIn, nfIn, 2 * NT + t, yh, yl, bias_regs(sBin, 2 * NT + t, h), lane16);
        const f32x16 Qp = proj_t<KS>(rIn, nfIn, t, xh, xl, bias_lanes(sBin, t, r), lane16);
        const f32x16 Kp = proj_t<KS>(rIn, nfIn, NT + t, yh, yl, bias_lanes(sBin, NT + t, r), lane16);
        VB kph[2], kpl[2], qph[2], qpl[2], doph[2], dopl[2];
        static_for<0, 2>([&](auto sc) {
            MPG_CI(s, sc);
            tile_frag(Kp, s, inv_zs, kph[s], kpl[s]);
            tile_frag(Qp, s, inv_zs, qph[s], qpl[s]);
            tile_frag(dOp, s, 1.f, doph[s], dopl[s]);
        });
        f32x16 dQt, dKt, dVt;
        static_for<0, 2>([&](auto ac) {
            MPG_CI(a, ac);
            VF qh, ql, kh, kl;
            tile_frag(Qn, a, inv_zs * sa * 0.25f, qh, ql);
            tile_frag(Kn, a, inv_zs * sa, kh, kl);
            VB vbh, vbl, dobh, dobl;
            tile_frag(Vn, a, inv_zs, vbh, vbl);
            tile_frag(dOn, a, 1.f, dobh, dobl);
            // ---- keys in registers, queries on lanes
            f32x16 s = mfma3(kh, kl, qh, ql, zero16());
            float mx = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) { s[i] = s[i] * sc2 + kneg[i]; mx = fmaxf(mx, s[i]); }
            mx = fmaxf(mx, other_half(mx));
            const float msafe = mx == -INFINITY ? 0.f : mx;   // (a query whose keys are all ignored: zero weights, as in mab_bwdS_kernel)
            float den = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) { s[i] = __builtin_amdgcn_exp2f(s[i] - msafe); den += s[i]; }
            den += other_half(den);
            const bool qlive = den > 0.f;
            const float inv_den = qlive ? 1.f / den : 0.f, cq = qlive ? mx + __builtin_amdgcn_logf(den) : INFINITY;   // log2
            const f32x16 dP = mfma3(vbh, vbl, dobh, dobl, zero16());
            float D = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) { s[i] *= inv_den; D += s[i] * dP[i]; }
            D += other_half(D);
            f32x16 dS;
#pragma unroll
            for (int i = 0; i < 16; ++i) dS[i] = s[i] * (dP[i] - D) * 0.25f;
            VB dsh[2], dsl[2];
            tile_frag(dS, 0, 1.f, dsh[0], dsl[0]);
            tile_frag(dS, 1, 1.f, dsh[1], dsl[1]);
            f32x16 dq = mfma3(kph[0], kpl[0], dsh[0], dsl[0], zero16());
            dq = mfma3(kph[1], kpl[1], dsh[1], dsl[1], dq);
            // ---- queries in registers, keys on lanes
            f32x16 sT = mfma3(qh, ql, kh, kl, zero16());
            const f32x16 dPT = mfma3(dobh, dobl, vbh, vbl, zero16());
            f32x16 pT, dST;
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * g + e, qi = 8 * g + 4 * h + e;   // the query this register belongs to
                    const float c_q = __shfl(cq, qi), D_q = __shfl(D, qi);
                    const float pr = key_off ? 0.f : __builtin_amdgcn_exp2f(sT[i] * sc2 - c_q);
                    pT[i] = pr;
                    dST[i] = pr * (dPT[i] - D_q) * 0.25f;
                }
            VB pth[2], ptl[2], dsth[2], dstl[2];
            static_for<0, 2>([&](auto sc) {
                MPG_CI(s2, sc);
                tile_frag(pT, s2, 1.f, pth[s2], ptl[s2]);
                tile_frag(dST, s2, 1.f, dsth[s2], dstl[s2]);
            });
            f32x16 dk = mfma3(qph[0], qpl[0], dsth[0], dstl[0], zero16());
            dk = mfma3(qph[1], qpl[1], dsth[1], dstl[1], dk);
            f32x16 dv = mfma3(doph[0], dopl[0], pth[0], ptl[0], zero16());
            dv = mfma3(doph[1], dopl[1], pth[1], ptl[1], dv);
#pragma unroll
            for (int j = 0; j < 8; ++j) { dQt[8 * a + j] = dq[8 * a + j]; dKt[8 * a + j] = dk[8 * a + j]; dVt[8 * a + j] = dv[8 * a + j]; }
        });
        if (p.dq != nullptr && xvalid) tile_to_rows(p.dq, p.lddq, xrow, t, h, dQt, 1.f);
        if (p.dk != nullptr && yvalid) {
            tile_to_rows(p.dk, p.lddkv, yrow, t, h, dKt, 1.f);
            tile_to_rows(p.dv, p.lddkv, yrow, t, h, dVt, 1.f);
        }
        // input gradients: dx += dq Wq ; (dy or dx) += dk Wk + dv Wv
        VB fh[2], fl[2];
        tile_frag(dQt, 0, 1.f, fh[0], fl[0]); tile_frag(dQt, 1, 1.f, fh[1], fl[1]);
        acc_wt<NT>(rInT, nfInT, 3 * KS, 2 * t, fh, fl, dxa, lane16);
        tile_frag(dKt, 0, 1.f, fh[0], fl[0]); tile_frag(dKt, 1, 1.f, fh[1], fl[1]);
        acc_wt<NT>(rInT, nfInT, 3 * KS, 2 * (NT + t), fh, fl, dkv_acc, lane16);
        tile_frag(dVt, 0, 1.f, fh[0], fl[0]); tile_frag(dVt, 1, 1.f, fh[1], fl[1]);
        acc_wt<NT>(rInT, nfInT, 3 * KS, 2 * (2 * NT + t), fh, fl, dkv_acc, lane16);
    });
    MAB_STAMP(4);
    static_for<0, NT>([&](auto tc) {
        MPG_CI(t, tc);
        if (p.dx != nullptr && xvalid) tile_to_rows(p.dx, p.lddx, xrow, t, h, dxa[t], 1.f);
        if constexpr (CROSS) {
            if (p.dy != nullptr && yvalid) tile_to_rows(p.dy, p.lddy, yrow, t, h, dya[t], 1.f);
        }
    });
    MAB_STAMP(5);
    }  // (the wave's jet)
    MAB_STAMPS_STORE;
}

// ---- The backward with TWO WAVES PER JET (E = 64), the split of mab_fwd_half: wave T owns tile T of du, dz, dza, the two heads
// of tile T in the attention (q, k, v, P recomputed for those heads only) and tile T of dx (dy).  Three meetings in LDS: du and
// dza are B fragments of products over ALL features, and the input gradient contracts over all of dq | dk | dv.  Each wave
// adds the terms of its dx tile in the order the one-wave kernel does, so the two give the same bits.  The weight images fill
// the LDS (144 of 160 KiB), so the exchange buffers are the images nobody needs any more, each behind one more barrier:
//     du  -> Wf   (free once every wave has recomputed u)         dza -> WfT (free once every wave has dz)
//     dq | dk | dv -> Win (free once every wave is through the attention)
template <int T, typename V>
MPG_DEV void acc_wt1(WImg rT, int nfragT, int KST, int ks0, const V* fh, const V* fl, f32x16& acc, int lane16) {
    static_for<0, 2>([&](auto sc) {
        MPG_CI(s, sc);
        const V wh = mab_wfrag<V>(rT, T * KST + ks0 + s, lane16), wl = mab_wfrag<V>(rT, nfragT + T * KST + ks0 + s, lane16);
        acc = mfma3(wh, wl, fh[s], fl[s], acc);
    });
}

template <int T, bool CROSS>
MPG_DEV void mab_bwd2_body(const MpgMab& p) {
    typedef f16x8 VF;
    typedef bf16x8 VB;
    constexpr int NT = 2, KS = 4, O = 1 - T;
    MAB_STAMPS_DECL;
    MAB_WAVE(p, MAB_STAMP(0), mab_st);
    const int pair = w >> 1;
    const float sc2 = 1.44269504088896341f / (sa * sa);   // (scores in the base-2 domain)
    constexpr int nfIn = 3 * NT * KS, nfE = NT * KS, nfInT = NT * 3 * KS;
    MAB_BWD_CARVE(NT);
    const int npair = blockDim.x >> 7;
    const long jet_raw = (long)blockIdx.x * npair + pair;
    const bool live = jet_raw < p.B;                   // (a pair without a jet goes through the motions: fills and barriers)
    const long jet = live ? jet_raw : (long)p.B - 1;
    const long xrow = jet * p.L + min(r, p.L - 1), yrow = jet * p.S + min(r, p.S - 1);
    // order of issue: biases and key mask (plain loads, used last), every row of the jet (loads the compiler does not count:
    // rows_request), the 144 KiB fill (36 LDS-DMA instructions per wave); the rows are converted UNDER the fill
    MAB_BWD_CARVE_BIASES;
    static_assert(NT == 2 && Lds::NBIAS == 256, "rows_wait counts the fill of an E = 64 block on four waves; a bias per thread");
    const int bi0 = threadIdx.x;
    const float bv0 = MAB_BWD_BIAS_AT(p, bi0);
    const KeyIgn kig = key_mask_load(p.ignore, p.x, jet, p.S, h);
    const float ign_r = (kig.on ? p.ignore + jet * p.S : p.x)[min(r, p.S - 1)];   // this lane as a KEY (transposed tiles)
    f32x4 dq_[4], zq[4 * NT], xq[4 * NT], yq[CROSS ? 4 * NT : 1];
    {
        const float* const pd = p.dout + xrow * p.lddout + 4 * h + 32 * T;
        static_for<0, 4>([&](auto ic) { MPG_CI(i, ic); dq_[i] = ld4_hidden<8 * i * 4>(pd); });
    }
    rows_request<NT>(p.save_z, p.E, xrow, h, zq);
    if constexpr (CROSS) rows_request<NT>(p.y, p.ldy, yrow, h, yq);
    rows_request<NT>(p.x, p.ldx, xrow, h, xq);
    MAB_BWD_FILL(p);
    rows_wait<36>(xq);                                 // (the youngest rows: everything requested before them is here too)
    rows_pin(zq);
    rows_pin4(dq_);
    if constexpr (CROSS) rows_pin(yq);
    f32x16 dzf, zt[NT], xt[NT], yt[CROSS ? NT : 1];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) dzf[4 * g + e] = dq_[g][e];
#pragma unroll
    for (int t = 0; t < NT; ++t) { zt[t] = pieces_tile(zq, t); xt[t] = pieces_tile(xq, t); }
    if constexpr (CROSS) {
#pragma unroll
        for (int t = 0; t < NT; ++t) yt[t] = pieces_tile(yq, t);
    }
    VF xh[KS], xl[KS], yh_[CROSS ? KS : 1], yl_[CROSS ? KS : 1], zh[KS], zl[KS];
    tiles_to_frags<NT>(zt, sa, zh, zl);
    tiles_to_frags<NT>(xt, sa, xh, xl);
    if constexpr (CROSS) tiles_to_frags<NT>(yt, sa, yh_, yl_);
    sBin[bi0] = bv0 * zs;
    const f32x16 kneg = key_mask_from(kig, p.S, h);
    const bool key_off = !(r < p.S) || (kig.on && ign_r != 0.f);
    __syncthreads();
    const WImg rIn = sIn, rF = sF, rInT = sInT, rOT = sOT, rFT = sFT;
    MAB_STAMP(1);
    // exchange slots of 1 KiB: [k-step or fragment index][hi | lo][lane]
    auto put = [&](char* base, int slot, const VB& hi, const VB& lo) {
        reinterpret_cast<VB*>(base)[(slot * 2 + 0) * 64 + lane] = hi;
        reinterpret_cast<VB*>(base)[(slot * 2 + 1) * 64 + lane] = lo;
    };
    auto get = [&](const char* base, int slot, VB& hi, VB& lo) {
        hi = reinterpret_cast<const VB*>(base)[(slot * 2 + 0) * 64 + lane];
        lo = reinterpret_cast<const VB*>(base)[(slot * 2 + 1) * 64 + lane];
    };
    const bool xvalid = live && r < p.L, yvalid = live && r < p.S;
    const float xlive = r < p.L ? 1.f : 0.f;
    const VF* yh = CROSS ? yh_ : xh;
    const VF* yl = CROSS ? yl_ : xl;

    // ---- feed-forward half, tile T
    VB dzah[KS], dzal[KS];
    f32x16 dxa;
    {
        VB duh[KS], dul[KS];
#pragma unroll
        for (int i = 0; i < 16; ++i) dzf[i] *= xlive;
        drop_tile(dzf, seed_lo, seed_hi, p.tag + 2, (uint32_t)xrow, T, h, p.thr_mab, p.sc_mab);
        const f32x16 u = proj_n<KS>(rF, nfE, T, zh, zl, bias_regs(sBf, T, h), lane16);
        f32x16 du;
#pragma unroll
        for (int i = 0; i < 16; ++i) du[i] = dzf[i] * ((p.ff_act && !(u[i] > 0.f)) ? p.alpha : 1.f);
        drop_tile(du, seed_lo, seed_hi, p.tag + 1, (uint32_t)xrow, T, h, p.thr_ff, p.sc_ff);
        if (p.du != nullptr && xvalid) tile_to_rows(p.du, p.E, xrow, T, h, du, 1.f);
        tile_frag(du, 0, 1.f, duh[2 * T], dul[2 * T]);
        tile_frag(du, 1, 1.f, duh[2 * T + 1], dul[2 * T + 1]);
        MAB_STAMP(2);
        __syncthreads();                               // every wave has its u: Wf's image is dead
        char* const x1 = sF + pair * (KS * 2048);
        put(x1, 2 * T, duh[2 * T], dul[2 * T]);
        put(x1, 2 * T + 1, duh[2 * T + 1], dul[2 * T + 1]);
        __syncthreads();
        get(x1, 2 * O, duh[2 * O], dul[2 * O]);
        get(x1, 2 * O + 1, duh[2 * O + 1], dul[2 * O + 1]);
        MAB_STAMP(3);
        f32x16 dz = proj_n<KS>(rFT, nfE, T, duh, dul, dzf, lane16);
        drop_tile(dz, seed_lo, seed_hi, p.tag + 0, (uint32_t)xrow, T, h, p.thr_mab, p.sc_mab);
        if (p.dza != nullptr && xvalid) tile_to_rows(p.dza, p.E, xrow, T, h, dz, 1.f);
        tile_frag(dz, 0, 1.f, dzah[2 * T], dzal[2 * T]);
        tile_frag(dz, 1, 1.f, dzah[2 * T + 1], dzal[2 * T + 1]);
        dxa = dz;
        __syncthreads();                               // every wave has its dz: WfT's image is dead
        char* const x2 = sFT + pair * (KS * 2048);
        put(x2, 2 * T, dzah[2 * T], dzal[2 * T]);
        put(x2, 2 * T + 1, dzah[2 * T + 1], dzal[2 * T + 1]);
        __syncthreads();
        get(x2, 2 * O, dzah[2 * O], dzal[2 * O]);
        get(x2, 2 * O + 1, dzah[2 * O + 1], dzal[2 * O + 1]);
    }
    f32x16 dya = zero16();
    MAB_STAMP(4);

    // ---- the attention of heads 2T, 2T + 1 (mab_bwd_kernel's tile loop body with t = T)
    VB gq_h[NT][2], gq_l[NT][2], gk_h[NT][2], gk_l[NT][2], gv_h[NT][2], gv_l[NT][2];
    {
        constexpr int t = T;
        const f32x16 dOn = proj_n<KS>(rOT, nfE, t, dzah, dzal, zero16(), lane16);
        const f32x16 dOp = proj_t<KS>(rOT, nfE, t, dzah, dzal, zero16(), lane16);
        const f32x16 Qn = proj_n<KS>(rIn, nfIn, t, xh, xl, bias_regs(sBin, t, h), lane16);
        const f32x16 Kn = proj_n<KS>(rIn, nfIn, NT + t, yh, yl, bias_regs(sBin, NT + t, h), lane16);
        const f32x16 Vn = proj_n<KS>(rIn, nfIn, 2 * NT + t, yh, yl, bias_regs(sBin, 2 * NT + t, h), lane16);
        const f32x16 Qp = proj_t<KS>(rIn, nfIn, t, xh, xl, bias_lanes(sBin, t, r), lane16);
        const f32x16 Kp = proj_t<KS>(rIn, nfIn, NT + t, yh, yl, bias_lanes(sBin, NT + t, r), lane16);
        VB kph[2], kpl[2], qph[2], qpl[2], doph[2], dopl[2];
        static_for<0, 2>([&](auto sc) {
            MPG_CI(s, sc);
            tile_frag(Kp, s, inv_zs, kph[s], kpl[s]);
            tile_frag(Qp, s, inv_zs, qph[s], qpl[s]);
            tile_frag(dOp, s, 1.f, doph[s], dopl[s]);
        });
        f32x16 dQt, dKt, dVt;
        static_for<0, 2>([&](auto ac) {
            MPG_CI(a, ac);
            VF qh, ql, kh, kl;
            tile_frag(Qn, a, inv_zs * sa * 0.25f, qh, ql);
            tile_frag(Kn, a, inv_zs * sa, kh, kl);
            VB vbh, vbl, dobh, dobl;
            tile_frag(Vn, a, inv_zs, vbh, vbl);
            tile_frag(dOn, a, 1.f, dobh, dobl);
            f32x16 s = mfma3(kh, kl, qh, ql, zero16());
            float mx = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) { s[i] = s[i] * sc2 + kneg[i]; mx = fmaxf(mx, s[i]); }
            mx = fmaxf(mx, other_half(mx));
            const float msafe = mx == -INFINITY ? 0.f : mx;   // (a query whose keys are all ignored: zero weights, as in mab_bwdS_kernel)
            float den = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) { s[i] = __builtin_amdgcn_exp2f(s[i] - msafe); den += s[i]; }
            den += other_half(den);
            const bool qlive = den > 0.f;
            const float inv_den = qlive ? 1.f / den : 0.f, cq = qlive ? mx + __builtin_amdgcn_logf(den) : INFINITY;   // log2
            const f32x16 dP = mfma3(vbh, vbl, dobh, dobl, zero16());
            float D = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) { s[i] *= inv_den; D += s[i] * dP[i]; }
            D += other_half(D);
            f32x16 dS;
#pragma unroll
            for (int i = 0; i < 16; ++i) dS[i] = s[i] * (dP[i] - D) * 0.25f;
            VB dsh[2], dsl[2];
            tile_frag(dS, 0, 1.f, dsh[0], dsl[0]);
            tile_frag(dS, 1, 1.f, dsh[1], dsl[1]);
            f32x16 dq = mfma3(kph[0], kpl[0], dsh[0], dsl[0], zero16());
            dq = mfma3(kph[1], kpl[1], dsh[1], dsl[1], dq);
            f32x16 sT = mfma3(qh, ql, kh, kl, zero16());
            const f32x16 dPT = mfma3(dobh, dobl, vbh, vbl, zero16());
            f32x16 pT, dST;
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * g + e, qi = 8 * g + 4 * h + e;
                    const float c_q = __shfl(cq, qi), D_q = __shfl(D, qi);
                    const float pr = key_off ? 0.f : __builtin_amdgcn_exp2f(sT[i] * sc2 - c_q);
                    pT[i] = pr;
                    dST[i] = pr * (dPT[i] - D_q) * 0.25f;
                }
            VB pth[2], ptl[2], dsth[2], dstl[2];
            static_for<0, 2>([&](auto sc) {
                MPG_CI(s2, sc);
                tile_frag(pT, s2, 1.f, pth[s2], ptl[s2]);
                tile_frag(dST, s2, 1.f, dsth[s2], dstl[s2]);
            });
            f32x16 dk = mfma3(qph[0], qpl[0], dsth[0], dstl[0], zero16());
            dk = mfma3(qph[1], qpl[1], dsth[1], dstl[1], dk);
            f32x16 dv = mfma3(doph[0], dopl[0], pth[0], ptl[0], zero16());
            dv = mfma3(doph[1], dopl[1], pth[1], ptl[1], dv);
#pragma unroll
            for (int j = 0; j < 8; ++j) { dQt[8 * a + j] = dq[8 * a + j]; dKt[8 * a + j] = dk[8 * a + j]; dVt[8 * a + j] = dv[8 * a + j]; }
        });
        if (p.dq != nullptr && xvalid) tile_to_rows(p.dq, p.lddq, xrow, t, h, dQt, 1.f);
        if (p.dk != nullptr && yvalid) {
            tile_to_rows(p.dk, p.lddkv, yrow, t, h, dKt, 1.f);
            tile_to_rows(p.dv, p.lddkv, yrow, t, h, dVt, 1.f);
        }
        static_for<0, 2>([&](auto sc) {
            MPG_CI(s, sc);
            tile_frag(dQt, s, 1.f, gq_h[T][s], gq_l[T][s]);
            tile_frag(dKt, s, 1.f, gk_h[T][s], gk_l[T][s]);
            tile_frag(dVt, s, 1.f, gv_h[T][s], gv_l[T][s]);
        });
    }
    MAB_STAMP(5);
    __syncthreads();                                   // every wave is through the attention: Win's image is dead
    char* const x3 = sIn + pair * (12 * 2048);         // slots: [tile][q | k | v][s]
    static_for<0, 2>([&](auto sc) {
        MPG_CI(s, sc);
        put(x3, (T * 3 + 0) * 2 + s, gq_h[T][s], gq_l[T][s]);
        put(x3, (T * 3 + 1) * 2 + s, gk_h[T][s], gk_l[T][s]);
        put(x3, (T * 3 + 2) * 2 + s, gv_h[T][s], gv_l[T][s]);
    });
    __syncthreads();
    static_for<0, 2>([&](auto sc) {
        MPG_CI(s, sc);
        get(x3, (O * 3 + 0) * 2 + s, gq_h[O][s], gq_l[O][s]);
        get(x3, (O * 3 + 1) * 2 + s, gk_h[O][s], gk_l[O][s]);
        get(x3, (O * 3 + 2) * 2 + s, gv_h[O][s], gv_l[O][s]);
    });
    MAB_STAMP(6);
    // input gradients of tile T: dx += dq Wq ; (dy or dx) += dk Wk + dv Wv, the heads' tiles in the one-wave kernel's order
    f32x16& dkv = CROSS ? dya : dxa;
    static_for<0, NT>([&](auto tc) {
        MPG_CI(t, tc);
        acc_wt1<T>(rInT, nfInT, 3 * KS, 2 * t, gq_h[t], gq_l[t], dxa, lane16);
        acc_wt1<T>(rInT, nfInT, 3 * KS, 2 * (NT + t), gk_h[t], gk_l[t], dkv, lane16);
        acc_wt1<T>(rInT, nfInT, 3 * KS, 2 * (2 * NT + t), gv_h[t], gv_l[t], dkv, lane16);
    });
    if (p.dx != nullptr && xvalid) tile_to_rows(p.dx, p.lddx, xrow, T, h, dxa, 1.f);
    if constexpr (CROSS) {
        if (p.dy != nullptr && yvalid) tile_to_rows(p.dy, p.lddy, yrow, T, h, dya, 1.f);
    }
    MAB_STAMP(7);
    MAB_STAMPS_STORE;
}

template <bool CROSS>
__global__ __launch_bounds__(256) void mab_bwd2_kernel(const MpgMab p) {
    if (((threadIdx.x >> 6) & 1) == 0) mab_bwd2_body<0, CROSS>(p);
    else mab_bwd2_body<1, CROSS>(p);
}

const MabGo MAB_BWD[2][2][2] = {MAB_CROSS_LN(mab_bwd_kernel, 1), MAB_CROSS_LN(mab_bwd_kernel, 2)};
const MabGo MAB_BWD2[2] = {MAB_GO(mab_bwd2_kernel<false>), MAB_GO(mab_bwd2_kernel<true>)};              // [cross]

}  // namespace

MAB_STAMPS_ENTRY(bwd)

extern "C" int mpg_mab_bwd(const MpgMab* p, void* stream) {
    if (const int rc = mab_check(p)) return rc;
    if (p->dout == nullptr || p->save_z == nullptr || (p->dk == nullptr) != (p->dv == nullptr)) return -5;
    if (p->lddout % 4 || (p->dq != nullptr && p->lddq % 4) || (p->dk != nullptr && p->lddkv % 4) ||
        (p->dx != nullptr && p->lddx % 4) || (p->dy != nullptr && p->lddy % 4)) return -3;
    if (const int rc = mab_ln_check(p, true)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool cross = p->y != p->x, ln = p->ln1_w != nullptr;
    const int NT = p->E / 32;
    if (p->L > 32 || p->S > 32 || getenv("MPG_MAB_BIG") != nullptr)   // large sets: a workgroup per jet, a wave per tile of 32 tokens
        return mab_bwd_big(p, st);
    if (NT == 2 && !ln && mab_split(p->B))                            // two waves per jet, two jets per workgroup
        return MAB_BWD2[cross](dim3((p->B + 1) / 2), dim3(256), mab_bwd_lds(NT), st, *p);
    return mab_launch(MAB_BWD[NT - 1][cross][ln], p, mab_bwd_lds(NT), st, true);   // (layer_norm=True: always one wave per jet)
}
