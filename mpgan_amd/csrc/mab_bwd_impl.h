// What the backward units of the one-launch attention blocks share (mab_bwd.hip: one and two waves per jet; mab_bwds.hip: large
// sets): the weight accumulation, the LayerNorm backward and the feed-forward half.
#pragma once
#include "mab_common.h"

namespace {
// ---------------------------------------------------------------------------------------------------------------------
// Backward of the block, one wave per jet again.  q, k, v, P and u are recomputed from x, y and the saved z with the
// forward's own arithmetic; gradients run as bf16 hi/lo products.  With S' = K Q' (keys in registers) the softmax
// statistics are per lane, and everything that contracts over KEYS follows from it directly:
//     dP = V dO'   (A = V tile registers, B = dO tile registers)      dS = P (dP - sum_keys dP P) / 4
//     dQ' = K' dS  (A = the K projection with swapped operands: features on lanes, keys in registers)
// What contracts over QUERIES needs the transposed tiles, and those are the SAME MFMAs with A and B exchanged:
//     S^T = Q K'   -> P^T = exp(S^T - c_query), c = max + log(sum) fetched per register from the lane that owns the query
//     dP^T = dO V' -> dS^T ;  dK' = Q' dS^T  (A = swapped-operand Q projection) ;  dV' = dO' P^T  (A = swapped-operand dO)
// so no tile is ever transposed through memory.  Rows of x past L carry a zero output gradient and keys past S or
// masked have P = 0, so padding contributes nothing.
template <int NT, typename V>
MPG_DEV void acc_wt(WImg rT, int nfragT, int KST, int ks0, const V* fh, const V* fl, f32x16* acc, int lane16) {
    static_for<0, NT>([&](auto tc) {
        MPG_CI(t, tc);
        static_for<0, 2>([&](auto sc) {
            MPG_CI(s, sc);
            const V wh = mab_wfrag<V>(rT, t * KST + ks0 + s, lane16), wl = mab_wfrag<V>(rT, nfragT + t * KST + ks0 + s, lane16);
            acc[t] = mfma3(wh, wl, fh[s], fl[s], acc[t]);
        });
    });
}

// LayerNorm backward for the tokens of a wave, in place on the gradient tiles: on entry g = dL/d(norm output), xin = the
// norm's INPUT (its statistics are recomputed); the rows of g and of g * xhat go to dn / gn (their column sums are the norm's
// bias and weight gradients: the grouped weight-gradient launch adds them up); on exit g = dL/d(norm input):
//   rstd (g w - mean_f(g w) - xhat mean_f(g w xhat)).
template <int NT>
MPG_DEV void ln_backward(f32x16 (&g)[NT], const f32x16 (&xin)[NT], const float* w, float eps, float* dn, float* gn, int E,
                         long row, bool valid, int h) {
    float mean, rstd;
    ln_stats<NT>(xin, eps, mean, rstd);
    float m1 = 0.f, m2 = 0.f;
    f32x16 xh[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const f32x16 wv = bias_regs(w, t, h);
        f32x16 gx;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            xh[t][i] = (xin[t][i] - mean) * rstd;
            gx[i] = g[t][i] * xh[t][i];
        }
        if (dn != nullptr && valid) { tile_to_rows(dn, E, row, t, h, g[t], 1.f); tile_to_rows(gn, E, row, t, h, gx, 1.f); }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            g[t][i] *= wv[i];
            m1 += g[t][i];
            m2 = fmaf(g[t][i], xh[t][i], m2);
        }
    }
    m1 += other_half(m1); m2 += other_half(m2);
    m1 *= 1.f / (32 * NT); m2 *= 1.f / (32 * NT);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) g[t][i] = rstd * (g[t][i] - m1 - xh[t][i] * m2);
}

// The feed-forward half of a block's backward on the 32 rows a wave holds: dzf = dropout'(dout) [through norm2] ;
// du = dzf drop_ff' act'(u) ; dz = dzf + du Wf ; dza = dropout'(dz) [through norm1].  In: dzf = the rows of dout, zt = the saved z,
// zat = the saved za (LN).  Out: du / dza rows (p.du, p.dza), dza as bf16 fragments, dxa = dza (the residual path of dx).
template <int NT, bool LN>
MPG_DEV void mab_bwd_ff(const MpgMab& p, f32x16 (&dzf)[NT], const f32x16 (&zt)[NT], const f32x16* zat, const float xlive, WImg rF, WImg rFT,
                        const float* sBf, const long xrow, const bool xvalid, const MabWave& wv, bf16x8* dzah, bf16x8* dzal,
                        f32x16 (&dxa)[NT]) {
    typedef f16x8 VF;
    typedef bf16x8 VB;
    const uint32_t seed_lo = wv.seed_lo, seed_hi = wv.seed_hi;
    const float sa = wv.sa, inv_zs = wv.inv_zs;
    const int h = wv.h, lane16 = wv.lane16;
    constexpr int KS = 2 * NT;
    constexpr int nfE = NT * KS;
    {
        VF zh[KS], zl[KS];
        tiles_to_frags<NT>(zt, sa, zh, zl);
        VB duh[KS], dul[KS];
        f32x16 ut[LN ? NT : 1];
        if constexpr (LN) {
            // norm2 sits between the second residual and the last dropout: its input z + dropout_ff(act(u)) is rebuilt as the
            // forward built it (u is needed below anyway), the gradient goes through the norm, and dzf is then what it is
            // without a norm -- the gradient with respect to that sum
            f32x16 op[NT];
            static_for<0, NT>([&](auto tc) {
                MPG_CI(t, tc);
#pragma unroll
                for (int i = 0; i < 16; ++i) dzf[t][i] *= xlive;
                drop_tile(dzf[t], seed_lo, seed_hi, p.tag + 2, (uint32_t)xrow, t, h, p.thr_mab, p.sc_mab);
                ut[t] = proj_n<KS>(rF, nfE, t, zh, zl, bias_regs(sBf, t, h), lane16);
                f32x16 a;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float v = ut[t][i] * inv_zs;
                    a[i] = p.ff_act ? lrelu(v, p.alpha) : v;
                }
                drop_tile(a, seed_lo, seed_hi, p.tag + 1, (uint32_t)xrow, t, h, p.thr_ff, p.sc_ff);
#pragma unroll
                for (int i = 0; i < 16; ++i) op[t][i] = zt[t][i] + a[i];
            });
            ln_backward<NT>(dzf, op, p.ln2_w, p.ln_eps, p.dn2, p.gn2, p.E, xrow, xvalid, h);
        }
        static_for<0, NT>([&](auto tc) {
            MPG_CI(t, tc);
            f32x16 u;
            if constexpr (LN) {
                u = ut[t];
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) dzf[t][i] *= xlive;
                drop_tile(dzf[t], seed_lo, seed_hi, p.tag + 2, (uint32_t)xrow, t, h, p.thr_mab, p.sc_mab);
                u = proj_n<KS>(rF, nfE, t, zh, zl, bias_regs(sBf, t, h), lane16);
            }
            f32x16 du;
#pragma unroll
            for (int i = 0; i < 16; ++i) du[i] = dzf[t][i] * ((p.ff_act && !(u[i] > 0.f)) ? p.alpha : 1.f);
            drop_tile(du, seed_lo, seed_hi, p.tag + 1, (uint32_t)xrow, t, h, p.thr_ff, p.sc_ff);
            if (p.du != nullptr && xvalid) tile_to_rows(p.du, p.E, xrow, t, h, du, 1.f);
            tile_frag(du, 0, 1.f, duh[2 * t], dul[2 * t]);
            tile_frag(du, 1, 1.f, duh[2 * t + 1], dul[2 * t + 1]);
        });
        if constexpr (LN) {
            // dz of every tile, through the first dropout: the gradient with respect to norm1's output; through the norm (its
            // input za was kept by the forward); what comes out is dza
            f32x16 dn[NT];
            static_for<0, NT>([&](auto tc) {
                MPG_CI(t, tc);
                dn[t] = proj_n<KS>(rFT, nfE, t, duh, dul, dzf[t], lane16);
                drop_tile(dn[t], seed_lo, seed_hi, p.tag + 0, (uint32_t)xrow, t, h, p.thr_mab, p.sc_mab);
            });
            ln_backward<NT>(dn, *reinterpret_cast<const f32x16 (*)[NT]>(zat), p.ln1_w, p.ln_eps, p.dn1, p.gn1, p.E, xrow, xvalid, h);
            static_for<0, NT>([&](auto tc) {
                MPG_CI(t, tc);
                if (p.dza != nullptr && xvalid) tile_to_rows(p.dza, p.E, xrow, t, h, dn[t], 1.f);
                tile_frag(dn[t], 0, 1.f, dzah[2 * t], dzal[2 * t]);
                tile_frag(dn[t], 1, 1.f, dzah[2 * t + 1], dzal[2 * t + 1]);
                dxa[t] = dn[t];
            });
        } else {
            static_for<0, NT>([&](auto tc) {
                MPG_CI(t, tc);
                f32x16 dz = proj_n<KS>(rFT, nfE, t, duh, dul, dzf[t], lane16);
                drop_tile(dz, seed_lo, seed_hi, p.tag + 0, (uint32_t)xrow, t, h, p.thr_mab, p.sc_mab);
                if (p.dza != nullptr && xvalid) tile_to_rows(p.dza, p.E, xrow, t, h, dz, 1.f);
                tile_frag(dz, 0, 1.f, dzah[2 * t], dzal[2 * t]);
                tile_frag(dz, 1, 1.f, dzah[2 * t + 1], dzal[2 * t + 1]);
                dxa[t] = dz;
            });
        }
    }
}

}  // namespace
