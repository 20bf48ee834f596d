// The forward kernels of the one-launch attention blocks (mab_common.h: the scheme, the helpers and the LDS layouts), their launch
// tables, mpg_mab_fwd and mpg_mab_chain_fwd.
#include "mab_common.h"

namespace {
// The attention of feature tile T on the 32 query rows a wave holds -- heads 2T and 2T + 1, which never look at the other heads:
// the Q, K, V projections, two heads of masked base-2 softmax, P V.  xh / xl: the query rows as fragments, yh / yl: the key / value
// rows, kneg: the additive key mask.  The output goes to save_o and, as B fragments of the out-projection, to oh / ol [2T], [2T + 1].
template <int NT, int T>
MPG_DEV void attn_tile(const MpgMab& p, const MabWave& wv, WImg rIn, const float* sBin, const f16x8* xh, const f16x8* xl, const f16x8* yh,
                       const f16x8* yl, const f32x16& kneg, const long xrow, const bool xvalid, const int lane16, f16x8* oh, f16x8* ol) {
    typedef f16x8 V;
    constexpr int KS = 2 * NT, nfIn = 3 * NT * KS;
    const float sa = wv.sa, inv_zs = wv.inv_zs;
    const int r = wv.r, h = wv.h;
    const f32x16 Qn = proj_n<KS>(rIn, nfIn, T, xh, xl, bias_regs(sBin, T, h), lane16);
    const f32x16 Kn = proj_n<KS>(rIn, nfIn, NT + T, yh, yl, bias_regs(sBin, NT + T, h), lane16);
    const f32x16 Vt = proj_t<KS>(rIn, nfIn, 2 * NT + T, yh, yl, bias_lanes(sBin, 2 * NT + T, r), lane16);
    V vh[2], vl[2];
    tile_frag(Vt, 0, inv_zs * sa, vh[0], vl[0]);
    tile_frag(Vt, 1, inv_zs * sa, vh[1], vl[1]);
    f32x16 Ot;
    static_for<0, 2>([&](auto ac) {
        MPG_CI(a, ac);                // head 2T + a = features 16a .. 16a+15 of the tile = registers 8a .. 8a+7
        V qh, ql, kh, kl;
        tile_frag(Qn, a, inv_zs * sa * 0.25f, qh, ql);   // 1/sqrt(d), d = 16
        tile_frag(Kn, a, inv_zs * sa, kh, kl);
        f32x16 s = mfma3(kh, kl, qh, ql, zero16());      // keys in registers, queries on lanes
        const float sc2 = 1.44269504088896341f / (sa * sa);   // scores in the base-2 domain: v_exp_f32 is 2^x
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) { s[i] = s[i] * sc2 + kneg[i]; mx = fmaxf(mx, s[i]); }
        mx = fmaxf(mx, other_half(mx));
        const float msafe = mx == -INFINITY ? 0.f : mx;   // (a query whose keys are all ignored: every term below is 0)
        float den = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) { s[i] = __builtin_amdgcn_exp2f(s[i] - msafe); den += s[i]; }
        den += other_half(den);
        const float pn = den > 0.f ? MAB_SP / den : 0.f;   // (... and gets zero attention weights)
        V ph[2], pl[2];
        tile_frag(s, 0, pn, ph[0], pl[0]);
        tile_frag(s, 1, pn, ph[1], pl[1]);
        f32x16 oa = mfma3(vh[0], vl[0], ph[0], pl[0], zero16());
        oa = mfma3(vh[1], vl[1], ph[1], pl[1], oa);
#pragma unroll
        for (int j = 0; j < 8; ++j) Ot[8 * a + j] = oa[8 * a + j];
    });
    // Ot = 256 sa o  (features 32T .. 32T+31 x queries)
    if (p.save_o != nullptr && xvalid) tile_to_rows(p.save_o, p.E, xrow, T, h, Ot, 1.f / (MAB_SP * sa));
    tile_frag(Ot, 0, 1.f / MAB_SP, oh[2 * T], ol[2 * T]);
    tile_frag(Ot, 1, 1.f / MAB_SP, oh[2 * T + 1], ol[2 * T + 1]);
}

// The half of a block behind the attention, on the 32 rows a wave holds: za = x + o Wo' + bo, [norm1], dropout, the feed-forward
// layer with its residual, [norm2], dropout.  oh / ol: the attention output as B fragments; xt: the rows' input tiles on entry, the
// block's OUTPUT rows on exit.  Shared by the one-wave kernels and the large-set kernel (a wave per tile of 32 queries).
template <int NT, bool LN>
MPG_DEV void mab_post(const MpgMab& p, const MabWave& wv, f32x16 (&xt)[NT], const f16x8* oh, const f16x8* ol, WImg rO, WImg rF,
                      const float* sBo, const float* sBf, const long xrow, const bool xvalid) {
    typedef f16x8 V;
    const uint32_t seed_lo = wv.seed_lo, seed_hi = wv.seed_hi;
    const float sa = wv.sa, inv_zs = wv.inv_zs;
    const int h = wv.h, lane16 = wv.lane16;
    MAB_STAMPS_OF(wv);
    constexpr int KS = 2 * NT;
    constexpr int nfE = NT * KS;
    MAB_STAMPP(3);
    // za = x + o Wo' + bo ; z = dropout(za)
    f32x16 z[NT];
    V zh[KS], zl[KS];
    if constexpr (LN) {
        // ... with norm1 between the residual and the dropout: every tile of za first (kept for the backward), then the norm
        static_for<0, NT>([&](auto tc) {
            MPG_CI(t, tc);
            const f32x16 acc = proj_n<KS>(rO, nfE, t, oh, ol, bias_regs(sBo, t, h), lane16);
#pragma unroll
            for (int i = 0; i < 16; ++i) z[t][i] = acc[i] * inv_zs + xt[t][i];
            if (p.save_za != nullptr && xvalid) tile_to_rows(p.save_za, p.E, xrow, t, h, z[t], 1.f);
        });
        ln_apply<NT>(z, p.ln1_w, p.ln1_b, p.ln_eps, h);
    }
    static_for<0, NT>([&](auto tc) {
        MPG_CI(t, tc);
        if constexpr (!LN) {
            const f32x16 acc = proj_n<KS>(rO, nfE, t, oh, ol, bias_regs(sBo, t, h), lane16);
#pragma unroll
            for (int i = 0; i < 16; ++i) z[t][i] = acc[i] * inv_zs + xt[t][i];
        }
        drop_tile(z[t], seed_lo, seed_hi, p.tag + 0, (uint32_t)xrow, t, h, p.thr_mab, p.sc_mab);
        if (p.save_z != nullptr && xvalid) tile_to_rows(p.save_z, p.E, xrow, t, h, z[t], 1.f);
        tile_frag(z[t], 0, sa, zh[2 * t], zl[2 * t]);
        tile_frag(z[t], 1, sa, zh[2 * t + 1], zl[2 * t + 1]);
    });
    MAB_STAMPP(4);
    // out = dropout([norm2](z + dropout_ff(LeakyReLU(z Wf' + bf))))
    f32x16 op[LN ? NT : 1];
    static_for<0, NT>([&](auto tc) {
        MPG_CI(t, tc);
        f32x16 u = proj_n<KS>(rF, nfE, t, zh, zl, bias_regs(sBf, t, h), lane16);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float v = u[i] * inv_zs;
            u[i] = p.ff_act ? lrelu(v, p.alpha) : v;
        }
        drop_tile(u, seed_lo, seed_hi, p.tag + 1, (uint32_t)xrow, t, h, p.thr_ff, p.sc_ff);
#pragma unroll
        for (int i = 0; i < 16; ++i) u[i] += z[t][i];
        if constexpr (LN) {
            op[t] = u;
        } else {
            drop_tile(u, seed_lo, seed_hi, p.tag + 2, (uint32_t)xrow, t, h, p.thr_mab, p.sc_mab);
            if (xvalid) tile_to_rows(p.out, p.ldo, xrow, t, h, u, 1.f);
            xt[t] = u;     // (the block's output rows, as the next block of a chain takes them; z[t] carried the residual)
        }
    });
    if constexpr (LN) {
        ln_apply<NT>(op, p.ln2_w, p.ln2_b, p.ln_eps, h);
        static_for<0, NT>([&](auto tc) {
            MPG_CI(t, tc);
            drop_tile(op[t], seed_lo, seed_hi, p.tag + 2, (uint32_t)xrow, t, h, p.thr_mab, p.sc_mab);
            if (xvalid) tile_to_rows(p.out, p.ldo, xrow, t, h, op[t], 1.f);
            xt[t] = op[t];
        });
    }
}

// One block on one jet (one wave).  xt: the block's query rows as accumulator-layout tiles on entry, its OUTPUT rows on exit (what
// the next block of a chain of self-attention blocks takes as its input: mab_chain_fwd_kernel); yt: the key / value rows
// (CROSS), kneg the additive key mask; the weight images and the pre-scaled biases are in LDS.
template <int NT, bool CROSS, bool LN = false>
MPG_DEV void mab_fwd_jet(const MpgMab& p, const MabWave& wv, f32x16 (&xt)[NT], const f32x16* yt, const f32x16& kneg, WImg rIn, WImg rO,
                         WImg rF, const float* sBin, const float* sBo, const float* sBf, const long xrow, const bool xvalid) {
    typedef f16x8 V;
    const float sa = wv.sa, inv_zs = wv.inv_zs;
    const int r = wv.r, h = wv.h, lane16 = wv.lane16;
    MAB_STAMPS_OF(wv);
    constexpr int KS = 2 * NT;
    constexpr int nfIn = 3 * NT * KS, nfE = NT * KS;
    V xh[KS], xl[KS], yh_[CROSS ? KS : 1], yl_[CROSS ? KS : 1];
    tiles_to_frags<NT>(xt, sa, xh, xl);
    if constexpr (CROSS) tiles_to_frags<NT>(yt, sa, yh_, yl_);
    const V* yh = CROSS ? yh_ : xh;
    const V* yl = CROSS ? yl_ : xl;

    MAB_STAMPP(2);
    V oh[KS], ol[KS];                     // attention output as B fragments of the out-projection
    static_for<0, NT>([&](auto tc) {
        MPG_CI(t, tc);
        attn_tile<NT, t>(p, wv, rIn, sBin, xh, xl, yh, yl, kneg, xrow, xvalid, lane16, oh, ol);
    });

    mab_post<NT, LN>(p, wv, xt, oh, ol, rO, rF, sBo, sBf, xrow, xvalid);
    MAB_STAMPP(5);
}

template <int NT, bool CROSS, bool LN = false>
__global__ __launch_bounds__(256) void mab_fwd_kernel(const MpgMab p) {
    typedef f16x8 V;
    constexpr int KS = 2 * NT;            // k-steps of 16 over E = 32 NT features
    MAB_STAMPS_DECL;
    MAB_WAVE(p, MAB_STAMP(0), mab_st);
    constexpr int nfIn = 3 * NT * KS, nfE = NT * KS;
    MAB_FWD_CARVE(NT);
    // the wave's first jet: its rows are requested BEFORE the weight fill (loads return in issue order; behind 80 KiB of
    // weights per workgroup they would arrive ~3,000 clk later, and their conversion can run while the fill lands)
    const int nw = blockDim.x >> 6;
    const long jet0 = (long)blockIdx.x * nw + w;
    f32x16 xt[NT], yt[CROSS ? NT : 1], kneg;
    auto load_rows = [&](long jet) {
        const long xr = jet * p.L + min(r, p.L - 1), yr = jet * p.S + min(r, p.S - 1);
#pragma unroll
        for (int t = 0; t < NT; ++t) xt[t] = rows_to_tile(p.x, p.ldx, xr, t, h);
        if constexpr (CROSS) {
#pragma unroll
            for (int t = 0; t < NT; ++t) yt[t] = rows_to_tile(p.y, p.ldy, yr, t, h);
        }
        kneg = key_mask_regs(p.ignore, p.x, jet, p.S, h);
    };
    load_rows(min(jet0, (long)p.B - 1));
    MAB_FWD_FILL(p);
    MAB_FWD_STAGE_BIASES(p);
    __syncthreads();
    const WImg rIn = sIn, rO = sO, rF = sF;
    MAB_STAMP(1);
    for (long jet = jet0; jet < p.B; jet += (long)gridDim.x * nw) {   // (no barrier inside)

    // rows past the end of a set are read from its last row and never stored; as keys they are masked
    const long xrow = jet * p.L + min(r, p.L - 1);
    const bool xvalid = r < p.L;
    // every global load of a jet is issued together: x (kept as tiles for the residual), y, the key mask
    if (jet != jet0) load_rows(jet);
    mab_fwd_jet<NT, CROSS, LN>(p, wv, xt, yt, kneg, rIn, rO, rF, sBin, sBo, sBf, xrow, xvalid);
    }  // jets of this wave
    MAB_STAMPS_STORE;
}

// ---- LARGE SETS (33 ... 160 tokens: --num-hits 150, gapt/model.py has no size limit).  One workgroup per jet, one wave per TILE of
// 32 queries.  A wave walks the key tiles with a running maximum / sum per (query, head) -- scores of one key tile at a time:
// keys in registers, queries on lanes, exactly the one-wave kernel's products --, projecting each key tile's K and V from its
// rows itself (the rows come out of L2; no exchange between the waves, no barrier behind the weight fill), rescales its output
// accumulators when the maximum moves, and runs the half behind the attention (mab_post) on its own 32 rows.  A query whose keys
// are all masked gets a zero attention output (torch's _safe_softmax).
template <int NT, bool LN>
__global__ __launch_bounds__(320) void mab_fwdN_kernel(const MpgMab p) {
    typedef f16x8 V;
    constexpr int KS = 2 * NT;
    MAB_WAVE(p, , nullptr);
    constexpr int nfIn = 3 * NT * KS, nfE = NT * KS;
    MAB_FWD_CARVE(NT);
    const long jet = blockIdx.x;
    const int nqt = (p.L + 31) >> 5, nkt = (p.S + 31) >> 5;
    const int tok = 32 * w + r;
    const long xrow = jet * p.L + min(tok, p.L - 1);
    const bool xvalid = tok < p.L;
    f32x16 xt[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) xt[t] = rows_to_tile(p.x, p.ldx, xrow, t, h);
    MAB_FWD_FILL(p);
    MAB_FWD_STAGE_BIASES(p);
    __syncthreads();
    const WImg rIn = sIn, rO = sO, rF = sF;
    const bool isq = w < nqt, isk = w < nkt;
    V qh[2 * NT], ql[2 * NT];             // the queries' heads as B fragments: head 2t + a
    if (isq) {
        V xh[KS], xl[KS];
        tiles_to_frags<NT>(xt, sa, xh, xl);
        static_for<0, NT>([&](auto tc) {
            MPG_CI(t, tc);
            const f32x16 Qn = proj_n<KS>(rIn, nfIn, t, xh, xl, bias_regs(sBin, t, h), lane16);
            tile_frag(Qn, 0, inv_zs * sa * 0.25f, qh[2 * t], ql[2 * t]);      // 1/sqrt(d), d = 16
            tile_frag(Qn, 1, inv_zs * sa * 0.25f, qh[2 * t + 1], ql[2 * t + 1]);
        });
    }
    // ---- the key side ONCE per key tile: wave w projects K and V of key tile w, and behind a barrier -- every wave is done with
    // Win's image then -- lays the fragments the attention takes down where that image was (3 tiles' worth) and in 32 KiB of
    // their own behind the biases: [key tile][feature tile][kh0 kl0 kh1 kl1 | vh0 vl0 vh1 vl1][lane] 16 B.  (Projected by every
    // query wave for itself they were 48 of the 84 MFMAs per key tile.)
    auto kv_slot = [&](int kt) -> char* {
        return kt < Lds::WIN_TILES ? sIn + kt * Lds::KVT : MAB_FWD_TAIL + (kt - Lds::WIN_TILES) * Lds::KVT;
    };
    {
        V kvf[8 * NT];
        if (isk) {
            const long yrow = jet * p.S + min(32 * w + r, p.S - 1);
            V yh[KS], yl[KS];
            rows_to_frags<KS>(p.y, p.ldy, yrow, sa, h, yh, yl);
            static_for<0, NT>([&](auto tc) {
                MPG_CI(t, tc);
                const f32x16 Kn = proj_n<KS>(rIn, nfIn, NT + t, yh, yl, bias_regs(sBin, NT + t, h), lane16);
                const f32x16 Vt = proj_t<KS>(rIn, nfIn, 2 * NT + t, yh, yl, bias_lanes(sBin, 2 * NT + t, r), lane16);
                tile_frag(Kn, 0, inv_zs * sa, kvf[8 * t + 0], kvf[8 * t + 1]);
                tile_frag(Kn, 1, inv_zs * sa, kvf[8 * t + 2], kvf[8 * t + 3]);
                tile_frag(Vt, 0, inv_zs * sa, kvf[8 * t + 4], kvf[8 * t + 5]);
                tile_frag(Vt, 1, inv_zs * sa, kvf[8 * t + 6], kvf[8 * t + 7]);
            });
        }
        __syncthreads();                  // every projection that reads Win's image is done
        if (isk) {
            V* const dst = reinterpret_cast<V*>(kv_slot(w));
#pragma unroll
            for (int i = 0; i < 8 * NT; ++i) dst[i * 64 + lane] = kvf[i];
        }
        __syncthreads();
    }
    if (!isq) return;                     // (a wave without a query tile: it has helped with the fill and the key side)
    const float sc2 = 1.44269504088896341f / (sa * sa);   // scores in the base-2 domain
    float mrun[2 * NT], den[2 * NT];
    f32x16 oacc[2 * NT];
#pragma unroll
    for (int i = 0; i < 2 * NT; ++i) { mrun[i] = -INFINITY; den[i] = 0.f; oacc[i] = zero16(); }
    for (int kt = 0; kt < nkt; ++kt) {
        const f32x16 kneg = key_mask_tile(p.ignore, p.x, jet, p.S, h, kt);
        const V* const src = reinterpret_cast<const V*>(kv_slot(kt));
        static_for<0, NT>([&](auto tc) {
            MPG_CI(t, tc);
            const V vh[2] = {src[(8 * t + 4) * 64 + lane], src[(8 * t + 6) * 64 + lane]};
            const V vl[2] = {src[(8 * t + 5) * 64 + lane], src[(8 * t + 7) * 64 + lane]};
            static_for<0, 2>([&](auto ac) {
                MPG_CI(a, ac);
                constexpr int hd = 2 * t + a;
                const V kh = src[(8 * t + 2 * a) * 64 + lane], kl = src[(8 * t + 2 * a + 1) * 64 + lane];
                f32x16 sx = mfma3(kh, kl, qh[hd], ql[hd], zero16());      // keys in registers, queries on lanes
                float mx = -INFINITY;
#pragma unroll
                for (int i = 0; i < 16; ++i) { sx[i] = sx[i] * sc2 + kneg[i]; mx = fmaxf(mx, sx[i]); }
                mx = fmaxf(mx, other_half(mx));
                const float mnew = fmaxf(mrun[hd], mx);
                const float msafe = mnew == -INFINITY ? 0.f : mnew;       // (nothing but masked keys so far: every term below is 0)
                const float resc = __builtin_amdgcn_exp2f(mrun[hd] - msafe);
                mrun[hd] = mnew;
                float part = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) { sx[i] = __builtin_amdgcn_exp2f(sx[i] - msafe); part += sx[i]; }
                part += other_half(part);
                den[hd] = den[hd] * resc + part;
                V ph[2], pl[2];
                tile_frag(sx, 0, MAB_SP, ph[0], pl[0]);
                tile_frag(sx, 1, MAB_SP, ph[1], pl[1]);
#pragma unroll
                for (int i = 0; i < 16; ++i) oacc[hd][i] *= resc;
                oacc[hd] = mfma3(vh[0], vl[0], ph[0], pl[0], oacc[hd]);
                oacc[hd] = mfma3(vh[1], vl[1], ph[1], pl[1], oacc[hd]);
            });
        });
    }
    V oh[KS], ol[KS];
    static_for<0, NT>([&](auto tc) {
        MPG_CI(t, tc);
        f32x16 Ot;
        static_for<0, 2>([&](auto ac) {
            MPG_CI(a, ac);
            constexpr int hd = 2 * t + a;
            const float inv = den[hd] > 0.f ? 1.f / den[hd] : 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) Ot[8 * a + j] = oacc[hd][8 * a + j] * inv;
        });
        // Ot = 256 sa o  (features 32t .. 32t+31 x queries)
        if (p.save_o != nullptr && xvalid) tile_to_rows(p.save_o, p.E, xrow, t, h, Ot, 1.f / (MAB_SP * sa));
        tile_frag(Ot, 0, 1.f / MAB_SP, oh[2 * t], ol[2 * t]);
        tile_frag(Ot, 1, 1.f / MAB_SP, oh[2 * t + 1], ol[2 * t + 1]);
    });
    mab_post<NT, LN>(p, wv, xt, oh, ol, rO, rF, sBo, sBf, xrow, xvalid);
}

// A CHAIN of self-attention blocks (the SABs of a GAPT network, gapt/model.py:261-262 / :341-342: x = sab(x, mask) in a loop) in
// one launch: a wave keeps its jet's rows in registers from block to block -- only the weights change (one cooperative refill
// of the LDS images per block, between two barriers) -- so a block's launch, its prologue and the round trip of its input rows
// through memory are paid once per chain.  Every block still writes what its backward needs (out = the next block's x,
// save_o, save_z) as the single launches do, with its own dropout sites: bit-identical to them.  One jet per wave.
template <int NT>
__global__ __launch_bounds__(256) void mab_chain_fwd_kernel(const MpgMabChain c) {
    constexpr int KS = 2 * NT;
    const MpgMab& p0 = c.blk[0];
    MAB_WAVE(p0, , nullptr);
    constexpr int nfIn = 3 * NT * KS, nfE = NT * KS;
    MAB_FWD_CARVE(NT);
    const int nw = blockDim.x >> 6;
    const long jet = (long)blockIdx.x * nw + w;
    const bool live = jet < p0.B;                      // (a wave without a jet still takes part in the fills and barriers)
    const long jc = live ? jet : (long)p0.B - 1;
    const long xrow = jc * p0.L + min(r, p0.L - 1);
    const bool xvalid = live && r < p0.L;
    f32x16 xt[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) xt[t] = rows_to_tile(p0.x, p0.ldx, xrow, t, h);
    const f32x16 kneg = key_mask_regs(p0.ignore, p0.x, jc, p0.S, h);
    static_for<0, MPG_MAB_CHAIN_MAX>([&](auto bc) {     // (compile-time index: a run-time one would move the argument block to scratch)
        MPG_CI(b, bc);
        if (b < c.n) {
            const MpgMab& p = c.blk[b];
            if (b > 0) __syncthreads();                 // every wave is done with the images of the block before
            MAB_FWD_FILL(p);
            MAB_FWD_STAGE_BIASES(p);
            __syncthreads();
            mab_fwd_jet<NT, false>(p, wv, xt, xt, kneg, sIn, sO, sF, sBin, sBo, sBf, xrow, xvalid);
        }
    });
}

// ---- TWO WAVES PER JET (E = 64, self-attention).  A block is a dependent chain of ~150 MFMAs and the hi/lo splits between
// them on ONE wave, and a launch of 512 jets leaves half of the chip's SIMDs without a wave.  Here wave `T` of a pair owns
// feature tile T of every tensor of the block -- heads 2T and 2T + 1 of the attention (which never look at the other heads),
// tile T of the out-projection, of the feed-forward layer and of the output -- and the pair meets twice per block in LDS:
// the attention output and z are needed by both as B fragments of the next product (each writes its two k-steps, reads the
// partner's two).  In a chain the output rows go across a third time, as the next block's x fragments.  Half the MFMAs, half
// the splits and half the softmax per wave; same arithmetic per element, hence the same bits as the one-wave form.
template <int T>
MPG_DEV void mab_fwd_half(const MpgMab& p, const MabWave& wv, f16x8* xh, f16x8* xl, const f16x8* yh, const f16x8* yl, f32x16& xtile,
                          const f32x16& kneg, WImg rIn, WImg rO, WImg rF, const float* sBin, const float* sBo, const float* sBf,
                          const long xrow, const bool xvalid, const int lane, char* xchA, char* xchB, const bool next_x) {
    typedef f16x8 V;
    const uint32_t seed_lo = wv.seed_lo, seed_hi = wv.seed_hi;
    const float sa = wv.sa, inv_zs = wv.inv_zs;
    const int r = wv.r, h = wv.h;
    MAB_STAMPS_OF(wv);
    constexpr int NT = 2, KS = 4, nfIn = 3 * NT * KS, nfE = NT * KS, O = 1 - T;
    const int lane16 = lane * 16;
    V* const fa = reinterpret_cast<V*>(xchA);
    V* const fb = reinterpret_cast<V*>(xchB);
    auto put = [&](V* f, int ks, const V& hi, const V& lo) { f[(ks * 2 + 0) * 64 + lane] = hi; f[(ks * 2 + 1) * 64 + lane] = lo; };
    auto get = [&](const V* f, int ks, V& hi, V& lo) { hi = f[(ks * 2 + 0) * 64 + lane]; lo = f[(ks * 2 + 1) * 64 + lane]; };
    V oh[KS], ol[KS];
    attn_tile<NT, T>(p, wv, rIn, sBin, xh, xl, yh, yl, kneg, xrow, xvalid, lane16, oh, ol);
    MAB_STAMPP(3);
    put(fa, 2 * T, oh[2 * T], ol[2 * T]);
    put(fa, 2 * T + 1, oh[2 * T + 1], ol[2 * T + 1]);
    __syncthreads();
    get(fa, 2 * O, oh[2 * O], ol[2 * O]);
    get(fa, 2 * O + 1, oh[2 * O + 1], ol[2 * O + 1]);
    MAB_STAMPP(4);
    // za = x + o Wo' + bo ; z = dropout(za): tile T
    f32x16 z;
    V zh[KS], zl[KS];
    {
        const f32x16 acc = proj_n<KS>(rO, nfE, T, oh, ol, bias_regs(sBo, T, h), lane16);
#pragma unroll
        for (int i = 0; i < 16; ++i) z[i] = acc[i] * inv_zs + xtile[i];
        drop_tile(z, seed_lo, seed_hi, p.tag + 0, (uint32_t)xrow, T, h, p.thr_mab, p.sc_mab);
        if (p.save_z != nullptr && xvalid) tile_to_rows(p.save_z, p.E, xrow, T, h, z, 1.f);
        tile_frag(z, 0, sa, zh[2 * T], zl[2 * T]);
        tile_frag(z, 1, sa, zh[2 * T + 1], zl[2 * T + 1]);
    }
    MAB_STAMPP(5);
    put(fb, 2 * T, zh[2 * T], zl[2 * T]);
    put(fb, 2 * T + 1, zh[2 * T + 1], zl[2 * T + 1]);
    __syncthreads();
    get(fb, 2 * O, zh[2 * O], zl[2 * O]);
    get(fb, 2 * O + 1, zh[2 * O + 1], zl[2 * O + 1]);
    MAB_STAMPP(6);
    // out = dropout(z + dropout_ff(LeakyReLU(z Wf' + bf))): tile T
    f32x16 u = proj_n<KS>(rF, nfE, T, zh, zl, bias_regs(sBf, T, h), lane16);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float v = u[i] * inv_zs;
        u[i] = p.ff_act ? lrelu(v, p.alpha) : v;
    }
    drop_tile(u, seed_lo, seed_hi, p.tag + 1, (uint32_t)xrow, T, h, p.thr_ff, p.sc_ff);
#pragma unroll
    for (int i = 0; i < 16; ++i) u[i] += z[i];
    drop_tile(u, seed_lo, seed_hi, p.tag + 2, (uint32_t)xrow, T, h, p.thr_mab, p.sc_mab);
    if (xvalid) tile_to_rows(p.out, p.ldo, xrow, T, h, u, 1.f);
    xtile = u;
    MAB_STAMPP(7);
    if (next_x) {   // the next block's x fragments: own k-steps from the registers, the partner's through the first buffer
        tile_frag(u, 0, sa, xh[2 * T], xl[2 * T]);
        tile_frag(u, 1, sa, xh[2 * T + 1], xl[2 * T + 1]);
        put(fa, 2 * T, xh[2 * T], xl[2 * T]);          // (the partner read its o fragments before the second barrier)
        put(fa, 2 * T + 1, xh[2 * T + 1], xl[2 * T + 1]);
        __syncthreads();
        get(fa, 2 * O, xh[2 * O], xl[2 * O]);
        get(fa, 2 * O + 1, xh[2 * O + 1], xl[2 * O + 1]);
    }
}

// the chain of self-attention blocks with two waves per jet; a workgroup of four waves carries two jets
template <int NW>   // waves of a workgroup: 4 (two jets) or 8 (four jets, two waves to a SIMD)
__global__ __launch_bounds__(64 * NW) void mab_chain_fwd2_kernel(const MpgMabChain c) {
    typedef f16x8 V;
    constexpr int NT = 2, KS = 4;
    const MpgMab& p0 = c.blk[0];
    MAB_WAVE(p0, const int pair = w >> 1; const int role = w & 1, nullptr);   // (the pair's split where it was: in front of the seed read)
    constexpr int nfIn = 3 * NT * KS, nfE = NT * KS;
    MAB_FWD_CARVE(NT);
    char* const xchA = MAB_FWD_TAIL + pair * 2 * MAB_XCH;
    char* const xchB = xchA + MAB_XCH;
    const int npair = blockDim.x >> 7;
    const long jet = (long)blockIdx.x * npair + pair;
    const bool live = jet < p0.B;                      // (a pair without a jet still takes part in the fills and barriers)
    const long jc = live ? jet : (long)p0.B - 1;
    const long xrow = jc * p0.L + min(r, p0.L - 1);
    const bool xvalid = live && r < p0.L;
    // order of issue: a block's biases and (first block) the key mask -- plain loads, used last --, the jet's rows (loads
    // the compiler does not count: rows_request), the fill; the rows are converted UNDER the fill, which takes the CU ~2,900 clk
    // to issue alone (tools/ubench/fill_rate.hip)
    V xh[KS], xl[KS];
    f32x16 xtile, kneg;
    const KeyIgn kig = key_mask_load(p0.ignore, p0.x, jc, p0.S, h);
    f32x4 xq[4 * NT];
    const int bi0 = min((int)threadIdx.x, Lds::NBIAS - 1), bi1 = min((int)threadIdx.x + 256, Lds::NBIAS - 1);
    static_assert(NT == 2 && (NW == 4 || NW == 8), "rows_wait counts the fill of an E = 64 block on NW waves");
    static_for<0, MPG_MAB_CHAIN_MAX>([&](auto bc) {
        MPG_CI(b, bc);
        if (b < c.n) {
            const MpgMab& p = c.blk[b];
            auto bias_at = [&](int i) { return MAB_FWD_BIAS_AT(p, i); };
            const float bv0 = bias_at(bi0), bv1 = bias_at(bi1);
            if (b == 0) rows_request<NT>(p0.x, p0.ldx, xrow, h, xq);
            if (b > 0) __syncthreads();                 // every wave is done with the images of the block before
            MAB_FWD_FILL(p);
            if (b == 0) {
                rows_wait<80 / NW>(xq);
                f32x16 xt[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) xt[t] = pieces_tile(xq, t);
                tiles_to_frags<NT>(xt, sa, xh, xl);
                xtile = role == 0 ? xt[0] : xt[1];
            }
            if (threadIdx.x < Lds::NBIAS) sBin[bi0] = bv0 * zs;
            if (NW == 4 && threadIdx.x + 256 < Lds::NBIAS) sBin[bi1] = bv1 * zs;
            if (b == 0) kneg = key_mask_from(kig, p0.S, h);
            __syncthreads();
            const bool nx = b + 1 < c.n;
            if (role == 0) mab_fwd_half<0>(p, wv, xh, xl, xh, xl, xtile, kneg, sIn, sO, sF, sBin, sBo, sBf, xrow, xvalid, lane, xchA, xchB, nx);
            else mab_fwd_half<1>(p, wv, xh, xl, xh, xl, xtile, kneg, sIn, sO, sF, sBin, sBo, sBf, xrow, xvalid, lane, xchA, xchB, nx);
        }
    });
}

// one block with two waves per jet, self- or cross-attention (the key / value rows y as a second set of fragments)
template <bool CROSS, int NW>
__global__ __launch_bounds__(64 * NW) void mab_fwd2_kernel(const MpgMab p) {
    typedef f16x8 V;
    constexpr int NT = 2, KS = 4;
    MAB_STAMPS_DECL;
    MAB_WAVE(p, MAB_STAMPP(0), mab_st);
    const int pair = w >> 1, role = w & 1;
    constexpr int nfIn = 3 * NT * KS, nfE = NT * KS;
    MAB_FWD_CARVE(NT);
    char* const xchA = MAB_FWD_TAIL + pair * 2 * MAB_XCH;
    char* const xchB = xchA + MAB_XCH;
    const int npair = blockDim.x >> 7;
    const long jet = (long)blockIdx.x * npair + pair;
    const bool live = jet < p.B;
    const long jc = live ? jet : (long)p.B - 1;
    const long xrow = jc * p.L + min(r, p.L - 1), yrow = jc * p.S + min(r, p.S - 1);
    const bool xvalid = live && r < p.L;
    // rows and key mask requested ahead of the weight fill, converted behind it (see mab_chain_fwd2_kernel)
    V xh[KS], xl[KS], yh_[CROSS ? KS : 1], yl_[CROSS ? KS : 1];
    f32x16 xtile;
    // order of issue: biases and key mask (plain loads, used last), the rows (uncounted loads), the fill; then the rows are
    // converted UNDER the fill (20 LDS-DMA instructions per wave behind them: rows_wait<20>)
    const int bi0 = min((int)threadIdx.x, Lds::NBIAS - 1), bi1 = min((int)threadIdx.x + 256, Lds::NBIAS - 1);
    auto bias_at = [&](int i) { return MAB_FWD_BIAS_AT(p, i); };
    const float bv0 = bias_at(bi0), bv1 = bias_at(bi1);
    const KeyIgn kig = key_mask_load(p.ignore, p.x, jc, p.S, h);
    f32x4 xq[4 * NT], yq[CROSS ? 4 * NT : 1];
    if constexpr (CROSS) rows_request<NT>(p.y, p.ldy, yrow, h, yq);
    rows_request<NT>(p.x, p.ldx, xrow, h, xq);
    static_assert(NT == 2 && (NW == 4 || NW == 8), "rows_wait counts the fill of an E = 64 block on NW waves");
    MAB_FWD_FILL(p);
    f32x16 xt[NT], yt[CROSS ? NT : 1];
    if constexpr (CROSS) {
        rows_wait<80 / NW + 4 * NT>(yq);
#pragma unroll
        for (int t = 0; t < NT; ++t) yt[t] = pieces_tile(yq, t);
        tiles_to_frags<NT>(yt, sa, yh_, yl_);
    }
    rows_wait<80 / NW>(xq);
#pragma unroll
    for (int t = 0; t < NT; ++t) xt[t] = pieces_tile(xq, t);
    tiles_to_frags<NT>(xt, sa, xh, xl);
    xtile = role == 0 ? xt[0] : xt[1];
    const V* yh = CROSS ? yh_ : xh;
    const V* yl = CROSS ? yl_ : xl;
    if (threadIdx.x < Lds::NBIAS) sBin[bi0] = bv0 * zs;
    if (NW == 4 && threadIdx.x + 256 < Lds::NBIAS) sBin[bi1] = bv1 * zs;
    const f32x16 kneg = key_mask_from(kig, p.S, h);
    __syncthreads();
    MAB_STAMPP(1);
    if (role == 0) mab_fwd_half<0>(p, wv, xh, xl, yh, yl, xtile, kneg, sIn, sO, sF, sBin, sBo, sBf, xrow, xvalid, lane, xchA, xchB, false);
    else mab_fwd_half<1>(p, wv, xh, xl, yh, yl, xtile, kneg, sIn, sO, sF, sBin, sBo, sBf, xrow, xvalid, lane, xchA, xchB, false);
    MAB_STAMPS_STORE;
}

const MabGo MAB_FWD[2][2][2] = {MAB_CROSS_LN(mab_fwd_kernel, 1), MAB_CROSS_LN(mab_fwd_kernel, 2)};      // [E / 32 - 1][cross][ln]
const MabGo MAB_FWDN[2][2] = {{MAB_GO(mab_fwdN_kernel<1, false>), MAB_GO(mab_fwdN_kernel<1, true>)},    // [E / 32 - 1][ln]
                              {MAB_GO(mab_fwdN_kernel<2, false>), MAB_GO(mab_fwdN_kernel<2, true>)}};
// the split kernels (two waves per jet) exist at E = 64 only, and never with LayerNorm
const MabGo MAB_FWD2[2][2] = {{MAB_GO(mab_fwd2_kernel<false, 4>), MAB_GO(mab_fwd2_kernel<false, 8>)},   // [cross][waves == 8]
                              {MAB_GO(mab_fwd2_kernel<true, 4>), MAB_GO(mab_fwd2_kernel<true, 8>)}};
const MabChainGo MAB_CHAIN[2] = {mpg_go<mab_chain_fwd_kernel<1>, MpgMabChain>, mpg_go<mab_chain_fwd_kernel<2>, MpgMabChain>};     // [E / 32 - 1]
const MabChainGo MAB_CHAIN2[2] = {mpg_go<mab_chain_fwd2_kernel<4>, MpgMabChain>, mpg_go<mab_chain_fwd2_kernel<8>, MpgMabChain>};  // [waves == 8]

}  // namespace

MAB_STAMPS_ENTRY(fwd)

extern "C" int mpg_mab_fwd(const MpgMab* p, void* stream) {
    if (const int rc = mab_check(p)) return rc;
    if (const int rc = mab_ln_check(p, false)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool cross = p->y != p->x, ln = p->ln1_w != nullptr;
    const int NT = p->E / 32;
    if (p->L > 32 || p->S > 32 || getenv("MPG_MAB_BIG") != nullptr)   // large sets: a workgroup per jet, a wave per tile of 32 queries
        return MAB_FWDN[NT - 1][ln](dim3(p->B), dim3(64 * ((std::max(p->L, p->S) + 31) / 32)), mab_big_lds(NT, false), st, *p);
    // layer_norm=True: one wave per jet (a token's statistics run over both feature tiles)
    if (const int nw2 = (NT == 2 && !ln) ? mab_split_fwd_waves(p->B) : 0) {
        const int npair = nw2 / 2;
        return MAB_FWD2[cross][nw2 == 8](dim3((p->B + npair - 1) / npair), dim3(64 * nw2), mab_fwd_lds(NT, npair), st, *p);
    }
    return mab_launch(MAB_FWD[NT - 1][cross][ln], p, mab_fwd_lds(NT), st);
}

extern "C" int mpg_mab_chain_fwd(const MpgMabChain* c, void* stream) {
    if (c->n < 1 || c->n > MPG_MAB_CHAIN_MAX) return -1;
    const MpgMab& p0 = c->blk[0];
    if (const int rc = mab_check(&p0)) return rc;
    if (p0.L > 32) return -1;             // (the chain keeps a jet's rows in ONE wave's registers)
    for (int b = 0; b < c->n; ++b) {
        const MpgMab& p = c->blk[b];
        // self-attention blocks of one shape on one set of jets, each taking the rows the one before it writes
        if (p.y != p.x || p.B != p0.B || p.L != p0.L || p.S != p0.L || p.E != p0.E || p.H != p0.H || p.ignore != p0.ignore ||
            p.seed != p0.seed || p.wscale != p0.wscale || p.ascale != p0.ascale || p.out == nullptr || p.ldo % 4 || p.ln1_w != nullptr) return -2;
        if (b > 0 && (p.x != c->blk[b - 1].out || p.ldx != c->blk[b - 1].ldo)) return -2;
        if (!(p.alpha >= 0.f && p.alpha <= 1.f)) return -4;
    }
    const int NT = p0.E / 32;
    hipStream_t st = (hipStream_t)stream;
    if (const int nw2 = NT == 2 ? mab_split_fwd_waves(p0.B) : 0) {   // two waves per jet, two or four jets per workgroup
        const int npair = nw2 / 2;
        return MAB_CHAIN2[nw2 == 8](dim3((p0.B + npair - 1) / npair), dim3(64 * nw2), mab_fwd_lds(NT, npair), st, *c);
    }
    const int nw = mab_waves(p0.B);       // one jet per wave: its rows stay in registers across the blocks
    return MAB_CHAIN[NT - 1](dim3((p0.B + nw - 1) / nw), dim3(64 * nw), mab_fwd_lds(NT), st, *c);
}
