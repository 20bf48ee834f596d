// One launch per multihead attention block of GAPT (MAB.forward, gapt/model.py:124-139), for sets of up to 32 tokens (and, further
// down, mab_fwdN_kernel / mab_bwdS_kernel for 33 ... 160):
//
//   q = x Wq' + bq ; k = y Wk' + bk ; v = y Wv' + bv            (nn.MultiheadAttention in-projection, packed [3E, E])
//   P_h = softmax(q_h k_h' / sqrt(d) + key mask) ; o_h = P_h v_h (per head, d = 16)
//   za = x + o Wo' + bo ; z = dropout(za)
//   u = z Wf' + bf ; out = dropout(z + dropout_ff(LeakyReLU(u)))  (MAB.ff = one Linear(E, E) [+ LeakyReLU])
//
// ONE WAVE PER JET; nothing but the weights is read twice and no intermediate leaves the registers.  Everything is a
// chain of 32x32x16 MFMAs in the chain layout of common.h: a tile is [32 features (registers) x 32 tokens (lanes)], and
// registers 8s..8s+7 of a tile ARE the B fragment of k-step s of the next product.  The attention itself stays in that
// layout because A and B fragments of this instruction have the same shape (lane = row or column, 8 k-values):
//   * S' = K Q'    : A = registers of the K tile, B = registers of the Q tile (one k-step = the 16 features of a head);
//                    the result has keys in registers and queries on lanes, so the softmax is a register reduction
//                    plus one exchange between the two lane halves
//   * O' = V' P'   : needs V with keys in registers and features on lanes -- that is the V projection with its two MFMA
//                    operands SWAPPED (activations as A, weights as B), so no transpose is ever made; P's registers are
//                    its B fragments.  The 16 valid rows of the two heads of a 32-feature tile are merged into one
//                    tile, which is again the B operand of the out-projection.
// Products run as fp16 hi/lo 3-term splits (common.h) with power-of-two operand scales; the backward kernel recomputes
// the same values and carries gradients as bf16 hi/lo.
//
// This header: what the units share -- fragment / row / projection helpers, a wave's context (MabWave, MAB_WAVE), the LDS layouts
// and the entry points' host helpers.  mab_fwd.hip: forward; mab_bwd.hip, mab_bwds.hip over mab_bwd_impl.h: backward.
#pragma once
#include "common.h"
#include "../../include/mpgan_amd.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>

namespace {

// diagnostic build (-DMPG_MABSTAMP, tools/mab_stamps.py): s_memtime at the phase boundaries, the waves of workgroup 0.  A __device__
// array is not shared across units, so each direction's unit has its own, and its own mpg_debug_mab_{fwd,bwd}_stamps to read it.
#ifdef MPG_MABSTAMP
__device__ unsigned long long g_mab_stamps[8 * 8];   // [wave][stamp]: up to eight waves (mab_fwd2_kernel<.., 8>)
#define MAB_STAMP(i) do { mab_st[i] = __builtin_amdgcn_s_memtime(); } while (0)
#define MAB_STAMPP(i) do { if (mab_st != nullptr) mab_st[i] = __builtin_amdgcn_s_memtime(); } while (0)
#define MAB_STAMPS_DECL unsigned long long mab_stv[8] = {}; unsigned long long* const mab_st = mab_stv   // a wave's stamps
#define MAB_STAMPS_OF(wv) unsigned long long* const mab_st = (wv).st                                      // ... inside a device function
#define MAB_STAMPS_STORE do { if (blockIdx.x == 0 && lane == 0) for (int i = 0; i < 8; ++i) g_mab_stamps[w * 8 + i] = mab_st[i]; } while (0)
#define MAB_STAMPS_ENTRY(dir) extern "C" int mpg_debug_mab_##dir##_stamps(unsigned long long* host_out) { \
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_mab_stamps), sizeof(g_mab_stamps)); }
#else
#define MAB_STAMP(i) do {} while (0)
#define MAB_STAMPP(i) do {} while (0)
#define MAB_STAMPS_DECL unsigned long long* const mab_st = nullptr
#define MAB_STAMPS_OF(wv) do {} while (0)
#define MAB_STAMPS_STORE do {} while (0)
#define MAB_STAMPS_ENTRY(dir)
#endif

constexpr float MAB_SP = 256.f;   // attention probabilities are split as 256 P (an fp16 lo half stays normal down to P ~ 1e-3)

MPG_DEV float4 mld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// Weight images live in LDS for the lifetime of a workgroup (a fragment fetched from L2 is ~1 us away and every product
// of the chain waits for its own): one cooperative copy, then ds_read_b128 per fragment.
typedef const char* WImg;
template <typename V>
MPG_DEV V mab_wfrag(WImg w, int frag, int lane16) {
    return *reinterpret_cast<const V*>(w + frag * 1024 + lane16);
}
// (LDS-DMA: 1 KiB per wave-instruction straight into LDS, no register staging, all of a wave's pieces in flight at once.
// Every workgroup of a launch wants the same image at the same moment; each starts at a piece of its own so that they do not
// all walk it from the same end -- measured to make no difference: the fill is not bound by L2 channels)
MPG_DEV void mab_fill(char* dst, const void* src, int bytes) {
    const int wave = threadIdx.x >> 6, nwav = blockDim.x >> 6, lane = threadIdx.x & 63;
    const int n = bytes / 1024;
    const int rot = ((int)(blockIdx.x >> 3) * 5) % n;      // (workgroups 8 apart share an XCD and its L2)
    for (int c = wave; c < n; c += nwav) {
        int cc = c + rot;
        cc = cc >= n ? cc - n : cc;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(static_cast<const char*>(src) + cc * 1024 + lane * 16),
                                         (__attribute__((address_space(3))) void*)(dst + cc * 1024), 16, 0, 0);
    }
}

// rows of a [*, E] matrix as B (or A) fragments: k-step ks, element j of lane half h = feature 16 ks + 8 (j >> 2) + 4 h + (j & 3)
template <int KS, typename V>
MPG_DEV void rows_to_frags(const float* base, int ld, long row, float scale, int h, V* hi, V* lo) {
    static_for<0, KS>([&](auto kc) {
        MPG_CI(ks, kc);
        const float4 a = mld4(base + row * ld + 16 * ks + 4 * h), b = mld4(base + row * ld + 16 * ks + 8 + 4 * h);
        const float v[8] = {a.x * scale, a.y * scale, a.z * scale, a.w * scale, b.x * scale, b.y * scale, b.z * scale, b.w * scale};
        split8(v, hi[ks], lo[ks]);
    });
}
// rows of a [*, E] matrix as an accumulator-layout tile: register 4g+e = feature 32 tile + 8g + 4h + e of the lane's row
MPG_DEV f32x16 rows_to_tile(const float* base, int ld, long row, int tile, int h) {
    f32x16 t;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 a = mld4(base + row * ld + 32 * tile + 8 * g + 4 * h);
        t[4 * g] = a.x; t[4 * g + 1] = a.y; t[4 * g + 2] = a.z; t[4 * g + 3] = a.w;
    }
    return t;
}
// ---- Row loads the compiler does not count.  While an LDS-DMA fill is in flight hipcc answers the first use of ANY loaded
// register with s_waitcnt vmcnt(0): a jet's rows, requested ahead of the fill, could only be touched once the whole image had
// landed, and their hi/lo conversion (~1,500 clk of VALU) ran behind the fill instead of under it.  Loaded by inline assembly
// the rows are invisible to that pass; rows_wait<N> is the counted wait -- N = the vector-memory instructions this wave has
// issued SINCE the rows (loads return in issue order) -- and ties the registers to itself so nothing reads them earlier.
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <int OFF>
MPG_DEV f32x4 ld4_hidden(const float* p) {
    f32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=&v"(v) : "v"(p), "n"(OFF) : "memory");
    return v;
}
// the rows of NT tiles: piece 4t + g = features 32t + 8g + 4h .. +3 of the lane's row
template <int NT>
MPG_DEV void rows_request(const float* base, int ld, long row, int h, f32x4* q) {
    const float* const p = base + row * ld + 4 * h;
    static_for<0, 4 * NT>([&](auto ic) {
        MPG_CI(i, ic);
        q[i] = ld4_hidden<(32 * (i / 4) + 8 * (i % 4)) * 4>(p);
    });
}
template <int N>
MPG_DEV void rows_wait(f32x4* q) {     // eight pieces
    asm volatile("s_waitcnt vmcnt(%8)" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4]), "+v"(q[5]), "+v"(q[6]), "+v"(q[7]) : "n"(N) : "memory");
}
// ... and eight more pieces that were requested BEFORE a set already waited for (in-order return: they are here too); the empty
// statement only ties the registers to this point
MPG_DEV void rows_pin(f32x4* q) {
    asm volatile("" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4]), "+v"(q[5]), "+v"(q[6]), "+v"(q[7]) : : "memory");
}
MPG_DEV void rows_pin4(f32x4* q) {
    asm volatile("" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]) : : "memory");
}
MPG_DEV f32x16 pieces_tile(const f32x4* q, int t) {
    f32x16 o;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) o[4 * g + e] = q[4 * t + g][e];
    return o;
}
MPG_DEV void tile_to_rows(float* base, int ld, long row, int tile, int h, const f32x16& t, float scale) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(base + row * ld + 32 * tile + 8 * g + 4 * h) =
            make_float4(t[4 * g] * scale, t[4 * g + 1] * scale, t[4 * g + 2] * scale, t[4 * g + 3] * scale);
}
// registers 8s..8s+7 of a tile, scaled, as one hi/lo fragment pair
template <typename V>
MPG_DEV void tile_frag(const f32x16& t, int s, float scale, V& hi, V& lo) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = t[8 * s + j] * scale;
    split8(v, hi, lo);
}
// all 2 NT fragments of NT row tiles (register 8s+j of tile t = element j of k-step 2t+s: the two layouts hold the same values)
template <int NT, typename V>
MPG_DEV void tiles_to_frags(const f32x16* t, float scale, V* hi, V* lo) {
    static_for<0, NT>([&](auto tc) {
        MPG_CI(tt, tc);
        tile_frag(t[tt], 0, scale, hi[2 * tt], lo[2 * tt]);
        tile_frag(t[tt], 1, scale, hi[2 * tt + 1], lo[2 * tt + 1]);
    });
}
// bias of the features a lane's accumulator registers hold (features in registers); the staged copies are pre-scaled
MPG_DEV f32x16 bias_regs(const float* bias, int tile, int h) {
    f32x16 t;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 a = mld4(bias + 32 * tile + 8 * g + 4 * h);
        t[4 * g] = a.x; t[4 * g + 1] = a.y; t[4 * g + 2] = a.z; t[4 * g + 3] = a.w;
    }
    return t;
}
// ... and with the features on the lanes (swapped-operand products)
MPG_DEV f32x16 bias_lanes(const float* bias, int tile, int r) {
    const float b = bias[32 * tile + r];
    f32x16 t;
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = b;
    return t;
}
// acc += W_tile x  (features of W's row tile `m` in registers, tokens on lanes): W image as A, activation fragments as B
template <int KS, typename V>
MPG_DEV f32x16 proj_n(WImg rw, int nfrag, int m, const V* xh, const V* xl, f32x16 acc, int lane16) {
    static_for<0, KS>([&](auto kc) {
        MPG_CI(ks, kc);
        const V wh = mab_wfrag<V>(rw, m * KS + ks, lane16), wl = mab_wfrag<V>(rw, nfrag + m * KS + ks, lane16);
        acc = mfma3(wh, wl, xh[ks], xl[ks], acc);
    });
    return acc;
}
// the same product with the operands swapped: tokens in registers, W's row tile on the lanes
template <int KS, typename V>
MPG_DEV f32x16 proj_t(WImg rw, int nfrag, int m, const V* xh, const V* xl, f32x16 acc, int lane16) {
    static_for<0, KS>([&](auto kc) {
        MPG_CI(ks, kc);
        const V wh = mab_wfrag<V>(rw, m * KS + ks, lane16), wl = mab_wfrag<V>(rw, nfrag + m * KS + ks, lane16);
        acc = mfma3(xh[ks], xl[ks], wh, wl, acc);
    });
    return acc;
}
MPG_DEV f32x16 zero16() {
    f32x16 t;
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = 0.f;
    return t;
}
MPG_DEV float other_half(float v) { return __shfl_xor(v, 32); }

// dropout keep mask times scale on an accumulator-layout tile (the hash of common.h: drop_keep_f(row, feature))
MPG_DEV void drop_tile(f32x16& t, uint32_t seed_lo, uint32_t seed_hi, uint32_t tag, uint32_t row, int tile, int h, uint32_t thr, float scale) {
    if (thr == 0u) return;
    if (thr == 128u) {
        const uint32_t w = drop_word(seed_lo, seed_hi, tag, row, DROP_BIT_GRP + (uint32_t)tile) >> (4 * h);
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) t[4 * g + e] = ((w >> (8 * g + e)) & 1u) ? t[4 * g + e] * scale : 0.f;
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const uint32_t w = drop_word(seed_lo, seed_hi, tag, row, (uint32_t)(8 * tile + 2 * g + h));
#pragma unroll
            for (int e = 0; e < 4; ++e) t[4 * g + e] = drop_keep(w, e, thr) ? t[4 * g + e] * scale : 0.f;
        }
    }
}

// additive key mask for the registers of a score tile with KEYS in registers: register 4g+e = key 8g + 4h + e.  In two halves,
// so that the loads can be issued ahead of a weight fill and the selects run behind it, and WITHOUT a branch on the pointer:
// tested per element, each load sat in a block of its own behind an s_waitcnt vmcnt(0) -- sixteen round trips to memory in
// a row at the head of every kernel; tested once, the join still waited for all of them before the fill was issued.  With no
// mask the sixteen loads read `safe` (any 32 readable floats: the caller passes its x rows) and the values are not looked at.
struct KeyIgn { float v[16]; bool on; };
MPG_DEV KeyIgn key_mask_load(const float* ignore, const float* safe, long jet, int S, int h) {
    KeyIgn k;
    k.on = ignore != nullptr;
    const float* const row = k.on ? ignore + jet * S : safe;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) k.v[4 * g + e] = row[min(8 * g + 4 * h + e, S - 1)];
    return k;
}
MPG_DEV f32x16 key_mask_from(const KeyIgn& k, int S, int h) {
    f32x16 t;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) t[4 * g + e] = (8 * g + 4 * h + e >= S || (k.on && k.v[4 * g + e] != 0.f)) ? -INFINITY : 0.f;
    return t;
}
MPG_DEV f32x16 key_mask_regs(const float* ignore, const float* safe, long jet, int S, int h) {
    return key_mask_from(key_mask_load(ignore, safe, jet, S, h), S, h);
}

// ---- A wave's context.  MabWave is what the device functions take of it, one argument in place of eight scalars.  MAB_WAVE is the
// kernels' prologue, ONE copy: it declares lane, w, r (the row of a tile this lane holds), h (its lane half), lane16, the seed
// words and the scales (activations carry sa, accumulators zs = sa * wscale) as locals and packs `wv`.  STAMP0: what stands
// between the geometry and the seed read (the diagnostic build's first stamp, a pair's split, or nothing); ST: the stamps or
// nullptr.  A macro, because built by a function the same instructions reach the scheduler in another order and every
// kernel's code comes out different (profiles/mab_units.txt).
// (no branch on the pointer: behind one, the wave waits for the seed before it issues its first load)
struct MabWave {
    uint32_t seed_lo, seed_hi;
    float sa, inv_zs;
    int r, h, lane16;
    unsigned long long* st;
};
#define MAB_WAVE(p, STAMP0, ST) \
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6; \
    const int r = lane & 31, h = lane >> 5, lane16 = lane * 16; \
    STAMP0; \
    const uint64_t sd = *((p).seed != nullptr ? (p).seed : reinterpret_cast<const uint64_t*>((p).x)); \
    const uint32_t seed_lo = (p).seed != nullptr ? (uint32_t)sd : 0u, seed_hi = (p).seed != nullptr ? (uint32_t)(sd >> 32) : 0u; \
    const float sa = (p).ascale > 0.f ? (p).ascale : 1.f, ws = (p).wscale > 0.f ? (p).wscale : 1.f; \
    const float zs = sa * ws, inv_zs = 1.f / zs; \
    const MabWave wv{seed_lo, seed_hi, sa, inv_zs, r, h, lane16, ST}

// ---- LayerNorm over the E = 32 NT features of a token (gapt/model.py:118-120: nn.LayerNorm(embed_dim), biased variance).  A
// token's features sit in the NT tiles' registers of lanes r and r + 32, so the two sums are in-lane adds and one exchange
// with the other half.  ln_stats: mean and 1 / sqrt(var + eps) (two passes: the variance from the centred values);
// ln_apply: t -> (t - mean) rstd w + b in place.
template <int NT>
MPG_DEV void ln_stats(const f32x16 (&t)[NT], float eps, float& mean, float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
#pragma unroll
        for (int i = 0; i < 16; ++i) s += t[tt][i];
    s += other_half(s);
    mean = s * (1.f / (32 * NT));
    float q = 0.f;
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
#pragma unroll
        for (int i = 0; i < 16; ++i) { const float d = t[tt][i] - mean; q = fmaf(d, d, q); }
    q += other_half(q);
    rstd = 1.f / sqrtf(q * (1.f / (32 * NT)) + eps);
}
template <int NT>
MPG_DEV void ln_apply(f32x16 (&t)[NT], const float* w, const float* b, float eps, int h) {
    float mean, rstd;
    ln_stats<NT>(t, eps, mean, rstd);
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
        const f32x16 wv = bias_regs(w, tt, h), bv = bias_regs(b, tt, h);
#pragma unroll
        for (int i = 0; i < 16; ++i) t[tt][i] = fmaf((t[tt][i] - mean) * rstd, wv[i], bv[i]);
    }
}

// the additive key mask of key tile kt of a large set (keys in registers, as key_mask_regs)
MPG_DEV f32x16 key_mask_tile(const float* ignore, const float* safe, long jet, int S, int h, int kt) {
    const bool on = ignore != nullptr;
    const float* const row = on ? ignore + jet * S : safe;
    f32x16 t;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int key = 32 * kt + 8 * g + 4 * h + e;
            const float v = row[on ? min(key, S - 1) : 0];
            t[4 * g + e] = (key >= S || (on && v != 0.f)) ? -INFINITY : 0.f;
        }
    return t;
}

// ---- LDS layouts, each defined ONCE: the kernels take their pointers from them (MAB_*_CARVE, under the names sIn, sO, ...) and
// the launches their byte counts.  A weight image is its hi fragments then its lo fragments, 1 KiB each; the biases are staged as
// floats, pre-scaled by zs (as the accumulators carry them).
constexpr int MAB_TOKMAX = 160;         // tokens of a set: 5 tiles of 32
constexpr int MAB_XCH = 4 * 2 * 1024;   // one exchange buffer of a pair of waves (E = 64): [k-step][hi | lo][lane] 16 B
#define MAB_SMEM extern __shared__ __attribute__((aligned(16))) char smem[]

// forward: Win | Wo | Wf | biases (in_proj [3E] | out_proj [E] | ff [E]) | tail.  The tail: two exchange buffers per pair of waves
// (two waves per jet), or the fragments of the key tiles that do not fit where Win's image was (large sets).
template <int NT>
struct MabFwdLds {
    static constexpr int KS = 2 * NT, NF_IN = 3 * NT * KS, NF_E = NT * KS;   // fragments of an image's hi (or lo) half
    static constexpr int WIN = 0, WO = WIN + 2048 * NF_IN, WF = WO + 2048 * NF_E, BIAS = WF + 2048 * NF_E;
    static constexpr int BO = 96 * NT, BF = 128 * NT, NBIAS = 160 * NT;      // (floats)
    static constexpr int TAIL = BIAS + 4 * NBIAS;
    static constexpr int KVT = 8 * NT * 1024;         // large sets: bytes of one key tile's K and V fragments ...
    static constexpr int WIN_TILES = 3 * NT / 2;      // ... and the key tiles that fit Win's image (12 NT^2 KiB / 8 NT KiB)
    static_assert(WIN_TILES * KVT <= 2048 * NF_IN, "the first key tiles' fragments lie where Win's image was");
    static constexpr int bytes(int pairs) { return TAIL + pairs * 2 * MAB_XCH; }
    static constexpr int BYTES_BIG = TAIL + (MAB_TOKMAX / 32 - WIN_TILES) * KVT;
};
static_assert(MAB_XCH == MabFwdLds<2>::KS * 2 * 1024, "an exchange buffer holds the hi and lo fragment of every k-step of E = 64");
static_assert(MabFwdLds<2>::BIAS == 80 * 1024, "rows_wait<80 / NW>: the fill of an E = 64 block is 80 LDS-DMA instructions of 1 KiB");
#define MAB_FWD_CARVE(NT) \
    using Lds = MabFwdLds<NT>; \
    MAB_SMEM; \
    char* const sIn = smem + Lds::WIN; \
    char* const sO = sIn + (Lds::WO - Lds::WIN); \
    char* const sF = sO + (Lds::WF - Lds::WO); \
    float* const sBin = reinterpret_cast<float*>(sF + (Lds::BIAS - Lds::WF)); \
    float* const sBo = sBin + Lds::BO; \
    float* const sBf = sBo + (Lds::BF - Lds::BO)
#define MAB_FWD_TAIL reinterpret_cast<char*>(sBf + (Lds::NBIAS - Lds::BF))   // (at its use, as the address arithmetic was written)
// the plain order of the fill and of the bias staging (a kernel whose order of issue is deliberate takes the offsets and
// MAB_FWD_BIAS_AT only)
#define MAB_FWD_FILL(p) \
    mab_fill(sIn, (p).Win, 2048 * Lds::NF_IN); mab_fill(sO, (p).Wo, 2048 * Lds::NF_E); mab_fill(sF, (p).Wf, 2048 * Lds::NF_E)
#define MAB_FWD_BIAS_AT(p, i) ((i) < Lds::BO ? (p).bin[i] : ((i) < Lds::BF ? (p).bo[(i) - Lds::BO] : (p).bf[(i) - Lds::BF]))
#define MAB_FWD_STAGE_BIASES(p) \
    for (int i = threadIdx.x; i < Lds::NBIAS; i += blockDim.x) sBin[i] = MAB_FWD_BIAS_AT(p, i) * zs

// backward, one or two waves per jet: Win | Wf | WinT | WoT | WfT | biases (in_proj [3E] | ff [E]).  (Two waves per jet: the exchange
// buffers are the images nobody needs any more, mab_bwd2_body.)
template <int NT>
struct MabBwdLds {
    static constexpr int KS = 2 * NT, NF_IN = 3 * NT * KS, NF_E = NT * KS, NF_INT = NT * 3 * KS;
    static constexpr int WIN = 0, WF = WIN + 2048 * NF_IN, WINT = WF + 2048 * NF_E, WOT = WINT + 2048 * NF_INT, WFT = WOT + 2048 * NF_E,
                         BIAS = WFT + 2048 * NF_E;
    static constexpr int BF = 96 * NT, NBIAS = 128 * NT;
    static constexpr int BYTES = BIAS + 4 * NBIAS;
};
static_assert(MabBwdLds<2>::BIAS == 144 * 1024, "rows_wait<36>: the fill of an E = 64 backward is 144 LDS-DMA instructions of 1 KiB, 36 on each of four waves");
#define MAB_BWD_CARVE(NT) \
    using Lds = MabBwdLds<NT>; \
    MAB_SMEM; \
    char* const sIn = smem + Lds::WIN; \
    char* const sF = sIn + (Lds::WF - Lds::WIN); \
    char* const sInT = sF + (Lds::WINT - Lds::WF); \
    char* const sOT = sInT + (Lds::WOT - Lds::WINT); \
    char* const sFT = sOT + (Lds::WFT - Lds::WOT)
#define MAB_BWD_CARVE_BIASES \
    float* const sBin = reinterpret_cast<float*>(sFT + (Lds::BIAS - Lds::WFT)); \
    float* const sBf = sBin + Lds::BF
#define MAB_BWD_FILL(p) \
    mab_fill(sIn, (p).Win, 2048 * Lds::NF_IN); mab_fill(sF, (p).Wf, 2048 * Lds::NF_E); mab_fill(sInT, (p).WinT, 2048 * Lds::NF_INT); \
    mab_fill(sOT, (p).WoT, 2048 * Lds::NF_E); mab_fill(sFT, (p).WfT, 2048 * Lds::NF_E)
#define MAB_BWD_BIAS_AT(p, i) ((i) < Lds::BF ? (p).bin[i] : (p).bf[(i) - Lds::BF])
#define MAB_BWD_STAGE_BIASES(p) \
    for (int i = threadIdx.x; i < Lds::NBIAS; i += blockDim.x) sBin[i] = MAB_BWD_BIAS_AT(p, i) * zs

// backward, large sets: Win | WoT | exchange | biases | statistics.  The exchange area holds Wf | WfT through the feed-forward
// half, then the key side or the query side of one feature tile for all five token tiles, then WinT's image (mab_bwdS_kernel);
// the statistics are three floats per (head, token).
template <int NT>
struct MabBigBwdLds {
    static constexpr int KS = 2 * NT, NF_IN = 3 * NT * KS, NF_E = NT * KS, NF_INT = NT * 3 * KS, NH = 2 * NT;
    static constexpr int XCH_BYTES = 80 * 1024;
    static constexpr int WIN = 0, WOT = WIN + 2048 * NF_IN, XCH = WOT + 2048 * NF_E, WF = XCH, WFT = WF + 2048 * NF_E,
                         BIAS = XCH + XCH_BYTES;
    static constexpr int BF = 96 * NT, NBIAS = 128 * NT;
    static constexpr int STATS = BIAS + 4 * NBIAS, BYTES = STATS + 4 * 3 * NH * MAB_TOKMAX;
    static_assert(2 * 2048 * NF_E <= XCH_BYTES && 2048 * NF_INT <= XCH_BYTES, "Wf, WfT and later WinT live in the exchange area");
    static_assert(MAB_TOKMAX / 32 * 16 * 1024 <= XCH_BYTES, "... and the query side (16 fragments) of every token tile");
};
#define MAB_BIG_BWD_CARVE(NT) \
    using Lds = MabBigBwdLds<NT>; \
    MAB_SMEM; \
    char* const sIn = smem + Lds::WIN; \
    char* const sOT = sIn + (Lds::WOT - Lds::WIN); \
    char* const sX = sOT + (Lds::XCH - Lds::WOT); \
    char* const sF = sX; \
    char* const sFT = sF + (Lds::WFT - Lds::WF); \
    float* const sBin = reinterpret_cast<float*>(sX + Lds::XCH_BYTES); \
    float* const sBf = sBin + Lds::BF; \
    float* const sCQ = sBin + Lds::NBIAS;            /* [head][token]: the maximum of a query's scores (+inf: the query attends to nothing) */ \
    float* const sID = sCQ + Lds::NH * MAB_TOKMAX;   /* [head][token]: 1 / sum_keys 2^(score - maximum) */ \
    float* const sDD = sID + Lds::NH * MAB_TOKMAX    /* [head][token]: sum_keys P dP */

int mab_check(const MpgMab* p) {
    if (p->B < 1 || p->L < 1 || p->S < 1 || p->L > MAB_TOKMAX || p->S > MAB_TOKMAX) return -1;   // (sets of up to 5 tiles of 32 tokens)
    if ((p->E != 32 && p->E != 64) || p->H * 16 != p->E) return -2;
    if (!(p->alpha >= 0.f && p->alpha <= 1.f)) return -4;
    if (p->ldx % 4 || p->ldy % 4 || p->ldo % 4) return -3;
    return 0;
}

// waves (= jets in flight) per workgroup: as many workgroups as CUs first, then up to four waves each
int mab_waves(int B) {
    static const int forced = getenv("MPG_MAB_WAVES") ? atoi(getenv("MPG_MAB_WAVES")) : 0;   // (experiments)
    if (forced >= 1 && forced <= 4) return forced;
    return B <= 256 ? 1 : (B <= 512 ? 2 : 4);
}

// E = 64: two waves per jet (mab_fwd_half, mab_bwd2_body) while the launch has fewer jets than the chip has SIMDs to give
// each two (256 CUs x 4 / 2 = 512): a shorter chain per wave on SIMDs that would idle.  Past that every SIMD has a jet of its
// own.  The FORWARD (under 256 registers) then doubles up to 1,024 jets: four jets = eight waves to a workgroup, two waves
// to a SIMD, one issuing its hi/lo splits and softmax while the other's MFMAs run; the backward (340-400 registers, one wave
// to a SIMD) keeps one wave per jet.  MPG_MAB_SPLIT=0 keeps one wave per jet everywhere, =2 splits at any size, =3 splits
// up to 512 jets only (the A/B of the doubled forward); read at every launch, so a test can hold the forms against each
// other in one process (they give the same bits).
int mab_split_mode() {
    const char* e = getenv("MPG_MAB_SPLIT");
    return e == nullptr ? 1 : atoi(e);
}
bool mab_split(int B) {
    const int mode = mab_split_mode();
    return mode == 2 || ((mode == 1 || mode == 3) && B <= 512);
}
// waves per workgroup of the split forward: 0 = not split
int mab_split_fwd_waves(int B) {
    const int mode = mab_split_mode();
    if (mode == 0) return 0;
    if (B <= 512) return 4;
    if (mode == 2 || (mode == 1 && B <= 1024)) return 8;
    return 0;
}

// ---- launches: every kernel is named once, in the tables at the end of its unit ----
// (common.h's mpg_go: the dynamic-LDS grant of ONE kernel, once per device, then its launch)
using MabGo = int (*)(dim3, dim3, int, hipStream_t, const MpgMab&);
using MabChainGo = int (*)(dim3, dim3, int, hipStream_t, const MpgMabChain&);
#define MAB_GO(...) mpg_go<__VA_ARGS__, MpgMab>
#define MAB_CROSS_LN(K, NT) {{MAB_GO(K<NT, false, false>), MAB_GO(K<NT, false, true>)}, {MAB_GO(K<NT, true, false>), MAB_GO(K<NT, true, true>)}}   // [cross][ln]

// small sets, a wave per jet: mab_waves() jets to a workgroup
int mab_launch(MabGo go, const MpgMab* p, int lds_bytes, hipStream_t st, bool one_jet_per_wave = false) {
    const int nw = mab_waves(p->B);
    const int grid = ((p->B + nw - 1) / nw < 1024 || one_jet_per_wave) ? (p->B + nw - 1) / nw : 1024;
    return go(dim3(grid), dim3(64 * nw), lds_bytes, st, *p);
}

// dynamic LDS bytes (NT = E / 32): the layouts' own
int mab_fwd_lds(int NT, int pairs = 0) { return NT == 1 ? MabFwdLds<1>::bytes(pairs) : MabFwdLds<2>::bytes(pairs); }
int mab_bwd_lds(int NT) { return NT == 1 ? MabBwdLds<1>::BYTES : MabBwdLds<2>::BYTES; }
int mab_big_lds(int NT, bool backward) {
    if (!backward) return NT == 1 ? MabFwdLds<1>::BYTES_BIG : MabFwdLds<2>::BYTES_BIG;
    return NT == 1 ? MabBigBwdLds<1>::BYTES : MabBigBwdLds<2>::BYTES;
}

// a block with layer_norm=True (ln1_w set) brings all of its norms' arguments: 0, or -6
int mab_ln_check(const MpgMab* p, bool backward) {
    if (p->ln1_w == nullptr) return 0;
    if (p->ln2_w == nullptr || !(p->ln_eps > 0.f)) return -6;
    if (!backward) return (p->ln1_b == nullptr || p->ln2_b == nullptr) ? -6 : 0;
    const bool rows = p->dn1 != nullptr;     // the rows of the norms' parameter gradients: all four or none
    return (p->save_za == nullptr || rows != (p->gn1 != nullptr) || rows != (p->dn2 != nullptr) || rows != (p->gn2 != nullptr)) ? -6 : 0;
}

}  // namespace

// the large-set backward is a unit of its own (mab_bwds.hip)
int mab_bwd_big(const MpgMab* p, hipStream_t st);
