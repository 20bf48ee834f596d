// mpg_set_encode_fwd: the equivariant stack ``phi`` of PCGAN's set encoder (ext_models/pcgan_model.py:4-42: PermEqui1_max,
// PermEqui2_max, PermEqui2_mean, each behind a Tanh or a Softplus) and the max over a jet's particles behind it (:89-91, :140-142)
// in one launch.  For jet b, h_0 = x[b] [N, K_0]; for layer l < L with m = the column-wise max (pools 1, 2) or mean (pool 3) of h_l
// over the jet's N rows:
//     pool 1   z = (h_l - m) Gamma_l^T + bias_l                    (the subtraction in fp32, in front of the operand split)
//     pool 2/3 z = h_l Gamma_l^T + bias_l - m Lambda_l^T
//     h_{l+1} = act(z),        pooled[b, c] = max_n h_L[n, c]
//
// Launch shape: grid ceil(B / J), 256 threads; a workgroup owns J = 128 / (32 NT) jets, NT = ceil(N / 32), as 128 rows of an fp32
// activation image H [128][SE_KP] in LDS (row 32 NT j + n = particle n of the workgroup's jet j; 130 KiB), which never leaves the CU.
// Particles are the ROWS and channels the COLUMNS of a 32x32x16 MFMA result (common.h), and WAVE w OWNS ROW TILE w for the whole
// launch: it is the only reader and the only writer of rows 32 w .. 32 w + 31 during a layer's product, so a layer's output goes
// over its input in place -- the tile's A fragments of ALL k (split into fp16 hi / lo, 16 k-steps x 8 registers) are in registers
// before the first column is produced.  A layer is
//   1. pool:     thread (jet j, column k) walks rows n = 0 .. N-1 of the jet in ascending order -- max by a strict ">", or the sum
//                ((h_0 + h_1) + h_2) + ... divided by N -- and leaves m[j][k] in LDS.  Rows >= N are never visited.
//   2. barrier;  operands: a wave reads its 32 rows from H, subtracts m (pool 1), puts ZERO in rows >= N, in the tiles of jets
//                >= B and in k >= K (a select, not a product: what H holds there is never used), splits.
//   3. product:  the weights pass through LDS in slabs of 32 columns x 128 k, already split and laid out as B fragments
//                ([k-step][hi | lo][lane] x 16 bytes; zero beyond K and beyond D), one slab at a time in the order (column tile,
//                Gamma | Lambda, k half): the 256 threads fetch the NEXT slab into registers (two groups of 8 k each, coalesced
//                along a weight row) while every wave multiplies the current one -- three MFMAs per k-step (mfma3) -- and store
//                it behind a barrier.  A slab feeds all four row tiles.  Pools 2 / 3 multiply m -- the same row in all 32 rows
//                of an A fragment -- with Lambda's slabs: the result holds (m Lambda^T)[c] in every register of lane c.
//   4. epilogue: behind a column tile's last slab z = acc + bias - (m Lambda^T) in fp32, the activation, h_{l+1} to the tile's own
//                rows of H, columns < D.  The last slab's barrier ends the layer.
// Behind the last layer step 1 runs once more as a max and writes pooled instead of m.
// Every reduction has one fixed order and nothing is atomic: a jet's bits depend neither on B, nor on its slot in a workgroup, nor
// on the grid, nor on the run.  Global reads: x[b, n < N, k < K_0], Gamma / Lambda[c < D, k < K], bias[c < D]; nothing else.
// LDS: H 133120 + m 4096 + slab 16384 = 153600 bytes of the CU's 163840.
#include "common.h"
#include "mpgan_amd.h"

namespace {

constexpr int SE_THREADS = 256;
constexpr int SE_ROWS = 128;                           // rows of a workgroup: four row tiles, one per wave
constexpr int SE_KP = MPG_SET_ENC_MAX_D + 4;           // row stride of H in floats (+4: a wave's 16-byte reads spread over all banks)
constexpr int SE_KS = MPG_SET_ENC_MAX_D / 16;          // k-steps at the widest layer
constexpr int SE_MAX_L = MPG_SET_ENC_MAX_LAYERS;
constexpr int SE_SLAB_K = 128;                         // k of a weight slab in LDS: 32 columns x 128 k as B fragments, hi and lo
constexpr int SE_SLAB_STEPS = SE_SLAB_K / 16;
constexpr int SE_LDS_BYTES = (SE_ROWS * SE_KP + 4 * MPG_SET_ENC_MAX_D) * 4 + SE_SLAB_STEPS * 2 * 64 * 16;

struct SEArgs {
    const float* x; float* pooled;
    const float* Gamma[SE_MAX_L]; const float* bias[SE_MAX_L]; const float* Lambda[SE_MAX_L];
    int D[SE_MAX_L];
    int wvec[SE_MAX_L];   // rows of the layer's weights may be read as aligned float4 pairs
    int ldx, ld_pooled;
    int B, N, K0, L, pool, act;
    int NT, J;          // row tiles per jet, jets per workgroup
};

// 8 consecutive k of one weight row, zero beyond K (and for a row that does not exist: row == nullptr)
MPG_DEV void se_load8(const float* row, int k0, int K, bool vec, float* v) {
    if (row == nullptr || k0 >= K) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0.f;
    } else if (vec && k0 + 8 <= K) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(row + k0);
        const f32x4 b = *reinterpret_cast<const f32x4*>(row + k0 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (k0 + j < K) ? row[k0 + j] : 0.f;
    }
}

// act 2: tanh as 1 - 2 / (e^{2z} + 1) (absolute error of a few 2^-24; e^{2z} = inf gives 1, 0 gives -1);
// act 3: torch's Softplus (beta 1, threshold 20)
MPG_DEV float se_act(float z, int act) {
    if (act == 2) return 1.f - __fdividef(2.f, __expf(2.f * z) + 1.f);
    return z > 20.f ? z : log1pf(__expf(z));
}

// step 1 of a layer (and the launch's last step): m[j][k] = max_n or mean_n of H[32 NT j + n][k], n ascending, for the live jets
MPG_DEV void se_pool(const SEArgs& p, const float* H, int K, bool mean, float* out, int ld_out, int live) {
    for (int it = threadIdx.x; it < live * K; it += SE_THREADS) {
        const int j = it / K, k = it - j * K;
        const float* col = H + (size_t)(32 * p.NT * j) * SE_KP + k;
        float m = col[0];
        if (mean) {
#pragma unroll 8
            for (int n = 1; n < p.N; ++n) m += col[n * SE_KP];
            m /= (float)p.N;
        } else {
#pragma unroll 8
            for (int n = 1; n < p.N; ++n) {
                const float v = col[n * SE_KP];
                if (v > m) m = v;
            }
        }
        out[(size_t)j * ld_out + k] = m;
    }
}

__global__ __launch_bounds__(SE_THREADS) void set_encode_kernel(const SEArgs p) {
    extern __shared__ __attribute__((aligned(16))) float se_lds[];
    float* H = se_lds;                          // [SE_ROWS][SE_KP]
    float* ms = se_lds + SE_ROWS * SE_KP;       // [4][MPG_SET_ENC_MAX_D]
    f16x8* ws = reinterpret_cast<f16x8*>(ms + 4 * MPG_SET_ENC_MAX_D);   // [SE_SLAB_STEPS][hi | lo][lane]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b0 = blockIdx.x * p.J;
    const int live = min(p.J, p.B - b0);        // jets of this workgroup
    // this wave's row tile: tile `ti` of the workgroup's jet `jl`
    const int jl = wave / p.NT, ti = wave - jl * p.NT;
    const bool wave_on = jl < live;             // (wave-uniform)
    const int n_lane = 32 * ti + r;             // the particle of this lane's A-fragment row
    const bool row_on = wave_on && n_lane < p.N;

    // h_0: x[b, n, k < K_0] of the live jets
    for (int it = tid; it < live * p.N * p.K0; it += SE_THREADS) {
        const int row = it / p.K0, k = it - row * p.K0;
        const int j = row / p.N, n = row - j * p.N;
        H[(32 * p.NT * j + n) * SE_KP + k] = p.x[((size_t)(b0 + j) * p.N + n) * p.ldx + k];
    }
    __syncthreads();

    int K = p.K0;
    for (int l = 0; l < p.L; ++l) {
        const int D = p.D[l];
        se_pool(p, H, K, p.pool == 3, ms, MPG_SET_ENC_MAX_D, live);
        __syncthreads();
        f16x8 ahi[SE_KS], alo[SE_KS];
        if (wave_on) {
            const int KS = (K + 15) >> 4;
            const float* mrow = ms + jl * MPG_SET_ENC_MAX_D;
            const float* hrow = H + (32 * wave + r) * SE_KP;
            static_for<0, SE_KS>([&](auto ss) {
                MPG_CI(s, ss);
                if (s < KS) {   // (uniform)
                    const int k0 = 16 * s + 8 * h;
                    const f32x4 a = *reinterpret_cast<const f32x4*>(hrow + k0);
                    const f32x4 c = *reinterpret_cast<const f32x4*>(hrow + k0 + 4);
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = c[j]; }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const bool on = row_on && k0 + j < K;
                        const float m = (p.pool == 1 && on) ? mrow[k0 + j] : 0.f;
                        v[j] = on ? v[j] - m : 0.f;
                    }
                    split8(v, ahi[s], alo[s]);
                }
            });
        }
        // the layer's weights, slab by slab: (column tile ct, Gamma | Lambda, half kh of the k range) in that order
        const bool wvec = p.wvec[l] != 0;
        const int CT = (D + 31) >> 5, KH = (K + SE_SLAB_K - 1) / SE_SLAB_K;
        const int per_ct = KH * (p.pool == 1 ? 1 : 2);
        const int nslab = CT * per_ct;
        float pf[2][8];       // this thread's two groups of 8 k of the NEXT slab, in flight while the current one is multiplied
        auto prefetch = [&](int idx) {
            const int ct = idx / per_ct, rem = idx - ct * per_ct;
            const int which = rem / KH, kh = rem - which * KH;
            const float* W = which ? p.Lambda[l] : p.Gamma[l];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int item = tid + SE_THREADS * i, c = 32 * ct + (item >> 4);
                se_load8(c < D ? W + (size_t)c * K : nullptr, SE_SLAB_K * kh + 8 * (item & 15), K, wvec, pf[i]);
            }
        };
        prefetch(0);
        f32x16 acc, accm;
        for (int idx = 0; idx < nslab; ++idx) {
            // stage: group g8 of column rr is lane (g8 & 1, rr) of the B fragment of k-step g8 >> 1
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int item = tid + SE_THREADS * i, rr = item >> 4, g8 = item & 15;
                f16x8 hi, lo;
                split8(pf[i], hi, lo);
                const int at = (g8 >> 1) * 128 + (g8 & 1) * 32 + rr;
                ws[at] = hi;
                ws[at + 64] = lo;
            }
            __syncthreads();
            if (idx + 1 < nslab) prefetch(idx + 1);
            const int ct = idx / per_ct, rem = idx - ct * per_ct;
            const int which = rem / KH, kh = rem - which * KH;
            if (wave_on) {
                if (rem == 0) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) { acc[q] = 0.f; accm[q] = 0.f; }
                }
                if (which == 0) {
                    static_for<0, SE_KS>([&](auto ss) {
                        MPG_CI(s, ss);
                        constexpr int sl = s % SE_SLAB_STEPS;
                        if (s / SE_SLAB_STEPS == kh && 16 * s < K)   // (uniform)
                            acc = mfma3(ahi[s], alo[s], ws[sl * 128 + lane], ws[sl * 128 + 64 + lane], acc);
                    });
                } else {
                    const float* mrow = ms + jl * MPG_SET_ENC_MAX_D;
#pragma unroll
                    for (int sl = 0; sl < SE_SLAB_STEPS; ++sl) {
                        const int k0 = SE_SLAB_K * kh + 16 * sl + 8 * h;
                        if (SE_SLAB_K * kh + 16 * sl < K) {   // (uniform)
                            float mv[8];
#pragma unroll
                            for (int j = 0; j < 8; ++j) mv[j] = (k0 + j < K) ? mrow[k0 + j] : 0.f;
                            f16x8 mhi, mlo;
                            split8(mv, mhi, mlo);
                            accm = mfma3(mhi, mlo, ws[sl * 128 + lane], ws[sl * 128 + 64 + lane], accm);
                        }
                    }
                }
                const int c = 32 * ct + r;
                if (rem == per_ct - 1 && c < D) {
                    const float bias = p.bias[l] != nullptr ? p.bias[l][c] : 0.f;
                    float* hout = H + (32 * wave + 4 * h) * SE_KP + c;
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const float z = acc[q] + bias - accm[q];
                        hout[(8 * (q >> 2) + (q & 3)) * SE_KP] = se_act(z, p.act);
                    }
                }
            }
            __syncthreads();   // the slab is free again; behind the last one: H holds the layer's output
        }
        K = D;
    }
    se_pool(p, H, K, false, p.pooled + (size_t)b0 * p.ld_pooled, p.ld_pooled, live);
}

bool se_aligned16(const void* q) { return ((uintptr_t)q & 15u) == 0; }

}  // namespace

extern "C" int mpg_set_encode_fwd(const MpgSetEncode* p, void* stream) {
    if (p == nullptr) return -2;
    if (p->B < 1 || p->N < 1 || p->N > MPG_SET_ENC_MAX_N || p->L < 1 || p->L > MPG_SET_ENC_MAX_LAYERS) return -1;
    if (p->K[0] < 1 || p->K[0] > MPG_SET_ENC_MAX_D) return -1;
    for (int l = 0; l < p->L; ++l) {
        if (p->D[l] < 1 || p->D[l] > MPG_SET_ENC_MAX_D) return -1;
        if (l + 1 < p->L && p->K[l + 1] != p->D[l]) return -1;
    }
    if (p->pool < 1 || p->pool > 3 || (p->act != 2 && p->act != 3)) return -3;
    if (p->x == nullptr || p->pooled == nullptr) return -2;
    for (int l = 0; l < p->L; ++l)
        if (p->Gamma[l] == nullptr || (p->pool != 1 && p->Lambda[l] == nullptr)) return -2;
    if (p->ldx < p->K[0] || p->ld_pooled < p->D[p->L - 1]) return -5;
    SEArgs a;
    a.x = p->x; a.pooled = p->pooled;
    for (int l = 0; l < SE_MAX_L; ++l) {
        const bool on = l < p->L;
        a.Gamma[l] = on ? p->Gamma[l] : nullptr;
        a.bias[l] = on ? p->bias[l] : nullptr;
        a.Lambda[l] = (on && p->pool != 1) ? p->Lambda[l] : nullptr;
        a.D[l] = on ? p->D[l] : 0;
        a.wvec[l] = on && p->K[l] % 4 == 0 && se_aligned16(a.Gamma[l]) && se_aligned16(a.Lambda[l]);
    }
    a.ldx = p->ldx; a.ld_pooled = p->ld_pooled;
    a.B = p->B; a.N = p->N; a.K0 = p->K[0]; a.L = p->L; a.pool = p->pool; a.act = p->act;
    a.NT = (p->N + 31) / 32;
    a.J = 4 / a.NT;
    const long long blocks = ((long long)p->B + a.J - 1) / a.J;
    if (blocks > 0x7fffffffLL) return -1;
    return mpg_go<set_encode_kernel>(dim3((unsigned)blocks), dim3(SE_THREADS), SE_LDS_BYTES, (hipStream_t)stream, a);
}
