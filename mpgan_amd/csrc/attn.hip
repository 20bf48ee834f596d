// Multi-head attention core of GAPT's MAB: per (jet, head)  P = softmax(q k^T / sqrt(d) + mask),  o = P v.
//
// Replaces the scaled-dot-product part of nn.MultiheadAttention as MAB uses it (gapt/model.py:107,
// :129: batch_first, key-ignore mask expanded over heads :127, need_weights=False) and its
// backward.  The projections around it (in_proj, out_proj, ff) run on mpg_gemm.  Sets here are
// tiny (L, S <= 150 particles or 10 inducing points, d = 16): the work is latency/launch bound, fp32 VALU.
//
// Fast path (S <= 32 keys, L <= 64 queries, d in {8, 16, 32}: every GAPT block at N = 30): ONE WAVE per (jet, head),
// four per workgroup; lane = query.  K and V sit in LDS and are read as broadcasts, the 32 scores of a query
// live in registers (fully unrolled), P is written once, transposed ([S][L]: lanes contiguous).  The backward
// keeps dS and P in LDS between its query-major half (dQ) and its key-major half (dK, dV).
// Anything larger takes the generic kernels below (one workgroup per (jet, head), scores through memory).
// mpg_attn_dd (behind them) is the second derivative the gradient penalty needs, for either layout of P.
#include "common.h"
#include "../../include/mpgan_amd.h"

namespace {
constexpr int DMAX = 32;
constexpr int AT_S = 32, AT_L = 64;  // fast-path limits

template <int D>
MPG_DEV void lds_row(const float* base, int row, float (&out)[D]) {  // broadcast read of one [D] row
#pragma unroll
    for (int c = 0; c < D; c += 4) {
        const float4 t = *reinterpret_cast<const float4*>(base + row * D + c);
        out[c] = t.x; out[c + 1] = t.y; out[c + 2] = t.z; out[c + 3] = t.w;
    }
}

template <int D, bool TWO>
__global__ __launch_bounds__(256) void attn_fwd_fast(const MpgAttn p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    // TWO (L <= 32): each 32-lane half of a wave owns its own (jet, head) pair (8 pairs per workgroup), else the wave one
    const int w = threadIdx.x >> 6, lane64 = threadIdx.x & 63;
    constexpr bool two = TWO;
    const int half = two ? lane64 >> 5 : 0, lane = two ? lane64 & 31 : lane64, nl = two ? 32 : 64;
    int pair = two ? (blockIdx.x * 4 + w) * 2 + half : blockIdx.x * 4 + w;   // (jet, head)
    const bool live = pair < p.B * p.H;
    if (!live) pair = p.B * p.H - 1;               // idle half: recompute the last pair, store nothing
    const int b = pair / p.H, hd = pair % p.H;
    float* ks = sm + (two ? w * 2 + half : w) * (2 * AT_S * D);   // [S][D]
    float* vs = ks + AT_S * D;
    for (int t = lane; t < p.S * (D / 4); t += nl) {
        const int s = t / (D / 4), c = 4 * (t % (D / 4));
        *reinterpret_cast<float4*>(ks + s * D + c) = *reinterpret_cast<const float4*>(p.k + (size_t)(b * p.S + s) * p.ldk + hd * D + c);
        *reinterpret_cast<float4*>(vs + s * D + c) = *reinterpret_cast<const float4*>(p.v + (size_t)(b * p.S + s) * p.ldv + hd * D + c);
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int l = lane;
    if (l >= p.L || !live) return;
    const float scale = rsqrtf((float)D);
    float q[D];
    {
        const float* qp = p.q + (size_t)(b * p.L + l) * p.ldq + hd * D;
#pragma unroll
        for (int c = 0; c < D; c += 4) {
            const float4 t = *reinterpret_cast<const float4*>(qp + c);
            q[c] = t.x * scale; q[c + 1] = t.y * scale; q[c + 2] = t.z * scale; q[c + 3] = t.w * scale;
        }
    }
    float sc[AT_S];
    float mx = -INFINITY;
#pragma unroll
    for (int s = 0; s < AT_S; ++s) {
        float x = -INFINITY;
        if (s < p.S) {  // wave-uniform
            float kr[D];
            lds_row<D>(ks, s, kr);
            x = 0.f;
#pragma unroll
            for (int c = 0; c < D; ++c) x += q[c] * kr[c];
            if (p.ignore != nullptr && p.ignore[b * p.S + s] != 0.f) x = -INFINITY;
        }
        sc[s] = x;
        mx = fmaxf(mx, x);
    }
    const float msafe = mx == -INFINITY ? 0.f : mx;   // (a query whose keys are all ignored: every term below is 0)
    float den = 0.f;
#pragma unroll
    for (int s = 0; s < AT_S; ++s) { sc[s] = __expf(sc[s] - msafe); den += sc[s]; }
    const float inv = den > 0.f ? 1.f / den : 0.f;     // (... and gets zero attention weights)
    float o[D];
#pragma unroll
    for (int c = 0; c < D; ++c) o[c] = 0.f;
    float* Pt = p.P + (size_t)pair * p.S * p.L;    // [S][L]
#pragma unroll
    for (int s = 0; s < AT_S; ++s) {
        if (s < p.S) {
            const float pr = sc[s] * inv;
            Pt[s * p.L + l] = pr;
            float vr[D];
            lds_row<D>(vs, s, vr);
#pragma unroll
            for (int c = 0; c < D; ++c) o[c] += pr * vr[c];
        }
    }
    float* op = p.o + (size_t)(b * p.L + l) * p.ldo + hd * D;
#pragma unroll
    for (int c = 0; c < D; c += 4) *reinterpret_cast<float4*>(op + c) = make_float4(o[c], o[c + 1], o[c + 2], o[c + 3]);
}

// backward: dV = P^T dO ; dP = dO V^T ; dS = P * (dP - rowsum(dP * P)) ; dQ = dS K / sqrt(d) ; dK = dS^T Q / sqrt(d)
template <int D, bool TWO>
__global__ __launch_bounds__(256) void attn_bwd_fast(const MpgAttn p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int w = threadIdx.x >> 6, lane64 = threadIdx.x & 63;
    constexpr bool two = TWO;            // (L <= 32, S <= 32): a 32-lane half per (jet, head) pair
    const int half = two ? lane64 >> 5 : 0, lane = two ? lane64 & 31 : lane64, nl = two ? 32 : 64;
    int pair = two ? (blockIdx.x * 4 + w) * 2 + half : blockIdx.x * 4 + w;
    const bool live = pair < p.B * p.H;
    if (!live) pair = p.B * p.H - 1;     // idle half: recompute the last pair, store nothing
    const int b = pair / p.H, hd = pair % p.H;
    const int capl = two ? 32 : AT_L;    // query capacity of this pair's LDS slice
    // row stride of dS / P: odd, so that the key-major reads (one row per lane) spread over the banks -- except where
    // four wave-sized slices with d = 32 would no longer fit the LDS
    const int ldl = (!two && D == 32) ? capl : capl + 1;
    const int PER = 2 * AT_S * D + 2 * capl * D + 2 * AT_S * ldl;
    float* ks = sm + (two ? w * 2 + half : w) * PER;   // [S][D]
    float* vs = ks + AT_S * D;           // [S][D]
    float* qs = vs + AT_S * D;           // [L][D]
    float* gs = qs + capl * D;           // [L][D]  dO
    float* dsl = gs + capl * D;          // [S][ldl]  dS (written query-major: lanes contiguous)
    float* pl = dsl + AT_S * ldl;        // [S][ldl]  P
    for (int t = lane; t < p.S * (D / 4); t += nl) {
        const int s = t / (D / 4), c = 4 * (t % (D / 4));
        *reinterpret_cast<float4*>(ks + s * D + c) = *reinterpret_cast<const float4*>(p.k + (size_t)(b * p.S + s) * p.ldk + hd * D + c);
        *reinterpret_cast<float4*>(vs + s * D + c) = *reinterpret_cast<const float4*>(p.v + (size_t)(b * p.S + s) * p.ldv + hd * D + c);
    }
    for (int t = lane; t < p.L * (D / 4); t += nl) {
        const int l = t / (D / 4), c = 4 * (t % (D / 4));
        *reinterpret_cast<float4*>(qs + l * D + c) = *reinterpret_cast<const float4*>(p.q + (size_t)(b * p.L + l) * p.ldq + hd * D + c);
        *reinterpret_cast<float4*>(gs + l * D + c) = *reinterpret_cast<const float4*>(p.d_o + (size_t)(b * p.L + l) * p.ldo + hd * D + c);
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const float scale = rsqrtf((float)D);
    const float* Pt = p.P + (size_t)pair * p.S * p.L;  // [S][L]
    if (lane < p.L && live) {  // ---- query-major half
        const int l = lane;
        float g[D];
        lds_row<D>(gs, l, g);
        float dp[AT_S], pr[AT_S];
        float dot = 0.f;
#pragma unroll
        for (int s = 0; s < AT_S; ++s) {
            dp[s] = 0.f; pr[s] = 0.f;
            if (s < p.S) {
                pr[s] = Pt[s * p.L + l];
                float vr[D];
                lds_row<D>(vs, s, vr);
#pragma unroll
                for (int c = 0; c < D; ++c) dp[s] += g[c] * vr[c];
                dot += dp[s] * pr[s];
            }
        }
        float dq[D];
#pragma unroll
        for (int c = 0; c < D; ++c) dq[c] = 0.f;
#pragma unroll
        for (int s = 0; s < AT_S; ++s) {
            if (s < p.S) {
                const float x = pr[s] * (dp[s] - dot);
                dsl[s * ldl + l] = x;
                pl[s * ldl + l] = pr[s];
                float kr[D];
                lds_row<D>(ks, s, kr);
#pragma unroll
                for (int c = 0; c < D; ++c) dq[c] += x * kr[c];
            }
        }
        float* qo = p.dq + (size_t)(b * p.L + l) * p.lddq + hd * D;
#pragma unroll
        for (int c = 0; c < D; c += 4)
            *reinterpret_cast<float4*>(qo + c) = make_float4(dq[c] * scale, dq[c + 1] * scale, dq[c + 2] * scale, dq[c + 3] * scale);
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane < p.S && live) {  // ---- key-major half
        const int s = lane;
        float dk[D], dv[D];
#pragma unroll
        for (int c = 0; c < D; ++c) { dk[c] = 0.f; dv[c] = 0.f; }
        for (int l = 0; l < p.L; ++l) {
            const float x = dsl[s * ldl + l], pr = pl[s * ldl + l];
            float qr[D], gr[D];
            lds_row<D>(qs, l, qr);
            lds_row<D>(gs, l, gr);
#pragma unroll
            for (int c = 0; c < D; ++c) { dk[c] += x * qr[c]; dv[c] += pr * gr[c]; }
        }
        float* ko = p.dk + (size_t)(b * p.S + s) * p.lddk + hd * D;
        float* vo = p.dv + (size_t)(b * p.S + s) * p.lddv + hd * D;
#pragma unroll
        for (int c = 0; c < D; c += 4) {
            *reinterpret_cast<float4*>(ko + c) = make_float4(dk[c] * scale, dk[c + 1] * scale, dk[c + 2] * scale, dk[c + 3] * scale);
            *reinterpret_cast<float4*>(vo + c) = make_float4(dv[c], dv[c + 1], dv[c + 2], dv[c + 3]);
        }
    }
}

// ---- generic kernels: one workgroup per (jet, head), scores through memory (P is [L][S] here)
__global__ __launch_bounds__(64) void attn_fwd_kernel(const MpgAttn p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.x / p.H, hd = blockIdx.x % p.H;
    const int d = p.d;
    float* ks = sm;              // [S][d]
    float* vs = sm + p.S * d;    // [S][d]
    for (int t = threadIdx.x; t < p.S * d; t += blockDim.x) {
        const int s = t / d, c = t % d;
        ks[t] = p.k[(size_t)(b * p.S + s) * p.ldk + hd * d + c];
        vs[t] = p.v[(size_t)(b * p.S + s) * p.ldv + hd * d + c];
    }
    __syncthreads();
    const float scale = rsqrtf((float)d);
    for (int l = threadIdx.x; l < p.L; l += blockDim.x) {
        float q[DMAX];
        const float* qp = p.q + (size_t)(b * p.L + l) * p.ldq + hd * d;
        for (int c = 0; c < d; ++c) q[c] = qp[c] * scale;
        float* prow = p.P + ((size_t)(b * p.H + hd) * p.L + l) * p.S;
        float mx = -INFINITY;
        for (int s = 0; s < p.S; ++s) {
            float sc = 0.f;
            for (int c = 0; c < d; ++c) sc += q[c] * ks[s * d + c];
            if (p.ignore != nullptr && p.ignore[b * p.S + s] != 0.f) sc = -INFINITY;
            prow[s] = sc;
            mx = fmaxf(mx, sc);
        }
        const float msafe = mx == -INFINITY ? 0.f : mx;   // (all keys ignored: zero attention weights)
        float den = 0.f;
        for (int s = 0; s < p.S; ++s) {
            const float e = __expf(prow[s] - msafe);
            prow[s] = e;
            den += e;
        }
        const float inv = den > 0.f ? 1.f / den : 0.f;
        float o[DMAX];
        for (int c = 0; c < d; ++c) o[c] = 0.f;
        for (int s = 0; s < p.S; ++s) {
            const float pr = prow[s] * inv;
            prow[s] = pr;
            for (int c = 0; c < d; ++c) o[c] += pr * vs[s * d + c];
        }
        float* op = p.o + (size_t)(b * p.L + l) * p.ldo + hd * d;
        for (int c = 0; c < d; ++c) op[c] = o[c];
    }
}

// backward: dV = P^T dO ; dP = dO V^T ; dS = P * (dP - rowsum(dP * P)) ; dQ = dS K / sqrt(d) ; dK = dS^T Q / sqrt(d)
__global__ __launch_bounds__(64) void attn_bwd_kernel(const MpgAttn p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.x / p.H, hd = blockIdx.x % p.H;
    const int d = p.d;
    float* ks = sm;                    // [S][d]
    float* vs = ks + p.S * d;          // [S][d]
    float* qs = vs + p.S * d;          // [L][d]
    float* gs = qs + p.L * d;          // [L][d]  dO
    float* ds = gs + p.L * d;          // [L][S]  dS
    for (int t = threadIdx.x; t < p.S * d; t += blockDim.x) {
        const int s = t / d, c = t % d;
        ks[t] = p.k[(size_t)(b * p.S + s) * p.ldk + hd * d + c];
        vs[t] = p.v[(size_t)(b * p.S + s) * p.ldv + hd * d + c];
    }
    for (int t = threadIdx.x; t < p.L * d; t += blockDim.x) {
        const int l = t / d, c = t % d;
        qs[t] = p.q[(size_t)(b * p.L + l) * p.ldq + hd * d + c];
        gs[t] = p.d_o[(size_t)(b * p.L + l) * p.ldo + hd * d + c];
    }
    __syncthreads();
    const float scale = rsqrtf((float)d);
    const float* Pb = p.P + (size_t)(b * p.H + hd) * p.L * p.S;
    for (int l = threadIdx.x; l < p.L; l += blockDim.x) {
        float g[DMAX];
        for (int c = 0; c < d; ++c) g[c] = gs[l * d + c];
        float dot = 0.f;
        for (int s = 0; s < p.S; ++s) {
            float dp = 0.f;
            for (int c = 0; c < d; ++c) dp += g[c] * vs[s * d + c];
            const float pr = Pb[l * p.S + s];
            ds[l * p.S + s] = dp;
            dot += dp * pr;
        }
        float dq[DMAX];
        for (int c = 0; c < d; ++c) dq[c] = 0.f;
        for (int s = 0; s < p.S; ++s) {
            const float x = Pb[l * p.S + s] * (ds[l * p.S + s] - dot);
            ds[l * p.S + s] = x;
            for (int c = 0; c < d; ++c) dq[c] += x * ks[s * d + c];
        }
        float* qo = p.dq + (size_t)(b * p.L + l) * p.lddq + hd * d;
        for (int c = 0; c < d; ++c) qo[c] = dq[c] * scale;
    }
    __syncthreads();
    for (int s = threadIdx.x; s < p.S; s += blockDim.x) {
        float dk[DMAX], dv[DMAX];
        for (int c = 0; c < d; ++c) { dk[c] = 0.f; dv[c] = 0.f; }
        for (int l = 0; l < p.L; ++l) {
            const float x = ds[l * p.S + s], pr = Pb[l * p.S + s];
            for (int c = 0; c < d; ++c) { dk[c] += x * qs[l * d + c]; dv[c] += pr * gs[l * d + c]; }
        }
        float* ko = p.dk + (size_t)(b * p.S + s) * p.lddk + hd * d;
        float* vo = p.dv + (size_t)(b * p.S + s) * p.lddv + hd * d;
        for (int c = 0; c < d; ++c) { ko[c] = dk[c] * scale; vo[c] = dv[c]; }
    }
}
// ---- second order: the gradients of Phi = <uq, dq> + <uk, dk> + <uv, dv> with respect to q, k, v and dO (DESIGN.md section 4,
// "Gradient penalty on the attention core").  One workgroup per (jet, head), a thread per query and then a thread per key; all seven
// operands of the pair sit in LDS.  No L x S tile is kept anywhere: a thread forms the four dot products of an element
//     A = G_l . v_s      Sd = c (uq_l . k_s + q_l . uk_s)      W = G_l . uv_s
// where it needs them (twice query-major, once key-major) and reads P as the forward left it.  With a = sum_s P A, r = sum_s P Sd:
//     dS = P (A - a)    Pd = P (Sd - r)    M = Sd (A - a) - r A + W    D2 = P (M - m),   m = sum_s P M = sum_s P Sd A - 2 a r + sum_s P W
// so ONE query-major pass gives the three row scalars.  Every sum runs in index order inside one thread: no atomics, the same bits
// from every launch.  An ignored key is skipped (its P is an exact 0: it contributes exactly nothing, its own gk / gv rows are
// zeros); a jet without a real key gets zeros everywhere.
template <int D>
MPG_DEV float dot_row(const float (&x)[D], const float* row) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < D; c += 4) {
        const float4 t = *reinterpret_cast<const float4*>(row + c);
        acc += x[c] * t.x; acc += x[c + 1] * t.y; acc += x[c + 2] * t.z; acc += x[c + 3] * t.w;
    }
    return acc;
}
template <int D>
MPG_DEV void axpy_row(float (&y)[D], float a, const float* row) {
#pragma unroll
    for (int c = 0; c < D; c += 4) {
        const float4 t = *reinterpret_cast<const float4*>(row + c);
        y[c] += a * t.x; y[c + 1] += a * t.y; y[c + 2] += a * t.z; y[c + 3] += a * t.w;
    }
}

template <int D>
__global__ __launch_bounds__(256) void attn_dd_kernel(const MpgAttnDD p, const int p_sl) {   // p_sl: P is [S][L] (else [L][S])
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int pair = blockIdx.x, b = pair / p.H, hd = pair % p.H;
    const int L = p.L, S = p.S;
    const bool hq = p.uq != nullptr, hk = p.uk != nullptr, hv = p.uv != nullptr;
    float* qs = sm;               // [L][D]
    float* gs = qs + L * D;       // [L][D]  dO
    float* uqs = gs + L * D;      // [L][D]
    float* ks = uqs + L * D;      // [S][D]
    float* vs = ks + S * D;
    float* uks = vs + S * D;
    float* uvs = uks + S * D;
    float* ar = uvs + S * D;      // [L] each: a, r, m
    float* rr = ar + L;
    float* mr = rr + L;
    float* ig = mr + L;           // [S]
    for (int t = threadIdx.x; t < L * D; t += blockDim.x) {
        const size_t row = (size_t)(b * L + t / D);
        const int c = hd * D + t % D;
        qs[t] = p.q[row * p.ldq + c];
        gs[t] = p.d_o[row * p.ldo + c];
        if (hq) uqs[t] = p.uq[row * p.lduq + c];
    }
    for (int t = threadIdx.x; t < S * D; t += blockDim.x) {
        const size_t row = (size_t)(b * S + t / D);
        const int c = hd * D + t % D;
        ks[t] = p.k[row * p.ldk + c];
        vs[t] = p.v[row * p.ldv + c];
        if (hk) uks[t] = p.uk[row * p.lduk + c];
        if (hv) uvs[t] = p.uv[row * p.lduv + c];
    }
    for (int s = threadIdx.x; s < S; s += blockDim.x) ig[s] = (p.ignore != nullptr && p.ignore[b * S + s] != 0.f) ? 1.f : 0.f;
    __syncthreads();
    const float scale = rsqrtf((float)D);
    const float* Pb = p.P + (size_t)pair * L * S;
    const int pl = p_sl ? 1 : S, ps = p_sl ? L : 1;   // strides of P in l and in s
    const bool want_q = p.gq != nullptr, want_o = p.gdo != nullptr, want_k = p.gk != nullptr, want_v = p.gv != nullptr;

    for (int l = threadIdx.x; l < L; l += blockDim.x) {   // ---- query-major: the row scalars, then gq and gdo
        float q[D], g[D], uq[D];
#pragma unroll
        for (int c = 0; c < D; ++c) { q[c] = qs[l * D + c]; g[c] = gs[l * D + c]; uq[c] = hq ? uqs[l * D + c] : 0.f; }
        const float* Pl = Pb + (size_t)l * pl;
        float a = 0.f, r = 0.f, t = 0.f, w = 0.f;
        for (int s = 0; s < S; ++s) {
            if (ig[s] != 0.f) continue;   // (workgroup-uniform)
            const float pr = Pl[s * ps];
            const float A = dot_row<D>(g, vs + s * D);
            float sd = 0.f;
            if (hq) sd += dot_row<D>(uq, ks + s * D);
            if (hk) sd += dot_row<D>(q, uks + s * D);
            sd *= scale;
            a += pr * A; r += pr * sd; t += pr * sd * A;
            if (hv) w += pr * dot_row<D>(g, uvs + s * D);
        }
        const float m = t - 2.f * a * r + w;
        ar[l] = a; rr[l] = r; mr[l] = m;
        if (!want_q && !want_o) continue;
        float gq[D], go[D];
#pragma unroll
        for (int c = 0; c < D; ++c) { gq[c] = 0.f; go[c] = 0.f; }
        for (int s = 0; s < S; ++s) {
            if (ig[s] != 0.f) continue;
            const float pr = Pl[s * ps];
            const float A = dot_row<D>(g, vs + s * D);
            float sd = 0.f;
            if (hq) sd += dot_row<D>(uq, ks + s * D);
            if (hk) sd += dot_row<D>(q, uks + s * D);
            sd *= scale;
            if (want_q) {
                const float W = hv ? dot_row<D>(g, uvs + s * D) : 0.f;
                const float d2 = pr * (sd * (A - a) - r * A + W - m);
                axpy_row<D>(gq, d2, ks + s * D);
                if (hk) axpy_row<D>(gq, pr * (A - a), uks + s * D);
            }
            if (want_o) {
                axpy_row<D>(go, pr * (sd - r), vs + s * D);
                if (hv) axpy_row<D>(go, pr, uvs + s * D);
            }
        }
        const size_t row = (size_t)(b * L + l);
        if (want_q) {
            float* o = p.gq + row * p.ldgq + hd * D;
#pragma unroll
            for (int c = 0; c < D; ++c) o[c] = gq[c] * scale;
        }
        if (want_o) {
            float* o = p.gdo + row * p.ldgdo + hd * D;
#pragma unroll
            for (int c = 0; c < D; ++c) o[c] = go[c];
        }
    }
    if (!want_k && !want_v) return;
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += blockDim.x) {   // ---- key-major: gk and gv
        float gk[D], gv[D];
#pragma unroll
        for (int c = 0; c < D; ++c) { gk[c] = 0.f; gv[c] = 0.f; }
        if (ig[s] == 0.f) {
            float k[D], v[D], uk[D], uv[D];
#pragma unroll
            for (int c = 0; c < D; ++c) {
                k[c] = ks[s * D + c]; v[c] = vs[s * D + c];
                uk[c] = hk ? uks[s * D + c] : 0.f; uv[c] = hv ? uvs[s * D + c] : 0.f;
            }
            const float* Ps = Pb + (size_t)s * ps;
            for (int l = 0; l < L; ++l) {
                const float pr = Ps[l * pl];
                const float a = ar[l], r = rr[l], m = mr[l];
                const float A = dot_row<D>(v, gs + l * D);
                float sd = 0.f;
                if (hq) sd += dot_row<D>(k, uqs + l * D);
                if (hk) sd += dot_row<D>(uk, qs + l * D);
                sd *= scale;
                if (want_k) {
                    const float W = hv ? dot_row<D>(uv, gs + l * D) : 0.f;
                    const float d2 = pr * (sd * (A - a) - r * A + W - m);
                    axpy_row<D>(gk, d2, qs + l * D);
                    if (hq) axpy_row<D>(gk, pr * (A - a), uqs + l * D);
                }
                if (want_v) axpy_row<D>(gv, pr * (sd - r), gs + l * D);
            }
        }
        const size_t row = (size_t)(b * S + s);
        if (want_k) {
            float* o = p.gk + row * p.ldgk + hd * D;
#pragma unroll
            for (int c = 0; c < D; ++c) o[c] = gk[c] * scale;
        }
        if (want_v) {
            float* o = p.gv + row * p.ldgv + hd * D;
#pragma unroll
            for (int c = 0; c < D; ++c) o[c] = gv[c];
        }
    }
}

// The fast path is chosen by shape alone (forward, backward and the second-order kernel must agree on the layout of P: [S][L] where
// this says yes, [L][S] elsewhere); its float4 row accesses then REQUIRE 16-byte aligned bases and strides -- anything else is an
// error, not a silent fallback.
static bool attn_fast_shape(int L, int S, int d) {
    return S <= AT_S && L <= AT_L && (d == 8 || d == 16 || d == 32);
}
static bool attn_fast_shape(const MpgAttn* p) { return attn_fast_shape(p->L, p->S, p->d); }
static bool attn_aligned(const MpgAttn* p, bool bwd) {
    auto al = [](const void* q, int ld) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0 && ld % 4 == 0; };
    bool ok = al(p->q, p->ldq) && al(p->k, p->ldk) && al(p->v, p->ldv);
    if (!bwd) ok = ok && al(p->o, p->ldo);
    else ok = ok && al(p->d_o, p->ldo) && al(p->dq, p->lddq) && al(p->dk, p->lddk) && al(p->dv, p->lddv);
    return ok;
}
}  // namespace

extern "C" int mpg_attn_fwd(const MpgAttn* p, void* stream) {
    if (p->d > DMAX || p->B <= 0) return -1;
    if (attn_fast_shape(p)) {
        if (!attn_aligned(p, false)) return -3;
        const bool two = p->L <= 32;
        const int ppw = two ? 8 : 4;  // (jet, head) pairs per workgroup
        const dim3 grid((p->B * p->H + ppw - 1) / ppw), block(256);
        const size_t lds = (size_t)ppw * 2 * AT_S * p->d * 4;
        hipStream_t st = (hipStream_t)stream;
#define MPG_ATTN_FWD(DV)                                                                          \
    do {                                                                                          \
        if (two) hipLaunchKernelGGL((attn_fwd_fast<DV, true>), grid, block, lds, st, *p);         \
        else hipLaunchKernelGGL((attn_fwd_fast<DV, false>), grid, block, lds, st, *p);            \
    } while (0)
        if (p->d == 8) MPG_ATTN_FWD(8);
        else if (p->d == 16) MPG_ATTN_FWD(16);
        else MPG_ATTN_FWD(32);
#undef MPG_ATTN_FWD
        return (int)hipGetLastError();
    }
    const size_t lds = (size_t)2 * p->S * p->d * 4;
    if (lds > 160 * 1024) return -2;
    return mpg_go<attn_fwd_kernel>(dim3(p->B * p->H), dim3(64), (int)lds, (hipStream_t)stream, *p);
}

extern "C" int mpg_attn_bwd(const MpgAttn* p, void* stream) {
    if (p->d > DMAX || p->B <= 0) return -1;
    if (attn_fast_shape(p)) {
        if (!attn_aligned(p, true)) return -3;
        auto need = [&](bool two) {
            const int capl = two ? 32 : AT_L, ldl = (!two && p->d == 32) ? capl : capl + 1;  // as in the kernel
            return (size_t)(two ? 8 : 4) * (2 * AT_S * p->d + 2 * capl * p->d + 2 * AT_S * ldl) * 4;
        };
        const bool two = p->L <= 32 && need(true) <= 160 * 1024;  // d = 32 does not fit eight pairs
        const int ppw = two ? 8 : 4;
        const dim3 grid((p->B * p->H + ppw - 1) / ppw), block(256);
        const size_t lds = need(two);
        using Go = int (*)(dim3, dim3, int, hipStream_t, const MpgAttn&);
        static constexpr Go GO[3][2] = {{mpg_go<attn_bwd_fast<8, false>, MpgAttn>, mpg_go<attn_bwd_fast<8, true>, MpgAttn>},   // [d: 8, 16, 32][two]
                                        {mpg_go<attn_bwd_fast<16, false>, MpgAttn>, mpg_go<attn_bwd_fast<16, true>, MpgAttn>},
                                        {mpg_go<attn_bwd_fast<32, false>, MpgAttn>, mpg_go<attn_bwd_fast<32, true>, MpgAttn>}};
        return GO[p->d == 8 ? 0 : (p->d == 16 ? 1 : 2)][two](grid, block, (int)lds, (hipStream_t)stream, *p);
    }
    const size_t lds = ((size_t)2 * p->S * p->d + 2 * p->L * p->d + (size_t)p->L * p->S) * 4;
    if (lds > 160 * 1024) return -2;
    return mpg_go<attn_bwd_kernel>(dim3(p->B * p->H), dim3(64), (int)lds, (hipStream_t)stream, *p);
}

extern "C" int mpg_attn_dd(const MpgAttnDD* p, void* stream) {
    constexpr int DD_MAX = 160;   // tokens on either side: every block GAPT builds at N = 30 and N = 150
    if (!(p->d == 8 || p->d == 16 || p->d == 32) || p->B <= 0 || p->H <= 0 || p->L < 1 || p->L > DD_MAX || p->S < 1 || p->S > DD_MAX) return -1;
    if (p->q == nullptr || p->k == nullptr || p->v == nullptr || p->d_o == nullptr || p->P == nullptr) return -2;
    const int E = p->H * p->d;
    auto ld_ok = [E](const void* ptr, int ld) { return ptr == nullptr || ld >= E; };
    if (!(ld_ok(p->q, p->ldq) && ld_ok(p->k, p->ldk) && ld_ok(p->v, p->ldv) && ld_ok(p->d_o, p->ldo) && ld_ok(p->uq, p->lduq) &&
          ld_ok(p->uk, p->lduk) && ld_ok(p->uv, p->lduv) && ld_ok(p->gq, p->ldgq) && ld_ok(p->gk, p->ldgk) && ld_ok(p->gv, p->ldgv) &&
          ld_ok(p->gdo, p->ldgdo)))
        return -5;
    if (p->gq == nullptr && p->gk == nullptr && p->gv == nullptr && p->gdo == nullptr) return 0;   // nothing wanted: nothing launched
    const int p_sl = attn_fast_shape(p->L, p->S, p->d) ? 1 : 0;
    const int longer = p->L > p->S ? p->L : p->S;
    const dim3 grid(p->B * p->H), block(longer <= 64 ? 64 : (longer <= 128 ? 128 : 192));   // a thread per query, then per key
    const size_t lds = ((size_t)(3 * p->L + 4 * p->S) * p->d + 3 * p->L + p->S) * 4;         // <= 145920 bytes
    using Go = int (*)(dim3, dim3, int, hipStream_t, const MpgAttnDD&, const int&);
    static constexpr Go GO[3] = {mpg_go<attn_dd_kernel<8>, MpgAttnDD, int>, mpg_go<attn_dd_kernel<16>, MpgAttnDD, int>,
                                 mpg_go<attn_dd_kernel<32>, MpgAttnDD, int>};
    return GO[p->d == 8 ? 0 : (p->d == 16 ? 1 : 2)](grid, block, (int)lds, (hipStream_t)stream, *p, p_sl);
}
