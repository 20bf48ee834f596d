// mpg_nnconv_fwd / mpg_nnconv_bwd: one edge-conditioned convolution (PyG's NNConv with aggr = "mean", root_weight, bias) of the
// GraphCNN-GAN generator (ext_models.py:75-157) on a k-nearest-neighbour graph, without a weight matrix per edge.
//
// With N(i) the set bits of receiver i's neighbour words (mpg_knn_sets), n_i their number (1 / n_i = 0 for an empty row) and
//   W3[(c,d), o] = nn_weight[(c Cout + o) Cin + d],   Bn[c, o] = nn_bias[c Cout + o]
// the layer  y_i = (1 / n_i) sum_j x_j ((nn_weight (x_j - x_i) + nn_bias).view(Cin, Cout)) + x_i root + bias  is
//   P_i[c,d] = (1 / n_i) sum_j x_j[c] (x_j[d] - x_i[d])        m_i[c] = (1 / n_i) sum_j x_j[c]        (j ascending)
//   y_i      = vec(P_i) W3 + m_i Bn + x_i root + bias
// one row of K = Cin (Cin + 2) against [K, Cout] per node.  The differences are taken in fp32 before any product and before the
// fp16 split: P is NOT formed as mean(x_j x_j^T) - m_i x_i^T, which loses a clustered jet (x = 32 + 1e-3 noise) to cancellation.
//
// Forward: grid (B, ceil(N / 32)), 256 threads.  Workgroup (b, t) keeps jet b's x in LDS as fp32 and owns the receivers 32 t ..:
// they are the ROWS and the output channels the COLUMNS of 32x32x16 MFMA results; every product takes three fp16 terms with fp32
// accumulate (mfma3 / split8 of common.h).  K runs in chunks of 16 groups of 8: a group is 8 consecutive d of one c (Cin rounded up
// to 8 per c, the pad is zero), built by one thread from the neighbour walk, written to the parked [P | m] row on request and
// staged in LDS as split A fragments ([k-step][hi | lo][lane] x 16 bytes); the B operands are read straight from nn_weight (k = d
// along a row of block c), nn_bias and root (k = c down a column).  The last chunk is [m_i | x_i] against [Bn ; root].  Wave w
// owns column tile w; chunks, groups and neighbours come in ascending order, there are no atomics: a jet's values depend neither
// on B, nor on its position in the batch, nor on the run.
//
// Backward (data side), two launches on the one stream:
//   1. G_i[c,d] = sum_o dy_i[o] W3[(c,d), o],  dm_i[c] = sum_o dy_i[o] Bn[c, o]  -> g [B N, Cin (Cin + 1)]  (fp32 FMAs, o ascending:
//      32 rows of dy in LDS per workgroup, a thread per column)
//   2. per jet, a thread per (node j, channel c), x in LDS:
//        dx_j[c] = sum_o dy_j[o] root[c, o] - sum_c' G_j[c', c] m_j[c']
//                  + sum_{i : j in N(i)} (1 / n_i) (dm_i[c] + sum_d G_i[c,d] (x_j[d] - x_i[d]) + sum_c' x_j[c'] G_i[c', c])
//      the listing receivers are found by walking column j of the bit words, i ascending.
// The four parameter gradients are GEMMs of the existing launches from the parked [P | m], x and dy.
#include "common.h"
#include "mpgan_amd.h"

namespace {

constexpr int NC_ROWS = 32;                               // receivers per forward workgroup / dy rows per G workgroup
constexpr int NC_THREADS = 256;
constexpr int NC_KG = 16;                                 // groups of 8 k in one staged chunk
constexpr int NC_FRAGS = (NC_KG / 2) * 2 * 64;            // [k-step][hi | lo][lane]
constexpr int NC_XLD = MPG_NNCONV_MAX_C + 1;              // row stride of x in LDS (odd: rows fall on different banks)
constexpr int NC_WORDS = (MPG_NNCONV_MAX_N + 31) / 32;    // neighbour words per receiver in LDS

// the fragment slot of (row, group kg of 8 k): k-step kg >> 1, lane half kg & 1
MPG_DEV int nc_slot(int row, int kg) { return ((kg >> 1) * 2) * 64 + (kg & 1) * 32 + row; }
// the row of accumulator register q in lane half h
MPG_DEV int nc_row(int q, int h) { return 8 * (q >> 2) + 4 * h + (q & 3); }

// jet's x -> LDS
MPG_DEV void nc_load_x(float* xs, const MpgNNConv& p, int jet, int tid) {
    for (int it = tid; it < p.N * p.Cin; it += NC_THREADS) {
        const int row = it / p.Cin, c = it % p.Cin;
        xs[row * NC_XLD + c] = p.x[((size_t)jet * p.N + row) * p.ld_x + c];
    }
}
// one neighbour word of receiver (jet, i); bits beyond N are dropped
MPG_DEV unsigned nc_word(const MpgNNConv& p, int jet, int i, int w) {
    const int W = (p.N + 31) >> 5;
    unsigned v = p.nbr[((size_t)jet * p.N + i) * W + w];
    const int left = p.N - 32 * w;
    if (left < 32) v &= (1u << left) - 1u;
    return v;
}

__global__ __launch_bounds__(NC_THREADS) void nnconv_fwd_kernel(const MpgNNConv p) {
    __shared__ f16x8 fs[NC_FRAGS];
    __shared__ float xs[MPG_NNCONV_MAX_N * NC_XLD];
    __shared__ unsigned nb[NC_ROWS * NC_WORDS];
    __shared__ float inv[NC_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int jet = blockIdx.x, i0 = blockIdx.y * NC_ROWS;
    const int live = min(NC_ROWS, p.N - i0);
    const int Cin = p.Cin, Cout = p.Cout, W = (p.N + 31) >> 5;
    const int G = (Cin + 7) >> 3;                // groups per c
    const int cpc = NC_KG / G;                   // c per chunk (>= 2)
    const int pmld = Cin * (Cin + 1);
    const int o = wave * 32 + r;                 // this lane's output channel
    const bool wave_on = wave * 32 < Cout;       // (wave-uniform)
    const bool col_on = o < Cout;

    nc_load_x(xs, p, jet, tid);
    for (int it = tid; it < NC_ROWS * NC_WORDS; it += NC_THREADS) {
        const int row = it / NC_WORDS, w = it % NC_WORDS;
        nb[it] = (row < live && w < W) ? nc_word(p, jet, i0 + row, w) : 0u;
    }
    __syncthreads();
    if (tid < NC_ROWS) {
        int cnt = 0;
        for (int w = 0; w < NC_WORDS; ++w) cnt += __popc(nb[tid * NC_WORDS + w]);
        inv[tid] = cnt ? 1.f / (float)cnt : 0.f;
    }
    __syncthreads();

    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;

    // vec(P_i) W3, cpc values of c per chunk
    for (int c0 = 0; c0 < Cin; c0 += cpc) {
        const int groups = min(cpc, Cin - c0) * G;
        const int ksteps = (groups + 1) >> 1;
        if (c0) __syncthreads();   // every wave is done with the previous chunk
        for (int it = tid; it < NC_ROWS * NC_KG; it += NC_THREADS) {
            const int row = it / NC_KG, kg = it % NC_KG;
            if (kg >= 2 * ksteps) continue;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.f;
            if (kg < groups && row < live) {
                const int c = c0 + kg / G, d0 = 8 * (kg % G);
                const float* xi = xs + (i0 + row) * NC_XLD;
                float xd[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) xd[e] = d0 + e < Cin ? xi[d0 + e] : 0.f;
                for (int w = 0; w < W; ++w) {
                    unsigned word = nb[row * NC_WORDS + w];
                    while (word) {
                        const int j = 32 * w + __ffs(word) - 1;
                        word &= word - 1u;
                        const float* xj = xs + j * NC_XLD;
                        const float xc = xj[c];
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = fmaf(xc, (d0 + e < Cin ? xj[d0 + e] : 0.f) - xd[e], v[e]);
                    }
                }
                float* park = p.pm != nullptr ? p.pm + ((size_t)jet * p.N + i0 + row) * pmld + c * Cin : nullptr;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    v[e] *= inv[row];
                    if (park != nullptr && d0 + e < Cin) park[d0 + e] = v[e];
                }
            }
            f16x8 hi, lo;
            split8(v, hi, lo);
            fs[nc_slot(row, kg)] = hi;
            fs[nc_slot(row, kg) + 64] = lo;
        }
        __syncthreads();
        if (!wave_on) continue;
        for (int s = 0; s < ksteps; ++s) {
            const int kg = 2 * s + h;
            const int c = c0 + kg / G, d0 = 8 * (kg % G);
            const float* wrow = (col_on && kg < groups) ? p.nn_weight + ((size_t)c * Cout + o) * Cin : nullptr;
            float wv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) wv[e] = (wrow != nullptr && d0 + e < Cin) ? wrow[d0 + e] : 0.f;
            f16x8 whi, wlo;
            split8(wv, whi, wlo);
            acc = mfma3(fs[(s * 2) * 64 + lane], fs[(s * 2 + 1) * 64 + lane], whi, wlo, acc);
        }
    }

    // [m_i | x_i] against [Bn ; root]: groups 0 .. G-1 are m, G .. 2G-1 are x_i
    {
        const int groups = 2 * G, ksteps = G;
        __syncthreads();
        for (int it = tid; it < NC_ROWS * NC_KG; it += NC_THREADS) {
            const int row = it / NC_KG, kg = it % NC_KG;
            if (kg >= groups) continue;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.f;
            if (row < live) {
                const int d0 = 8 * (kg % G);
                if (kg < G) {
                    for (int w = 0; w < W; ++w) {
                        unsigned word = nb[row * NC_WORDS + w];
                        while (word) {
                            const int j = 32 * w + __ffs(word) - 1;
                            word &= word - 1u;
                            const float* xj = xs + j * NC_XLD;
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[e] += d0 + e < Cin ? xj[d0 + e] : 0.f;
                        }
                    }
                    float* park = p.pm != nullptr ? p.pm + ((size_t)jet * p.N + i0 + row) * pmld + Cin * Cin : nullptr;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        v[e] *= inv[row];
                        if (park != nullptr && d0 + e < Cin) park[d0 + e] = v[e];
                    }
                } else {
                    const float* xi = xs + (i0 + row) * NC_XLD;
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = d0 + e < Cin ? xi[d0 + e] : 0.f;
                }
            }
            f16x8 hi, lo;
            split8(v, hi, lo);
            fs[nc_slot(row, kg)] = hi;
            fs[nc_slot(row, kg) + 64] = lo;
        }
        __syncthreads();
        if (wave_on) {
            for (int s = 0; s < ksteps; ++s) {
                const int kg = 2 * s + h;
                const float* Wm = kg < G ? p.nn_bias : p.root;   // element (k = c, col o) at Wm[c Cout + o]
                const int d0 = 8 * (kg % G);
                float wv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) wv[e] = (col_on && d0 + e < Cin) ? Wm[(size_t)(d0 + e) * Cout + o] : 0.f;
                f16x8 whi, wlo;
                split8(wv, whi, wlo);
                acc = mfma3(fs[(s * 2) * 64 + lane], fs[(s * 2 + 1) * 64 + lane], whi, wlo, acc);
            }
        }
    }
    if (!col_on) return;
    const float bias = p.bias[o];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = nc_row(q, h);
        if (row < live) p.y[((size_t)jet * p.N + i0 + row) * p.ld_y + o] = acc[q] + bias;
    }
}

// backward 1: g[row, :] = [G | dm] of 32 rows of dy
__global__ __launch_bounds__(NC_THREADS) void nnconv_g_kernel(const MpgNNConv p) {
    __shared__ float dys[MPG_NNCONV_MAX_C * NC_ROWS];   // [o][row]
    const int tid = threadIdx.x;
    const int rows = p.B * p.N, r0 = blockIdx.x * NC_ROWS;
    const int live = min(NC_ROWS, rows - r0);
    const int Cin = p.Cin, Cout = p.Cout;
    const int cols = Cin * (Cin + 1);
    for (int it = tid; it < Cout * NC_ROWS; it += NC_THREADS) {
        const int row = it / Cout, oo = it % Cout;
        dys[oo * NC_ROWS + row] = row < live ? p.dy[(size_t)(r0 + row) * p.ld_dy + oo] : 0.f;
    }
    __syncthreads();
    for (int n = tid; n < cols; n += NC_THREADS) {
        const float* w;
        int stride;
        if (n < Cin * Cin) {
            const int c = n / Cin, d = n % Cin;
            w = p.nn_weight + (size_t)c * Cout * Cin + d;
            stride = Cin;
        } else {
            w = p.nn_bias + (size_t)(n - Cin * Cin) * Cout;
            stride = 1;
        }
        float acc[NC_ROWS];
#pragma unroll
        for (int q = 0; q < NC_ROWS; ++q) acc[q] = 0.f;
        for (int oo = 0; oo < Cout; ++oo) {
            const float wv = w[(size_t)oo * stride];
#pragma unroll
            for (int q = 0; q < NC_ROWS; ++q) acc[q] = fmaf(dys[oo * NC_ROWS + q], wv, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < NC_ROWS; ++q)
            if (q < live) p.g[(size_t)(r0 + q) * cols + n] = acc[q];
    }
}

// backward 2: dx of one jet
__global__ __launch_bounds__(NC_THREADS) void nnconv_dx_kernel(const MpgNNConv p) {
    __shared__ float xs[MPG_NNCONV_MAX_N * NC_XLD];
    __shared__ unsigned nb[MPG_NNCONV_MAX_N * NC_WORDS];
    __shared__ float inv[MPG_NNCONV_MAX_N];
    const int tid = threadIdx.x, jet = blockIdx.x;
    const int N = p.N, Cin = p.Cin, Cout = p.Cout, W = (N + 31) >> 5;
    const int cols = Cin * (Cin + 1);
    nc_load_x(xs, p, jet, tid);
    for (int it = tid; it < N * NC_WORDS; it += NC_THREADS) {
        const int row = it / NC_WORDS, w = it % NC_WORDS;
        nb[it] = w < W ? nc_word(p, jet, row, w) : 0u;
    }
    __syncthreads();
    for (int i = tid; i < N; i += NC_THREADS) {
        int cnt = 0;
        for (int w = 0; w < NC_WORDS; ++w) cnt += __popc(nb[i * NC_WORDS + w]);
        inv[i] = cnt ? 1.f / (float)cnt : 0.f;
    }
    __syncthreads();
    for (int it = tid; it < N * Cin; it += NC_THREADS) {
        const int j = it / Cin, c = it % Cin;
        const size_t rj = (size_t)jet * N + j;
        const float* xj = xs + j * NC_XLD;
        // the receiver's own shares
        float acc = 0.f;
        for (int oo = 0; oo < Cout; ++oo) acc = fmaf(p.dy[rj * p.ld_dy + oo], p.root[(size_t)c * Cout + oo], acc);
        const float* gj = p.g + rj * cols;
        const float* mj = p.pm + rj * cols + Cin * Cin;
        float own = 0.f;
        for (int cc = 0; cc < Cin; ++cc) own = fmaf(gj[cc * Cin + c], mj[cc], own);
        acc -= own;
        // the sender's share: the receivers that list j, ascending
        const unsigned bit = 1u << (j & 31);
        const int wj = j >> 5;
        for (int i = 0; i < N; ++i) {
            if (!(nb[i * NC_WORDS + wj] & bit)) continue;
            const float* gi = p.g + ((size_t)jet * N + i) * cols;
            const float* xi = xs + i * NC_XLD;
            float s = gi[Cin * Cin + c];
            for (int d = 0; d < Cin; ++d) s = fmaf(gi[c * Cin + d], xj[d] - xi[d], s);
            for (int cc = 0; cc < Cin; ++cc) s = fmaf(xj[cc], gi[cc * Cin + c], s);
            acc = fmaf(inv[i], s, acc);
        }
        p.dx[rj * p.ld_dx + c] = acc;
    }
}

// what both entry points refuse, before the first HIP call
int nc_check(const MpgNNConv* p) {
    if (p->B < 1 || p->B > MPG_NNCONV_MAX_B || p->N < 1 || p->N > MPG_NNCONV_MAX_N) return -1;
    if (p->Cin < 1 || p->Cin > MPG_NNCONV_MAX_C || p->Cout < 1 || p->Cout > MPG_NNCONV_MAX_C) return -1;
    if (p->x == nullptr || p->nbr == nullptr || p->nn_weight == nullptr || p->nn_bias == nullptr || p->root == nullptr) return -2;
    if (p->ld_x < p->Cin) return -5;
    return 0;
}

}  // namespace

extern "C" int mpg_nnconv_fwd(const MpgNNConv* p, void* stream) {
    if (p == nullptr) return -2;
    if (const int e = nc_check(p)) return e;
    if (p->bias == nullptr || p->y == nullptr) return -2;
    if (p->ld_y < p->Cout) return -5;
    const dim3 grid(p->B, (p->N + NC_ROWS - 1) / NC_ROWS), block(NC_THREADS);
    hipLaunchKernelGGL(nnconv_fwd_kernel, grid, block, 0, (hipStream_t)stream, *p);
    return (int)hipGetLastError();
}

extern "C" int mpg_nnconv_bwd(const MpgNNConv* p, void* stream) {
    if (p == nullptr) return -2;
    if (const int e = nc_check(p)) return e;
    if (p->pm == nullptr || p->dy == nullptr || p->g == nullptr || p->dx == nullptr) return -2;
    if (p->ld_dy < p->Cout || p->ld_dx < p->Cin) return -5;
    const int rows = p->B * p->N;
    hipLaunchKernelGGL(nnconv_g_kernel, dim3((rows + NC_ROWS - 1) / NC_ROWS), dim3(NC_THREADS), 0, (hipStream_t)stream, *p);
    if (const int e = (int)hipGetLastError()) return e;
    hipLaunchKernelGGL(nnconv_dx_kernel, dim3(p->B), dim3(NC_THREADS), 0, (hipStream_t)stream, *p);
    return (int)hipGetLastError();
}
