// mpg_tree_gcn_fwd / mpg_tree_gcn_bwd: one TreeGCN layer of the TreeGAN generator (ext_models.py:211-282) in one launch per direction.
//
// Layer d has P parent nodes, degree g, widths in -> out.  With anc_i(p) = p / (P / P_i) the ancestor of node p on level i <= d:
//   root[b,p]  = sum_{i<=d} tree[i][b, anc_i(p)] W_root[i]^T
//   u[b,p,:]   = LeakyReLU_alpha(tree[d][b,p,:] W_branch[p])            [g in]; child c = p g + j owns u[b,p, j in : (j+1) in]
//   h[b,c]     = u_c Wc^T + root[b, c / g],      Wc = W_loop.1 W_loop.0  [out, in]  (formed by a launch before this one)
//   y[b,c]     = act ? LeakyReLU_alpha(h + bias[c % g]) : h + bias[c % g]          (bias NULL = 0)
// The [rows, in support] activation of W_loop never exists.
//
// Launch shape (both directions): grid (ceil(B / 32), P), 256 threads.  Workgroup (bt, p) owns the 32 jets b0 = 32 bt .. of node p:
// W_branch[p] is a different matrix per node, so the rows that share a B operand are the jets of one node.  Jets are the ROWS and
// channels the COLUMNS of the 32x32x16 MFMA results; every product takes three 16-bit terms with fp32 accumulate (mfma3 / split8 of
// common.h): fp16 hi / lo in the forward, bf16 hi / lo in the backward (cotangents of any magnitude).  A operands are staged in LDS
// as split fragments ([k-step][hi | lo][lane] x 16 bytes, 16 KiB for 128 k), B operands are read straight from the weights.
//
// Forward, in this order (fixed: no atomics, a jet's values depend neither on B, nor on its row in the tile, nor on the grid):
//   1. for i = 0 .. d: stage the jets' rows of tree[i][:, anc_i(p)]; wave w adds their product with W_root[i]^T into the root
//      accumulator of column tile w (k ascending).  The last staged level is tree[d][:, p] itself.
//   2. u = lrelu(x W_branch[p]): wave w owns column tiles w, w + 4 of g in <= 256; u goes to LDS in fp32 (and to memory, u != NULL).
//   3. for j = 0 .. g-1: stage u_j from LDS; wave w: acc = root, += u_j Wc^T (k ascending), + bias, activation, store.
// Rows beyond B, columns beyond the widths and k beyond K are zero-filled in registers; nothing beyond them is read or written.
//
// Backward (data side), given dy = dL/dy [B, P g, out]:
//   1. for j = 0 .. g-1: dz_j = dy_j (y_j > 0 ? 1 : alpha) (act; else dy_j) -> memory and, split, LDS; S += dz_j in registers
//      (j ascending); wave w: du_j = (dz_j Wc) (u_j > 0 ? 1 : alpha) for column tile w of in -> memory and LDS (fp32).
//   2. S[b,p] -> memory.   3. dx[b,p] = du[b,p] W_branch[p]^T (k = g in ascending, staged in chunks of 128) -> memory (dx != NULL).
// The sums over descendants, the products with W_root[i] and every parameter gradient are GEMMs of the existing launches.
#include "common.h"
#include "mpgan_amd.h"

namespace {

constexpr int TG_ROWS = 32;                          // jets per workgroup
constexpr int TG_THREADS = 256;
constexpr int TG_KMAX = 128;                         // k of one staged operand
constexpr int TG_KG = TG_KMAX / 8;                   // groups of 8 k per row
constexpr int TG_FRAGS = (TG_KMAX / 16) * 2 * 64;    // [k-step][hi | lo][lane]
constexpr int TG_ULD = MPG_TREE_GCN_MAX_BRANCH + 1;  // row stride of the fp32 u / du tile in LDS (odd: rows fall on different banks)

// the fragment slot of (row, group kg of 8 k): k-step kg >> 1, lane half kg & 1
MPG_DEV int tg_slot(int row, int kg) { return ((kg >> 1) * 2) * 64 + (kg & 1) * 32 + row; }

// 8 consecutive k of one row in memory, zero beyond K and for a row that does not exist
MPG_DEV void tg_load8(const float* row, int k0, int K, float* v) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (row != nullptr && k0 + j < K) ? row[k0 + j] : 0.f;
}

// B fragment of k-step s from a matrix whose k runs along a row (element (k, col) at W[col ld + k]): lane (r, h) takes k = 16 s + 8 h + j
template <typename V>
MPG_DEV void tg_bfrag_rowk(const float* wrow, int k0, int K, V& hi, V& lo) {
    float v[8];
    tg_load8(wrow, k0, K, v);
    split8(v, hi, lo);
}
// ... from a matrix whose k runs down a column (element (k, col) at W[k ld + col]); ``col_on``: the lane's column exists
template <typename V>
MPG_DEV void tg_bfrag_colk(const float* W, int ld, int col, bool col_on, int k0, int K, V& hi, V& lo) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (col_on && k0 + j < K) ? W[(size_t)(k0 + j) * ld + col] : 0.f;
    split8(v, hi, lo);
}

// stage K <= 128 columns of the tile's 32 rows from memory (row i at base + i stride, rows >= live are zero) as split A fragments
template <typename V>
MPG_DEV void tg_stage_mem(V* fs, const float* base, size_t stride, int live, int K, int tid) {
    const int kgs = ((K + 15) >> 4) * 2;
    for (int it = tid; it < TG_ROWS * TG_KG; it += TG_THREADS) {
        const int row = it / TG_KG, kg = it % TG_KG;
        if (kg >= kgs) continue;
        float v[8];
        tg_load8(row < live ? base + (size_t)row * stride : nullptr, 8 * kg, K, v);
        V hi, lo;
        split8(v, hi, lo);
        fs[tg_slot(row, kg)] = hi;
        fs[tg_slot(row, kg) + 64] = lo;
    }
}
// ... from columns col0 .. col0 + K - 1 of the fp32 tile in LDS
template <typename V>
MPG_DEV void tg_stage_lds(V* fs, const float* tile, int col0, int K, int tid) {
    const int kgs = ((K + 15) >> 4) * 2;
    for (int it = tid; it < TG_ROWS * TG_KG; it += TG_THREADS) {
        const int row = it / TG_KG, kg = it % TG_KG;
        if (kg >= kgs) continue;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (8 * kg + j < K) ? tile[row * TG_ULD + col0 + 8 * kg + j] : 0.f;
        V hi, lo;
        split8(v, hi, lo);
        fs[tg_slot(row, kg)] = hi;
        fs[tg_slot(row, kg) + 64] = lo;
    }
}

MPG_DEV f32x16 tg_zero() {
    f32x16 a;
#pragma unroll
    for (int q = 0; q < 16; ++q) a[q] = 0.f;
    return a;
}
// the row of accumulator register q in lane half h
MPG_DEV int tg_row(int q, int h) { return 8 * (q >> 2) + 4 * h + (q & 3); }

__global__ __launch_bounds__(TG_THREADS) void tree_gcn_fwd_kernel(const MpgTreeGcn p) {
    __shared__ f16x8 fs[TG_FRAGS];
    __shared__ float ut[TG_ROWS * TG_ULD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int node = blockIdx.y, b0 = blockIdx.x * TG_ROWS;
    const int live = min(TG_ROWS, p.B - b0);
    const int gin = p.g * p.in;
    const int c = wave * 32 + r;                 // this lane's output channel
    const bool wave_on = wave * 32 < p.out;      // (wave-uniform)
    const bool col_on = c < p.out;

    // 1. root: the ancestors' rows times W_root[i]^T, level by level
    f32x16 root = tg_zero();
    for (int i = 0; i <= p.d; ++i) {
        const int K = p.width[i], Pi = p.nodes[i];
        const int q = node / (p.P / Pi);
        if (i) __syncthreads();   // every wave is done with the previous level
        tg_stage_mem(fs, p.level[i] + ((size_t)b0 * Pi + q) * K, (size_t)Pi * K, live, K, tid);
        __syncthreads();
        if (wave_on) {
            const float* wrow = col_on ? p.W_root[i] + (size_t)c * K : nullptr;
            for (int s = 0; 16 * s < K; ++s) {
                f16x8 whi, wlo;
                tg_bfrag_rowk(wrow, 16 * s + 8 * h, K, whi, wlo);
                root = mfma3(fs[(s * 2) * 64 + lane], fs[(s * 2 + 1) * 64 + lane], whi, wlo, root);
            }
        }
    }

    // 2. u = lrelu(x W_branch[node]); fs still holds x = tree[d][:, node]
    const float* Wb = p.W_branch + (size_t)node * p.in * gin;
    for (int t = wave; t * 32 < gin; t += 4) {
        const int col = t * 32 + r;
        f32x16 acc = tg_zero();
        for (int s = 0; 16 * s < p.in; ++s) {
            f16x8 whi, wlo;
            tg_bfrag_colk(Wb, gin, col, col < gin, 16 * s + 8 * h, p.in, whi, wlo);
            acc = mfma3(fs[(s * 2) * 64 + lane], fs[(s * 2 + 1) * 64 + lane], whi, wlo, acc);
        }
        if (col < gin) {
#pragma unroll
            for (int q = 0; q < 16; ++q) ut[tg_row(q, h) * TG_ULD + col] = lrelu(acc[q], p.alpha);
        }
    }
    __syncthreads();   // u is complete, and every wave is done with x
    if (p.u != nullptr) {
        for (int it = tid; it < live * gin; it += TG_THREADS) {
            const int row = it / gin, col = it % gin;
            const int j = col / p.in, k = col % p.in;
            p.u[(((size_t)(b0 + row) * p.P + node) * p.g + j) * p.ld_u + k] = ut[row * TG_ULD + col];
        }
    }

    // 3. the children
    const float* wrow = col_on ? p.Wc + (size_t)c * p.in : nullptr;
    for (int j = 0; j < p.g; ++j) {
        if (j) __syncthreads();   // every wave is done with the previous child
        tg_stage_lds(fs, ut, j * p.in, p.in, tid);
        __syncthreads();
        if (!wave_on) continue;
        f32x16 acc = root;
        for (int s = 0; 16 * s < p.in; ++s) {
            f16x8 whi, wlo;
            tg_bfrag_rowk(wrow, 16 * s + 8 * h, p.in, whi, wlo);
            acc = mfma3(fs[(s * 2) * 64 + lane], fs[(s * 2 + 1) * 64 + lane], whi, wlo, acc);
        }
        if (!col_on) continue;
        const float bias = p.bias != nullptr ? p.bias[j * p.out + c] : 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = tg_row(q, h);
            if (row < live) {
                const float z = acc[q] + bias;
                p.y[(((size_t)(b0 + row) * p.P + node) * p.g + j) * p.ld_y + c] = p.act ? lrelu(z, p.alpha) : z;
            }
        }
    }
}

__global__ __launch_bounds__(TG_THREADS) void tree_gcn_bwd_kernel(const MpgTreeGcn p) {
    __shared__ bf16x8 fs[TG_FRAGS];
    __shared__ float dut[TG_ROWS * TG_ULD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int node = blockIdx.y, b0 = blockIdx.x * TG_ROWS;
    const int live = min(TG_ROWS, p.B - b0);
    const int gin = p.g * p.in;
    const int n = wave * 32 + r;                 // this lane's input channel
    const bool wave_on = wave * 32 < p.in;       // (wave-uniform)
    const bool col_on = n < p.in;
    const int kgs = ((p.out + 15) >> 4) * 2;

    // a thread's two staging items (row, 8 channels) are the same for every child: S stays in its registers
    float S[2][8];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int e = 0; e < 8; ++e) S[a][e] = 0.f;

    for (int j = 0; j < p.g; ++j) {
        if (j) __syncthreads();   // every wave is done with the previous child's dz
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int it = tid + a * TG_THREADS;
            const int row = it / TG_KG, kg = it % TG_KG;
            if (kg >= kgs) continue;
            float v[8];
            const size_t at = ((size_t)(b0 + row) * p.P + node) * p.g + j;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = 8 * kg + e;
                float d = 0.f;
                if (row < live && k < p.out) {
                    d = p.dy[at * p.ld_dy + k];
                    if (p.act) d *= lrelu_grad(p.y[at * p.ld_y + k], p.alpha);
                    p.dz[at * p.ld_dz + k] = d;
                }
                v[e] = d;
                S[a][e] += d;
            }
            bf16x8 hi, lo;
            split8(v, hi, lo);
            fs[tg_slot(row, kg)] = hi;
            fs[tg_slot(row, kg) + 64] = lo;
        }
        __syncthreads();
        if (!wave_on) continue;
        f32x16 acc = tg_zero();
        for (int s = 0; 16 * s < p.out; ++s) {
            bf16x8 whi, wlo;
            tg_bfrag_colk(p.Wc, p.in, n, col_on, 16 * s + 8 * h, p.out, whi, wlo);
            acc = mfma3(fs[(s * 2) * 64 + lane], fs[(s * 2 + 1) * 64 + lane], whi, wlo, acc);
        }
        if (!col_on) continue;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = tg_row(q, h);
            float d = 0.f;
            if (row < live) {
                const size_t at = ((size_t)(b0 + row) * p.P + node) * p.g + j;
                d = acc[q] * lrelu_grad(p.u[at * p.ld_u + n], p.alpha);
                p.du[at * p.in + n] = d;
            }
            dut[row * TG_ULD + j * p.in + n] = d;
        }
    }

#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int it = tid + a * TG_THREADS;
        const int row = it / TG_KG, kg = it % TG_KG;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (row < live && 8 * kg + e < p.out) p.S[((size_t)(b0 + row) * p.P + node) * p.out + 8 * kg + e] = S[a][e];
    }
    if (p.dx == nullptr) return;

    // dx = du W_branch[node]^T over k = g in, in chunks of 128
    const float* wrow = col_on ? p.W_branch + (size_t)node * p.in * gin + (size_t)n * gin : nullptr;
    f32x16 acc = tg_zero();
    for (int kc = 0; kc < gin; kc += TG_KMAX) {
        __syncthreads();   // du is complete (first chunk); every wave is done with the previous chunk
        const int K = min(TG_KMAX, gin - kc);
        tg_stage_lds(fs, dut, kc, K, tid);
        __syncthreads();
        if (wave_on) {
            for (int s = 0; 16 * s < K; ++s) {
                bf16x8 whi, wlo;
                tg_bfrag_rowk(wrow, kc + 16 * s + 8 * h, gin, whi, wlo);
                acc = mfma3(fs[(s * 2) * 64 + lane], fs[(s * 2 + 1) * 64 + lane], whi, wlo, acc);
            }
        }
    }
    if (!col_on) return;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = tg_row(q, h);
        if (row < live) p.dx[((size_t)(b0 + row) * p.P + node) * p.in + n] = acc[q];
    }
}

// what both entry points refuse, before the first HIP call
int tg_check(const MpgTreeGcn* p) {
    if (p->B < 1 || p->P < 1 || p->g < 1 || p->in < 1 || p->out < 1) return -1;
    if (p->d < 0 || p->d >= MPG_TREE_GCN_MAX_LEVELS) return -1;
    if (p->in > MPG_TREE_GCN_MAX_WIDTH || p->out > MPG_TREE_GCN_MAX_WIDTH) return -1;
    if ((long long)p->g * p->in > MPG_TREE_GCN_MAX_BRANCH || (long long)p->P * p->g > MPG_TREE_GCN_MAX_NODES) return -1;
    for (int i = 0; i <= p->d; ++i) {
        if (p->width[i] < 1 || p->width[i] > MPG_TREE_GCN_MAX_WIDTH || p->nodes[i] < 1) return -1;
        if (p->nodes[i] > p->P || p->P % p->nodes[i] != 0) return -3;
    }
    if (p->width[p->d] != p->in || p->nodes[p->d] != p->P) return -3;
    if (!(p->alpha >= 0.f && p->alpha <= 1.f)) return -4;   // lrelu() is max(v, alpha v)
    return 0;
}

}  // namespace

extern "C" int mpg_tree_gcn_fwd(const MpgTreeGcn* p, void* stream) {
    if (p == nullptr) return -2;
    if (const int e = tg_check(p)) return e;
    if (p->W_branch == nullptr || p->Wc == nullptr || p->y == nullptr) return -2;
    for (int i = 0; i <= p->d; ++i)
        if (p->level[i] == nullptr || p->W_root[i] == nullptr) return -2;
    if (p->ld_y < p->out || (p->u != nullptr && p->ld_u < p->in)) return -5;
    const dim3 grid((p->B + TG_ROWS - 1) / TG_ROWS, p->P), block(TG_THREADS);
    hipLaunchKernelGGL(tree_gcn_fwd_kernel, grid, block, 0, (hipStream_t)stream, *p);
    return (int)hipGetLastError();
}

extern "C" int mpg_tree_gcn_bwd(const MpgTreeGcn* p, void* stream) {
    if (p == nullptr) return -2;
    if (const int e = tg_check(p)) return e;
    if (p->W_branch == nullptr || p->Wc == nullptr || p->u == nullptr || p->dy == nullptr || p->dz == nullptr || p->S == nullptr
        || p->du == nullptr || (p->act && p->y == nullptr))
        return -2;
    if (p->ld_dy < p->out || p->ld_dz < p->out || p->ld_u < p->in || (p->act && p->ld_y < p->out)) return -5;
    const dim3 grid((p->B + TG_ROWS - 1) / TG_ROWS, p->P), block(TG_THREADS);
    hipLaunchKernelGGL(tree_gcn_bwd_kernel, grid, block, 0, (hipStream_t)stream, *p);
    return (int)hipGetLastError();
}
