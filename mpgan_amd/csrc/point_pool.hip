// mpg_point_pool_fwd / mpg_point_pool_bwd: the last per-particle layer of a set-pooling discriminator together with its pooling over
// the particles of a jet (rGAND: ext_models.py:70-71, max; PointNetMixD: ext_models.py:203-206, max | mean).
//
//   z[b,n,c] = sum_k x[(b N + n) ldx + k] W[c ldw + k] + bias[c],   y = act ? LeakyReLU_alpha(z) : z
//   pooled[b, c] = max_n y,  pooled[b, (mode & 1 ? C : 0) + c] = (sum_n y) / N
//
// The activation [B N, C] is the widest tensor of these nets and its only reader is the column-wise reduction, so it never leaves
// the registers: with particles as the ROWS and channels as the COLUMNS of a 32x32x16 MFMA result a lane holds one channel
// (column r = lane & 31) and 16 particles (rows 8g + 4h + t, h = lane >> 5, register 4g + t; common.h), and the pooling is an
// in-lane reduction over the accumulator registers followed by one exchange between the two lane halves.
//
// Launch shape: grid (ceil(C / 128), B), 256 threads.  Workgroup (cg, b) owns jet b and the four 32-column tiles 4 cg .. 4 cg + 3,
// one per wave.  x of the jet is staged in LDS in chunks of 64 k, already split into fp16 hi / lo and laid out as MFMA A fragments
// ([k-step][row tile][hi | lo][lane] x 16 bytes: a wave's ds_read_b128 is contiguous over its lanes), shared by the four waves.
// A wave takes the B fragment of a k-step straight from W (8 consecutive k of row c: 32 bytes), splits it once and applies it to all
// ceil(N / 32) row tiles, whose accumulators it keeps (NT x 16 registers, NT <= 5).  Products: three fp16 terms, fp32 accumulate
// (mfma3 / split8 of common.h); k beyond K, rows beyond N and columns beyond C are zero-filled in registers -- nothing is read
// beyond a row's K columns.  The bias is added in fp32 behind the last k-step.
//
// Order of the reductions (fixed: a jet's results depend neither on B, nor on the grid, nor on the run; no atomics):
//   a lane walks its rows in increasing order -- row tile 0 .. NT-1, then g = 0 .. 3, then t = 0 .. 3 -- skipping rows >= N:
//   sum:     s_h = ((y_r0 + y_r1) + y_r2) + ...  over the rows of lane half h;   mean = (s_0 + s_1) / N
//   max:     a strict ">" over the same walk (the lowest row among equals stays), then the halves: the larger value, the lower
//            row where both are equal.
// Sign words (neg != NULL): bit (c & 31) of neg[(b N + n) ceil(C / 32) + (c >> 5)] is set where !(z > 0) -- one ballot per
// accumulator register gives the word of row 8g + t in its low and of row 8g + 4 + t in its high half.
//
// The backward launch expands the cotangent of pooled into dz [B N, C]; dx, dW and db are GEMMs of the existing launches.
#include "common.h"
#include "mpgan_amd.h"

namespace {

constexpr int PP_KC = 64;          // k per LDS chunk
constexpr int PP_STEPS = PP_KC / 16;
constexpr int PP_THREADS = 256;

struct PPArgs {
    const float* x; const float* W; const float* bias;
    float* pooled; int* argmax; uint32_t* neg;
    int ldx, ldw, ld_pooled;
    int N, K, C, act, mode;
    float alpha;
    int xvec, wvec;   // rows of x / W may be read as aligned float4 pairs
};

// 8 consecutive k of one row, zero beyond K (and for a row that does not exist: row == nullptr)
MPG_DEV void load8(const float* row, int k0, int K, bool vec, float* v) {
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

template <int NT>
__global__ __launch_bounds__(PP_THREADS) void point_pool_fwd_kernel(const PPArgs p) {
    // [k-step][row tile][hi | lo][lane]
    __shared__ f16x8 xs[PP_STEPS * NT * 2 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int b = blockIdx.y;
    const int ct = blockIdx.x * 4 + wave;       // this wave's column tile
    const int c = ct * 32 + r;                  // this lane's channel
    const bool wave_on = ct * 32 < p.C;         // (wave-uniform)
    const bool col_on = c < p.C;
    const float* xjet = p.x + (size_t)b * p.N * p.ldx;
    const float* wrow = col_on ? p.W + (size_t)c * p.ldw : nullptr;

    f32x16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[i][q] = 0.f;

    for (int kc = 0; kc < p.K; kc += PP_KC) {
        if (kc) __syncthreads();   // every wave is done with the previous chunk
        // stage: item = (row, group of 8 k); the fragment of k-step s holds k = 16 s + 8 h' + j in lane (h', row & 31)
        for (int it = tid; it < NT * 32 * (PP_KC / 8); it += PP_THREADS) {
            const int row = it / (PP_KC / 8), kg = it % (PP_KC / 8);
            float v[8];
            load8(row < p.N ? xjet + (size_t)row * p.ldx : nullptr, kc + 8 * kg, p.K, p.xvec, v);
            f16x8 hi, lo;
            split8(v, hi, lo);
            const int at = (((kg >> 1) * NT + (row >> 5)) * 2) * 64 + (kg & 1) * 32 + (row & 31);
            xs[at] = hi;
            xs[at + 64] = lo;
        }
        __syncthreads();
        if (wave_on) {
#pragma unroll
            for (int s = 0; s < PP_STEPS; ++s) {
                if (kc + 16 * s < p.K) {   // (uniform)
                    float wv[8];
                    load8(wrow, kc + 16 * s + 8 * h, p.K, p.wvec, wv);
                    f16x8 whi, wlo;
                    split8(wv, whi, wlo);
#pragma unroll
                    for (int i = 0; i < NT; ++i) {
                        const f16x8 ahi = xs[((s * NT + i) * 2) * 64 + lane];
                        const f16x8 alo = xs[((s * NT + i) * 2 + 1) * 64 + lane];
                        acc[i] = mfma3(ahi, alo, whi, wlo, acc[i]);
                    }
                }
            }
        }
    }
    if (!wave_on) return;

    const float bias = (col_on && p.bias != nullptr) ? p.bias[c] : 0.f;
    const int CW = (p.C + 31) >> 5;
    float vmax = -__builtin_inff(), vsum = 0.f;
    int imax = 0;
    static_for<0, NT>([&](auto ii) {
        MPG_CI(i, ii);
        uint32_t myword = 0u;
        static_for<0, 16>([&](auto qq) {
            MPG_CI(q, qq);
            const int row = 32 * i + 8 * (q >> 2) + 4 * h + (q & 3);
            const float z = acc[i][q] + bias;
            if (p.neg != nullptr) {
                const unsigned long long bits = __builtin_amdgcn_ballot_w64(col_on && !(z > 0.f));
                // the word of row 8g + t sits in the low half, that of row 8g + 4 + t in the high half: lane (h, q) keeps it
                if (r == q) myword = h ? (uint32_t)(bits >> 32) : (uint32_t)bits;
            }
            const float y = p.act ? lrelu(z, p.alpha) : z;
            if (row < p.N) {
                vsum += y;
                if (y > vmax) { vmax = y; imax = row; }
            }
        });
        if (p.neg != nullptr && r < 16) {
            const int row = 32 * i + 8 * (r >> 2) + 4 * h + (r & 3);
            if (row < p.N) p.neg[((size_t)b * p.N + row) * CW + ct] = myword;
        }
    });
    // the two lane halves
    const float omax = __shfl_xor(vmax, 32);
    const int oidx = __shfl_xor(imax, 32);
    const float osum = __shfl_xor(vsum, 32);
    if (omax > vmax || (omax == vmax && oidx < imax)) { vmax = omax; imax = oidx; }
    const float s01 = h ? osum + vsum : vsum + osum;   // s_0 + s_1 in both halves
    if (h == 0 && col_on) {
        float* out = p.pooled + (size_t)b * p.ld_pooled;
        if (p.mode & 1) {
            out[c] = vmax;
            if (p.argmax != nullptr) p.argmax[(size_t)b * p.C + c] = imax;
        }
        if (p.mode & 2) out[((p.mode & 1) ? p.C : 0) + c] = s01 / (float)p.N;
    }
}

struct PPBwdArgs {
    const float* g; const int* argmax; const uint32_t* neg; float* dz;
    int ld_g, ld_dz;
    int N, C, act, mode;
    float alpha;
    long long groups;   // B N ceil(C / 4)
    int vec;            // rows of dz take aligned float4 stores
};

// dz[b,n,c] = slope (gmax[b,c] [n == argmax[b,c]] + gmean[b,c] / N): a thread per (row, four consecutive channels)
__global__ __launch_bounds__(256) void point_pool_bwd_kernel(const PPBwdArgs p) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= p.groups) return;
    const int C4 = (p.C + 3) >> 2;
    const long long row = id / C4;
    const int c0 = (int)(id % C4) * 4;
    const long long b = row / p.N;
    const int n = (int)(row % p.N);
    const int CW = (p.C + 31) >> 5;
    const uint32_t word = (p.act && p.neg != nullptr) ? p.neg[row * CW + (c0 >> 5)] : 0u;
    const float* g = p.g + b * p.ld_g;
    const int mean0 = (p.mode & 1) ? p.C : 0;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = c0 + j;
        float d = 0.f;
        if (c < p.C) {
            if ((p.mode & 1) && p.argmax[b * p.C + c] == n) d = g[c];
            if (p.mode & 2) d += g[mean0 + c] / (float)p.N;
            if ((word >> (c & 31)) & 1u) d *= p.alpha;
        }
        v[j] = d;
    }
    float* out = p.dz + row * p.ld_dz + c0;
    if (p.vec && c0 + 4 <= p.C) {
        *reinterpret_cast<f32x4*>(out) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c0 + j < p.C) out[j] = v[j];
    }
}

// what both entry points refuse, before the first HIP call
int pp_check_sizes(const MpgPointPool* p) {
    if (p->B < 1 || p->N < 1 || p->N > MPG_POINT_POOL_MAX_N || p->C < 1 || p->C > MPG_POINT_POOL_MAX_C) return -1;
    if ((p->mode & ~3) != 0 || p->mode == 0) return -3;
    if (!(p->alpha >= 0.f && p->alpha <= 1.f)) return -4;   // lrelu() is max(v, alpha v)
    if (p->f16 != 1) return -6;
    return 0;
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15u) == 0; }

}  // namespace

extern "C" int mpg_point_pool_fwd(const MpgPointPool* p, void* stream) {
    if (p->K < 1 || p->K > MPG_POINT_POOL_MAX_K) return -1;
    if (const int e = pp_check_sizes(p)) return e;
    if (p->x == nullptr || p->W == nullptr || p->pooled == nullptr) return -2;
    const int width = p->C * ((p->mode & 1) + ((p->mode >> 1) & 1));
    if (p->ldx < p->K || p->ldw < p->K || p->ld_pooled < width) return -5;
    PPArgs a;
    a.x = p->x; a.W = p->W; a.bias = p->bias;
    a.pooled = p->pooled; a.argmax = (p->mode & 1) ? p->argmax : nullptr; a.neg = p->neg;
    a.ldx = p->ldx; a.ldw = p->ldw; a.ld_pooled = p->ld_pooled;
    a.N = p->N; a.K = p->K; a.C = p->C; a.act = p->act != 0; a.mode = p->mode; a.alpha = p->alpha;
    a.xvec = aligned16(p->x) && p->ldx % 4 == 0;
    a.wvec = aligned16(p->W) && p->ldw % 4 == 0;
    const dim3 grid((p->C + 127) / 128, p->B), block(PP_THREADS);
    hipStream_t st = (hipStream_t)stream;
    switch ((p->N + 31) / 32) {
        case 1: hipLaunchKernelGGL(point_pool_fwd_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(point_pool_fwd_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(point_pool_fwd_kernel<3>, grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL(point_pool_fwd_kernel<4>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(point_pool_fwd_kernel<5>, grid, block, 0, st, a); break;
    }
    return (int)hipGetLastError();
}

extern "C" int mpg_point_pool_bwd(const MpgPointPool* p, void* stream) {
    if (const int e = pp_check_sizes(p)) return e;
    if (p->gpooled == nullptr || p->dz == nullptr || ((p->mode & 1) && p->argmax == nullptr) || (p->act && p->neg == nullptr)) return -2;
    const int width = p->C * ((p->mode & 1) + ((p->mode >> 1) & 1));
    if (p->ld_gpooled < width || p->ld_dz < p->C) return -5;
    PPBwdArgs a;
    a.g = p->gpooled; a.argmax = p->argmax; a.neg = p->neg; a.dz = p->dz;
    a.ld_g = p->ld_gpooled; a.ld_dz = p->ld_dz;
    a.N = p->N; a.C = p->C; a.act = p->act != 0; a.mode = p->mode; a.alpha = p->alpha;
    a.groups = (long long)p->B * p->N * ((p->C + 3) / 4);
    a.vec = aligned16(p->dz) && p->ld_dz % 4 == 0;
    const long long blocks = (a.groups + 255) / 256;
    if (blocks > 0x7fffffffLL) return -7;
    hipLaunchKernelGGL(point_pool_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
