// mpg_jet_efps_d4: the 21 connected ("prime") energy-flow polynomials of degree <= 4 of each jet (hadronic measure, beta = 1) --
// what FPD and KPD (mpgan_amd/evaluation.py) are computed from; the 15 composite ones of energyflow's d<=4 set are products
// of these columns and are formed by the caller.  include/mpgan_amd.h has the table of graphs and closed forms.
//
// Shaped like jet_obs_kernel (jet_obs.hip): one workgroup per jet, 64 threads for N <= 32, 256 otherwise, thread t owns
// particle slot t; the particles with pT != 0 are compacted to slots 0 .. n-1; Theta (theta_ij = sqrt(d_eta^2 + d_phi^2)) is
// recomputed from eta, phi in LDS wherever it is used and never stored.
//   1. the O(N^2) vectors, one row per thread: T_k = (Theta^{o k}) z for k = 1 .. 4 (T_1 = w, T_2 = u), then v = Theta (z o w)
//      and q = (Theta o Theta)(z o w); 17 of the 21 columns are sums over particles of products of these;
//   2. the O(N^3) object M = Theta diag(z) Theta, one 32 x 32 tile of its upper triangle at a time on v_mfma_f32_32x32x2_f32
//      (exact fp32 FMA chain), each tile reduced as soon as it is complete into the four sums that need M -- triangle,
//      triangle with one edge doubled, triangle + pendant, 4-cycle -- off-diagonal tiles standing for their transposes too;
//   3. every reduction is a fixed tree (per-lane partials in a fixed order, xor-butterfly per wave, waves in index order).
// Every summand is non-negative: no cancellation, fp32 throughout.
#include "jet_common.h"
#include "../../include/mpgan_amd.h"

namespace {

constexpr int kEfpSmall = 6;   // per-particle LDS arrays

template <int BS>
__global__ __launch_bounds__(BS) void jet_efps_d4_kernel(const float* __restrict__ jets, int ld_jet, int ld_part, int N, int Np,
                                                         int normed, float* __restrict__ efp) {
    constexpr int NW = BS / 64;
    extern __shared__ float lds[];
    float* s_pt = lds;
    float* s_z = lds + Np;
    float* s_eta = lds + 2 * Np;
    float* s_phi = lds + 3 * Np;
    float* s_w = lds + 4 * Np;     // Theta z
    float* s_zw = lds + 5 * Np;    // z o w
    float* red = lds + kEfpSmall * Np;
    int* cnt = (int*)(red + 8 * NW);

    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;

    // ---- load, compact the particles with pT != 0 to slots 0 .. n-1 (original order kept)
    float eta = 0.f, phi = 0.f, pt = 0.f;
    if (t < N) {
        const float* src = jets + (size_t)b * ld_jet + (size_t)t * ld_part;
        eta = src[0]; phi = src[1]; pt = src[2];
    }
    const bool real = pt != 0.f;
    const unsigned long long bal = __ballot(real);
    if (lane == 0) cnt[wv] = __popcll(bal);
    __syncthreads();
    int n = 0, off = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int c = cnt[w];
        off += w < wv ? c : 0;
        n += c;
    }
    if (real) {
        const int dst = off + __popcll(bal & ((1ull << lane) - 1ull));
        s_pt[dst] = pt; s_eta[dst] = eta; s_phi[dst] = phi;
    }
    if (t >= n && t < Np) { s_pt[t] = 0.f; s_eta[t] = 0.f; s_phi[t] = 0.f; }   // (a real particle's thread may own one of these)
    __syncthreads();

    // ---- z; thread t now owns compacted particle t
    float my_pt = 0.f, my_eta = 0.f, my_phi = 0.f;
    if (t < n) { my_pt = s_pt[t]; my_eta = s_eta[t]; my_phi = s_phi[t]; }
    float sums[1] = {my_pt};
    block_sums<NW>(sums, red);
    const float spt = sums[0];
    const float my_z = (normed && spt != 0.f) ? my_pt / spt : my_pt;
    if (t < Np) s_z[t] = t < n ? my_z : 0.f;
    __syncthreads();

    // ---- 1. the O(N^2) vectors
    float t1 = 0.f, t2 = 0.f, t3 = 0.f, t4 = 0.f;
    if (t < n) {
        for (int j = 0; j < n; ++j) {
            const float a = theta(my_eta, my_phi, s_eta[j], s_phi[j]), zj = s_z[j];
            const float a2 = a * a;
            t1 += a * zj;
            t2 += a2 * zj;
            t3 += a2 * a * zj;
            t4 += a2 * a2 * zj;
        }
    }
    const float my_w = t1, my_zw = my_z * t1;
    if (t < Np) { s_w[t] = t < n ? my_w : 0.f; s_zw[t] = t < n ? my_zw : 0.f; }
    __syncthreads();
    float my_v = 0.f, my_q = 0.f;
    if (t < n) {
        for (int j = 0; j < n; ++j) {
            const float a = theta(my_eta, my_phi, s_eta[j], s_phi[j]), x = s_zw[j];
            my_v += a * x;
            my_q += a * a * x;
        }
    }

    // ---- 2. tiles (ta <= tc) of M = Theta diag(z) Theta, reduced as they complete
    const int nt = (n + 31) >> 5, npair = nt * (nt + 1) / 2;
    const int kmax = (n + 7) & ~7;       // z is zero on rows n .. kmax-1 (kmax <= Np)
    const int col = lane & 31, kk = lane >> 5;
    float s_tri = 0.f, s_tri2 = 0.f, s_paw = 0.f, s_cyc = 0.f;
    for (int p = wv; p < npair; p += NW) {
        int ta = 0, rem = p;
        while (rem >= nt - ta) { rem -= nt - ta; ++ta; }
        const int tc = ta + rem;
        const int a0 = ta * 32, c0 = tc * 32;
        const float ea = s_eta[a0 + col], pa = s_phi[a0 + col], ec = s_eta[c0 + col], pc = s_phi[c0 + col];
        f32x16 acc = {};
        for (int k = 0; k < kmax; k += 8) {
            float av[4], bv[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int r = k + 2 * s + kk;
                const float er = s_eta[r], pr = s_phi[r];
                av[s] = theta(er, pr, ea, pa) * s_z[r];   // A[i][r] = theta_{a0+i, r} z_r
                bv[s] = theta(er, pr, ec, pc);            // B[r][j] = theta_{r, c0+j}
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc, 0, 0, 0);
        }
        const int j = c0 + col;
        const float zj = s_z[j], wj = s_w[j];
        const float sym = ta == tc ? 1.f : 2.f;   // tile (tc, ta) is this one transposed
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = a0 + (r & 3) + 8 * (r >> 2) + 4 * kk;
            const float m = acc[r], zz = s_z[i] * zj, tij = theta(s_eta[i], s_phi[i], ec, pc);
            const float zzm = zz * m, tm = zzm * tij;
            s_tri += sym * tm;
            s_tri2 += sym * tm * tij;
            s_cyc += sym * zzm * m;
            s_paw += (ta == tc ? wj : s_w[i] + wj) * tm;
        }
    }

    // ---- 3. the 21 columns (order: include/mpgan_amd.h)
    const float zT2 = my_z * t2, w2 = my_w * my_w;
    float e0[8] = {my_z, my_zw, zT2, my_zw * my_w, my_z * t3, zT2 * my_w, s_tri, my_zw * my_v};
    float e1[8] = {my_zw * w2, my_z * t4, my_z * t3 * my_w, zT2 * t2, s_tri2, zT2 * my_v, my_zw * my_q, zT2 * w2};
    float e2[5] = {s_paw, s_cyc, my_z * my_v * my_v, my_z * w2 * w2, my_z * w2 * my_v};
    block_sums<NW>(e0, red);
    block_sums<NW>(e1, red);
    block_sums<NW>(e2, red);
    if (t == 0) {
        float* f = efp + (size_t)b * MPG_JET_EFPS_D4_PRIMES;
#pragma unroll
        for (int k = 0; k < 8; ++k) { f[k] = e0[k]; f[8 + k] = e1[k]; }
#pragma unroll
        for (int k = 0; k < 5; ++k) f[16 + k] = e2[k];
    }
}

}  // namespace

extern "C" int mpg_jet_efps_d4(const float* jets, int ld_jet, int ld_part, int n, int N, int flags, float* efp, void* stream) {
    const int normed = (flags & MPG_JET_OBS_NORMED) != 0;
    if (n < 1 || N < 1 || N > MPG_JET_OBS_MAX_N || ld_part < 3 || (long long)ld_jet < (long long)(N - 1) * ld_part + 3) return -1;
    if (jets == nullptr || efp == nullptr || (flags & ~MPG_JET_OBS_NORMED)) return -2;
    const int Np = (N + 31) & ~31;
    hipStream_t st = (hipStream_t)stream;
    if (N <= 32) {
        const int lds = (kEfpSmall * Np + 16 * 1) * (int)sizeof(float);
        hipLaunchKernelGGL(jet_efps_d4_kernel<64>, dim3(n), dim3(64), lds, st, jets, ld_jet, ld_part, N, Np, normed, efp);
    } else {
        const int lds = (kEfpSmall * Np + 16 * 4) * (int)sizeof(float);
        hipLaunchKernelGGL(jet_efps_d4_kernel<256>, dim3(n), dim3(256), lds, st, jets, ld_jet, ld_part, N, Np, normed, efp);
    }
    return (int)hipGetLastError();
}
