// mpg_jet_obs: per-jet observables of the evaluation metrics (mpgan_amd/evaluation.py) -- the jet four-vector (pt, eta, phi,
// mass) and the five connected 4-vertex, 4-edge energy-flow polynomials (hadronic measure, beta = 1).  One workgroup per jet:
// 64 threads for N <= 32, 256 otherwise; thread t owns particle slot t.
//
//   1. load and compact: the particles with pT != 0 move to slots 0 .. n-1 in their original order (a ballot + prefix count),
//      slots n .. Np-1 hold zeros, so padding anywhere in the jet costs nothing further;
//   2. sums of pT and of the four-vector components; z = pT / sum pT (or pT);
//   3. the O(N^2) vectors w = Theta z, u = (Theta o Theta) z, v = Theta (z o w), q = (Theta o Theta)(z o w) and the pairwise
//      mass term, one row per thread;
//   4. M = Theta diag(z) Theta one 32 x 32 tile at a time on v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain); M is symmetric,
//      so only tiles ta <= tc are formed, the off-diagonal ones counted twice; each tile is reduced into the paw and 4-cycle
//      sums as soon as it is complete and then dropped;
//   Theta (theta_ij = sqrt(d_eta^2 + d_phi^2)) is never stored: each use recomputes it from eta, phi in LDS.  Its square root
//   and subtractions fit beside the MFMA (64 cycles each), and the workgroup's LDS stays at a few KiB, so several jets share
//   a CU and hide each other's latency (a stored 160 x 160 Theta, 100 KiB, left one jet per CU and ran 4x slower at N = 150).
//   Slots n .. Np-1 have z = 0, which zeroes every term they enter;
//   5. every reduction is a fixed tree (per-lane partials in a fixed order, xor-butterfly per wave, waves summed in index
//      order): two launches on the same input give the same bits.
#include "jet_common.h"
#include "../../include/mpgan_amd.h"

namespace {

constexpr int kSmall = 10;   // per-particle LDS arrays

template <int BS>
__global__ __launch_bounds__(BS) void jet_obs_kernel(const float* __restrict__ jets, int ld_jet, int ld_part, int N, int Np,
                                                     int do_efp, int normed, float* __restrict__ kin, float* __restrict__ efp) {
    constexpr int NW = BS / 64;
    extern __shared__ float lds[];
    float* s_pt = lds;
    float* s_z = lds + Np;
    float* s_eta = lds + 2 * Np;
    float* s_phi = lds + 3 * Np;
    float* s_sh = lds + 4 * Np;    // sinh(eta / 2)
    float* s_ch = lds + 5 * Np;    // cosh(eta / 2)
    float* s_sn = lds + 6 * Np;    // sin(phi / 2)
    float* s_cs = lds + 7 * Np;    // cos(phi / 2)
    float* s_w = lds + 8 * Np;     // Theta z
    float* s_zw = lds + 9 * Np;    // z o w
    float* red = lds + kSmall * Np;
    int* cnt = (int*)(red + 8 * NW);

    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;

    // ---- 1. load, compact the particles with pT != 0 to slots 0 .. n-1 (original order kept)
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
        s_sh[dst] = sinhf(0.5f * eta); s_ch[dst] = coshf(0.5f * eta);
        s_sn[dst] = sinf(0.5f * phi); s_cs[dst] = cosf(0.5f * phi);
    }
    if (t >= n && t < Np) {   // (a real particle's thread may own one of these slots too)
        s_pt[t] = 0.f; s_eta[t] = 0.f; s_phi[t] = 0.f;
        s_sh[t] = 0.f; s_ch[t] = 0.f; s_sn[t] = 0.f; s_cs[t] = 0.f;
    }
    __syncthreads();

    // ---- 2. sums; thread t now owns compacted particle t
    float my_pt = 0.f, my_eta = 0.f, my_phi = 0.f;
    if (t < n) { my_pt = s_pt[t]; my_eta = s_eta[t]; my_phi = s_phi[t]; }
    float sums[4] = {my_pt, my_pt * cosf(my_phi), my_pt * sinf(my_phi), my_pt * sinhf(my_eta)};
    block_sums<NW>(sums, red);
    const float spt = sums[0];
    const float my_z = (normed && spt != 0.f) ? my_pt / spt : my_pt;
    if (t < Np) s_z[t] = t < n ? my_z : 0.f;

    // pairwise mass term: cosh(d_eta) - cos(d_phi) = 2 sinh^2(d_eta / 2) + 2 sin^2(d_phi / 2), no cancellation
    float msum = 0.f;
    if (t < n) {
        const float shi = s_sh[t], chi = s_ch[t], sni = s_sn[t], csi = s_cs[t];
        for (int j = 0; j < n; ++j) {
            const float d1 = shi * s_ch[j] - chi * s_sh[j];
            const float d2 = sni * s_cs[j] - csi * s_sn[j];
            msum += s_pt[j] * (d1 * d1 + d2 * d2);
        }
        msum *= 2.f * my_pt;
    }

    float e[6] = {msum, 0.f, 0.f, 0.f, 0.f, 0.f};   // mass^2, k0, k1, k2, k3, k4
    if (do_efp) {
        // ---- 3. the O(N^2) vectors
        __syncthreads();   // s_z complete
        float my_w = 0.f, my_u = 0.f;
        if (t < n) {
            for (int j = 0; j < n; ++j) {
                const float a = theta(my_eta, my_phi, s_eta[j], s_phi[j]), zj = s_z[j];
                my_w += a * zj;
                my_u += a * a * zj;
            }
        }
        const float my_zw = my_z * my_w;
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
        e[1] = my_z * my_u * my_v;           // a=b-c-d, end edge doubled
        e[2] = my_zw * my_q;                 // a-b=c-d, middle edge doubled
        e[3] = my_z * my_u * my_w * my_w;    // 3-star, one edge doubled

        // ---- 4. tiles (ta <= tc) of M = Theta diag(z) Theta, reduced as they complete
        const int nt = (n + 31) >> 5, npair = nt * (nt + 1) / 2;
        const int kmax = (n + 7) & ~7;       // z is zero on rows n .. kmax-1 (kmax <= Np)
        const int col = lane & 31, kk = lane >> 5;
        float s3 = 0.f, s4 = 0.f;
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
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = a0 + (r & 3) + 8 * (r >> 2) + 4 * kk;
                const float m = acc[r], zz = s_z[i] * zj, tij = theta(s_eta[i], s_phi[i], ec, pc);
                if (ta == tc) {
                    s4 += zz * m * m;
                    s3 += zz * wj * tij * m;
                } else {   // tile (tc, ta) is this one transposed
                    s4 += 2.f * zz * m * m;
                    s3 += zz * (s_w[i] + wj) * tij * m;
                }
            }
        }
        e[4] = s3;   // triangle + pendant
        e[5] = s4;   // 4-cycle
    }
    block_sums<NW>(e, red);

    if (t == 0) {
        const float px = sums[1], py = sums[2], pz = sums[3];
        const float jpt = hypotf(px, py);
        float* o = kin + (size_t)b * 4;
        o[0] = jpt;
        o[1] = jpt > 0.f ? asinhf(pz / jpt) : 0.f;
        o[2] = atan2f(py, px);
        o[3] = sqrtf(fmaxf(e[0], 0.f));
        if (do_efp) {
            float* f = efp + (size_t)b * 5;
#pragma unroll
            for (int k = 0; k < 5; ++k) f[k] = e[1 + k];
        }
    }
}

}  // namespace

extern "C" int mpg_jet_obs(const float* jets, int ld_jet, int ld_part, int n, int N, int flags, float* kin, float* efp,
                           void* stream) {
    const int do_efp = (flags & MPG_JET_OBS_EFP) != 0, normed = (flags & MPG_JET_OBS_NORMED) != 0;
    if (n < 1 || N < 1 || N > MPG_JET_OBS_MAX_N || ld_part < 3 || (long long)ld_jet < (long long)(N - 1) * ld_part + 3) return -1;
    if (jets == nullptr || kin == nullptr || (do_efp && efp == nullptr) || (flags & ~(MPG_JET_OBS_EFP | MPG_JET_OBS_NORMED))) return -2;
    const int Np = (N + 31) & ~31;
    hipStream_t st = (hipStream_t)stream;
    if (N <= 32) {
        const int lds = (kSmall * Np + 16 * 1) * (int)sizeof(float);
        hipLaunchKernelGGL(jet_obs_kernel<64>, dim3(n), dim3(64), lds, st, jets, ld_jet, ld_part, N, Np, do_efp, normed, kin, efp);
    } else {
        const int lds = (kSmall * Np + 16 * 4) * (int)sizeof(float);
        hipLaunchKernelGGL(jet_obs_kernel<256>, dim3(n), dim3(256), lds, st, jets, ld_jet, ld_part, N, Np, do_efp, normed, kin, efp);
    }
    return (int)hipGetLastError();
}
