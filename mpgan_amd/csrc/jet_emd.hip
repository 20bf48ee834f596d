// mpg_jet_emd / mpg_jet_emd_host: the exact energy mover's distance between every jet of one set and every jet of another
// (the definition is in include/mpgan_amd.h), the hot path of coverage and MMD (mpgan_amd/evaluation.py).
//
// Solver: successive shortest paths with node potentials on the bipartite transportation problem.  The sources are the
// particles of jet a with pT > 0 (compacted, original order) and one slack source, the sinks those of jet b and one slack
// sink; the slack of the heavier jet has weight 0 and is left out of every search.  Sources are served in index order: a
// Dijkstra search from the first source with supply left, on reduced costs c_ij + pi_i - pi_j >= 0 (forward arcs i -> j always,
// backward arcs j -> i where flow f_ij > 0), stops at the first sink popped that still has demand; the flow along that path
// grows by delta = min(supply, demand, backward flows on the path) > 0 and pi_v += d_v - d_target on the popped nodes.  The
// quantity that equals delta becomes exactly 0, so every augmentation retires a source, a sink or a backward arc: no
// zero-length (degenerate) step exists, whatever ties duplicate particles or slack-free pairs put into the costs.
//
// Every loop is bounded: a search pops at most `nodes` nodes, a path has at most `nodes` arcs, and the augmentations stop at
// emd_cap(N) (a function of N only).  A pair that reaches the cap -- or whose search finds no sink, which non-finite
// coordinates can cause -- ships what is left in index order (a feasible plan, an upper bound) and reports status 1 (or 2).
//
// One code for both builds (emd_solve, templated on the scalar type and on a "lanes" policy): thread `lane` of W owns the
// nodes lane, lane + W, ... (K register slots); the policy supplies the cross-lane steps.
//   * GPU (fp32): W = 64, one wave per pair, 4 pairs per workgroup at N <= 31 (K = 1: a node per lane).  The argmin of a pop
//     is four DPP steps inside the rows of 16 lanes, four v_readlane and a ballot; the popped node's coordinates and potential
//     come through v_readlane as well, and every cost is recomputed from the coordinates (a subtract pair, an FMA, a square
//     root) -- no cost matrix.  LDS per wave: the coordinates (3 (2N + 2) values) and the flows f[sink][source]
//     ((N + 1)^2 values): 4.6 KiB at N = 30, 95 KiB at N = 150 (one wave per workgroup then; such pairs are latency bound).
//     Only lane 0 writes flows, the lanes of the wave read them one search later; a wave's LDS operations complete in order.
//   * host (fp64): W = 1, the same statements run as plain loops; std::thread workers take pairs from an atomic counter.
// out[i, j] depends on the values of a[i] and b[j] alone: no atomics, every sum in a fixed order.
#include "common.h"
#include "../../include/mpgan_amd.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <thread>
#include <vector>

namespace {

#define EMD_HD __host__ __device__ __forceinline__

constexpr int kEmdMaxNodes = 2 * MPG_JET_OBS_MAX_N + 2;

// augmentations allowed per pair, 16 per node.  Each retires a source, a sink or a backward arc; synthetic jets took 70 to 104
// on average and 217 at most at N = 30 (cap 992), 430 to 750 and 1471 at N = 150 (cap 4832) (DESIGN.md Part I section 4).
EMD_HD int emd_cap(int N) { return 32 * (N + 1); }

EMD_HD float emd_sqrt(float x) { return sqrtf(x); }
EMD_HD double emd_sqrt(double x) { return sqrt(x); }

template <typename T>
EMD_HD T emd_theta(T e1, T p1, T e2, T p2, T inv_r) {
    const T de = e1 - e2, dp = p1 - p2;
    return emd_sqrt(de * de + dp * dp) * inv_r;
}

// ---------------------------------------------------------------------------------------------------- lanes policies
template <typename T>
struct HostLanes {
    static constexpr int W = 1;
    EMD_HD int lane() const { return 0; }
    EMD_HD T min_all(T x) const { return x; }
    EMD_HD T sum_all(T x) const { return x; }
    EMD_HD int first_lane(bool p) const { return p ? 0 : -1; }
    template <typename U, int K>
    EMD_HD U get(const U (&x)[K], int u) const { return x[u]; }
    EMD_HD void prefix(bool f, int& before, int& total) const { before = 0; total = f ? 1 : 0; }
    EMD_HD void sync() const {}
};

MPG_DEV int emd_rl(int x, int l) { return __builtin_amdgcn_readlane(x, l); }
MPG_DEV float emd_rl(float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }
MPG_DEV double emd_rl(double x, int l) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// DPP moves inside a row of 16 lanes (all 64 lanes are active wherever these run)
template <int CTRL>
MPG_DEV float emd_dpp(float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false)); }
template <int CTRL>
MPG_DEV double emd_dpp(double x) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, 0xf, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)((unsigned long long)b >> 32), CTRL, 0xf, 0xf, false);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// (the keys are never NaN: a candidate distance is stored only where it compares below the old one)
MPG_DEV float emd_min(float a, float b) { return __builtin_fminf(a, b); }
MPG_DEV double emd_min(double a, double b) { return __builtin_fmin(a, b); }

template <typename T>
struct WaveLanes {
    static constexpr int W = 64;
    MPG_DEV int lane() const { return threadIdx.x & 63; }
    // minimum over the wave, the same bits in every lane: lanes ^1, ^2 (quad permutes), the other quad pair (row_half_mirror),
    // the other half row (row_mirror), then the four rows through v_readlane
    MPG_DEV T min_all(T x) const {
        x = emd_min(x, emd_dpp<0xB1>(x));
        x = emd_min(x, emd_dpp<0x4E>(x));
        x = emd_min(x, emd_dpp<0x141>(x));
        x = emd_min(x, emd_dpp<0x140>(x));
        return emd_min(emd_min(emd_rl(x, 0), emd_rl(x, 16)), emd_min(emd_rl(x, 32), emd_rl(x, 48)));
    }
    MPG_DEV T sum_all(T x) const {   // fixed xor butterfly: the same bits in every lane
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
        return x;
    }
    MPG_DEV int first_lane(bool p) const {
        const unsigned long long b = __ballot(p);
        return b ? __builtin_ctzll(b) : -1;
    }
    // slot u / 64 of lane u % 64; u is the same in every lane
    template <typename U, int K>
    MPG_DEV U get(const U (&x)[K], int u) const {
        const int uu = __builtin_amdgcn_readfirstlane(u), slot = uu >> 6;
        U v = x[0];
#pragma unroll
        for (int k = 1; k < K; ++k) v = slot == k ? x[k] : v;
        return emd_rl(v, uu & 63);
    }
    MPG_DEV void prefix(bool f, int& before, int& total) const {
        const unsigned long long b = __ballot(f);
        before = __popcll(b & ((1ull << lane()) - 1ull));
        total = __popcll(b);
    }
    MPG_DEV void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
};

// ---------------------------------------------------------------------------------------------------- the solver
// Scratch of one pair (LDS on the GPU, heap on the host), in units of T: eta, phi, pT of the nodes (3 x ldn) and the flows.
EMD_HD int emd_ldn(int N) { return 2 * N + 2; }
EMD_HD int emd_scratch(int N) { return 3 * emd_ldn(N) + (N + 1) * (N + 1); }

// particles of one jet with pT > 0 -> nodes off .. off + count - 1, original order; returns count
template <class P, typename T>
EMD_HD int emd_compact(const P& p, const float* jet, int ld_part, int N, T* s_eta, T* s_phi, T* s_w, int off) {
    int cnt = 0;
    for (int base = 0; base < N; base += P::W) {
        const int i = base + p.lane();
        float e = 0.f, ph = 0.f, pt = 0.f;
        if (i < N) { e = jet[(size_t)i * ld_part]; ph = jet[(size_t)i * ld_part + 1]; pt = jet[(size_t)i * ld_part + 2]; }
        const bool real = pt > 0.f;
        int before, total;
        p.prefix(real, before, total);
        if (real) {
            const int d = off + cnt + before;
            s_eta[d] = (T)e; s_phi[d] = (T)ph; s_w[d] = (T)pt;
        }
        cnt += total;
    }
    return cnt;
}

template <class P, typename T>
EMD_HD T emd_sum(const P& p, const T* x, int n) {
    T s = 0;
    for (int i = p.lane(); i < n; i += P::W) s += x[i];
    return p.sum_all(s);
}

// K: register slots per lane, K * P::W >= nodes.  Returns the distance; status 0 / 1 (cap) / 2 (no path); iters = augmentations.
template <class P, typename T, int K>
EMD_HD T emd_solve(const P& p, const float* ja, const float* jb, int ld_part, int N, T inv_r, int cap, T* mem, int& status,
                   int& iters) {
    constexpr int W = P::W;
    constexpr int UNR = W == 1 ? 1 : K;   // the host runs its slots as a plain loop
    const T INF = std::numeric_limits<T>::infinity();
    const int lane = p.lane(), ldn = emd_ldn(N);
    T* s_eta = mem;
    T* s_phi = mem + ldn;
    T* s_w = mem + 2 * ldn;
    T* F = mem + 3 * ldn;   // F[(j - n1) * n1 + i]: flow from source i to sink j

    // ---- nodes: a's particles, the slack source, b's particles, the slack sink
    const int na = emd_compact(p, ja, ld_part, N, s_eta, s_phi, s_w, 0);
    const int n1 = na + 1;
    const int nb = emd_compact(p, jb, ld_part, N, s_eta, s_phi, s_w, n1);
    const int n2 = nb + 1, nodes = n1 + n2;
    const int slack_a = na, slack_b = nodes - 1;
    p.sync();
    const T sum_a = emd_sum(p, s_w, na), sum_b = emd_sum(p, s_w + n1, nb);
    const T d = sum_a - sum_b;
    const T w_slack_a = d < 0 ? -d : (T)0, w_slack_b = d > 0 ? d : (T)0;
    if (lane == 0) {
        s_eta[slack_a] = 0; s_phi[slack_a] = 0; s_w[slack_a] = w_slack_a;
        s_eta[slack_b] = 0; s_phi[slack_b] = 0; s_w[slack_b] = w_slack_b;
    }
    for (int i = lane; i < n1 * n2; i += W) F[i] = 0;
    p.sync();
    // a slack of weight 0 takes no part (it can neither end a path nor carry flow back)
    const int dead_a = w_slack_a > 0 ? -1 : slack_a, dead_b = w_slack_b > 0 ? -1 : slack_b;

    T eta[K], phi[K], w[K], pi[K], key[K], dfin[K];
    int prev[K];
#pragma unroll UNR
    for (int k = 0; k < K; ++k) {
        const int v = lane + W * k;
        const bool in = v < nodes;
        eta[k] = in ? s_eta[v] : (T)0;
        phi[k] = in ? s_phi[v] : (T)0;
        w[k] = in ? s_w[v] : (T)0;
        pi[k] = 0; key[k] = INF; dfin[k] = INF; prev[k] = -1;
        if (!in && W == 1) break;
    }

    status = 0;
    iters = 0;
    const int max_rounds = cap + 1;
    for (int round = 0; round < max_rounds; ++round) {
        // ---- the first source with supply left, and whether any sink still has demand
        int s = -1;
        bool demand = false;
#pragma unroll UNR
        for (int k = 0; k < K; ++k) {
            const int v = lane + W * k;
            if (W == 1 && v >= nodes) break;
            if (s < 0) {
                const int l = p.first_lane(v < n1 && w[k] > 0);
                if (l >= 0) s = l + W * k;
            }
            demand = demand || p.first_lane(v >= n1 && v < nodes && w[k] > 0) >= 0;
        }
        if (s < 0 || !demand) break;   // all shipped (what rounding of the two sums leaves is dropped)
        if (iters >= cap) { status = 1; break; }
        ++iters;

        // ---- Dijkstra from s on the reduced costs, to the first sink with demand
#pragma unroll UNR
        for (int k = 0; k < K; ++k) {
            const int v = lane + W * k;
            if (W == 1 && v >= nodes) break;
            key[k] = v == s ? (T)0 : INF; dfin[k] = INF; prev[k] = -1;
        }
        int t = -1;
        T dt = 0;
        for (int pop = 0; pop < nodes; ++pop) {
            T best = INF;
            int bv = 0;
#pragma unroll UNR
            for (int k = 0; k < K; ++k) {
                const int v = lane + W * k;
                if (W == 1 && v >= nodes) break;
                if (key[k] < best) { best = key[k]; bv = v; }
            }
            const T du = p.min_all(best);
            if (!(du < INF)) break;
            const int ul = p.first_lane(best == du);
            int bvs[1] = {bv};
            const int u = W == 1 ? bv : p.get(bvs, ul);
            const T wu = p.get(w, u);
            if (u >= n1 && wu > 0) { t = u; dt = du; }
            const T eu = p.get(eta, u), pu = p.get(phi, u), piu = p.get(pi, u);
            const bool u_src = u < n1, u_slack = u == slack_a || u == slack_b;
            const T* Fu = F + (u_src ? u : (u - n1) * n1);   // a source's flows at stride n1, a sink's contiguous
#pragma unroll UNR
            for (int k = 0; k < K; ++k) {
                const int v = lane + W * k;
                if (W == 1 && v >= nodes) break;
                if (v == u) { dfin[k] = key[k]; key[k] = INF; continue; }
                if (t >= 0 || v >= nodes || dfin[k] < INF || v == dead_a || v == dead_b || (v < n1) == u_src) continue;
                const T c = (u_slack || v == slack_a || v == slack_b) ? (T)1 : emd_theta(eu, pu, eta[k], phi[k], inv_r);
                T rc;
                if (u_src) {
                    rc = c + piu - pi[k];
                } else {
                    if (!(Fu[v] > 0)) continue;
                    rc = piu - pi[k] - c;
                }
                const T nd = du + (rc < 0 ? (T)0 : rc);   // (a NaN cost stays NaN and relaxes nothing)
                if (nd < key[k]) { key[k] = nd; prev[k] = u; }
            }
            if (t >= 0) break;
        }
        if (t < 0) { status = 2; break; }
#pragma unroll UNR
        for (int k = 0; k < K; ++k) {
            if (W == 1 && lane + W * k >= nodes) break;
            if (dfin[k] < INF) pi[k] += dfin[k] - dt;
        }

        // ---- the path t <- source <- sink <- ... <- s: its bottleneck, then the update
        T delta = p.get(w, t);
        {
            const T ws = p.get(w, s);
            delta = ws < delta ? ws : delta;
        }
        int cur = t;
        for (int hop = 0; hop < nodes; ++hop) {
            const int u = p.get(prev, cur);
            if (u == s || u < 0) break;
            const int j = p.get(prev, u);
            if (j < n1) break;
            const T f = F[(j - n1) * n1 + u];
            delta = f < delta ? f : delta;
            cur = j;
        }
        cur = t;
        for (int hop = 0; hop < nodes; ++hop) {
            const int u = p.get(prev, cur);
            if (u < 0) break;
            if (lane == 0) F[(cur - n1) * n1 + u] += delta;
            if (u == s) break;
            const int j = p.get(prev, u);
            if (j < n1) break;
            if (lane == 0) F[(j - n1) * n1 + u] -= delta;
            cur = j;
        }
#pragma unroll UNR
        for (int k = 0; k < K; ++k) {
            const int v = lane + W * k;
            if (W == 1 && v >= nodes) break;
            if (v == s || v == t) w[k] -= delta;
        }
        p.sync();
    }

    if (status != 0) {
        // what is left goes source by source to the sinks in index order: feasible, an upper bound
        int i = 0, j = n1;
        for (int step = 0; step < 2 * nodes && i < n1 && j < nodes; ++step) {
            const T wi = p.get(w, i), wj = p.get(w, j);
            if (!(wi > 0)) { ++i; continue; }
            if (!(wj > 0)) { ++j; continue; }
            const T m = wi < wj ? wi : wj;
            if (lane == 0) F[(j - n1) * n1 + i] += m;
#pragma unroll UNR
            for (int k = 0; k < K; ++k) {
                const int v = lane + W * k;
                if (W == 1 && v >= nodes) break;
                if (v == i || v == j) w[k] -= m;
            }
        }
        p.sync();
    }

    // ---- objective: flows times costs, lane-strided then one fixed butterfly
    T obj = 0;
    for (int idx = lane; idx < n1 * n2; idx += W) {
        const T f = F[idx];
        if (f > 0) {
            const int i = idx % n1, j = n1 + idx / n1;
            const T c = (i == slack_a || j == slack_b) ? (T)1 : emd_theta(s_eta[i], s_phi[i], s_eta[j], s_phi[j], inv_r);
            obj += f * c;
        }
    }
    return p.sum_all(obj);
}

// ---------------------------------------------------------------------------------------------------- GPU
template <int K>
__global__ __launch_bounds__(256) void jet_emd_kernel(const float* __restrict__ a, int ld_jet_a, const float* __restrict__ b,
                                                      int ld_jet_b, int ld_part, int na, int nb, int N, float inv_r, int cap,
                                                      int stride, float* __restrict__ out, int* __restrict__ status) {
    extern __shared__ __align__(16) float emd_lds[];
    const int wave = threadIdx.x >> 6;
    const long long pair = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
    if (pair >= (long long)na * nb) return;   // whole waves leave: the 64 lanes of a working wave stay together
    const int i = (int)(pair / nb), j = (int)(pair % nb);
    WaveLanes<float> p;
    int st, it;
    const float r = emd_solve<WaveLanes<float>, float, K>(p, a + (size_t)i * ld_jet_a, b + (size_t)j * ld_jet_b, ld_part, N, inv_r,
                                                          cap, emd_lds + (size_t)wave * stride, st, it);
    if (p.lane() == 0) {
        out[pair] = r;
        if (status != nullptr) status[pair] = st;
    }
}

int emd_check(const float* a, int ld_jet_a, const float* b, int ld_jet_b, int ld_part, int na, int nb, int N, float R,
              const void* out) {
    if (na < 1 || nb < 1 || N < 1 || N > MPG_JET_OBS_MAX_N || ld_part < 3 || !(R > 0.f) ||
        (long long)na * nb > 0x7fffffffLL) return -1;
    const long long need = (long long)(N - 1) * ld_part + 3;
    if ((long long)ld_jet_a < need || (long long)ld_jet_b < need) return -1;
    if (a == nullptr || b == nullptr || out == nullptr) return -2;
    return 0;
}

// ---------------------------------------------------------------------------------------------------- host
int emd_host_run(const float* a, int ld_jet_a, const float* b, int ld_jet_b, int ld_part, int na, int nb, int N, float R,
                 double* out, int* status, int* iters, int threads) {
    const int bad = emd_check(a, ld_jet_a, b, ld_jet_b, ld_part, na, nb, N, R, out);
    if (bad) return bad;
    const int total = na * nb, cap = emd_cap(N);
    const int nt = std::max(1, std::min({threads, 16, total}));
    std::atomic<int> next{0};
    auto work = [&]() {
        std::vector<double> mem((size_t)emd_scratch(N));
        HostLanes<double> p;
        for (;;) {
            const int pair = next.fetch_add(1, std::memory_order_relaxed);
            if (pair >= total) break;
            int st, it;
            out[pair] = emd_solve<HostLanes<double>, double, kEmdMaxNodes>(
                p, a + (size_t)(pair / nb) * ld_jet_a, b + (size_t)(pair % nb) * ld_jet_b, ld_part, N, 1.0 / (double)R, cap,
                mem.data(), st, it);
            if (status != nullptr) status[pair] = st;
            if (iters != nullptr) iters[pair] = it;
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
    return 0;
}

}  // namespace

extern "C" int mpg_jet_emd(const float* a, int ld_jet_a, const float* b, int ld_jet_b, int ld_part, int na, int nb, int N,
                           float R, float* out, int* status, void* stream) {
    const int bad = emd_check(a, ld_jet_a, b, ld_jet_b, ld_part, na, nb, N, R, out);
    if (bad) return bad;
    const int stride = (emd_scratch(N) + 3) & ~3, bytes1 = stride * (int)sizeof(float);
    const int wpb = std::max(1, std::min(4, 65536 / bytes1));
    const int lds = wpb * bytes1, cap = emd_cap(N), nodes = emd_ldn(N);
    const long long pairs = (long long)na * nb;
    const dim3 grid((unsigned)((pairs + wpb - 1) / wpb)), block(64 * wpb);
    const float inv_r = 1.f / R;
    hipStream_t st = (hipStream_t)stream;
    if (nodes <= 64) {
        hipLaunchKernelGGL(jet_emd_kernel<1>, grid, block, lds, st, a, ld_jet_a, b, ld_jet_b, ld_part, na, nb, N, inv_r, cap, stride, out, status);
    } else if (nodes <= 128) {
        hipLaunchKernelGGL(jet_emd_kernel<2>, grid, block, lds, st, a, ld_jet_a, b, ld_jet_b, ld_part, na, nb, N, inv_r, cap, stride, out, status);
    } else {
        static_assert(6 * 64 >= kEmdMaxNodes, "six slots per lane hold every node");
        return mpg_go<jet_emd_kernel<6>>(grid, block, lds, st, a, ld_jet_a, b, ld_jet_b, ld_part, na, nb, N, inv_r, cap, stride, out, status);
    }
    return (int)hipGetLastError();
}

extern "C" int mpg_jet_emd_host(const float* a, int ld_jet_a, const float* b, int ld_jet_b, int ld_part, int na, int nb, int N,
                                float R, double* out, int* status, int threads) {
    return emd_host_run(a, ld_jet_a, b, ld_jet_b, ld_part, na, nb, N, R, out, status, nullptr, threads);
}

extern "C" int mpg_jet_emd_host_iters(const float* a, int ld_jet_a, const float* b, int ld_jet_b, int ld_part, int na, int nb,
                                      int N, float R, double* out, int* status, int* iters, int threads) {
    return emd_host_run(a, ld_jet_a, b, ld_jet_b, ld_part, na, nb, N, R, out, status, iters, threads);
}
