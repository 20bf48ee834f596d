// Spectral normalisation of Linear layers (the reference's mpgan/spectral_normalization.py:29-46) as ONE grouped launch per set of
// layers: power iteration, sigma and the normalised weight W_eff = W_bar / sigma, and -- for the backward -- the gradient with
// respect to W_bar with u and v held constant.  include/mpgan_amd.h states the arithmetic; this file is its one body: sn_forward
// and sn_backward are written against a "team" (its lanes, its waves, a barrier, a sum over the team) and are instantiated for a
// workgroup of 1024 threads (SnDevTeam) and for one host thread (SnHostTeam: mpg_spectral_norm_host / mpg_spectral_norm_bwd_host).
//
// One workgroup per job.  W stays in global memory (256 x 256 fp32 is 256 KiB: it is read from L2 on every pass after the first);
// the vectors are worked on in the job's own u_out / v_out, so R and C are bounded by nothing.  Every access is a scalar fp32 load
// or store: W is a view into a flat parameter buffer and starts wherever the parameters before it end.
//   t = W^T u   a wave per row, a lane per column (64 columns at a time): coalesced; the waves' partial columns meet in LDS and
//               wave 0 adds them in wave order
//   s = W v     a wave per row, lanes strided over the columns, added by shuffles
// Every sum has a fixed order -- a lane's strided partial, shuffles within the wave, the waves' words in LDS added in wave order --
// so two runs from the same inputs agree bit for bit.  No atomics.
// The old u is consumed by the first W^T u, into v_out; the parameters' own u and v are stored last, behind the barriers of
// everything that read them.
#include "common.h"
#include "../../include/mpgan_amd.h"

namespace {

constexpr int SN_THREADS = 1024, SN_WAVES = SN_THREADS / 64;
constexpr float SN_EPS = 1e-12f;
// A thread's loads of one round are all issued before any of its stores: the compiler may not move a load across a store that
// could alias it (W_eff against W, dW against G), and a loop of load -> store -> load pays one trip to L2 per element.
constexpr int SN_RB = 4;   // rows of W a wave takes through ONE sweep of the columns (forward products)
constexpr int SN_EB = 8;   // elements per thread and round (element-wise passes), rows per wave and round (backward)

struct SnDevTeam {
    static constexpr int LW = 64, NW = SN_WAVES;
    int tid, lane, wave;
    float* part;   // LDS [NW * LW]
    float* red;    // LDS [NW]
    __device__ void sync() const { __syncthreads(); }
    __device__ float wave_sum(float x) const {   // (lane 0 holds the sum)
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
        return x;
    }
    __device__ float team_sum(float x) const {   // (every thread gets the sum)
        x = wave_sum(x);
        if (lane == 0) red[wave] = x;
        __syncthreads();
        float s = 0.f;
        for (int w = 0; w < NW; ++w) s += red[w];
        __syncthreads();
        return s;
    }
};

struct SnHostTeam {
    static constexpr int LW = 1, NW = 1;
    int tid = 0, lane = 0, wave = 0;
    float part_[1], red_[1];
    float* part = part_;
    MPG_HD void sync() const {}
    MPG_HD float wave_sum(float x) const { return x; }
    MPG_HD float team_sum(float x) const { return x; }
};

// t[c] = sum_r W[r, c] u[r]
template <class T>
MPG_HD void sn_matvec_t(const T& tm, const float* W, int R, int C, const float* u, float* t) {
    for (int c0 = 0; c0 < C; c0 += T::LW) {
        const int c = c0 + tm.lane;
        float acc = 0.f;
        if (c < C) {
#pragma unroll 8
            for (int r = tm.wave; r < R; r += T::NW) acc += W[(size_t)r * C + c] * u[r];
        }
        tm.part[tm.wave * T::LW + tm.lane] = acc;
        tm.sync();
        if (tm.wave == 0 && c < C) {
            float s = 0.f;
            for (int w = 0; w < T::NW; ++w) s += tm.part[w * T::LW + tm.lane];
            t[c] = s;
        }
        tm.sync();
    }
}

// SN_RB rows of W times v -- rows r0, r0 + NW, ... (those below R) -- in one sweep of the columns, so that the rows' loads are in
// flight together; lane 0 of the wave holds d[k].  Per row the sum runs as for one row alone: a lane's columns in order, then the shuffles.
template <class T>
MPG_HD void sn_row_dots(const T& tm, const float* W, int R, int C, int r0, const float* v, float* d) {
    float acc[SN_RB];
#pragma unroll
    for (int k = 0; k < SN_RB; ++k) acc[k] = 0.f;
    for (int c = tm.lane; c < C; c += T::LW) {
        const float vc = v[c];
#pragma unroll
        for (int k = 0; k < SN_RB; ++k) {
            const int r = r0 + k * T::NW;
            if (r < R) acc[k] += W[(size_t)r * C + c] * vc;
        }
    }
#pragma unroll
    for (int k = 0; k < SN_RB; ++k) d[k] = tm.wave_sum(acc[k]);
}

template <class T>
MPG_HD float sn_sumsq(const T& tm, const float* x, int n) {
    float acc = 0.f;
    for (int i = tm.tid; i < n; i += T::LW * T::NW) acc += x[i] * x[i];
    return tm.team_sum(acc);
}

template <class T>
MPG_HD void sn_forward(const T& tm, const MpgSpectralJob& J, int P) {
    constexpr int NT = T::LW * T::NW;
    const int R = J.R, C = J.C;
    const float* W = J.W;
    float *uo = J.u_out, *vo = J.v_out;
    for (int i = tm.tid; i < R; i += NT) uo[i] = J.u[i];
    for (int i = tm.tid; i < C; i += NT) vo[i] = J.v[i];
    tm.sync();
    float sigma = 0.f;
    if (P < 1) {   // sigma = u . (W v) on the vectors as they stand
        float acc = 0.f;
        for (int r0 = tm.wave; r0 < R; r0 += T::NW * SN_RB) {
            float d[SN_RB];
            sn_row_dots(tm, W, R, C, r0, vo, d);
            if (tm.lane == 0) {
#pragma unroll
                for (int k = 0; k < SN_RB; ++k)
                    if (r0 + k * T::NW < R) acc += uo[r0 + k * T::NW] * d[k];
            }
        }
        sigma = tm.team_sum(acc);
    }
    for (int p = 0; p < P; ++p) {
        sn_matvec_t(tm, W, R, C, uo, vo);                     // t = W^T u
        const float nt = sqrtf(sn_sumsq(tm, vo, C)) + SN_EPS;
        for (int i = tm.tid; i < C; i += NT) vo[i] = vo[i] / nt;
        tm.sync();
        for (int r0 = tm.wave; r0 < R; r0 += T::NW * SN_RB) {   // s = W v
            float d[SN_RB];
            sn_row_dots(tm, W, R, C, r0, vo, d);
            if (tm.lane == 0) {
#pragma unroll
                for (int k = 0; k < SN_RB; ++k)
                    if (r0 + k * T::NW < R) uo[r0 + k * T::NW] = d[k];
            }
        }
        tm.sync();
        const float ns = sqrtf(sn_sumsq(tm, uo, R)) + SN_EPS;
        float acc = 0.f;                                      // u . s, s the product just formed
        for (int i = tm.tid; i < R; i += NT) {
            const float s = uo[i], un = s / ns;
            acc += un * s;
            uo[i] = un;
        }
        sigma = tm.team_sum(acc);                             // (its barriers order the stores above before the next pass)
    }
    const float inv = 1.0f / (sigma + SN_EPS);
    const size_t n = (size_t)R * C;
    for (size_t i0 = tm.tid; i0 < n; i0 += (size_t)NT * SN_EB) {
        float w[SN_EB];
#pragma unroll
        for (int k = 0; k < SN_EB; ++k) w[k] = i0 + (size_t)k * NT < n ? W[i0 + (size_t)k * NT] : 0.f;
#pragma unroll
        for (int k = 0; k < SN_EB; ++k)
            if (i0 + (size_t)k * NT < n) J.W_eff[i0 + (size_t)k * NT] = w[k] * inv;
    }
    if (tm.tid == 0) *J.inv_sigma = inv;
    if (P >= 1) {   // the parameters' own vectors, at their own addresses: every read of the old ones lies behind a barrier
        for (int i = tm.tid; i < R; i += NT) J.u[i] = uo[i];
        for (int i = tm.tid; i < C; i += NT) J.v[i] = vo[i];
    }
}

template <class T>
MPG_HD void sn_backward(const T& tm, const MpgSpectralBwdJob& J) {
    constexpr int NT = T::LW * T::NW;
    const int R = J.R, C = J.C;
    const size_t n = (size_t)R * C;
    float acc = 0.f;
#pragma unroll 8
    for (size_t i = tm.tid; i < n; i += NT) acc += J.G[i] * J.W_eff[i];
    const float inner = tm.team_sum(acc), inv = *J.inv_sigma;
    for (int r0 = tm.wave; r0 < R; r0 += T::NW * SN_EB) {      // SN_EB rows per wave and round: rows r0, r0 + NW, ...
        float iu[SN_EB];
#pragma unroll
        for (int k = 0; k < SN_EB; ++k) iu[k] = r0 + k * T::NW < R ? inner * J.u[r0 + k * T::NW] : 0.f;
        for (int c = tm.lane; c < C; c += T::LW) {
            const float vc = J.v[c];
            float g[SN_EB], o[SN_EB];
#pragma unroll
            for (int k = 0; k < SN_EB; ++k) {
                const size_t i = (size_t)(r0 + k * T::NW) * C + c;
                const bool in = r0 + k * T::NW < R;
                g[k] = in ? J.G[i] : 0.f;
                o[k] = (in && J.accumulate) ? J.dW[i] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < SN_EB; ++k) {
                const float d = (g[k] - iu[k] * vc) * inv;
                if (r0 + k * T::NW < R) J.dW[(size_t)(r0 + k * T::NW) * C + c] = J.accumulate ? o[k] + d : d;
            }
        }
    }
}

struct SnJobs { MpgSpectralJob j[MPG_SPECTRAL_MAX_JOBS]; };
struct SnBwdJobs { MpgSpectralBwdJob j[MPG_SPECTRAL_MAX_JOBS]; };

__device__ SnDevTeam sn_team(float* part, float* red) {
    SnDevTeam tm;
    tm.tid = threadIdx.x;
    tm.lane = threadIdx.x & 63;
    tm.wave = threadIdx.x >> 6;
    tm.part = part;
    tm.red = red;
    return tm;
}

__global__ __launch_bounds__(SN_THREADS) void spectral_norm_kernel(const SnJobs jobs, int P) {
    __shared__ float part[SN_THREADS];
    __shared__ float red[SN_WAVES];
    sn_forward(sn_team(part, red), jobs.j[blockIdx.x], P);
}

__global__ __launch_bounds__(SN_THREADS) void spectral_norm_bwd_kernel(const SnBwdJobs jobs) {
    __shared__ float part[SN_THREADS];
    __shared__ float red[SN_WAVES];
    sn_backward(sn_team(part, red), jobs.j[blockIdx.x]);
}

// 0, or the argument error: -1 a NULL pointer, a size below 1, a negative iteration count or a job count outside
// [1, MPG_SPECTRAL_MAX_JOBS]; -2 two jobs that name the same u or the same v (two workgroups would iterate one state); -3 fresh
// outputs that are a job's own state (u_out == u, v_out == v).
int sn_args(const MpgSpectralJob* jobs, int njobs, int P) {
    if (jobs == nullptr || njobs < 1 || njobs > MPG_SPECTRAL_MAX_JOBS || P < 0) return -1;
    for (int q = 0; q < njobs; ++q) {
        const MpgSpectralJob& J = jobs[q];
        if (!J.W || !J.u || !J.v || !J.W_eff || !J.u_out || !J.v_out || !J.inv_sigma || J.R < 1 || J.C < 1) return -1;
        if (J.u_out == J.u || J.v_out == J.v) return -3;
        for (int p = 0; p < q; ++p)
            if (jobs[p].u == J.u || jobs[p].v == J.v) return -2;
    }
    return 0;
}

int sn_bwd_args(const MpgSpectralBwdJob* jobs, int njobs) {
    if (jobs == nullptr || njobs < 1 || njobs > MPG_SPECTRAL_MAX_JOBS) return -1;
    for (int q = 0; q < njobs; ++q) {
        const MpgSpectralBwdJob& J = jobs[q];
        if (!J.G || !J.W_eff || !J.u || !J.v || !J.inv_sigma || !J.dW || J.R < 1 || J.C < 1) return -1;
    }
    return 0;
}

}  // namespace

extern "C" int mpg_spectral_norm(const MpgSpectralJob* jobs, int njobs, int power_iterations, void* stream) {
    const int rc = sn_args(jobs, njobs, power_iterations);
    if (rc) return rc;
    SnJobs sj;
    for (int q = 0; q < njobs; ++q) sj.j[q] = jobs[q];
    hipLaunchKernelGGL(spectral_norm_kernel, dim3(njobs), dim3(SN_THREADS), 0, (hipStream_t)stream, sj, power_iterations);
    return (int)hipGetLastError();
}

extern "C" int mpg_spectral_norm_bwd(const MpgSpectralBwdJob* jobs, int njobs, void* stream) {
    const int rc = sn_bwd_args(jobs, njobs);
    if (rc) return rc;
    SnBwdJobs sj;
    for (int q = 0; q < njobs; ++q) sj.j[q] = jobs[q];
    hipLaunchKernelGGL(spectral_norm_bwd_kernel, dim3(njobs), dim3(SN_THREADS), 0, (hipStream_t)stream, sj);
    return (int)hipGetLastError();
}

extern "C" int mpg_spectral_norm_host(const MpgSpectralJob* jobs, int njobs, int power_iterations) {
    const int rc = sn_args(jobs, njobs, power_iterations);
    if (rc) return rc;
    for (int q = 0; q < njobs; ++q) sn_forward(SnHostTeam(), jobs[q], power_iterations);
    return 0;
}

extern "C" int mpg_spectral_norm_bwd_host(const MpgSpectralBwdJob* jobs, int njobs) {
    const int rc = sn_bwd_args(jobs, njobs);
    if (rc) return rc;
    for (int q = 0; q < njobs; ++q) sn_backward(SnHostTeam(), jobs[q]);
    return 0;
}
