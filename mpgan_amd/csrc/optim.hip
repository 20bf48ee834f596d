// Fused optimiser steps over one flat parameter buffer (one launch per network per step).
//
// Replace torch.optim.{RMSprop, Adam, Adadelta}(...).step() as the reference configures them
// (setup_training.py:1511-1523):
//   rmsprop  (default)  lr only: alpha = 0.99, eps = 1e-8, no momentum, not centered, no weight decay
//                       v = alpha v + (1 - alpha) g^2 ;  p -= lr * g / (sqrt(v) + eps)
//   adam                lr, betas = (beta1, beta2), weight_decay = 5e-4 (L2, added to the gradient), eps = 1e-8
//                       m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
//   adadelta            lr, rho = 0.9, eps = 1e-6
//                       v = rho v + (1-rho) g^2 ; d = sqrt(u + eps)/sqrt(v + eps) * g ; u = rho u + (1-rho) d^2 ; p -= lr d
// `gscale` multiplies the gradient first (1/world_size after a summing all-reduce).  Adam's step count lives in
// device memory (a captured hipGraph must see it advance on every replay).  `zero_grad` != 0: the gradient buffer is
// cleared behind its last use (the next backward accumulates into zeros: optimizer.zero_grad() of train.py:419 / :494
// without a launch of its own).
//
// The averaged form (mpg_*_ema; the rule is stated in include/mpgan_amd.h): the same loops with the exponential moving average
// of the parameters as two more memory streams -- the new parameter value is in a register when it is stored.  The kernels are
// templates on a bool; the instantiation without the average reads and writes what it always did.  The average's step word t
// is read by every workgroup at the top and moved on by the workgroup that arrives last on the ticket beside it
// (last_arrival, csrc/draws.h -- the loader's cursor moves the same way): no workgroup of the launch can still be about to read
// the old value when the new one is written, and there is no launch for it.  ema_coef / ema_fold are one body for the device and
// for mpg_ema_update_host.
#include "draws.h"

// What a launch at step word t does with every element: `track` (t < start: the average follows the weights) or the fold with
// om = 1 - beta_t.  Every operation is one fp32 operation rounded to nearest even, and none is contracted: the bodies are plain
// operators under `fp contract(off)`, the same text for the device and the host.  (Not __fsub_rn / __fmul_rn / __fadd_rn: the
// compiler's headers define them as the plain operators, compiled under the header's own contraction setting, and inlined here
// the multiply and the sum came out as one v_fmac_f32.  The quotient is __fdiv_rn's on the device, as in csrc/ada.hip: correctly
// rounded whatever the build's division flags.)
struct EmaCoef { bool track; float om; };

MPG_HD float ema_div(float a, float b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

MPG_HD EmaCoef ema_coef(uint32_t t, float beta, int start, int warmup) {
#pragma clang fp contract(off)
    if (t < (uint32_t)start) return {true, 0.f};
    float beta_t = beta;
    if (warmup) {
        const uint32_t since = t - (uint32_t)start;
        const float k = (float)(since < (1u << 24) ? since : (1u << 24));     // (exact: an integer <= 2^24)
        const float num = 1.f + k, den = 10.f + k;
        const float ramp = ema_div(num, den);
        beta_t = ramp < beta ? ramp : beta;
    }
    const float om = 1.f - beta_t;
    return {false, om};
}

MPG_HD float ema_fold(EmaCoef c, float e, float p_new) {
#pragma clang fp contract(off)
    if (c.track) return p_new;
    const float d = p_new - e;
    const float m = c.om * d;
    return e + m;
}

namespace {
// the head and the tail of an averaged launch: every workgroup reads t first and arrives last
template <bool EMA>
MPG_DEV EmaCoef ema_begin(const MpgEma& a, uint32_t& t) {
    if constexpr (!EMA) return {true, 0.f};
    t = __hip_atomic_load(a.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return ema_coef(t, a.beta, a.start, a.warmup);
}
template <bool EMA>
MPG_DEV void ema_end(const MpgEma& a, uint32_t t) {
    if constexpr (EMA) {
        // (behind the barrier every lane of the workgroup has used t: its stores to the average carry values made from it)
        __syncthreads();
        if (threadIdx.x == 0 && last_arrival(a.state + 1)) {
            __hip_atomic_store(a.state + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.state, t + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The controlled launches (mpg_*_ctl): lr and gscale are what mpg_step_control (csrc/step_control.hip) left in out[0] / out[1],
// read once, here; the arguments of the same names are not looked at.  A third template parameter: the instantiations without it
// read and write what they always did.
template <bool CTL>
MPG_DEV void ctl_read(const float* __restrict__ ctl_out, float& lr, float& gscale) {
    if constexpr (CTL) {
        lr = ctl_out[0];
        gscale = ctl_out[1];
    }
}

template <bool EMA, bool CTL>
__global__ void rmsprop_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ v, size_t n,
                               float lr, float alpha, float eps, float gscale, int zero_grad, uint64_t* __restrict__ counter, uint64_t counter_add,
                               MpgEma ema, const float* __restrict__ ctl_out) {
    ctl_read<CTL>(ctl_out, lr, gscale);
    if (counter != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *counter += counter_add;
    uint32_t t = 0;
    const EmaCoef ec = ema_begin<EMA>(ema, t);
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const float gi = g[i] * gscale;
        const float vi = alpha * v[i] + (1.f - alpha) * gi * gi;
        v[i] = vi;
        const float pn = p[i] - lr * gi / (sqrtf(vi) + eps);
        p[i] = pn;
        if constexpr (EMA) ema.ema[i] = ema_fold(ec, ema.ema[i], pn);
        if (zero_grad) g[i] = 0.f;
    }
    ema_end<EMA>(ema, t);
}

template <bool EMA, bool CTL>
__global__ void adam_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            const float* __restrict__ step, size_t n, float lr, float b1, float b2, float eps, float wd,
                            float gscale, int zero_grad, uint64_t* __restrict__ counter, uint64_t counter_add, MpgEma ema,
                            const float* __restrict__ ctl_out) {
    ctl_read<CTL>(ctl_out, lr, gscale);
    if (counter != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *counter += counter_add;
    uint32_t te = 0;
    const EmaCoef ec = ema_begin<EMA>(ema, te);
    const float t = *step + 1.f;
    const float bc1 = 1.f - powf(b1, t), bc2s = sqrtf(1.f - powf(b2, t));
    const float step_size = lr / bc1;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const float pi = p[i];
        const float gi = g[i] * gscale + wd * pi;
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        const float pn = pi - step_size * mi / (sqrtf(vi) / bc2s + eps);
        p[i] = pn;
        if constexpr (EMA) ema.ema[i] = ema_fold(ec, ema.ema[i], pn);
        if (zero_grad) g[i] = 0.f;
    }
    ema_end<EMA>(ema, te);
}
__global__ void step_inc_kernel(float* step) { *step += 1.f; }

template <bool EMA, bool CTL>
__global__ void adadelta_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ v, float* __restrict__ u,
                                size_t n, float lr, float rho, float eps, float gscale, int zero_grad, uint64_t* __restrict__ counter, uint64_t counter_add,
                                MpgEma ema, const float* __restrict__ ctl_out) {
    ctl_read<CTL>(ctl_out, lr, gscale);
    if (counter != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *counter += counter_add;
    uint32_t t = 0;
    const EmaCoef ec = ema_begin<EMA>(ema, t);
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const float gi = g[i] * gscale;
        const float vi = rho * v[i] + (1.f - rho) * gi * gi;
        const float d = sqrtf(u[i] + eps) / sqrtf(vi + eps) * gi;
        v[i] = vi;
        u[i] = rho * u[i] + (1.f - rho) * d * d;
        const float pn = p[i] - lr * d;
        p[i] = pn;
        if constexpr (EMA) ema.ema[i] = ema_fold(ec, ema.ema[i], pn);
        if (zero_grad) g[i] = 0.f;
    }
    ema_end<EMA>(ema, t);
}

// out[i] = mean + std * z_i, z ~ N(0, 1): counter-based (two hashes of (seed, tag, pair index) -> Box-Muller, one pair of
// values per thread), so a captured hipGraph draws fresh values on every replay from the device-resident seed alone
__global__ void normal_kernel(float* __restrict__ out, size_t n, const uint64_t* __restrict__ seed, uint32_t tag, float mean, float std) {
    const SeedWords s = seed_words(seed);
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x, npair = (n + 1) / 2;
    for (; i < npair; i += stride) {
        const NormalPair z = normal_pair(s, tag, i, std);
        out[2 * i] = mean + z.r * z.cs;
        if (2 * i + 1 < n) out[2 * i + 1] = mean + z.r * z.sn;
    }
}

// The generator's input noise AND its jets' masks (mask_c, mpgan/model.py:689-699: the n = int(label N) particles with the
// smallest first noise feature) in one launch: the ranking reads nothing but the noise just drawn.  One workgroup per jet;
// the values are mpg_normal's (same pair indices over the flat [B, N, L] tensor), the mask mpg_rank_mask's.
__global__ __launch_bounds__(256) void normal_rank_mask_kernel(float* __restrict__ out, int N, int L, const uint64_t* __restrict__ seed,
                                                               uint32_t tag, float mean, float std, const float* __restrict__ labels,
                                                               int ld_lab, float* __restrict__ mask, float* __restrict__ ignore) {
    extern __shared__ float first[];   // [N]: the first feature of every particle
    const SeedWords s = seed_words(seed);
    const int b = blockIdx.x;
    const size_t per_jet = (size_t)N * L, pair0 = (size_t)b * per_jet / 2, npair = per_jet / 2;   // (N L even: checked by the launcher)
    for (size_t q = threadIdx.x; q < npair; q += blockDim.x) {
        const size_t i = pair0 + q;
        const NormalPair z = normal_pair(s, tag, i, std);
        const float v0 = mean + z.r * z.cs, v1 = mean + z.r * z.sn;
        out[2 * i] = v0;
        out[2 * i + 1] = v1;
        const size_t e0 = 2 * q;                       // element index within the jet
        if (e0 % L == 0) first[e0 / L] = v0;
        if ((e0 + 1) % L == 0) first[(e0 + 1) / L] = v1;   // (L == 1 only)
    }
    __syncthreads();
    const int n_minus_1 = (int)(labels[(size_t)b * ld_lab] * (float)N) - 1;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        const float xi = first[i];
        int rank = 0;
        for (int j = 0; j < N; ++j) {
            const float xj = first[j];
            rank += (xj < xi) || (xj == xi && j < i);
        }
        mask[(size_t)b * N + i] = rank <= n_minus_1 ? 1.f : 0.f;
        if (ignore != nullptr) ignore[(size_t)b * N + i] = rank <= n_minus_1 ? 0.f : 1.f;
    }
}

inline int nblocks(uint64_t n) { return (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048); }
// The averaged launches: at most one workgroup per CU of an MI355X.  Every workgroup arrives once on the ticket, the arrivals on
// one word are served one after the other, and the launch ends with the last: over G's 361 123 parameters (1411 workgroups under
// nblocks) the launch took 19.2 us against 4.1 us without the average, 9.2 us capped at 512 workgroups, 7.0 us at 256 or 128,
// 9.1 us at 64 (too few waves for the loop's loads).  The elements' arithmetic does not depend on the grid.
constexpr int EMA_MAX_BLOCKS = 256;
template <bool EMA>
inline int nblocks_for(uint64_t n) { return EMA && nblocks(n) > EMA_MAX_BLOCKS ? EMA_MAX_BLOCKS : nblocks(n); }

// an MpgEma block the averaged entry points take (n: the launch's element count)
bool ema_args_ok(const MpgEma* a, uint64_t n) {
    if (a == nullptr || a->ema == nullptr || a->state == nullptr || n == 0) return false;
    return a->beta >= 0.f && a->beta < 1.f && a->start >= 0;      // (a NaN fails both comparisons)
}

template <bool EMA, bool CTL = false>
int rmsprop_launch(float* p, float* g, float* v, uint64_t n, float lr, float alpha, float eps, float gscale, int zero_grad,
                   uint64_t* counter, uint64_t counter_add, const MpgEma& ema, void* stream, const float* ctl_out = nullptr) {
    hipLaunchKernelGGL((rmsprop_kernel<EMA, CTL>), dim3(nblocks_for<EMA>(n)), dim3(256), 0, (hipStream_t)stream, p, g, v, (size_t)n, lr,
                       alpha, eps, gscale, zero_grad, counter, counter_add, ema, ctl_out);
    return (int)hipGetLastError();
}

template <bool EMA, bool CTL = false>
int adam_launch(float* p, float* g, float* m, float* v, float* step, uint64_t n, float lr, float beta1, float beta2, float eps,
                float weight_decay, float gscale, int zero_grad, uint64_t* counter, uint64_t counter_add, const MpgEma& ema, void* stream,
                const float* ctl_out = nullptr) {
    hipLaunchKernelGGL((adam_kernel<EMA, CTL>), dim3(nblocks_for<EMA>(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, step, (size_t)n,
                       lr, beta1, beta2, eps, weight_decay, gscale, zero_grad, counter, counter_add, ema, ctl_out);
    hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step);
    return (int)hipGetLastError();
}

template <bool EMA, bool CTL = false>
int adadelta_launch(float* p, float* g, float* v, float* u, uint64_t n, float lr, float rho, float eps, float gscale, int zero_grad,
                    uint64_t* counter, uint64_t counter_add, const MpgEma& ema, void* stream, const float* ctl_out = nullptr) {
    hipLaunchKernelGGL((adadelta_kernel<EMA, CTL>), dim3(nblocks_for<EMA>(n)), dim3(256), 0, (hipStream_t)stream, p, g, v, u, (size_t)n,
                       lr, rho, eps, gscale, zero_grad, counter, counter_add, ema, ctl_out);
    return (int)hipGetLastError();
}

// what a controlled entry point needs of its blocks: the words mpg_step_control wrote; a NULL ema is the launch without the average
bool ctl_args_ok(const MpgStepCtl* ctl, const MpgEma* ema, uint64_t n) {
    return ctl != nullptr && ctl->out != nullptr && n != 0 && (ema == nullptr || ema_args_ok(ema, n));
}
}  // namespace

extern "C" int mpg_rmsprop(float* p, float* g, float* v, uint64_t n, float lr, float alpha, float eps,
                           float gscale, int zero_grad, uint64_t* counter, uint64_t counter_add, void* stream) {
    if (n == 0) return counter != nullptr ? -1 : 0;
    return rmsprop_launch<false>(p, g, v, n, lr, alpha, eps, gscale, zero_grad, counter, counter_add, MpgEma{}, stream);
}

extern "C" int mpg_rmsprop_ema(float* p, float* g, float* v, uint64_t n, float lr, float alpha, float eps,
                               float gscale, int zero_grad, uint64_t* counter, uint64_t counter_add, const MpgEma* ema, void* stream) {
    if (!ema_args_ok(ema, n)) return -1;
    return rmsprop_launch<true>(p, g, v, n, lr, alpha, eps, gscale, zero_grad, counter, counter_add, *ema, stream);
}

extern "C" int mpg_adam(float* p, float* g, float* m, float* v, float* step, uint64_t n, float lr, float beta1,
                        float beta2, float eps, float weight_decay, float gscale, int zero_grad, uint64_t* counter, uint64_t counter_add,
                        void* stream) {
    if (n == 0) return counter != nullptr ? -1 : 0;
    if (step == nullptr) return -1;
    return adam_launch<false>(p, g, m, v, step, n, lr, beta1, beta2, eps, weight_decay, gscale, zero_grad, counter, counter_add,
                              MpgEma{}, stream);
}

extern "C" int mpg_adam_ema(float* p, float* g, float* m, float* v, float* step, uint64_t n, float lr, float beta1,
                            float beta2, float eps, float weight_decay, float gscale, int zero_grad, uint64_t* counter,
                            uint64_t counter_add, const MpgEma* ema, void* stream) {
    if (!ema_args_ok(ema, n) || step == nullptr) return -1;
    return adam_launch<true>(p, g, m, v, step, n, lr, beta1, beta2, eps, weight_decay, gscale, zero_grad, counter, counter_add,
                             *ema, stream);
}

extern "C" int mpg_adadelta(float* p, float* g, float* v, float* u, uint64_t n, float lr, float rho, float eps,
                            float gscale, int zero_grad, uint64_t* counter, uint64_t counter_add, void* stream) {
    if (n == 0) return counter != nullptr ? -1 : 0;
    return adadelta_launch<false>(p, g, v, u, n, lr, rho, eps, gscale, zero_grad, counter, counter_add, MpgEma{}, stream);
}

extern "C" int mpg_adadelta_ema(float* p, float* g, float* v, float* u, uint64_t n, float lr, float rho, float eps,
                                float gscale, int zero_grad, uint64_t* counter, uint64_t counter_add, const MpgEma* ema, void* stream) {
    if (!ema_args_ok(ema, n)) return -1;
    return adadelta_launch<true>(p, g, v, u, n, lr, rho, eps, gscale, zero_grad, counter, counter_add, *ema, stream);
}

extern "C" int mpg_rmsprop_ctl(float* p, float* g, float* v, uint64_t n, float lr, float alpha, float eps, float gscale, int zero_grad,
                               uint64_t* counter, uint64_t counter_add, const MpgStepCtl* ctl, const MpgEma* ema, void* stream) {
    if (!ctl_args_ok(ctl, ema, n)) return -1;
    if (ema != nullptr)
        return rmsprop_launch<true, true>(p, g, v, n, lr, alpha, eps, gscale, zero_grad, counter, counter_add, *ema, stream, ctl->out);
    return rmsprop_launch<false, true>(p, g, v, n, lr, alpha, eps, gscale, zero_grad, counter, counter_add, MpgEma{}, stream, ctl->out);
}

extern "C" int mpg_adam_ctl(float* p, float* g, float* m, float* v, float* step, uint64_t n, float lr, float beta1, float beta2, float eps,
                            float weight_decay, float gscale, int zero_grad, uint64_t* counter, uint64_t counter_add,
                            const MpgStepCtl* ctl, const MpgEma* ema, void* stream) {
    if (!ctl_args_ok(ctl, ema, n) || step == nullptr) return -1;
    if (ema != nullptr)
        return adam_launch<true, true>(p, g, m, v, step, n, lr, beta1, beta2, eps, weight_decay, gscale, zero_grad, counter, counter_add,
                                       *ema, stream, ctl->out);
    return adam_launch<false, true>(p, g, m, v, step, n, lr, beta1, beta2, eps, weight_decay, gscale, zero_grad, counter, counter_add,
                                    MpgEma{}, stream, ctl->out);
}

extern "C" int mpg_adadelta_ctl(float* p, float* g, float* v, float* u, uint64_t n, float lr, float rho, float eps, float gscale,
                                int zero_grad, uint64_t* counter, uint64_t counter_add, const MpgStepCtl* ctl, const MpgEma* ema,
                                void* stream) {
    if (!ctl_args_ok(ctl, ema, n)) return -1;
    if (ema != nullptr)
        return adadelta_launch<true, true>(p, g, v, u, n, lr, rho, eps, gscale, zero_grad, counter, counter_add, *ema, stream,
                                           ctl->out);
    return adadelta_launch<false, true>(p, g, v, u, n, lr, rho, eps, gscale, zero_grad, counter, counter_add, MpgEma{}, stream,
                                        ctl->out);
}

extern "C" int mpg_ema_update_host(float* e, const float* p_new, uint64_t n, uint32_t t, float beta, int start, int warmup) {
    if (e == nullptr || p_new == nullptr || n == 0 || !(beta >= 0.f && beta < 1.f) || start < 0) return -1;
    const EmaCoef c = ema_coef(t, beta, start, warmup);
    for (uint64_t i = 0; i < n; ++i) e[i] = ema_fold(c, e[i], p_new[i]);
    return 0;
}

extern "C" int mpg_normal(float* out, uint64_t n, const uint64_t* seed, uint32_t tag, float mean, float std, void* stream) {
    if (n == 0) return 0;
    if (seed == nullptr || !(std >= 0.f)) return -1;
    hipLaunchKernelGGL(normal_kernel, dim3(nblocks((n + 1) / 2)), dim3(256), 0, (hipStream_t)stream, out, (size_t)n, seed, tag, mean, std);
    return (int)hipGetLastError();
}

extern "C" int mpg_normal_rank_mask(float* out, int B, int N, int L, const uint64_t* seed, uint32_t tag, float mean, float std,
                                    const float* labels, int ld_lab, float* mask, float* ignore, void* stream) {
    if (B <= 0 || N <= 0 || L <= 0 || N > 8192 || ((size_t)N * L) % 2) return -1;
    if (seed == nullptr || labels == nullptr || mask == nullptr || !(std >= 0.f)) return -1;
    hipLaunchKernelGGL(normal_rank_mask_kernel, dim3(B), dim3(256), N * sizeof(float), (hipStream_t)stream, out, N, L, seed, tag, mean,
                       std, labels, ld_lab, mask, ignore);
    return (int)hipGetLastError();
}
