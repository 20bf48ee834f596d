// The optimizer-step control: the learning-rate schedule and the gradient clipping of one network as ONE small launch in front of
// its optimizer launch, inside the captured iteration (the rule is stated in include/mpgan_amd.h).  The launch leaves
// out = {lr_eff, s, norm, factor} in device memory; the `_ctl` optimizer entry points (csrc/optim.hip) read lr = out[0] and
// gscale = out[1] at the top of their kernels, so neither is a constant of the hipGraph any more.
//
// The norm: at most 256 workgroups of 256 threads, a fixed function of n (step_blocks).  Every thread adds the squares of its
// strided elements in index order, in fp64; the workgroup adds its 256 sums in a fixed tree through LDS; thread 0 stores the
// workgroup's partial, releases it at agent scope and arrives on the ticket (last_arrival, csrc/draws.h).  The workgroup that
// arrives last acquires at agent scope -- every wave of it for its own loads -- reads the partials into LDS and thread 0 adds them
// in workgroup order: the same bits from every launch on the same buffer.  That thread then runs the rule's scalar part
// (step_rule: one body for the device and for mpg_step_control_host), writes out, moves t on and puts the ticket back to zero --
// the ordering of ema_end (csrc/optim.hip) and of mpg_batch_feed.  With no norm wanted the launch is one workgroup and reads no
// gradient.  mpg_step_control_host walks the same grid in the same order on host memory.
#include "draws.h"

constexpr int STEP_THREADS = 256, STEP_MAX_BLOCKS = 256;
constexpr uint32_t STEP_KNOT_MAX = 1u << 24;      // (knot steps convert to fp32 exactly up to here)

MPG_HD int step_blocks(uint64_t n) {
    const uint64_t b = (n + STEP_THREADS - 1) / STEP_THREADS;
    return b < 1 ? 1 : (b > STEP_MAX_BLOCKS ? STEP_MAX_BLOCKS : (int)b);
}

MPG_HD float step_div(float a, float b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __fdiv_rn(a, b);      // the correctly rounded quotient, whatever the build's division flags
#else
    return a / b;
#endif
}

// acc + (gscale * g)^2: the product in fp32 (one rounding), the square and the sum in fp64, nothing contracted
MPG_HD double step_sq_acc(double acc, float g, float gscale) {
#pragma clang fp contract(off)
    const float x = gscale * g;
    const double d = (double)x;
    const double q = d * d;
    return acc + q;
}

MPG_HD double step_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}

MPG_HD bool step_clips(float max_norm) { return max_norm > 0.f && max_norm <= 3.402823466e38f; }      // (not <= 0, not +inf, not a NaN)

// The rule's scalar part for the step about to be taken at step word t.  Every operation is one fp32 operation rounded to nearest
// even, none contracted (plain operators under `fp contract(off)`, as ema_coef: csrc/optim.hip says why not __fmul_rn).
struct StepRule { float lr_eff, s, factor, gmul; };

MPG_HD StepRule step_rule(uint32_t t, float base, int nknots, const uint32_t* knot_step, const float* knot_f, float gscale,
                          float max_norm, float norm) {
#pragma clang fp contract(off)
    float factor = 1.f;
    if (nknots > 0) {
        const int last = nknots - 1;
        if (t <= knot_step[0]) factor = knot_f[0];
        else if (t >= knot_step[last]) factor = knot_f[last];
        else {
            int k = 0;
            while (k + 1 < last && t >= knot_step[k + 1]) ++k;      // knot_step[k] <= t < knot_step[k + 1]
            const float num = (float)(t - knot_step[k]), den = (float)(knot_step[k + 1] - knot_step[k]);      // (exact: <= 2^24)
            const float w = step_div(num, den);
            const float d = knot_f[k + 1] - knot_f[k];
            const float m = w * d;
            factor = knot_f[k] + m;
        }
    }
    const float lr_eff = base * factor;
    float gmul = 1.f;
    if (step_clips(max_norm)) {
        const float den = norm + 1e-6f;
        const float q = step_div(max_norm, den);
        gmul = q > 1.f ? 1.f : q;      // min(1, q); a NaN stays one, as in torch's clamp
    }
    const float s = gscale * gmul;
    return {lr_eff, s, factor, gmul};
}

// what the one finishing thread writes: out, then t + 1 (stopping at 2^32 - 1); the caller stores the words
MPG_HD uint32_t step_finish(const MpgStepCtl& c, uint32_t t, float gscale, bool need_norm, double S) {
    const float norm = need_norm ? (float)sqrt(S) : 0.f;
    const StepRule r = step_rule(t, c.base[0], c.nknots, c.knot_step, c.knot_f, gscale, c.max_norm, norm);
    c.out[0] = r.lr_eff;
    c.out[1] = r.s;
    c.out[2] = norm;
    c.out[3] = r.factor;
    return t == 0xFFFFFFFFu ? t : t + 1u;
}

namespace {

__global__ __launch_bounds__(STEP_THREADS) void step_control_kernel(const float* __restrict__ g, size_t n, float gscale, MpgStepCtl c,
                                                                    int need_norm) {
    __shared__ double sh[STEP_THREADS];
    __shared__ int is_last;
    const int tid = threadIdx.x;
    if (need_norm) {
        double acc = 0.0;
        const size_t stride = (size_t)gridDim.x * STEP_THREADS;
        for (size_t i = (size_t)blockIdx.x * STEP_THREADS + tid; i < n; i += stride) acc = step_sq_acc(acc, g[i], gscale);
        sh[tid] = acc;
        __syncthreads();
        for (int s = STEP_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) sh[tid] = step_add(sh[tid], sh[tid + s]);
            __syncthreads();
        }
    }
    if (tid == 0) {
        if (need_norm) {
            c.partials[blockIdx.x] = sh[0];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");      // the partial has left this XCD before the arrival is seen
        }
        is_last = last_arrival(c.state + 1) ? 1 : 0;
    }
    __syncthreads();
    if (!is_last) return;
    // the workgroup that arrived last: every other workgroup's partial is released
    double S = 0.0;
    if (need_norm) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");          // (every wave, for the loads it makes itself)
        if (tid < (int)gridDim.x) sh[tid] = c.partials[tid];
        __syncthreads();
        if (tid == 0)
            for (int b = 0; b < (int)gridDim.x; ++b) S = step_add(S, sh[b]);
    }
    if (tid == 0) {
        const uint32_t t = __hip_atomic_load(c.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t t_next = step_finish(c, t, gscale, need_norm != 0, S);
        __hip_atomic_store(c.state + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(c.state, t_next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

bool finite_f(float v) { return v - v == 0.f; }

bool step_ctl_ok(const float* g, uint64_t n, float gscale, const MpgStepCtl* c) {
    if (c == nullptr || c->state == nullptr || c->base == nullptr || c->out == nullptr || c->partials == nullptr) return false;
    if (c->nknots < 0 || c->nknots > MPG_LR_KNOTS) return false;
    for (int k = 0; k < c->nknots; ++k) {
        if (c->knot_step[k] > STEP_KNOT_MAX || (k > 0 && c->knot_step[k] <= c->knot_step[k - 1])) return false;
        if (!finite_f(c->knot_f[k]) || !(c->knot_f[k] >= 0.f)) return false;
    }
    if (c->max_norm != c->max_norm || gscale != gscale) return false;
    const bool need_norm = c->want_norm != 0 || step_clips(c->max_norm);
    return !need_norm || (g != nullptr && n > 0);
}

}  // namespace

extern "C" int mpg_step_control(const float* g, uint64_t n, float gscale, const MpgStepCtl* ctl, void* stream) {
    if (!step_ctl_ok(g, n, gscale, ctl)) return -1;
    const int need_norm = ctl->want_norm != 0 || step_clips(ctl->max_norm);
    hipLaunchKernelGGL(step_control_kernel, dim3(need_norm ? step_blocks(n) : 1), dim3(STEP_THREADS), 0, (hipStream_t)stream, g,
                       (size_t)n, gscale, *ctl, need_norm);
    return (int)hipGetLastError();
}

extern "C" int mpg_step_control_host(const float* g, uint64_t n, float gscale, const MpgStepCtl* ctl) {
    if (!step_ctl_ok(g, n, gscale, ctl)) return -1;
    const bool need_norm = ctl->want_norm != 0 || step_clips(ctl->max_norm);
    double S = 0.0;
    if (need_norm) {
        const int nb = step_blocks(n);
        const uint64_t stride = (uint64_t)nb * STEP_THREADS;
        double sh[STEP_THREADS];
        for (int b = 0; b < nb; ++b) {      // the launch's grid, workgroup by workgroup
            for (int tid = 0; tid < STEP_THREADS; ++tid) {
                double acc = 0.0;
                for (uint64_t i = (uint64_t)b * STEP_THREADS + tid; i < n; i += stride) acc = step_sq_acc(acc, g[i], gscale);
                sh[tid] = acc;
            }
            for (int s = STEP_THREADS / 2; s > 0; s >>= 1)
                for (int tid = 0; tid < s; ++tid) sh[tid] = step_add(sh[tid], sh[tid + s]);
            ctl->partials[b] = sh[0];
        }
        for (int b = 0; b < nb; ++b) S = step_add(S, ctl->partials[b]);
    }
    ctl->state[0] = step_finish(*ctl, ctl->state[0], gscale, need_norm, S);
    ctl->state[1] = 0u;
    return 0;
}
