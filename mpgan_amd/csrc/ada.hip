// Adaptive augmentation probability (ADA: Karras et al. 2020, "Training generative adversarial networks with limited data") as
// one small launch behind the D step's head: the controller that settles mpg_augment's p from the discriminator's own outputs on
// the real jets, inside the captured iteration.  The reference names the option (--adaptive-prob, setup_training.py:399) and
// never fills the value it reads (augment_p[-1], train.py:440, :510): the statement in include/mpgan_amd.h is the specification.
//
// One workgroup of 256 threads strides over the n_real outputs; each lane counts sign(out - mid) as an integer, the counts are
// added within a wave by shuffles and across the four waves through LDS, and lane 0 alone moves the state, p and r (plain vector
// loads and stores: one thread of one workgroup, no atomics, no ticket).  Everything is integer up to one fp32 divide and one
// fp32 add or subtract, so the result does not depend on the order of the reduction; ada_sign and ada_finish are one body for
// the device and for mpg_ada_update_host.
//
// Data-parallel ranks settle ONE p from the global sign sum, and the launch comes apart at `state[0] += s` for them:
// mpg_ada_count stores a rank's own s as a float into a slot at the tail of D's flat gradient buffer, the gradient all-reduce adds
// the ranks' slots (integers of magnitude <= 2^24: exact in fp32 in any order), and mpg_ada_settle -- one thread, first in the
// segment behind the all-reduce -- takes the sum back as an integer and runs ada_finish on it.  ada_slot is its reading of the
// slot: anything that is not an integer within [-n_real_total, n_real_total] says the collective is broken.
#include "common.h"
#include "../../include/mpgan_amd.h"

// +1 above mid, -1 below, 0 at mid and for a NaN (both comparisons false)
MPG_HD int ada_sign(float v, float mid) { return (int)(v > mid) - (int)(v < mid); }

MPG_HD float ada_div(float a, float b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __fdiv_rn(a, b);      // the correctly rounded quotient, whatever the build's division flags
#else
    return a / b;
#endif
}

// what one thread does with the launch's sign sum s
MPG_HD void ada_finish(int s, int n_real, float target, float step, int interval, int32_t* state, float* aug_p, float* r_out) {
    const int32_t sum = state[0] + s, steps = state[1] + 1;
    if (steps != interval) {
        state[0] = sum;
        state[1] = steps;
        return;
    }
    const float r = ada_div((float)sum, (float)(n_real * interval));
    float p = *aug_p;
    if (r > target) p = p + step;
    else if (r < target) p = p - step;
    p = p < 0.f ? 0.f : (p > 1.f ? 1.f : p);
    *aug_p = p;
    *r_out = r;
    state[0] = 0;
    state[1] = 0;
}

// the all-reduced slot as the integer it must be: false for a NaN, a fraction or a magnitude beyond n_total (<= 2^30)
MPG_HD bool ada_slot(float v, int n_total, int* s) {
    if (!(v >= -1073741824.f && v <= 1073741824.f)) return false;      // (a NaN fails both; the conversion below is then defined)
    const int i = (int)v;
    if ((float)i != v || i > n_total || i < -n_total) return false;
    *s = i;
    return true;
}

// what the settle's one thread does with the slot
MPG_HD void ada_settle_one(const float* slot, int n_real_total, float target, float step, int interval, int32_t* state, float* aug_p,
                           float* r_out) {
    int s;
    if (ada_slot(slot[0], n_real_total, &s)) ada_finish(s, n_real_total, target, step, interval, state, aug_p, r_out);
    else *r_out = __builtin_nanf("");
}

namespace {

// the workgroup's sign sum over out[0 .. n_real): valid in thread 0 (256 threads, wave_sum: four words of LDS)
__device__ __forceinline__ int ada_block_count(const float* __restrict__ out, int n_real, float mid, int* wave_sum) {
    const int tid = threadIdx.x;
    int s = 0;
    for (int b = tid; b < n_real; b += 256) s += ada_sign(out[b], mid);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = s;
    __syncthreads();
    return tid == 0 ? wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3] : 0;
}

__global__ __launch_bounds__(256) void ada_update_kernel(const float* __restrict__ out, int n_real, float mid, float target, float step,
                                                         int interval, int32_t* state, float* aug_p, float* r_out) {
    __shared__ int wave_sum[4];
    const int s = ada_block_count(out, n_real, mid, wave_sum);
    if (threadIdx.x == 0) ada_finish(s, n_real, target, step, interval, state, aug_p, r_out);
}

__global__ __launch_bounds__(256) void ada_count_kernel(const float* __restrict__ out, int n_real, float mid, float* slot) {
    __shared__ int wave_sum[4];
    const int s = ada_block_count(out, n_real, mid, wave_sum);
    if (threadIdx.x == 0) slot[0] = (float)s;      // (|s| <= n_real <= 2^24: exact; a store, whatever the slot held)
}

__global__ __launch_bounds__(64) void ada_settle_kernel(const float* slot, int n_real_total, float target, float step, int interval,
                                                        int32_t* state, float* aug_p, float* r_out) {
    if (threadIdx.x == 0) ada_settle_one(slot, n_real_total, target, step, interval, state, aug_p, r_out);
}

bool ada_args_ok(const float* out, int n_real, float target, float step, int interval, const int32_t* state, const float* aug_p,
                 const float* r_out) {
    if (out == nullptr || state == nullptr || aug_p == nullptr || r_out == nullptr) return false;
    if (n_real < 1 || n_real > (1 << 30) || interval < 1) return false;
    if ((int64_t)n_real * (int64_t)interval > 0x7fffffffLL) return false;      // (the sign sum and the divisor stay in int32)
    return target >= 0.f && target <= 1.f && step >= 0.f;                      // (a NaN fails every comparison)
}

constexpr int ADA_COUNT_MAX = 1 << 24;      // a rank's count, and the ranks' sum, stay exact in fp32 up to here

bool ada_count_ok(const float* out, int n_real, const float* slot) {
    return out != nullptr && slot != nullptr && n_real >= 1 && n_real <= ADA_COUNT_MAX;
}

}  // namespace

extern "C" int mpg_ada_update(const float* out, int n_real, float mid, float target, float step, int interval, int32_t* state,
                              float* aug_p, float* r_out, void* stream) {
    if (!ada_args_ok(out, n_real, target, step, interval, state, aug_p, r_out)) return -1;
    hipLaunchKernelGGL(ada_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, out, n_real, mid, target, step, interval, state,
                       aug_p, r_out);
    return (int)hipGetLastError();
}

extern "C" int mpg_ada_update_host(const float* out, int n_real, float mid, float target, float step, int interval, int32_t* state,
                                   float* aug_p, float* r_out) {
    if (!ada_args_ok(out, n_real, target, step, interval, state, aug_p, r_out)) return -1;
    int s = 0;
    for (int b = 0; b < n_real; ++b) s += ada_sign(out[b], mid);
    ada_finish(s, n_real, target, step, interval, state, aug_p, r_out);
    return 0;
}

extern "C" int mpg_ada_count(const float* out, int n_real, float mid, float* slot, void* stream) {
    if (!ada_count_ok(out, n_real, slot)) return -1;
    hipLaunchKernelGGL(ada_count_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, out, n_real, mid, slot);
    return (int)hipGetLastError();
}

extern "C" int mpg_ada_count_host(const float* out, int n_real, float mid, float* slot) {
    if (!ada_count_ok(out, n_real, slot)) return -1;
    int s = 0;
    for (int b = 0; b < n_real; ++b) s += ada_sign(out[b], mid);
    slot[0] = (float)s;
    return 0;
}

extern "C" int mpg_ada_settle(const float* slot, int n_real_total, float target, float step, int interval, int32_t* state, float* aug_p,
                              float* r_out, void* stream) {
    if (!ada_args_ok(slot, n_real_total, target, step, interval, state, aug_p, r_out)) return -1;
    hipLaunchKernelGGL(ada_settle_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, slot, n_real_total, target, step, interval, state,
                       aug_p, r_out);
    return (int)hipGetLastError();
}

extern "C" int mpg_ada_settle_host(const float* slot, int n_real_total, float target, float step, int interval, int32_t* state,
                                   float* aug_p, float* r_out) {
    if (!ada_args_ok(slot, n_real_total, target, step, interval, state, aug_p, r_out)) return -1;
    ada_settle_one(slot, n_real_total, target, step, interval, state, aug_p, r_out);
    return 0;
}
