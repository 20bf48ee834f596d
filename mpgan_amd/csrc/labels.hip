// Label smoothing and label noise of calc_D_loss (reference train.py:341-363, --label-smoothing / --label-noise) drawn on
// the device: the D step's per-jet targets from the device-resident seed (the dropout / noise / augmentation seed: a replayed
// hipGraph draws new labels), in a small launch of its own in front of the fused head, which only reads them.
//
// One workgroup of 256 threads strides over the 2B jets (rows [0, B) the real half).  A jet's label is two hashes, so every
// pass recomputes it instead of parking it: pass 1 sums each half, pass 2 sums the squared distances to the half's mean, pass 3
// writes.  Each sum is a thread's strided partial, then a tree over the 256 partials in LDS: one fixed order, no atomics.
// The statement of the draws is in include/mpgan_amd.h.
#include "draws.h"

namespace {

// Y of jet b before any broadcasting: the smoothed (or 1 / 0) label, then the flip
MPG_DEV float label_draw(uint32_t lo, uint32_t hi, uint32_t tag, uint32_t b, bool real, int smoothing, float noise) {
    const float us = u24(drop_word(lo, hi, tag, b, 0)), un = u24(drop_word(lo, hi, tag, b, 1));
    float y = real ? 1.f : 0.f;
    if (smoothing) y = real ? fmaf(0.5f, us, 0.7f) : 0.3f * us;      // U[0.7, 1.2) / U[0, 0.3): one rounding each
    if (un < noise) y = real ? 0.f : 1.f;
    return y;
}

// red[0] = sum of the 256 values, in tree order; every thread returns it
MPG_DEV float block_sum(float* red, float v) {
    const int tid = threadIdx.x;
    __syncthreads();          // (the buffer's last readers are done)
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void label_targets_kernel(const uint64_t* __restrict__ seed, uint32_t tag, int B, int smoothing,
                                                            float noise, float* __restrict__ targets, float* __restrict__ extra,
                                                            float* __restrict__ drawn) {
    __shared__ float red[256];
    const SeedWords s = seed_words(seed);
    const int tid = threadIdx.x, n = 2 * B;
    auto y_of = [&](int b) { return label_draw(s.lo, s.hi, tag, (uint32_t)b, b < B, smoothing, noise); };
    float mean_r = 0.f, mean_f = 0.f, ex = 0.f;
    if (smoothing) {
        // MSELoss(out [B, 1], Y [B]) broadcasts to [B, B]: mean_ij (out_i - Y_j)^2 = mean_i (out_i - mean Y)^2 + popvar(Y)
        float sr = 0.f, sf = 0.f;
        for (int b = tid; b < n; b += 256) { const float y = y_of(b); if (b < B) sr += y; else sf += y; }
        mean_r = block_sum(red, sr) / (float)B;
        mean_f = block_sum(red, sf) / (float)B;
        float qr = 0.f, qf = 0.f;
        for (int b = tid; b < n; b += 256) {
            const float d = y_of(b) - (b < B ? mean_r : mean_f);
            if (b < B) qr += d * d; else qf += d * d;
        }
        const float var_r = block_sum(red, qr) / (float)B;
        const float var_f = block_sum(red, qf) / (float)B;
        ex = var_r + var_f;
    }
    for (int b = tid; b < n; b += 256) {
        const float y = y_of(b);
        targets[b] = smoothing ? (b < B ? mean_r : mean_f) : y;
        if (drawn != nullptr) drawn[b] = y;
    }
    if (tid == 0) extra[0] = ex;
}

}  // namespace

extern "C" int mpg_label_targets(int B, int smoothing, float noise, const uint64_t* seed, uint32_t tag, float* targets,
                                 float* extra, float* drawn, void* stream) {
    if (B <= 0 || B > (1 << 30) || seed == nullptr || targets == nullptr || extra == nullptr) return -1;
    if (!(noise >= 0.f && noise <= 1.f)) return -1;
    hipLaunchKernelGGL(label_targets_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, seed, tag, B, smoothing ? 1 : 0, noise,
                       targets, extra, drawn);
    return (int)hipGetLastError();
}
