// Jet augmentation inside the captured training iteration (mpgan/augment.py, reference train.py:438-442, :508-511):
// random 90-degree rotation, flip, translation and scaling of a jet's (eta, phi), each mixed in per jet with probability p.
//
// Every stage is affine and acts on the whole jet, so the mixed composition is ONE affine map per jet,
//   y_xy = A x_xy + t,
// built from the device-resident seed (the dropout / noise seed: a replayed hipGraph draws new maps) and applied with two
// FMAs per particle.  One workgroup (one wave) per jet: the map depends on blockIdx.x and kernel arguments alone, so the
// hashes are wave-uniform work; the lanes do the particles.  Columns >= 2 (pT, a mask column) pass through; padded particles
// are moved like any other, as the reference moves them.  The statement of the draws is in include/mpgan_amd.h.
#include "draws.h"

namespace {
struct AugMap { float a00, a01, a10, a11, t0, t1; };

// draw `i` of jet `b`: the 24 high bits of the word as u in [0, 1)
MPG_DEV uint32_t aug_word(uint32_t lo, uint32_t hi, uint32_t tag, uint32_t b, uint32_t i) { return drop_word(lo, hi, tag, b, i); }

MPG_DEV AugMap aug_map(SeedWords s, uint32_t tag, uint32_t b, float p, int flags, float translate_ratio, float scale_sd) {
    const uint32_t lo = s.lo, hi = s.hi;
    AugMap m = {1.f, 0.f, 0.f, 1.f, 0.f, 0.f};
    // rand_mix: a stage is taken where u < p -- and never at p == 1 (the reference returns the untouched batch there)
    const bool on = p != 1.f;
    auto take = [&](uint32_t i) { return on && u24(aug_word(lo, hi, tag, b, i)) < p; };
    if ((flags & MPG_AUG_R90) && take(0)) {
        const uint32_t k = aug_word(lo, hi, tag, b, 1) >> 30;          // floor(4 u)
        const float c = k == 0 ? 1.f : (k == 2 ? -1.f : 0.f), s = k == 1 ? 1.f : (k == 3 ? -1.f : 0.f);
        m.a00 = c; m.a01 = 0.f - s; m.a10 = s; m.a11 = c;               // (first stage: A = R^k I, t = 0)
    }
    if ((flags & MPG_AUG_FLIP) && take(2)) {
        const float sx = u24(aug_word(lo, hi, tag, b, 3)) >= 0.5f ? 1.f : -1.f;
        const float sy = u24(aug_word(lo, hi, tag, b, 4)) >= 0.5f ? 1.f : -1.f;
        m.a00 *= sx; m.a01 *= sx; m.t0 *= sx;
        m.a10 *= sy; m.a11 *= sy; m.t1 *= sy;
    }
    if ((flags & MPG_AUG_TRANSLATE) && take(5)) {
        m.t0 += (u24(aug_word(lo, hi, tag, b, 6)) - 0.5f) * translate_ratio;
        m.t1 += (u24(aug_word(lo, hi, tag, b, 7)) - 0.5f) * translate_ratio;
    }
    if ((flags & MPG_AUG_SCALE) && take(8)) {
        // one standard normal from two uniforms in (0, 1), as mpg_normal forms its own
        const float u1 = u24_open(aug_word(lo, hi, tag, b, 9));
        const float u2 = u24_open(aug_word(lo, hi, tag, b, 10));
        const float z = sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
        const float f = expf(scale_sd * z);
        m.a00 *= f; m.a01 *= f; m.a10 *= f; m.a11 *= f; m.t0 *= f; m.t1 *= f;
    }
    return m;
}

__global__ __launch_bounds__(64) void augment_kernel(const float* x, float* y, size_t jet_stride, int ld, int F, int N,
                                                     const uint64_t* __restrict__ seed, uint32_t tag, const float* __restrict__ p,
                                                     int flags, float translate_ratio, float scale_sd, float* __restrict__ params) {
    const uint32_t b = blockIdx.x;
    const AugMap m = aug_map(seed_words(seed), tag, b, *p, flags, translate_ratio, scale_sd);
    if (threadIdx.x == 0) {
        float* q = params + (size_t)b * 6;
        q[0] = m.a00; q[1] = m.a01; q[2] = m.a10; q[3] = m.a11; q[4] = m.t0; q[5] = m.t1;
    }
    const float* xj = x + (size_t)b * jet_stride;
    float* yj = y + (size_t)b * jet_stride;
    // the identity map hands the values on as they are (no -0 + 0 = +0): a step with p = 0 is bit for bit the step without
    const bool ident = m.a00 == 1.f && m.a01 == 0.f && m.a10 == 0.f && m.a11 == 1.f && m.t0 == 0.f && m.t1 == 0.f;
    if (ident && xj == yj) return;
    for (int i = threadIdx.x; i < N; i += 64) {
        const float* xr = xj + (size_t)i * ld;
        float* yr = yj + (size_t)i * ld;
        const float x0 = xr[0], x1 = xr[1];     // (both read before either is written: y may be x)
        yr[0] = ident ? x0 : fmaf(m.a00, x0, fmaf(m.a01, x1, m.t0));
        yr[1] = ident ? x1 : fmaf(m.a10, x0, fmaf(m.a11, x1, m.t1));
        if (xj != yj)
            for (int f = 2; f < F; ++f) yr[f] = xr[f];
    }
}

// dx_xy = A^T dy_xy, columns >= 2 copied
__global__ __launch_bounds__(64) void augment_bwd_kernel(const float* dy, float* dx, size_t jet_stride, int ld, int F, int N,
                                                         const float* __restrict__ params) {
    const uint32_t b = blockIdx.x;
    const float* q = params + (size_t)b * 6;
    const float a00 = q[0], a01 = q[1], a10 = q[2], a11 = q[3];
    const float* gj = dy + (size_t)b * jet_stride;
    float* dj = dx + (size_t)b * jet_stride;
    for (int i = threadIdx.x; i < N; i += 64) {
        const float* gr = gj + (size_t)i * ld;
        float* dr = dj + (size_t)i * ld;
        const float g0 = gr[0], g1 = gr[1];
        dr[0] = fmaf(a00, g0, a10 * g1);
        dr[1] = fmaf(a01, g0, a11 * g1);
        if (gj != dj)
            for (int f = 2; f < F; ++f) dr[f] = gr[f];
    }
}

inline bool bad_shape(uint64_t jet_stride, int ld, int F, int B, int N) {
    return B <= 0 || N < 0 || F < 2 || ld < F || (N > 0 && jet_stride < (uint64_t)N * (uint64_t)ld);
}
}  // namespace

extern "C" int mpg_augment(const float* x, float* y, uint64_t jet_stride, int ld, int F, int B, int N, const uint64_t* seed,
                           uint32_t tag, const float* p, int flags, float translate_ratio, float scale_sd, float* params,
                           void* stream) {
    if (bad_shape(jet_stride, ld, F, B, N) || seed == nullptr || p == nullptr || params == nullptr) return -1;
    if (N > 0 && (x == nullptr || y == nullptr)) return -1;
    if (flags & ~(MPG_AUG_R90 | MPG_AUG_FLIP | MPG_AUG_TRANSLATE | MPG_AUG_SCALE)) return -1;
    hipLaunchKernelGGL(augment_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, x, y, (size_t)jet_stride, ld, F, N, seed, tag, p,
                       flags, translate_ratio, scale_sd, params);
    return (int)hipGetLastError();
}

extern "C" int mpg_augment_bwd(const float* dy, float* dx, uint64_t jet_stride, int ld, int F, int B, int N, const float* params,
                               void* stream) {
    if (bad_shape(jet_stride, ld, F, B, N) || N == 0 || dy == nullptr || dx == nullptr || params == nullptr) return -1;
    hipLaunchKernelGGL(augment_bwd_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, dy, dx, (size_t)jet_stride, ld, F, N, params);
    return (int)hipGetLastError();
}
