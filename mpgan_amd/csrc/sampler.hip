// Bulk generation as a stream of rows (gen.JetSampler): the two small launches around a chunk's generator forward.
//
// mpg_label_pick   the chunk's labels: jet b of the launch is row g = *cursor + b of the stream and takes table[idx(g)], idx a
//                  keyed hash of the row alone (pick_index below: one body for the device and for mpg_label_pick_host).
// mpg_jets_finish  the epilogue of the reference's gen.py:127-141 -- undo shift / norm / max, zero the particles that are not
//                  real, clamp pT at 0 -- written straight into the caller's [total, N, 3] array at the chunk's rows, one thread
//                  per particle (rows of 12 bytes: no alignment beyond a float's is assumed).  Rows at or beyond `total` are not
//                  written: the last chunk of a call may be short.
//
// The cursor and the noise seed of the NEXT chunk move in mpg_jets_finish itself, behind every workgroup's read of the cursor,
// exactly as mpg_batch_feed moves its cursor (csrc/loader.hip): every workgroup reads the cursor first -- its stores' addresses
// and its `row < total` branch depend on the value, so the read has returned -- and arrives on an agent-scope counter last; the
// workgroup that arrives last, told by the value the add returns, writes cursor + B and the seed word of chunk (cursor + B) / B
// and puts the counter back to zero.  mpg_jets_finish_stride moves the cursor by `stride` instead of B: rank r of W data-parallel
// ranks owns the chunks c = r (mod W) of the one global stream and strides by W B.  Both launches are bound by latency (a chunk
// of 4096 jets of 30 particles moves 3.4 MB).
#include "draws.h"

constexpr uint64_t CHUNK_SEED_STEP = 0x9E3779B97F4A7C15ull;

// table index of stream row g: multiply-shift of one hash word onto [0, n) (n <= 2^31 - 1)
MPG_HD uint32_t pick_index(uint64_t key, uint64_t g, uint32_t n) {
    const uint32_t w = drop_word((uint32_t)key, (uint32_t)(key >> 32), MPG_PICK_TAG, (uint32_t)g, (uint32_t)(g >> 32));
    return (uint32_t)(((uint64_t)w * (uint64_t)n) >> 32);
}

namespace {
struct Unnorm { float mx[3], nrm[3], sh[3]; };

__global__ __launch_bounds__(256) void label_pick_kernel(const float* __restrict__ table, uint32_t n, uint64_t key,
                                                         const uint64_t* cursor, int B, float* __restrict__ labels) {
    const uint64_t cur = __hip_atomic_load(cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int b = blockIdx.x * 256 + (int)threadIdx.x;
    if (b < B) labels[b] = table[pick_index(key, cur + (uint64_t)b, n)];
}

__global__ __launch_bounds__(256) void jets_finish_kernel(const float* __restrict__ feat, int ld_feat, const float* __restrict__ mask,
                                                          int B, int N, Unnorm u, float* __restrict__ out, float* __restrict__ mask_out,
                                                          uint64_t row0, uint64_t total, uint64_t key, uint64_t stride,
                                                          uint64_t* cursor, uint64_t* seed, unsigned int* ticket) {
#pragma clang fp contract(off)   // subtract, divide, multiply: three roundings, as data.unnormalise_jets makes them
    const uint64_t cur = __hip_atomic_load(cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;          // particle of the chunk
    if (t < (size_t)B * N) {
        const uint64_t r = cur + (uint64_t)(t / (size_t)N) - row0;    // row of `out` (a cursor behind row0 wraps beyond total)
        if (r < total) {
            const size_t e = (size_t)r * N + t % (size_t)N;
            const float* x = feat + t * (size_t)ld_feat;
            const bool real = mask == nullptr || __fsub_rn(mask[t], 0.5f) >= 0.5f;
            float v[3];
#pragma unroll
            for (int f = 0; f < 3; ++f)
                v[f] = real ? __fmul_rn(__fdiv_rn(__fsub_rn(x[f], u.sh[f]), u.nrm[f]), u.mx[f]) : 0.f;
            if (v[2] < 0.f) v[2] = 0.f;
            float* q = out + 3 * e;
            q[0] = v[0]; q[1] = v[1]; q[2] = v[2];
            if (mask_out != nullptr) mask_out[e] = real ? 1.f : 0.f;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (last_arrival(ticket)) {
            const uint64_t next = cur + stride;      // (a rank of W: W B, its next chunk of the global stream)
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(seed, key + (next / (uint64_t)B) * CHUNK_SEED_STEP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(cursor, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
}  // namespace

extern "C" int mpg_label_pick(const float* table, int64_t n, uint64_t key, const uint64_t* cursor, int B, float* labels,
                              void* stream) {
    if (n < 1 || n > 0x7fffffffLL || B < 1 || table == nullptr || cursor == nullptr || labels == nullptr) return -1;
    hipLaunchKernelGGL(label_pick_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, table, (uint32_t)n, key, cursor, B,
                       labels);
    return (int)hipGetLastError();
}

extern "C" int mpg_label_pick_host(uint64_t key, uint64_t pos0, int64_t count, int64_t n, int32_t* out) {
    if (n < 1 || n > 0x7fffffffLL || count < 0 || (count > 0 && out == nullptr)) return -1;
    for (int64_t c = 0; c < count; ++c) out[c] = (int32_t)pick_index(key, pos0 + (uint64_t)c, (uint32_t)n);
    return 0;
}

extern "C" int mpg_jets_finish_stride(const float* feat, int ld_feat, const float* mask, int B, int N, const float* maxes,
                                      const float* norms, const float* shifts, float* out, float* mask_out, uint64_t row0,
                                      int64_t total, uint64_t key, int64_t stride, uint64_t* cursor, uint64_t* seed, uint32_t* ticket,
                                      void* stream) {
    if (B < 1 || N < 1 || total < 0 || ld_feat < 3 || stride < 1) return -1;
    if (feat == nullptr || out == nullptr || cursor == nullptr || seed == nullptr || ticket == nullptr) return -1;
    if (maxes == nullptr || norms == nullptr || shifts == nullptr) return -1;
    if ((uint64_t)B * (uint64_t)N > 0x7fffffffull * 256ull) return -1;       // (the grid's x extent)
    Unnorm u;
    for (int f = 0; f < 3; ++f) { u.mx[f] = maxes[f]; u.nrm[f] = norms[f]; u.sh[f] = shifts[f]; }
    const unsigned int grid = (unsigned int)(((uint64_t)B * N + 255) / 256);
    hipLaunchKernelGGL(jets_finish_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, feat, ld_feat, mask, B, N, u, out, mask_out,
                       row0, (uint64_t)total, key, (uint64_t)stride, cursor, seed, ticket);
    return (int)hipGetLastError();
}

extern "C" int mpg_jets_finish(const float* feat, int ld_feat, const float* mask, int B, int N, const float* maxes,
                               const float* norms, const float* shifts, float* out, float* mask_out, uint64_t row0, int64_t total,
                               uint64_t key, uint64_t* cursor, uint64_t* seed, uint32_t* ticket, void* stream) {
    return mpg_jets_finish_stride(feat, ld_feat, mask, B, N, maxes, norms, shifts, out, mask_out, row0, total, key, (int64_t)B, cursor,
                                  seed, ticket, stream);
}
