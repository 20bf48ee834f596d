// The batch feed of a device-resident data set: what TrainStep.set_batch writes (eight ATen launches behind a host copy) as
// ONE launch inside the captured iteration.  Jet j of the launch takes stream position *cursor + j, whose data-set row is
// shuffle_row(key, position, n) (csrc/shuffle.h): the order of the jets is a function of (key, cursor) alone.
//
// A particle row is one aligned float4.  A jet has a wave's lanes over its particles -- or half a wave's at N <= 32, two jets per
// wave --, four waves per workgroup; every lane of a jet computes the jet's row itself (a few dozen integer operations; nothing is
// exchanged).  The launch moves ~120 KB at B = 256 and is bound by latency: plain loads and stores, no LDS, no register tile.
//
// The cursor moves on by `stride` in the SAME launch, behind the last read of it: every workgroup reads the cursor first and
// arrives on an agent-scope counter last (its gather's addresses depend on the value read, so the read has returned by then);
// the workgroup that arrives last -- told by the value the add returns -- writes cursor + stride and puts the counter back to
// zero for the next launch (the arrival counters of the sender-chunked edge launches work the same way).
#include "shuffle.h"
#include "draws.h"

namespace {
struct FeedOut { float *data, *labels, *dcat, *x3, *mask2, *ign2, *labels2; };

__global__ __launch_bounds__(256) void batch_feed_kernel(const float4* __restrict__ particles, const float* __restrict__ labels_in,
                                                         uint64_t n, int N, uint64_t key, uint64_t* cursor, unsigned int* ticket,
                                                         int B, uint64_t stride, FeedOut o) {
    const uint64_t cur = __hip_atomic_load(cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int width = N <= 32 ? 32 : 64;                   // lanes per jet
    const int j = blockIdx.x * (256 / width) + (int)threadIdx.x / width, lane = (int)threadIdx.x % width;
    if (j < B) {
        const size_t row = shuffle_row(key, cur + (uint64_t)j, n);
        const float4* src = particles + row * (size_t)N;
        for (int i = lane; i < N; i += width) {
            const float4 v = src[i];
            const size_t e = (size_t)j * N + i;
            if (o.data) reinterpret_cast<float4*>(o.data)[e] = v;
            if (o.dcat) reinterpret_cast<float4*>(o.dcat)[e] = v;
            if (o.x3) { float* q = o.x3 + 3 * e; q[0] = v.x; q[1] = v.y; q[2] = v.z; }
            if (o.mask2) o.mask2[e] = v.w + 0.5f;
            if (o.ign2) o.ign2[e] = 0.5f - v.w;
        }
        if (lane == 0 && labels_in != nullptr) {
            const float l = labels_in[row];
            if (o.labels) o.labels[j] = l;
            if (o.labels2) { o.labels2[j] = l; o.labels2[B + j] = l; }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (last_arrival(ticket)) {
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(cursor, cur + stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }
}  // namespace

extern "C" int mpg_batch_feed(const float* particles, const float* labels_in, int64_t n, int N, uint64_t key, uint64_t* cursor,
                              uint32_t* ticket, int B, uint64_t stride, float* data, float* labels, float* dcat, float* x3,
                              float* mask2, float* ign2, float* labels2, void* stream) {
    if (n < 1 || n > 0x7fffffffLL || B < 1 || N < 1 || cursor == nullptr || ticket == nullptr || particles == nullptr) return -1;
    if (labels_in == nullptr && (labels != nullptr || labels2 != nullptr)) return -1;
    if (misaligned(particles) || misaligned(data) || misaligned(dcat)) return -2;   // (rows move as float4)
    const FeedOut o = {data, labels, dcat, x3, mask2, ign2, labels2};
    const int per_wg = 256 / (N <= 32 ? 32 : 64);
    hipLaunchKernelGGL(batch_feed_kernel, dim3((B + per_wg - 1) / per_wg), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(particles), labels_in, (uint64_t)n, N, key, cursor, ticket, B, stride, o);
    return (int)hipGetLastError();
}

extern "C" int mpg_shuffle_index_host(uint64_t key, uint64_t pos0, int64_t count, int64_t n, int32_t* out) {
    if (n < 1 || n > 0x7fffffffLL || count < 0 || (count > 0 && out == nullptr)) return -1;
    for (int64_t c = 0; c < count; ++c) out[c] = (int32_t)shuffle_row(key, pos0 + (uint64_t)c, (uint64_t)n);
    return 0;
}
