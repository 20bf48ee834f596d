// What the small kernels around the training iteration share: the uniforms of a hash word, the seed's two words, mpg_normal's
// Box-Muller pair, the arrival ticket of a launch that moves its own cursor -- and the check of the tag table of
// include/mpgan_amd.h (every family of draws hashes under tags of its own).
#pragma once
#include "common.h"
#include "../../include/mpgan_amd.h"

namespace draws_detail {
struct Span { uint64_t tag, n; };
constexpr Span SPANS[] = {{MPG_NOISE_TAG, MPG_NOISE_TAG_SPAN}, {MPG_AUG_TAG, MPG_AUG_TAG_SPAN}, {MPG_LABEL_TAG, MPG_LABEL_TAG_SPAN},
                          {MPG_SHUFFLE_TAG, MPG_SHUFFLE_TAG_SPAN}, {MPG_PICK_TAG, MPG_PICK_TAG_SPAN}};
constexpr bool tags_ok() {
    for (int i = 0; i < 5; ++i) {
        if (SPANS[i].n < 1u || SPANS[i].tag < (1u << 27) || SPANS[i].tag + SPANS[i].n > (1ull << 32)) return false;
        for (int j = 0; j < i; ++j)
            if (SPANS[i].tag < SPANS[j].tag + SPANS[j].n && SPANS[j].tag < SPANS[i].tag + SPANS[i].n) return false;
    }
    return true;
}
}  // namespace draws_detail
static_assert(draws_detail::tags_ok(), "the tag spans of include/mpgan_amd.h: pairwise disjoint, at or above the dropout sites' 2^27");

// the 24 high bits of a hash word as u in [0, 1) / in (0, 1)
MPG_DEV float u24(uint32_t w) { return (float)(w >> 8) * (1.f / 16777216.f); }
MPG_DEV float u24_open(uint32_t w) { return ((float)(w >> 8) + 0.5f) * (1.f / 16777216.f); }

struct SeedWords { uint32_t lo, hi; };
MPG_DEV SeedWords seed_words(const uint64_t* seed) {
    const uint64_t sd = *seed;
    return {(uint32_t)sd, (uint32_t)(sd >> 32)};
}

// Pair i of mpg_normal's stream: the values are mean + r * cs and mean + r * sn.  One body for normal_kernel and
// normal_rank_mask_kernel (csrc/optim.hip), which must draw the same bits.
struct NormalPair { float r, sn, cs; };
MPG_DEV NormalPair normal_pair(SeedWords s, uint32_t tag, size_t i, float std) {
    // (the pair index goes through the mixer twice, the second time with the words swapped: two independent 32-bit streams)
    const uint32_t a = drop_word(s.lo, s.hi, tag, (uint32_t)i, (uint32_t)(i >> 32));
    const uint32_t b = drop_word(s.hi ^ 0x9E3779B9u, s.lo, tag + 0x7F4A7C15u, (uint32_t)i ^ a, (uint32_t)(i >> 32) + 1u);
    const float u1 = u24_open(a), u2 = u24_open(b);
    NormalPair p;
    p.r = sqrtf(-2.f * logf(u1)) * std;
    sincosf(6.283185307179586f * u2, &p.sn, &p.cs);
    return p;
}

// One arrival of a workgroup on the launch's agent-scope counter: true for the workgroup that arrives last.  The caller moves
// its cursor and puts the counter back to zero.
MPG_DEV bool last_arrival(unsigned int* ticket) {
    return __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
}
