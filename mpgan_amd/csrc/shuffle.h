// The keyed shuffle of the device-resident data set: perm(key, epoch, i, n), a bijection of [0, n) computed per jet from
// (key, epoch, i) alone -- no permutation buffer, nothing to save but the key and a cursor.  One body for the device (the
// gather of csrc/loader.hip) and the host (mpg_shuffle_index_host); the statement is in include/mpgan_amd.h.
//
// A balanced Feistel network over 2h bits (2^(2h) < 4n) is a bijection of [0, 2^(2h)) whatever its round function is;
// walking -- applying it again while the result is >= n -- restricts it to a bijection of [0, n) (the walk follows the cycle
// of i, which returns to [0, n) because it started there), in fewer than four rounds of the network on average.
#pragma once
#include "common.h"
#include "../../include/mpgan_amd.h"

constexpr int SHUFFLE_ROUNDS = 4;

MPG_HD uint32_t shuffle_perm(uint64_t key, uint64_t epoch, uint32_t i, uint32_t n) {
    if (n <= 1u) return 0u;
    const uint32_t key_lo = (uint32_t)key, key_hi = (uint32_t)(key >> 32), ep = (uint32_t)epoch;
    int k = 0;
    while (k < 32 && ((n - 1u) >> k) != 0u) ++k;          // bit length of n - 1
    const int h = (k + 1) / 2;                              // (n <= 2^31: h <= 16, the two halves fit one word)
    const uint32_t half = (1u << h) - 1u;
    uint32_t x = i;
    do {
        uint32_t L = x >> h, R = x & half;
        for (int r = 0; r < SHUFFLE_ROUNDS; ++r) {
            const uint32_t t = L ^ (drop_word(key_lo, key_hi, MPG_SHUFFLE_TAG + (uint32_t)r, R, ep) & half);
            L = R;
            R = t;
        }
        x = (L << h) | R;
    } while (x >= n);
    return x;
}

// data-set row of stream position g: the stream is continuous, epoch g / n, place g % n
MPG_HD uint32_t shuffle_row(uint64_t key, uint64_t g, uint64_t n) { return shuffle_perm(key, g / n, (uint32_t)(g % n), (uint32_t)n); }
