// dn_permute.h -- the keyed permutation of a PPO epoch's samples (dn_minibatch, dn_minibatch_permutation): plain C++ for host and device,
// and the only place that holds it.  pi is a bijection of [0, M), 1 <= M <= 2^31 - 1, keyed by (seed, epoch) and evaluated per element in
// O(1): a six-round balanced Feistel cipher on 2h bits, 2^(2h) < 4 M, walked until the value falls below M (cycle walking: a pass is a
// bijection of the cipher's domain, so the walk from a value below M comes back below M, and distinct starts end at distinct values).
// No permutation array, no sort, no atomics: a minibatch needs its own slots of pi only, in any order, on any number of workgroups.
//   b = max(1, bit_length(M - 1)); h = max(1, (b + 1) / 2); mask = 2^h - 1
//   round keys: x = seed ^ (epoch * 0xD1342543DE82EF95); six times x += 0x9E3779B97F4A7C15, k_r = splitmix64's mix of x >> 32
//   a pass over v: L = (v >> h) & mask, R = v & mask; six times F = fmix32(R + k_r) >> (32 - h), (L, R) = (R, (L ^ F) & mask); L << h | R
// fmix32 is murmur3's finaliser.  Every operation is an integer one: host and device give the same values.
#pragma once

#include <stdint.h>

#ifdef __HIP__
#define DN_PERMUTE_FN __host__ __device__ inline
#else
#define DN_PERMUTE_FN inline
#endif

constexpr int DN_PERMUTE_ROUNDS = 6;
constexpr long long DN_PERMUTE_MAX = 0x7fffffffll;     // the largest M

struct DnPermutation {
    uint32_t k[DN_PERMUTE_ROUNDS];                     // the round keys
    uint32_t h, mask, m;                               // bits of a half, 2^h - 1, M
};

DN_PERMUTE_FN uint32_t dn_permute_fmix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// The permutation of [0, m) under (seed, epoch); m in 1 .. DN_PERMUTE_MAX is the caller's to check.
DN_PERMUTE_FN DnPermutation dn_permute_make(const uint64_t seed, const uint64_t epoch, const uint32_t m)
{
    DnPermutation p;
    uint32_t b = 0;
    for (uint32_t t = m - 1; t; t >>= 1) ++b;          // bit_length(m - 1)
    if (b < 1) b = 1;
    p.h = (b + 1) / 2;                                 // >= 1, <= 16
    p.mask = (1u << p.h) - 1u;
    p.m = m;
    uint64_t x = seed ^ (epoch * 0xD1342543DE82EF95ull);
    for (int r = 0; r < DN_PERMUTE_ROUNDS; ++r) {      // splitmix64
        x += 0x9E3779B97F4A7C15ull;
        uint64_t z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        p.k[r] = (uint32_t)(z >> 32);
    }
    return p;
}

// pi(i), 0 <= i < p.m
DN_PERMUTE_FN uint32_t dn_permute_at(const DnPermutation &p, const uint32_t i)
{
    uint32_t v = i;
    do {
        uint32_t l = (v >> p.h) & p.mask, r = v & p.mask;
        for (int j = 0; j < DN_PERMUTE_ROUNDS; ++j) {
            const uint32_t f = dn_permute_fmix32(r + p.k[j]) >> (32u - p.h);
            const uint32_t t = (l ^ f) & p.mask;
            l = r;
            r = t;
        }
        v = (l << p.h) | r;
    } while (v >= p.m);
    return v;
}
