// dn_replay_draw.h -- the keyed draw of a replay minibatch (dn_replay_sample, dn_replay_indices): plain C++ for host and device, and the
// only place that holds it.  Row j of a call keyed by (seed, draw) over S valid slots and N drones, 1 <= S, N <= 2^31 - 1, is a slot and
// a drone drawn independently of every other row, with replacement, as SB3's ReplayBuffer.sample draws them [from recall]:
//   x    = seed ^ (draw * 0xD1342543DE82EF95)                 dn_permute.h's keying
//   z    = the (j + 1)-th splitmix64 output from the state x: x + (j + 1) * 0x9E3779B97F4A7C15 through splitmix64's mix
//   raw  = ((z >> 32) * S) >> 32,  env = ((z & 0xFFFFFFFF) * N) >> 32            64-bit products of 32-bit halves
//   slot = raw + (skip >= 0 && raw >= skip)                   skip: the slot being replaced (a full ring mid-cycle), or -1
// The multiply-shift is NOT rejection sampled: a value's probability is floor or ceil of 2^32 / S (or N) over 2^32, so it differs from
// the uniform 1 / S by less than 2^-32.  Row j does not depend on the number of rows of the call: G B rows are G independent batches of
// B.  Every operation is an integer one: host and device give the same values.  The flat sample index is slot * N + env, an int64.
#pragma once

#include <stdint.h>

#ifdef __HIP__
#define DN_REPLAY_FN __host__ __device__ inline
#else
#define DN_REPLAY_FN inline
#endif

constexpr long long DN_REPLAY_MAX = 0x7fffffffll;      // the largest S, N and number of rows of a call

struct DnReplayPick {
    uint32_t slot, env;
};

// The state every row of a call starts from.
DN_REPLAY_FN uint64_t dn_replay_key(const uint64_t seed, const uint64_t draw) { return seed ^ (draw * 0xD1342543DE82EF95ull); }

// Row j under `key`; s, n in 1 .. DN_REPLAY_MAX and skip in -1 .. s are the caller's to check.
DN_REPLAY_FN DnReplayPick dn_replay_draw_at(const uint64_t key, const uint64_t j, const uint32_t s, const uint32_t n, const int64_t skip)
{
    uint64_t z = key + (j + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const uint32_t raw = (uint32_t)(((z >> 32) * s) >> 32);                    // < s
    DnReplayPick p;
    p.slot = raw + (uint32_t)(skip >= 0 && (int64_t)raw >= skip);              // <= s
    p.env = (uint32_t)(((z & 0xFFFFFFFFull) * n) >> 32);                       // < n
    return p;
}

DN_REPLAY_FN int64_t dn_replay_flat(const DnReplayPick p, const uint32_t n) { return (int64_t)p.slot * (int64_t)n + (int64_t)p.env; }
