// check_bf16_split -- csrc/dn_bf16_split.h on the host, against the rules written out independently: for every float32 exponent, for
// all-ones mantissas (rounding carries), subnormals and a few million pseudo-random bit patterns
//   hi is the round-to-nearest-even bfloat16 of x (found here by comparing the two neighbouring bf16 values in double),
//   lo is the same rounding of the float32 x - hi, and |x - hi - lo| <= 2^-16 |x| (below |x| = 2^-118, where lo is on bf16's subnormal
//   grid: <= 2^-134),
//   the pair form packs the same bits,
// and zeros, infinities and NaN do what the header's comment says.  Prints one JSON line; exit status 0 = all held.
#include "dn_bf16_split.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

static float from_bits(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t bits_of(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// round to nearest even of a finite x onto the bf16 grid, by the definition: the two neighbours, the nearer one, the even one at a tie
static uint16_t nearest_even(float x)
{
    const uint32_t u = bits_of(x);
    const uint16_t down = (uint16_t)(u >> 16);                 // truncation: the neighbour towards zero
    const uint16_t up = (uint16_t)(down + 1);                  // the next magnitude (may be infinity)
    const double xd = std::fabs((double)x);
    const double dd = std::fabs((double)from_bits((uint32_t)down << 16));
    const bool up_inf = (up & 0x7fff) == 0x7f80;
    const double ud = up_inf ? std::ldexp(1.0, 128) : std::fabs((double)from_bits((uint32_t)up << 16));     // infinity stands for 2^128
    const double a = xd - dd, b = ud - xd;
    if (a < b) return down;
    if (b < a) return up;
    return (down & 1) ? up : down;
}

static long long checked = 0, failures = 0;
static double worst = 0.0;

static void fail(const char *what, float x)
{
    if (failures++ < 10) std::fprintf(stderr, "%s at x = %a (0x%08x)\n", what, (double)x, bits_of(x));
}

static void check(float x)
{
    ++checked;
    uint16_t hi, lo;
    dn_bf16_split(x, &hi, &lo);
    const uint32_t mag = bits_of(x) & 0x7fffffffu;
    if (mag > 0x7f800000u) {                                   // NaN: two quiet NaNs
        if ((hi & 0x7fc0) != 0x7fc0 || (lo & 0x7fc0) != 0x7fc0) fail("NaN", x);
        return;
    }
    if (mag == 0x7f800000u) {                                  // infinity: itself and a NaN
        if (hi != (uint16_t)(bits_of(x) >> 16) || (lo & 0x7fc0) != 0x7fc0) fail("infinity", x);
        return;
    }
    if (hi != nearest_even(x)) fail("hi is not the nearest-even bf16", x);
    const float h = dn_bf16_widen(hi);
    if (std::isinf(h)) {                                       // the top 2^15 finite values: hi = +-inf, lo = -+inf
        if (mag < 0x7f7f8000u || lo != (uint16_t)((hi ^ 0x8000))) fail("overflow", x);
        return;
    }
    const float d = x - h;
    if ((double)d != (double)x - (double)h) fail("x - hi is not exact", x);
    if (lo != nearest_even(d)) fail("lo is not the nearest-even bf16 of x - hi", x);
    if (mag == 0 && (hi != (uint16_t)(bits_of(x) >> 16) || lo != 0)) fail("zero", x);
    const double rest = std::fabs((double)x - (double)h - (double)dn_bf16_widen(lo));
    // bf16 has float32's exponent range, so below |x| = 2^-118 lo runs into the subnormal grid of spacing 2^-133 and the remainder is
    // bounded absolutely, by half that spacing, instead
    if (std::fabs((double)x) >= std::ldexp(1.0, -118)) {
        const double rel = rest / std::fabs((double)x);
        if (rel > worst) worst = rel;
        if (rel > std::ldexp(1.0, -16)) fail("|x - hi - lo| > 2^-16 |x|", x);
    } else if (rest > std::ldexp(1.0, -134)) {
        fail("|x - hi - lo| > 2^-134 below 2^-118", x);
    }
    uint32_t ph, pl;
    dn_bf16_split_pair(x, -x, &ph, &pl);
    uint16_t nh, nl;
    dn_bf16_split(-x, &nh, &nl);
    if (ph != ((uint32_t)hi | ((uint32_t)nh << 16)) || pl != ((uint32_t)lo | ((uint32_t)nl << 16))) fail("pair form", x);
}

int main(int argc, char **argv)
{
    const long long random = argc > 1 ? std::atoll(argv[1]) : 4000000;
    for (uint32_t e = 0; e < 256; ++e)                         // every exponent, subnormals and infinity / NaN included
        for (uint32_t s = 0; s < 2; ++s) {
            const uint32_t base = (s << 31) | (e << 23);
            const uint32_t mant[] = {0u, 1u, 0x7fffffu, 0x7ffffeu, 0x400000u, 0x3fffffu, 0x008000u, 0x007fffu, 0x018000u, 0x017fffu,
                                     0x7f8000u, 0x7f7fffu, 0x7f8001u, 0x00ffffu, 0x010000u, 0x7f0000u, 0x7fff80u, 0x000080u};
            for (uint32_t m : mant) check(from_bits(base | m));
            for (uint32_t m = 0; m < 0x800000u; m += 0x1fff) check(from_bits(base | m));
        }
    for (uint32_t m = 0; m < 0x800000u; m += 7) check(from_bits(m));                 // subnormals, densely
    uint64_t z = 0x9e3779b97f4a7c15ull;
    for (long long i = 0; i < random; ++i) {                   // splitmix64
        z += 0x9e3779b97f4a7c15ull;
        uint64_t v = z;
        v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
        v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
        v ^= v >> 31;
        check(from_bits((uint32_t)v));
    }
    std::printf("{\"checked\": %lld, \"failures\": %lld, \"worst_relative_rest\": %.6e}\n", checked, failures, worst);
    return failures ? 1 : 0;
}
