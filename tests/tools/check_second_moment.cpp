// dn_restore_second_moment / second_moment (csrc/dn_second_moment.h), the rule by which dn_set_state rebuilds the observation
// normaliser's second moment M2 = var x count from a dn_env_state, over a fixed seeded walk.  Host code only: dn_second_moment.h is the
// one project header included.
//
// Prints {"cases": n, "edges": e, "lossy": l, "bad": b}; exit status 1 when b > 0.  The walk: three count families x 400 000 draws, each
// with an M2 log-uniform over [1e-12, 1e6] from a splitmix64 stream (seed 20240610) --
//     count = 1e-4 + k, k uniform in 0..5000 (k = 0: the 1e-4 RunningMeanStd starts at; otherwise what a drone's count is after k rows),
//     count = k, k uniform in 1..5000 (a producer that starts at 0),
//     count = an integer uniform in 1..2^40 (long runs);
// then the edges: M2 = 0, denormal M2 (the smallest and the largest), the reset pair (1e-4, 1e-4), and counts 1e-4 / 1 / 2^53 / 1e15 + 1e-4 /
// 1e300 with the M2 1e-12, 1, 1e6.  For every pair, with var = M2 / count as dn_get_state forms it, `bad` counts
//   - a verbatim hint (M2 itself) that does not come back bit for bit;
//   - an edited var -- the previous pair's M2 over this count, and 0.25 -- with the hint left stale whose result does not divide back to
//     the edited var (both edits have an M2 that does: the first is a quotient by this count, the second a power of two);
//   - a zero hint (a producer that does not fill it) with nonzero var that does not give exactly second_moment(var, count);
//   - an edited count (hint left stale) whose result does not divide back to the var given: twice the count (var x 2 count has the bits
//     of var x count, so an M2 exists), and count + 1 wherever some M2 within two ulp of var x (count + 1) divides back at all;
// and, once, the counts dn_set_state refuses: 0, -0, -1, NaN, +inf, -inf must fail dn_rms_count_ok and (the non-positive ones and NaN)
// must not take the hint; 1e-4, the smallest denormal and 1e300 must pass it.
// `lossy` counts the pairs the old rule alone would have got wrong: second_moment(M2 / count, count) != M2.
#include "dn_second_moment.h"

#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

static uint64_t g_state = 20240610u;
static uint64_t next_u64()
{
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double next_unit() { return (double)(next_u64() >> 11) * 0x1.0p-53; }      // [0, 1)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static long g_cases = 0, g_lossy = 0, g_bad = 0;

// Whether any double within two ulp of var x count divides back to var: a var that is no quotient by this count may have none (where
// M2 sits low in its binade and var high in its own, neighbouring M2 divide to values two ulp of var apart).
static bool reachable(double var, double count)
{
    double m = var * count;
    m = std::nextafter(std::nextafter(m, -HUGE_VAL), -HUGE_VAL);
    for (int k = 0; k < 5; ++k, m = std::nextafter(m, HUGE_VAL))
        if (m / count == var) return true;
    return false;
}

static void check_pair(double m2, double count, double other_m2)
{
    ++g_cases;
    const double var = m2 / count;
    if (!same_bits(dn_restore_second_moment(var, count, m2), m2)) ++g_bad;
    if (!same_bits(second_moment(var, count), m2)) ++g_lossy;
    const double edits[2] = {other_m2 / count, 0.25};
    for (double edited : edits) {
        const double got = dn_restore_second_moment(edited, count, m2);
        if (got / count != edited) ++g_bad;
    }
    if (var != 0.0 && !same_bits(dn_restore_second_moment(var, count, 0.0), second_moment(var, count))) ++g_bad;
    if (var != 0.0 && dn_restore_second_moment(var, count, 0.0) / count != var) ++g_bad;
    const double twice = 2.0 * count, plus = count + 1.0;
    if (dn_restore_second_moment(var, twice, m2) / twice != var) ++g_bad;
    if (plus != count && reachable(var, plus) && dn_restore_second_moment(var, plus, m2) / plus != var) ++g_bad;
}

int main()
{
    const double lo = std::log(1e-12), span = std::log(1e6) - lo;
    const long per_family = 400000;
    double prev = 1.0;
    for (int family = 0; family < 3; ++family)
        for (long i = 0; i < per_family; ++i) {
            const double m2 = std::exp(lo + span * next_unit());
            const uint64_t r = next_u64();
            const double count = family == 0 ? 1e-4 + (double)(r % 5001u) : family == 1 ? (double)(1 + r % 5000u) : (double)(1 + (r >> 24));
            check_pair(m2, count, prev);
            prev = m2;
        }
    const long walked = g_cases;
    const double edge_counts[] = {1e-4, 1.0, 0x1.0p53, 1e15 + 1e-4, 1e300};
    const double edge_m2[] = {0.0, std::numeric_limits<double>::denorm_min(), DBL_MIN - std::numeric_limits<double>::denorm_min(), 1e-12, 1e-4, 1.0, 1e6};
    for (double count : edge_counts)
        for (double m2 : edge_m2) {
            // a denormal var has fewer bits than M2: the pairs whose var = M2 / count is not a normal number or zero keep the verbatim
            // and zero-hint checks of check_pair, and the edit to 0.25 (the quotient edit needs a var that some M2 divides to)
            const double var = m2 / count;
            if (var == 0.0 || var >= DBL_MIN) { check_pair(m2, count, 1.0); continue; }
            ++g_cases;
            if (!same_bits(dn_restore_second_moment(var, count, m2), m2)) ++g_bad;
            if (!same_bits(dn_restore_second_moment(var, count, 0.0), second_moment(var, count))) ++g_bad;
            if (dn_restore_second_moment(0.25, count, m2) / count != 0.25) ++g_bad;
        }
    if (!same_bits(dn_restore_second_moment(1.0, 1e-4, 1.0 * 1e-4), 1e-4)) ++g_bad;      // dn_reset's words: var 1 held as 1.0 * 1e-4
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double refused[] = {0.0, -0.0, -1.0, nan, inf, -inf};
    for (double count : refused) {
        ++g_cases;
        if (dn_rms_count_ok(count)) ++g_bad;
        if (count == inf) continue;
        // no hint is taken: the result is var x count as second_moment passes it through (a NaN compares by its bits being a NaN)
        const double got = dn_restore_second_moment(0.5, count, 0.5 * 3.0), want = second_moment(0.5, count);
        if (!(same_bits(got, want) || (got != got && want != want)) || same_bits(got, 1.5)) ++g_bad;
    }
    const double taken[] = {1e-4, std::numeric_limits<double>::denorm_min(), 1e300};
    for (double count : taken) {
        ++g_cases;
        if (!dn_rms_count_ok(count)) ++g_bad;
    }
    std::printf("{\"cases\": %ld, \"edges\": %ld, \"lossy\": %ld, \"bad\": %ld}\n", g_cases, g_cases - walked, g_lossy, g_bad);
    return g_bad > 0 ? 1 : 0;
}
