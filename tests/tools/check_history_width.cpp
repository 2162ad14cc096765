// dn_history_row_width (csrc/dn_internal.h): the width of a history row of F observation frames, A action frames and E extra columns,
// over F = -1 .. 6, A = -2 .. 6, E = -1 .. 70 and three extreme inputs, against the rule written out independently of the function:
// refuse (0) outside 1 <= F <= 4, 0 <= A <= 4, E >= 0, else count the columns one by one, step up to a multiple of 4, and refuse beyond
// 64.  Prints {"cases": n, "bad": b}; exit status 1 when b > 0.  Host code only.
#include "dn_internal.h"

#include <climits>
#include <cstdio>

static int want_width(long long f, long long a, long long e)
{
    if (f < 1 || f > 4 || a < 0 || a > 4 || e < 0) return 0;
    long long cols = 0;
    for (long long j = 0; j < f; ++j) cols += 13;
    for (long long j = 0; j < a; ++j) cols += 4;
    cols += e;
    while (cols % 4) ++cols;
    return cols <= 64 ? (int)cols : 0;
}

int main()
{
    int cases = 0, bad = 0;
    const auto check = [&](int f, int a, int e) {
        const int got = dn_history_row_width(f, a, e), want = want_width(f, a, e);
        if (got != want) {
            ++bad;
            std::fprintf(stderr, "F %d A %d E %d: dn_history_row_width = %d, want %d\n", f, a, e, got, want);
        }
        ++cases;
    };
    for (int f = -1; f <= 6; ++f)
        for (int a = -2; a <= 6; ++a)
            for (int e = -1; e <= 70; ++e) check(f, a, e);
    check(4, 4, INT_MAX);           // no overflow on the way to the refusal
    check(INT_MAX, INT_MAX, INT_MAX);
    check(INT_MIN, INT_MIN, INT_MIN);
    std::printf("{\"cases\": %d, \"bad\": %d}\n", cases, bad);
    return bad ? 1 : 0;
}
