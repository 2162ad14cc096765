// check_argcheck.cpp -- csrc/dn_argcheck.h on the host: dn_ranges_overlap against the rule written out independently (128-bit interval
// arithmetic, and case by case at the top of the address space), and the three walks over DnArg tables with the offending entry first,
// in the middle, last and absent, with and without optional NULLs.  Prints {"cases": n, "bad": b}; exit status 1 when b > 0.
// The addresses are numbers: nothing here is ever followed.
#include "dn_argcheck.h"

#include <cstdio>
#include <initializer_list>

typedef unsigned __int128 u128;

static long long cases = 0, bad = 0;

static const void *at(uintptr_t a) { return (const void *)a; }

static void expect(bool got, bool want, const char *what, unsigned long long a, unsigned long long ab, unsigned long long b, unsigned long long bb)
{
    ++cases;
    if (got != want) {
        ++bad;
        fprintf(stderr, "%s: [%#llx + %llu) [%#llx + %llu): got %d, want %d\n", what, a, ab, b, bb, (int)got, (int)want);
    }
}

// the rule for ranges that end at or below UINTPTR_MAX: two half-open intervals meet iff the larger start is below the smaller end
static bool intervals_meet(uintptr_t a, uintptr_t ab, uintptr_t b, uintptr_t bb)
{
    if (a == 0 || b == 0 || ab == 0 || bb == 0) return false;
    const u128 ae = (u128)a + ab, be = (u128)b + bb;
    const u128 lo = a > b ? a : b, hi = ae < be ? ae : be;
    return lo < hi;
}

static void both_orders(uintptr_t a, uintptr_t ab, uintptr_t b, uintptr_t bb, bool want, const char *what)
{
    expect(dn_ranges_overlap(at(a), ab, at(b), bb), want, what, a, ab, b, bb);
    expect(dn_ranges_overlap(at(b), bb, at(a), ab), want, what, b, bb, a, ab);
}

static void walk_ranges()
{
    // apart, touching, sharing one byte, nested, equal; zero bytes on either side
    const uintptr_t A = 0x1000, sizes_a[] = {0, 1, 16}, sizes_b[] = {0, 1, 4, 16, 64};
    for (uintptr_t ab : sizes_a)
        for (int d = -20; d <= 20; ++d)
            for (uintptr_t bb : sizes_b) {
                const uintptr_t b = A + (uintptr_t)(intptr_t)d;
                both_orders(A, ab, b, bb, intervals_meet(A, ab, b, bb), "grid");
            }
    // a NULL pointer on either side, and on both
    for (uintptr_t ab : {(uintptr_t)0, (uintptr_t)16})
        for (uintptr_t bb : {(uintptr_t)0, (uintptr_t)16}) {
            expect(dn_ranges_overlap(nullptr, ab, at(8), bb), false, "null a", 0, ab, 8, bb);
            expect(dn_ranges_overlap(at(8), ab, nullptr, bb), false, "null b", 8, ab, 0, bb);
            expect(dn_ranges_overlap(nullptr, ab, nullptr, bb), false, "null both", 0, ab, 0, bb);
        }
    // the top of the address space.  T ends at UINTPTR_MAX: the interval rule holds.  W ends one past it (its end wraps to 0): it
    // overlaps nothing, itself included -- the arithmetic the entry points have always had.
    const uintptr_t M = UINTPTR_MAX, T = M - 16, W = M - 15;
    const struct { uintptr_t b, bb; bool with_t; } near_top[] = {
        {M - 32, 16, false}, {M - 32, 17, true}, {M - 8, 4, true}, {M - 1, 1, true}, {T, 16, true}};
    for (const auto &c : near_top) {
        both_orders(T, 16, c.b, c.bb, c.with_t, "ends at UINTPTR_MAX");
        if (intervals_meet(T, 16, c.b, c.bb) != c.with_t) ++bad;       // the table above against the interval rule
        both_orders(W, 16, c.b, c.bb, false, "ends one past UINTPTR_MAX");
    }
    both_orders(W, 16, W, 16, false, "ends one past UINTPTR_MAX");
}

static void expect_entry(const DnArg *got, const DnArg *want, const char *what, int where, bool nulls)
{
    ++cases;
    if (got != want) {
        ++bad;
        fprintf(stderr, "%s: offender %d, optional nulls %d: got entry %s, want %s\n", what, where, (int)nulls, got ? got->name : "none",
                want ? want->name : "none");
    }
}

// five entries, 64 bytes each and 256 apart from `base`; entries 1 and 3 are optional, and NULL when nulls is set
static void fill(DnArg (&t)[5], uintptr_t base, bool nulls)
{
    static const char *const names[] = {"e0", "e1", "e2", "e3", "e4"};
    for (int i = 0; i < 5; ++i) t[i] = DnArg{names[i], at(base + 256u * (uintptr_t)i), 64, i % 2 == 1};
    if (nulls) t[1].p = t[3].p = nullptr;
}

static void walk_tables()
{
    const int offenders[] = {0, 2, 4, -1};      // first, middle, last, absent
    for (bool nulls : {false, true})
        for (int where : offenders) {
            DnArg t[5];
            // a required pointer that is NULL
            fill(t, 0x10000, nulls);
            if (where >= 0) t[where].p = nullptr;
            expect_entry(dn_first_missing(t), where >= 0 ? &t[where] : nullptr, "missing", where, nulls);
            // a pointer off an 8-byte and off a 4-byte boundary; the pointers after it are off as well, the first one is reported
            for (uintptr_t mask : {(uintptr_t)7, (uintptr_t)3}) {
                fill(t, 0x10000, nulls);
                for (int i = where; i >= 0 && i < 5; ++i)
                    if (t[i].p) t[i].p = at((uintptr_t)t[i].p + (mask == 7 ? 4 : 2));
                expect_entry(dn_first_misaligned(t, mask), where >= 0 ? &t[where] : nullptr, mask == 7 ? "misaligned 8" : "misaligned 4", where, nulls);
            }
            // an output that shares its last byte with the start of the input of the same index
            DnArg in[5], out[5];
            fill(in, 0x10000, nulls);
            fill(out, 0x20000, nulls);
            if (where >= 0) out[where].p = at((uintptr_t)in[where].p - 63);
            const DnArg *o = nullptr, *i = nullptr;
            const bool found = dn_first_overlap(out, in, &o, &i);
            expect_entry(found ? o : nullptr, where >= 0 ? &out[where] : nullptr, "overlap: output", where, nulls);
            expect_entry(found ? i : nullptr, where >= 0 ? &in[where] : nullptr, "overlap: input", where, nulls);
        }
    // two pairs overlap: the outputs are the outer loop, so (out 0, in 4) is reported before (out 2, in 0)
    for (bool nulls : {false, true}) {
        DnArg in[5], out[5];
        fill(in, 0x10000, nulls);
        fill(out, 0x20000, nulls);
        out[2].p = in[0].p;
        out[0].p = at((uintptr_t)in[4].p + 32);
        const DnArg *o = nullptr, *i = nullptr;
        const bool found = dn_first_overlap(out, in, &o, &i);
        expect_entry(found ? o : nullptr, &out[0], "overlap order: output", 0, nulls);
        expect_entry(found ? i : nullptr, &in[4], "overlap order: input", 4, nulls);
    }
    // the scratch predicate
    const struct { long long have; bool is_short; } scratch[] = {{-1, true}, {0, true}, {15, true}, {16, false}, {17, false}, {1ll << 62, false}};
    for (const auto &c : scratch) {
        ++cases;
        if (dn_scratch_short(c.have, 16) != c.is_short) ++bad;
    }
}

int main()
{
    walk_ranges();
    walk_tables();
    printf("{\"cases\": %lld, \"bad\": %lld}\n", cases, bad);
    return bad > 0 ? 1 : 0;
}
