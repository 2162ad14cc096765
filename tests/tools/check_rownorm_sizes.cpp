// dn_rownorm_scratch_doubles / dn_rownorm_blocks (csrc/dn_internal.h): the scratch of dn_rownorm over width 1 .. 64, k in {1, 2, 64} and
// n in {1, 63, 64, 65, 1000, 2^21}, against the rule dn_internal.h states, written out independently of the functions: per step one
// partial of 2 width doubles per block of DN_ROWNORM_BLOCK_ROWS rows (the last block may be short) and one snapshot of 2 width doubles.
// Asserts that the size is positive, covers partials + snapshots, grows with k and with n, and that bad arguments are refused (0) without
// overflow.  Prints {"cases": n, "bad": b}; exit status 1 when b > 0.  Host code only.
#include "dn_internal.h"

#include <climits>
#include <cstdio>

static long long want_doubles(long long k, long long n, int w)
{
    long long blocks = 0;
    for (long long row = 0; row < n; row += DN_ROWNORM_BLOCK_ROWS) ++blocks;
    long long d = 0;
    for (long long t = 0; t < k; ++t) d += blocks * 2 * w + 2 * w;
    return d;
}

int main()
{
    int cases = 0, bad = 0;
    const long long ks[] = {1, 2, 64}, ns[] = {1, 63, 64, 65, 1000, 1ll << 21};
    for (int w = 1; w <= DN_ROWNORM_MAX_WIDTH; ++w) {
        long long prev_k[6] = {0, 0, 0, 0, 0, 0};          // the size at the previous k, per n
        for (long long k : ks) {
            long long prev_n = 0;
            int ni = 0;
            for (long long n : ns) {
                const long long got = dn_rownorm_scratch_doubles(k, n, w), want = want_doubles(k, n, w);
                const bool ok = got > 0 && got == want && got >= prev_n && got > prev_k[ni];
                if (!ok) {
                    ++bad;
                    std::fprintf(stderr, "w %d k %lld n %lld: %lld doubles, want %lld (previous n %lld, previous k %lld)\n", w, k, n, got, want,
                                 prev_n, prev_k[ni]);
                }
                prev_n = prev_k[ni++] = got;
                ++cases;
            }
        }
    }
    const auto refused = [&](long long k, long long n, int w) {
        if (dn_rownorm_scratch_doubles(k, n, w) != 0) {
            ++bad;
            std::fprintf(stderr, "k %lld n %lld w %d is not refused\n", k, n, w);
        }
        ++cases;
    };
    refused(1, 1, 0);
    refused(1, 1, 65);
    refused(1, 1, -1);
    refused(0, 1, 13);
    refused(1, 0, 13);
    refused(-1, -1, 13);
    refused(LLONG_MAX, LLONG_MAX, 64);      // no overflow on the way to the refusal
    refused(LLONG_MAX, 1, 64);
    refused(1, LLONG_MAX, 64);
    refused(LLONG_MIN, LLONG_MIN, INT_MIN);
    std::printf("{\"cases\": %d, \"bad\": %d}\n", cases, bad);
    return bad ? 1 : 0;
}
