// dn_retnorm_scratch_doubles / dn_retnorm_chunks / dn_retnorm_grids_ok (csrc/dn_internal.h): the scratch and the grids of dn_retnorm over
// k in {1, 2, 64} and n in {1, 63, 64, 65, 1000, 2^21}, against the rule dn_internal.h states, written out independently of the functions:
// per step one partial of 2 doubles per block of DN_ROWNORM_BLOCK_ROWS drones (the last block may be short) and one snapshot of 2
// doubles; one scale workgroup per DN_RETNORM_CHUNK rewards of a step.  Asserts that the size is positive, covers partials + snapshots,
// grows with k and with n, that the grids of these shapes are accepted, and that bad arguments are refused (0 / false) without overflow.
// Prints {"cases": n, "bad": b}; exit status 1 when b > 0.  Host code only.
#include "dn_internal.h"

#include <climits>
#include <cstdio>

static long long want_doubles(long long k, long long n)
{
    long long blocks = 0;
    for (long long row = 0; row < n; row += DN_ROWNORM_BLOCK_ROWS) ++blocks;
    long long d = 0;
    for (long long t = 0; t < k; ++t) d += blocks * 2 + 2;
    return d;
}

static long long want_chunks(long long n)
{
    long long chunks = 0;
    for (long long e = 0; e < n; e += DN_RETNORM_CHUNK) ++chunks;
    return chunks;
}

int main()
{
    int cases = 0, bad = 0;
    const long long ks[] = {1, 2, 64}, ns[] = {1, 63, 64, 65, 1000, 1ll << 21};
    long long prev_k[6] = {0, 0, 0, 0, 0, 0};              // the size at the previous k, per n
    for (long long k : ks) {
        long long prev_n = 0;
        int ni = 0;
        for (long long n : ns) {
            const long long got = dn_retnorm_scratch_doubles(k, n), want = want_doubles(k, n);
            const bool ok = got > 0 && got == want && got >= prev_n && got > prev_k[ni] && dn_retnorm_chunks(n) == want_chunks(n) &&
                            dn_retnorm_grids_ok(k, n);
            if (!ok) {
                ++bad;
                std::fprintf(stderr, "k %lld n %lld: %lld doubles, want %lld (previous n %lld, previous k %lld); %lld chunks, want %lld; grids %d\n",
                             k, n, got, want, prev_n, prev_k[ni], dn_retnorm_chunks(n), want_chunks(n), (int)dn_retnorm_grids_ok(k, n));
            }
            prev_n = prev_k[ni++] = got;
            ++cases;
        }
    }
    const auto refused = [&](long long k, long long n) {
        if (dn_retnorm_scratch_doubles(k, n) != 0) {
            ++bad;
            std::fprintf(stderr, "k %lld n %lld is not refused\n", k, n);
        }
        ++cases;
    };
    refused(0, 1);
    refused(1, 0);
    refused(-1, -1);
    refused(LLONG_MAX, LLONG_MAX);      // no overflow on the way to the refusal
    refused(LLONG_MAX, 1);
    refused(LLONG_MIN, LLONG_MIN);
    const auto grid = [&](long long k, long long n, bool want) {
        if (dn_retnorm_grids_ok(k, n) != want) {
            ++bad;
            std::fprintf(stderr, "grids of k %lld n %lld: %s\n", k, n, want ? "refused" : "not refused");
        }
        ++cases;
    };
    grid(0x7fffffffll, DN_RETNORM_CHUNK, true);            // 2^31 - 1 scale workgroups
    grid(0x7fffffffll, DN_RETNORM_CHUNK + 1, false);       // two chunks per step
    grid(1ll << 20, 1ll << 23, false);                     // 2^20 x 2048 = 2^31
    grid(1, 0x7fffffffll * DN_ROWNORM_BLOCK_ROWS, true);   // 2^31 - 1 blocks
    grid(1, 0x7fffffffll * DN_ROWNORM_BLOCK_ROWS + 1, false);
    grid(LLONG_MAX, LLONG_MAX, false);
    grid(0, 1, false);
    grid(1, LLONG_MIN, false);
    std::printf("{\"cases\": %d, \"bad\": %d}\n", cases, bad);
    return bad ? 1 : 0;
}
