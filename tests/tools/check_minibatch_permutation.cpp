// check_minibatch_permutation.cpp -- the keyed permutation of csrc/dn_permute.h as a stand-alone host program (tests/test_minibatch_cpu.py
// builds it with the host compiler, plainly and under the address and undefined-behaviour sanitizers).  For every (M, seed, epoch) of the
// test it checks with a bitmap that pi is a bijection of [0, M) and prints pi, one line each: "M seed epoch : pi(0) pi(1) ...".  The last
// line is a JSON object with the number of cases and of failures; the exit status is 1 when there is a failure.
#include <cstdio>
#include <vector>

#include "dn_permute.h"

int main()
{
    const uint32_t sizes[] = {1, 2, 3, 4, 5, 17, 64, 1000, 1025, 4097, 65537};
    const uint64_t seeds[] = {0, 7, ~0ull}, epochs[] = {0, 1, 1ull << 40};
    int cases = 0, bad = 0;
    for (const uint32_t m : sizes)
        for (const uint64_t seed : seeds)
            for (const uint64_t epoch : epochs) {
                const DnPermutation p = dn_permute_make(seed, epoch, m);
                std::vector<bool> seen(m, false);
                std::printf("%u %llu %llu :", m, (unsigned long long)seed, (unsigned long long)epoch);
                bool ok = true;
                for (uint32_t i = 0; i < m; ++i) {
                    const uint32_t v = dn_permute_at(p, i);
                    std::printf(" %u", v);
                    if (v >= m || seen[v]) ok = false;
                    else seen[v] = true;
                }
                std::printf("\n");
                ++cases;
                bad += !ok;
            }
    std::printf("{\"cases\": %d, \"bad\": %d}\n", cases, bad);
    return bad ? 1 : 0;
}
