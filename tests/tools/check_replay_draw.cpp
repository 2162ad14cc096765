// check_replay_draw.cpp -- the keyed replay draw of csrc/dn_replay_draw.h as a stand-alone host program (tests/test_replay_cpu.py builds it
// with the host compiler, plainly and under the address and undefined-behaviour sanitizers).  For every case it prints the first rows, one
// line each: "seed draw S N skip : slot env slot env ...", after checking over 4096 rows that every slot is in [0, S + (skip >= 0)) and
// never `skip`, every drone in [0, N), and that row j read on its own is row j of the run.  The last line is a JSON object with the
// number of cases and of failures; the exit status is 1 when there is a failure.
#include <cstdio>
#include <vector>

#include "dn_replay_draw.h"

struct Case {
    uint64_t seed, draw;
    uint32_t s, n;
    int64_t skip;
};

int main()
{
    const uint32_t big = (uint32_t)DN_REPLAY_MAX;
    const Case cases[] = {{0, 0, 5, 7, -1},       {1, 2, 5, 7, 2},          {~0ull, ~0ull, big, big, -1}, {0x0123456789ABCDEFull, 1ull << 40, 1000, 32768, 0},
                          {7, 3, 1, 1, -1},       {7, 3, 1, 1, 0},          {7, 3, 1, 1, 1},              {9, 1, 63, 65, 63},
                          {9, 1ull << 63, 3, 1, 1}, {~0ull, 0, big, 1, big}, {0xDEADBEEF, 5, 1, big, -1}};
    const int rows = 4096, shown = 8;
    int n_cases = 0, bad = 0;
    for (const Case &c : cases) {
        const uint64_t key = dn_replay_key(c.seed, c.draw);
        std::vector<DnReplayPick> run(rows);
        bool ok = true;
        for (int j = 0; j < rows; ++j) {
            run[j] = dn_replay_draw_at(key, (uint64_t)j, c.s, c.n, c.skip);
            const int64_t slot = run[j].slot, flat = dn_replay_flat(run[j], c.n);
            if (slot >= (int64_t)c.s + (c.skip >= 0) || slot == c.skip || run[j].env >= c.n) ok = false;
            if (flat != slot * (int64_t)c.n + run[j].env || flat < 0) ok = false;
        }
        for (int j = rows - 1; j >= 0; j -= 7) {           // any row on its own, in any order
            const DnReplayPick p = dn_replay_draw_at(dn_replay_key(c.seed, c.draw), (uint64_t)j, c.s, c.n, c.skip);
            if (p.slot != run[j].slot || p.env != run[j].env) ok = false;
        }
        std::printf("%llu %llu %u %u %lld :", (unsigned long long)c.seed, (unsigned long long)c.draw, c.s, c.n, (long long)c.skip);
        for (int j = 0; j < shown; ++j) std::printf(" %u %u", run[j].slot, run[j].env);
        std::printf("\n");
        ++n_cases;
        bad += !ok;
    }
    std::printf("{\"cases\": %d, \"bad\": %d}\n", n_cases, bad);
    return bad ? 1 : 0;
}
