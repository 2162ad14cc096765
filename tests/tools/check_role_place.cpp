// dn_place_roles (csrc/dn_role_place.h), the roles of a five-wave tile from the SIMDs its waves landed on, over its whole domain.  Host
// code only: dn_role_place.h is the one project header included.
//
// Prints {"cases": n, "named": m, "same": s, "forced": f, "ranked": r, "bad": b}; exit status 1 when b > 0.  The walk: all 4^5 = 1 024
// placements (wave 0's SIMD slowest), each for a CU's first and second tile.  `named` counts the placements the table names, `bad` counts
//   - results that are no permutation of the five roles, or whose packed form disagrees with dn_place_role wave by wave;
//   - placements the table does not name -- every one that is not 2 1 1 1 waves per SIMD, found here by counting, not by the header --
//     that do not give the wave-index orders L Q A N X | A N L Q X written out below;
//   - named placements whose result differs from the table row read by a rank found here by sorting;
//   - the spot rows: the eight placements the hardware makes (a cyclic walk 0 2 1 3 from each start), which must give the wave orders
//     X L Q A N in a first tile and A N Q L X in a second, written out by hand from profiles/role_placement.md.
// The overload that takes the fallback orders as an argument (what the sweep build of the five-wave kernel calls, tests/test_gpu_role_sweep.py):
//   - same: 2 048 = the walk above once more; with the shipped table and the shipped orders it gives dn_place_roles, wave by wave;
//   - forced: 245 760 = 120 x 1 024 x 2; with a table of eight rows "-----" and the orders (pi, pi rotated by two places), pi each of the
//     120 permutations of L A Q X N, wave w of a first tile gets pi[w] and of a second tile pi[(w + 2) % 5], whatever the placement;
//   - ranked: 57 600 = 120 x 240 x 2; with all four rows of a tile equal to pi (second tile: pi rotated) and the shipped orders, a placement
//     with 2 1 1 1 waves per SIMD gives the wave of rank r (found here by sorting) the row's letter r.
// A case whose five waves do not all get the stated role counts once in `bad`.
#include "dn_role_place.h"

#include <algorithm>
#include <cstdio>

static const char LETTERS[] = "LAQXN";
static_assert(dn_role_of_letter('L') == 0 && dn_role_of_letter('A') == 1 && dn_role_of_letter('Q') == 2 && dn_role_of_letter('X') == 3 &&
              dn_role_of_letter('N') == 4, "role numbers of the kernel's branches");
constexpr int SPOT[5] = {2, 1, 3, 0, 2};
static_assert(dn_place_roles(SPOT, false) == (3u | 0u << 3 | 2u << 6 | 1u << 9 | 4u << 12), "usable in a constant expression: X L Q A N");

int main()
{
    const char today[2][6] = {"LQANX", "ANLQX"};
    long cases = 0, named = 0, bad = 0;
    for (int code = 0; code < 1024; ++code)
        for (int second = 0; second < 2; ++second) {
            int simd[5];
            for (int w = 0; w < 5; ++w) simd[w] = (code >> (2 * (4 - w))) & 3;
            const unsigned packed = dn_place_roles(simd, second != 0);
            ++cases;
            unsigned seen = 0;
            int role[5];
            for (int w = 0; w < 5; ++w) {
                role[w] = (int)((packed >> (3 * w)) & 7u);
                if (role[w] > 4 || role[w] != dn_place_role(simd, second != 0, w)) { ++bad; role[w] = 0; }
                seen |= 1u << role[w];
            }
            if (seen != 31u || (packed >> 15) != 0u) ++bad;
            int count[4] = {0, 0, 0, 0}, doubled = -1;
            for (int w = 0; w < 5; ++w) ++count[simd[w]];
            bool is_2111 = true;
            for (int s = 0; s < 4; ++s) {
                if (count[s] == 0 || count[s] > 2) is_2111 = false;
                if (count[s] == 2) doubled = s;
            }
            if (is_2111 != (dn_place_pattern(simd) >= 0) || (is_2111 && dn_place_pattern(simd) != doubled)) ++bad;
            const char *row = is_2111 ? DN_ROLE_TABLE.row[second][doubled] : nullptr;
            if (row && row[0] != '-') {
                ++named;
                int order[5] = {0, 1, 2, 3, 4};
                std::sort(order, order + 5, [&](int a, int b) { return simd[a] != simd[b] ? simd[a] < simd[b] : a < b; });
                for (int rank = 0; rank < 5; ++rank)
                    if (LETTERS[role[order[rank]]] != row[rank]) ++bad;
            } else {
                for (int w = 0; w < 5; ++w)
                    if (LETTERS[role[w]] != today[second][w]) ++bad;
            }
        }
    const int cycle[4] = {0, 2, 1, 3};
    const char want[2][6] = {"XLQAN", "ANQLX"};
    for (int start = 0; start < 4; ++start)
        for (int second = 0; second < 2; ++second) {
            int simd[5];
            for (int w = 0; w < 5; ++w) simd[w] = cycle[(start + w) % 4];
            for (int w = 0; w < 5; ++w)
                if (LETTERS[dn_place_role(simd, second != 0, w)] != want[second][w]) ++bad;
        }
    long same = 0, forced = 0, ranked = 0;
    const DnRoleTable dashes = {{{"-----", "-----", "-----", "-----"}, {"-----", "-----", "-----", "-----"}}};
    char pi[6] = "ALNQX";                                   // sorted: std::next_permutation walks all 120
    int perms = 0;
    do {
        ++perms;
        char order[2][6] = {};
        DnRoleTable rows = {};
        for (int w = 0; w < 5; ++w) { order[0][w] = pi[w]; order[1][w] = pi[(w + 2) % 5]; }
        for (int tile = 0; tile < 2; ++tile)
            for (int pattern = 0; pattern < 4; ++pattern)
                for (int k = 0; k < 6; ++k) rows.row[tile][pattern][k] = order[tile][k];
        for (int code = 0; code < 1024; ++code)
            for (int second = 0; second < 2; ++second) {
                int simd[5], count[4] = {0, 0, 0, 0};
                for (int w = 0; w < 5; ++w) { simd[w] = (code >> (2 * (4 - w))) & 3; ++count[simd[w]]; }
                bool ok = true;
                if (perms == 1) {                           // the shipped table and orders: once
                    for (int w = 0; w < 5; ++w)
                        ok = ok && dn_place_role_with(DN_ROLE_TABLE, DN_ROLE_ORDER, simd, second != 0, w) == (int)((dn_place_roles(simd, second != 0) >> (3 * w)) & 7u);
                    ++same;
                    if (!ok) ++bad;
                    ok = true;
                }
                for (int w = 0; w < 5; ++w)
                    ok = ok && LETTERS[dn_place_role_with(dashes, order, simd, second != 0, w)] == order[second][w];
                ++forced;
                if (!ok) ++bad;
                if (count[0] == 0 || count[1] == 0 || count[2] == 0 || count[3] == 0) continue;        // five waves on four SIMDs, none empty: 2 1 1 1
                int by_rank[5] = {0, 1, 2, 3, 4};
                std::sort(by_rank, by_rank + 5, [&](int a, int b) { return simd[a] != simd[b] ? simd[a] < simd[b] : a < b; });
                ok = true;
                for (int rank = 0; rank < 5; ++rank)
                    ok = ok && LETTERS[dn_place_role_with(rows, DN_ROLE_ORDER, simd, second != 0, by_rank[rank])] == order[second][rank];
                ++ranked;
                if (!ok) ++bad;
            }
    } while (std::next_permutation(pi, pi + 5));
    if (perms != 120) ++bad;
    std::printf("{\"cases\": %ld, \"named\": %ld, \"same\": %ld, \"forced\": %ld, \"ranked\": %ld, \"bad\": %ld}\n", cases, named, same, forced, ranked, bad);
    return bad > 0 ? 1 : 0;
}
