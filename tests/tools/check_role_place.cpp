// dn_place_roles (csrc/dn_role_place.h), the roles of a five-wave tile from the SIMDs its waves landed on, over its whole domain.  Host
// code only: dn_role_place.h is the one project header included.
//
// Prints {"cases": n, "named": m, "bad": b}; exit status 1 when b > 0.  The walk: all 4^5 = 1 024 placements (wave 0's SIMD slowest), each
// for a CU's first and second tile.  `named` counts the placements the table names, `bad` counts
//   - results that are no permutation of the five roles, or whose packed form disagrees with dn_place_role wave by wave;
//   - placements the table does not name -- every one that is not 2 1 1 1 waves per SIMD, found here by counting, not by the header --
//     that do not give the wave-index orders L Q A N X | A N L Q X written out below;
//   - named placements whose result differs from the table row read by a rank found here by sorting;
//   - the spot rows: the eight placements the hardware makes (a cyclic walk 0 2 1 3 from each start), which must give the wave orders
//     X L Q A N in a first tile and A N Q L X in a second, written out by hand from profiles/role_placement.md.
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
    std::printf("{\"cases\": %ld, \"named\": %ld, \"bad\": %ld}\n", cases, named, bad);
    return bad > 0 ? 1 : 0;
}
