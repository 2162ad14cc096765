// dn_role_place.h -- which wave of a five-wave tile runs which role, from the SIMDs the hardware put the waves on.
//
// Standard C++ only (constexpr functions, which the device compiler takes as they are): the five-wave fused step calls
// dn_place_role on the device, and tests/tools/check_role_place.cpp walks dn_place_roles over all 4^5 placements on the CPU.
//
// The step's results do not depend on the answer: a role only says which wave runs which function (tests/test_gpu_role_sweep.py runs
// the kernel under all 120 assignments a tile can get).  What depends on it is which roles share a SIMD, i.e. the step time
// (profiles/role_placement.md).
#ifndef DN_ROLE_PLACE_H
#define DN_ROLE_PLACE_H

constexpr int DN_ROLE_L = 0, DN_ROLE_A = 1, DN_ROLE_Q = 2, DN_ROLE_X = 3, DN_ROLE_N = 4, DN_ROLES = 5;

constexpr int dn_role_of_letter(char ch) { return ch == 'L' ? DN_ROLE_L : ch == 'A' ? DN_ROLE_A : ch == 'Q' ? DN_ROLE_Q : ch == 'X' ? DN_ROLE_X : DN_ROLE_N; }

// The wave-index orders (round 3): wave w of a CU's first tile runs DN_ROLE_ORDER[0][w], of its second tile DN_ROLE_ORDER[1][w].
// They hold for every placement the table below does not name (none was seen in 24 576 workgroup-launches of the census).
constexpr char DN_ROLE_ORDER[2][6] = {"LQANX", "ANLQX"};

// A placement the table names has every SIMD of the CU hold one wave of the tile and one SIMD hold two: the PATTERN is that SIMD's id.
// The waves are ranked by (SIMD id, wave index); the table gives the role of each rank.  A row of five '-' names nothing.
struct DnRoleTable { char row[2][4][6]; };      // [second tile][doubled SIMD][rank]

// What the census found (profiles/role_placement.md): a workgroup's waves go to the SIMDs in the cyclic order 0 2 1 3 from a start
// that differs from CU to CU, so waves 0 and 4 share the start SIMD; the second tile of a CU (tile b + num_cus beside tile b) starts
// one place further on in 98.6 % of CU-launches.  With p the start of the first tile, the ten waves of a CU sit
//     place p: T1w0 T1w4 T2w3     p + 1: T1w1 T2w0 T2w4     p + 2: T1w2 T2w1     p + 3: T1w3 T2w2
// The rows below are the winner of the sweep over all 120 x 120 pairs of wave orders (profiles/sweep_5w_roles.py), X L Q A N in a
// CU's first tile and A N Q L X in its second, stated per doubled SIMD:
//     place p: X1 N1 L2           p + 1: L1 A2 X2           p + 2: Q1 N2         p + 3: A1 Q2
// Each tile keeps its two lightest roles (X and N; A and X beside the other tile's L) on the SIMD that holds two of its waves.
// 32 768 drones, 64-step launches: 1.221 us per step against 1.265 with the orders above in every placement.
constexpr DnRoleTable DN_ROLE_TABLE = {{{"XNQLA", "QXNAL", "ALXNQ", "LAQXN"}, {"AXQNL", "QAXLN", "LNAXQ", "NLQAX"}}};

// The doubled SIMD of a named pattern, -1 of any other placement (a SIMD id is two bits, as HW_ID gives it).
constexpr int dn_place_pattern(const int simd[DN_ROLES])
{
    unsigned counts = 0;                                    // one nibble per SIMD
    for (int w = 0; w < DN_ROLES; ++w) counts += 1u << (4 * (simd[w] & 3));
    const unsigned extra = counts - 0x1111u;                // 2 1 1 1 in some order: one bit, in the doubled SIMD's nibble
    return extra == 0x1u ? 0 : extra == 0x10u ? 1 : extra == 0x100u ? 2 : extra == 0x1000u ? 3 : -1;
}

// The rank of wave w among the tile's five by (SIMD id, wave index).
constexpr int dn_place_rank(const int simd[DN_ROLES], int w)
{
    int rank = 0;
    for (int v = 0; v < DN_ROLES; ++v) {
        const int a = simd[v] & 3, b = simd[w] & 3;
        rank += (a < b || (a == b && v < w)) ? 1 : 0;
    }
    return rank;
}

// The role of wave w under `table`, and under the wave-index orders `order` in every placement the table does not name.  With a table of
// eight rows "-----" wave w runs order[tile][w] whatever the placement: how the sweep build of the kernel forces an assignment
// (tests/test_gpu_role_sweep.py).
constexpr int dn_place_role_with(const DnRoleTable &table, const char (&order)[2][6], const int simd[DN_ROLES], bool second_tile, int w)
{
    const int pattern = dn_place_pattern(simd);
    if (pattern >= 0 && table.row[second_tile ? 1 : 0][pattern][0] != '-')
        return dn_role_of_letter(table.row[second_tile ? 1 : 0][pattern][dn_place_rank(simd, w)]);
    return dn_role_of_letter(order[second_tile ? 1 : 0][w]);
}

// The role of wave w under `table` and the orders above.
constexpr int dn_place_role_with(const DnRoleTable &table, const int simd[DN_ROLES], bool second_tile, int w)
{
    return dn_place_role_with(table, DN_ROLE_ORDER, simd, second_tile, w);
}

// The role of wave w: what the kernel asks.
constexpr int dn_place_role(const int simd[DN_ROLES], bool second_tile, int w) { return dn_place_role_with(DN_ROLE_TABLE, simd, second_tile, w); }

// THE function: the five waves' SIMD ids -> the five roles, three bits each, wave 0 lowest.
constexpr unsigned dn_place_roles(const int simd[DN_ROLES], bool second_tile)
{
    unsigned packed = 0;
    for (int w = 0; w < DN_ROLES; ++w) packed |= (unsigned)dn_place_role(simd, second_tile, w) << (3 * w);
    return packed;
}

#endif
