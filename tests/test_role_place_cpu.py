"""The roles of a five-wave tile from the SIMDs its waves landed on (csrc/dn_role_place.h dn_place_roles) over all 4^5 placements, on the
CPU: a stand-alone host program, built plainly and under the address and undefined-behaviour sanitizers, and run as its own process."""
import pytest

import host_program_support


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_every_placement_gives_a_permutation_of_the_roles(tmp_path, sanitize):
    """tests/tools/check_role_place.cpp states the walk: 1 024 placements x first / second tile of a CU; every result a permutation of
    L A Q X N; the placements the table does not name (all but the 4 x 10 x 3! = 240 with 2 1 1 1 waves per SIMD) give the wave-index
    orders L Q A N X | A N L Q X; the named ones the table row by rank; the eight placements the hardware makes give X L Q A N | A N Q L X.
    The overload that takes the fallback orders as an argument (the sweep build's, tests/test_gpu_role_sweep.py): with the shipped table and
    orders it is dn_place_roles on all 2 048 cases; with a table that names nothing and each of the 120 orders (second tile: rotated by two
    places) wave w gets order[tile][w] on all 120 x 2 048 cases; with all rows of a tile equal to one of the 120 permutations the wave of
    rank r gets the row's letter r on the 120 x 480 cases with 2 1 1 1 waves per SIMD."""
    exe = host_program_support.build("check_role_place", tmp_path, sanitize=sanitize)
    assert host_program_support.run(exe) == {"cases": 2048, "named": 480, "same": 2048, "forced": 120 * 2048, "ranked": 120 * 480, "bad": 0}
