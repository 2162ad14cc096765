"""The roles of a five-wave tile from the SIMDs its waves landed on (csrc/dn_role_place.h dn_place_roles) over all 4^5 placements, on the
CPU: a stand-alone host program, built plainly and under the address and undefined-behaviour sanitizers, and run as its own process."""
import pytest

import host_program_support


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_every_placement_gives_a_permutation_of_the_roles(tmp_path, sanitize):
    """tests/tools/check_role_place.cpp states the walk: 1 024 placements x first / second tile of a CU; every result a permutation of
    L A Q X N; the placements the table does not name (all but the 4 x 10 x 3! = 240 with 2 1 1 1 waves per SIMD) give the wave-index
    orders L Q A N X | A N L Q X; the named ones the table row by rank; the eight placements the hardware makes give X L Q A N | A N Q L X."""
    exe = host_program_support.build("check_role_place", tmp_path, sanitize=sanitize)
    assert host_program_support.run(exe) == {"cases": 2048, "named": 480, "bad": 0}
