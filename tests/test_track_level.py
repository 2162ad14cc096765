"""dn_model_level (csrc/dn_internal.h) with the track bank: tests/tools/check_track_level.cpp walks the 144 combinations of
tests/tools/check_model_level.cpp with the bank off (the old answer) and on (DN_M_GOAL: the bank rides in the deepest family and adds no
level).  Host code only: built with the host compiler against the HIP headers, once plainly and once as a stand-alone program under the
address and undefined-behaviour sanitizers, and run as its own process.  No GPU."""
import pytest

import host_program_support


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_bank_on_is_the_goal_level_and_bank_off_changes_nothing(tmp_path, sanitize):
    exe = host_program_support.build("check_track_level", tmp_path, sanitize=sanitize, hip_headers=True)
    if exe is None:
        pytest.skip("the HIP headers are not installed")
    assert host_program_support.run(exe) == {"cases": 288, "bad": 0}
