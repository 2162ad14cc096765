"""The kernel-shape pick of dn_create (csrc/dn_shapes.h dn_pick_shapes) over its whole domain, on the CPU: a stand-alone host program,
built plainly and under the address and undefined-behaviour sanitizers, and run as its own process."""
import pytest

from kernel_shapes_support import build_program, run_program

# 144 configuration classes x (six device sizes without overrides + two device sizes x 44 DN_WAVES / DN_WAVES_SINGLE pairs) x every fleet
# of 1 .. 8 num_cus + 2 tiles x two fleet sizes per tile count
CASES = 144 * 2 * ((8 * (1 + 8 + 32 + 64 + 256 + 304) + 6 * 2) + 44 * (8 * (32 + 256) + 2 * 2))
# What the program printed when dn_pick_shapes was the run of overwrites dn_create held before the pick had a home of its own, moved
# verbatim: the readable form must print the same.
DIGEST = "c9f1dc9c8dff0749"


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_pick_over_its_whole_domain_as_a_host_program(tmp_path, sanitize):
    """tests/tools/check_kernel_shapes.cpp states the walk and its order; beside the digest it asserts that a fleet's pick depends on its
    tile count alone, and the hand-derived spot rows (the 256-CU table of the measurement notes, the forced one-wave cases, DN_WAVES=2 and
    DN_WAVES=3x)."""
    assert CASES == 30782592
    assert run_program(build_program(tmp_path, sanitize)) == {"cases": CASES, "digest": DIGEST, "bad": 0}


def test_the_program_prints_one_pick_for_a_given_configuration(tmp_path):
    exe = build_program(tmp_path)
    assert run_program(exe, num_cus=256, num_envs=32768, normalize_obs=1) == {"fused": 5, "single": 3}
    assert run_program(exe, num_cus=256, num_envs=32768, normalize_obs=1, dn_waves="4", dn_waves_single="1") == {"fused": 4, "single": 1}
    assert run_program(exe, num_cus=32, num_envs=4096, clip_rew=1) == {"fused": 3, "single": 1}
