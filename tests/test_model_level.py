"""dn_model_level (csrc/dn_internal.h) names the kernel family a step launch takes: the deepest per-drone model that is on, the privileged
and goal rows counting only when enabled AND bound.  tests/tools/check_model_level.cpp walks all 144 combinations against that rule, written
out independently of the function.  Host code only: built with the host compiler against the HIP headers, once plainly and once under the
address and undefined-behaviour sanitizers, and run as its own process.  No GPU."""
import pytest

import host_program_support


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_model_level_is_the_deepest_model_that_counts(tmp_path, sanitize):
    exe = host_program_support.build("check_model_level", tmp_path, sanitize=sanitize, hip_headers=True)
    if exe is None:
        pytest.skip("the HIP headers are not installed")
    assert host_program_support.run(exe) == {"cases": 144, "bad": 0}
