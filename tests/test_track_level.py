"""dn_model_level (csrc/dn_internal.h) with the track bank: tests/tools/check_track_level.cpp walks the 144 combinations of
tests/tools/check_model_level.cpp with the bank off (the old answer) and on (DN_M_GOAL: the bank rides in the deepest family and adds no
level).  Host code only: built with the host compiler against the HIP headers, once plainly and once as a stand-alone program under the
address and undefined-behaviour sanitizers, and run as its own process.  No GPU."""
import json
import os
import subprocess

import pytest

from test_model_level import ROOT, rocm_include


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_bank_on_is_the_goal_level_and_bank_off_changes_nothing(tmp_path, sanitize):
    inc = rocm_include()
    if inc is None:
        pytest.skip("the HIP headers are not installed")
    exe = str(tmp_path / "check_track_level")
    src = os.path.join(ROOT, "tests", "tools", "check_track_level.cpp")
    csrc = os.path.join(ROOT, "drl-dronenavigation_amd", "csrc")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-I" + csrc] + flags + [src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert json.loads(out.stdout) == {"cases": 288, "bad": 0}
