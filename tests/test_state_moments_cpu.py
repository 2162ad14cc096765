"""The rule by which dn_set_state restores the observation normaliser's second moment from a dn_env_state (csrc/dn_second_moment.h
dn_restore_second_moment) over 1.2 million seeded (M2, count) pairs and the edges, on the CPU: a stand-alone host program, built plainly and
under the address and undefined-behaviour sanitizers, and run as its own process."""
import pytest

import host_program_support


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_hint_restores_every_second_moment_and_edits_are_honoured(tmp_path, sanitize):
    """tests/tools/check_second_moment.cpp states the walk and what counts as bad: a verbatim hint that does not come back bit for bit, an
    edited var or count that does not read back, a zero hint that does not give second_moment(var, count), a count dn_set_state must
    refuse that passes.  `lossy` is what the rule before ABI 10 -- second_moment(M2 / count, count) alone -- got wrong on the same walk:
    it must be above zero, or the walk would not cover the case the hint exists for (about 9 % of the pairs: profiles/NOTES.md)."""
    exe = host_program_support.build("check_second_moment", tmp_path, sanitize=sanitize)
    got = host_program_support.run(exe, timeout=120)
    lossy = got.pop("lossy")
    assert got == {"cases": 1200044, "edges": 44, "bad": 0}
    assert 0 < lossy < got["cases"], lossy
