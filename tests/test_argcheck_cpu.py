"""csrc/dn_argcheck.h, the argument checks the entry points of the C ABI share: tests/tools/check_argcheck.cpp walks dn_ranges_overlap
against the interval rule in 128-bit arithmetic (ranges apart, touching, sharing one byte, nested; zero bytes; a NULL on either side; a
range that ends at UINTPTR_MAX and one that ends one past it) and the three walks over DnArg tables with the offending entry first, in
the middle, last and absent, with and without optional NULLs.  Host code only: built with the host compiler, once plainly and once under
the address and undefined-behaviour sanitizers, and run as its own process.  No GPU."""
import pytest

import host_program_support

GRID = 3 * 41 * 5 * 2           # sizes of a x offsets of b x sizes of b, in both argument orders
NULLS = 2 * 2 * 3               # sizes x sizes x {a, b, both} NULL
TOP = 5 * (2 + 2) + 2           # five neighbours of a range that ends at UINTPTR_MAX and of one that ends one past it; that one against itself
TABLES = 2 * 4 * (1 + 2 + 2)    # {no NULLs, optional NULLs} x {first, middle, last, absent} x (missing, two alignments, the overlap pair)
ORDER = 2 * 2                   # two overlapping pairs: the pair reported, with and without optional NULLs
SCRATCH = 6


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_shared_argument_checks_as_a_host_program(tmp_path, sanitize):
    exe = host_program_support.build("check_argcheck", tmp_path, sanitize=sanitize, extra_flags=("-Wall", "-Werror"))
    assert host_program_support.run(exe) == {"cases": GRID + NULLS + TOP + TABLES + ORDER + SCRATCH, "bad": 0}
