"""The fleet-wide row normaliser (include/dronenav.h dn_rownorm), the part that needs no GPU: the five entry points are declared,
exported and bound; the state and scratch sizes; every refusal of dn_rownorm / dn_rownorm_init, which validate before their first device
call, so the pointers here are never followed; the Python surface's own refusals; and the scratch-size rule as a stand-alone host
program, plainly and under the address and undefined-behaviour sanitizers."""
import ctypes as C
import math
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import rownorm_support as R  # noqa: E402
import abi_support as abi  # noqa: E402
import host_program_support  # noqa: E402

NAMES = ("dn_rownorm_config", "dn_rownorm_state_doubles", "dn_rownorm_scratch_bytes", "dn_rownorm_init", "dn_rownorm")
INVALID = -1


@pytest.fixture(scope="module")
def pkg():
    import drl_dronenavigation_amd as p
    p.build.build_library()
    return p


def test_the_five_names_are_declared_exported_and_bound(pkg):
    header, code = abi.header_text(comments=True), abi.header_text()
    assert re.search(r"typedef struct dn_rownorm_config \{\s*int32_t width;\s*float clip;\s*double epsilon;\s*\} dn_rownorm_config;", code)
    abi.check_names(*NAMES[1:])
    assert "normalize.py:10-47" in header and header.count("normalize.py:") >= 5        # every entry point cites the reference
    abi.check_layout(pkg._capi.DnRownormConfig, 16, width=0, clip=4, epsilon=8)
    assert pkg.RowNormalizer is pkg.rownorm.RowNormalizer and "RowNormalizer" in pkg.__all__
    abi.check_version()


def test_state_and_scratch_sizes(pkg):
    lib = pkg._capi.load()
    for w in range(1, 65):
        assert lib.dn_rownorm_state_doubles(w) == 1 + 2 * w
    for w in (0, 65, -1):
        assert lib.dn_rownorm_state_doubles(w) <= 0 and b"width must be in 1..64" in lib.dn_last_error()
    blocks = lambda n: -(-n // R.BLOCK_ROWS)       # noqa: E731
    for k, n, w in ((1, 1, 1), (1, 1024, 52), (1, 1025, 52), (32, 32768, 64), (1, 1 << 21, 52), (3, 2049, 21)):
        want = 8 * k * (blocks(n) + 1) * 2 * w
        assert lib.dn_rownorm_scratch_bytes(k, n, w) == -(-want // 16) * 16, (k, n, w)
    for k, n, w in ((0, 1, 13), (1, 0, 13), (1, 1, 0), (1, 1, 65), (1 << 62, 1 << 62, 64)):
        assert lib.dn_rownorm_scratch_bytes(k, n, w) <= 0, (k, n, w)


def _call(lib, K, *, cfg=(52, 10.0, 1e-8), stats=0x10000, k=1, n=64, rows=0x20000, out=0x40000, update=1, scratch=0x80000, scratch_bytes=None):
    c = None if cfg is None else C.byref(K.DnRownormConfig(*cfg))
    if scratch_bytes is None:
        scratch_bytes = 1 << 30
    rc = lib.dn_rownorm(c, stats, k, n, rows, out, update, scratch, scratch_bytes, 0, None)
    return rc, lib.dn_last_error().decode()


ROW_BYTES = 64 * 52 * 4
REFUSALS = [
    ("null_cfg", dict(cfg=None), "cfg is required"),
    ("null_stats", dict(stats=None), "stats, rows and scratch are required"),
    ("null_rows", dict(rows=None), "stats, rows and scratch are required"),
    ("null_scratch", dict(scratch=None), "stats, rows and scratch are required"),
    ("width_0", dict(cfg=(0, 10.0, 1e-8)), "width must be in 1..64 (got 0)"),
    ("width_65", dict(cfg=(65, 10.0, 1e-8)), "width must be in 1..64 (got 65)"),
    ("width_negative", dict(cfg=(-1, 10.0, 1e-8)), "width must be in 1..64 (got -1)"),
    ("k_0", dict(k=0), "k and n must be >= 1"),
    ("n_0", dict(n=0), "k and n must be >= 1"),
    ("n_negative", dict(n=-5), "k and n must be >= 1"),
    ("clip_0", dict(cfg=(52, 0.0, 1e-8)), "clip must be > 0"),
    ("clip_negative", dict(cfg=(52, -1.0, 1e-8)), "clip must be > 0"),
    ("clip_nan", dict(cfg=(52, math.nan, 1e-8)), "clip must be > 0"),
    ("epsilon_negative", dict(cfg=(52, 10.0, -1e-8)), "epsilon must be >= 0"),
    ("epsilon_nan", dict(cfg=(52, 10.0, math.nan)), "epsilon must be >= 0"),
    ("no_out_without_update", dict(out=None, update=0), "out is required with update = 0"),
    ("update_2", dict(update=2), "update must be 0 or 1"),
    ("out_overlaps_from_above", dict(out=0x20000 + 4), "out overlaps rows"),
    ("out_overlaps_last_word", dict(out=0x20000 + ROW_BYTES - 4), "out overlaps rows"),
    ("out_overlaps_from_below", dict(rows=0x40000, out=0x40000 - ROW_BYTES + 4), "out overlaps rows"),
    ("scratch_one_byte_short", dict(scratch_bytes="short"), "scratch_bytes is too small"),
    ("scratch_0", dict(scratch_bytes=0), "scratch_bytes is too small"),
    ("stats_misaligned", dict(stats=0x10004), "stats and scratch must be 8-byte aligned"),
    ("scratch_misaligned", dict(scratch=0x80004), "stats and scratch must be 8-byte aligned"),
    ("rows_misaligned", dict(rows=0x20002), "rows and out must be 4-byte aligned"),
    ("out_misaligned", dict(out=0x40001), "rows and out must be 4-byte aligned"),
]


@pytest.mark.parametrize("kw,message", [pytest.param(*r[1:], id=r[0]) for r in REFUSALS])
def test_dn_rownorm_refuses(pkg, kw, message):
    """Every case returns DN_ERR_INVALID_ARGUMENT with its own text on dummy pointers: none gets as far as a device call."""
    K = pkg._capi
    lib = K.load()
    kw = dict(kw)
    if kw.get("scratch_bytes") == "short":
        kw["scratch_bytes"] = lib.dn_rownorm_scratch_bytes(1, 64, 52) - 1
    rc, msg = _call(lib, K, **kw)
    assert rc == INVALID, msg
    assert message in msg, msg


def test_the_refusals_are_not_the_dummies_own(pkg):
    """The unchanged dummy call -- also in place, with out exactly behind rows, with an infinite clip and with epsilon 0 -- passes every
    check but one chosen here, the last one validation makes: each refusal above is caused by what it changes."""
    K = pkg._capi
    lib = K.load()
    for kw in (dict(), dict(out=0x20000), dict(out=0x20000 + ROW_BYTES), dict(cfg=(52, math.inf, 0.0)), dict(out=None),
               dict(scratch_bytes=lib.dn_rownorm_scratch_bytes(1, 64, 52))):
        rc, msg = _call(lib, K, rows=0x20002, **kw)
        assert rc == INVALID and "rows and out must be 4-byte aligned" in msg, (kw, msg)


def test_dn_rownorm_init_refuses(pkg):
    K = pkg._capi
    lib = K.load()
    cfg = K.DnRownormConfig(52, 10.0, 1e-8)
    assert lib.dn_rownorm_init(None, 0x1000, 0, None) == INVALID and b"cfg is required" in lib.dn_last_error()
    assert lib.dn_rownorm_init(C.byref(cfg), None, 0, None) == INVALID and b"stats is required" in lib.dn_last_error()
    assert lib.dn_rownorm_init(C.byref(cfg), 0x1004, 0, None) == INVALID and b"8-byte aligned" in lib.dn_last_error()
    assert lib.dn_rownorm_init(C.byref(K.DnRownormConfig(65, 10.0, 1e-8)), 0x1000, 0, None) == INVALID
    assert b"width must be in 1..64" in lib.dn_last_error()


def test_python_surface_refuses_without_a_device(pkg):
    from drl_dronenavigation_amd import collector
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.RowNormalizer(52, "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.RowNormalizer(52, torch.device("cpu"), clip=5.0)
    for bad in (0, 65, -1, 13.0, True):
        with pytest.raises(ValueError, match="width"):
            pkg.RowNormalizer(bad, "cpu")
    for kw, word in ((dict(clip=0.0), "clip"), (dict(clip=math.nan), "clip"), (dict(epsilon=-1.0), "epsilon"), (dict(epsilon=math.nan), "epsilon")):
        with pytest.raises(ValueError, match=word):
            pkg.RowNormalizer(52, "cpu", **kw)
    # RolloutCollector: what it can say about the two arguments before it looks at the env
    with pytest.raises(ValueError, match="value_norm needs value_input='privileged'"):
        collector.RolloutCollector(None, None, 4, value_norm=object())
    with pytest.raises(TypeError, match="value_norm must be a RowNormalizer"):
        collector.RolloutCollector(None, None, 4, value_fn=lambda x: x, value_input="privileged", value_norm=object())
    with pytest.raises(TypeError, match="policy_norm must be a RowNormalizer"):
        collector.RolloutCollector(None, None, 4, policy_norm=(52, 10.0))
    with pytest.raises(TypeError, match="DroneVecEnv"):                # with both left at None the first complaint is the old one
        collector.RolloutCollector(None, None, 4)


def test_reference_agrees_with_itself_in_two_summation_orders():
    """The 1e-9 bars of the GPU test on the reference alone: np.mean / np.var against the same moments from float64 sums taken in
    reversed row order agree to 1e-12 on the test data, three successive updates of a few thousand rows."""
    rng = np.random.default_rng(0)
    x = R.make_rows(rng, 3, 2049, 52)
    a, b = R.RunningMeanStd(52), R.RunningMeanStd(52)
    for t in range(3):
        a.update(x[t])
        b.update(x[t][::-1].copy())
    std = np.sqrt(a.var)
    assert a.count == b.count == 1e-4 + 3 * 2049
    assert (np.abs(a.mean - b.mean) <= 1e-12 * (np.abs(a.mean) + std)).all()
    assert (np.abs(a.var - b.var) <= 1e-12 * a.var).all()
    rotor, const, zero = R.special_columns(52)
    prior = R.ROTOR ** 2 * 1e-4 / a.count              # what the prior's mean of 0 with its count of 1e-4 leaves in the variance
    assert abs(a.mean[rotor] - R.ROTOR) < 0.1 and 0.9 + prior < a.var[rotor] < 1.1 + prior
    # the prior (count 1e-4, var 1) never leaves: the constant and the zero column do not reach variance exactly 0
    assert 0 < a.var[zero] < 1e-7 and 0 < a.var[const] < 1e-6 and a.mean[zero] == 0.0


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_scratch_size_rule_as_a_host_program(tmp_path, sanitize):
    """tests/tools/check_rownorm_sizes.cpp walks width 1 .. 64 x k {1, 2, 64} x n {1, 63, 64, 65, 1000, 2^21} and ten refusals; built
    with the host compiler against the HIP headers, plainly and under the address and undefined-behaviour sanitizers, and run as its own
    process."""
    exe = host_program_support.build("check_rownorm_sizes", tmp_path, sanitize=sanitize, hip_headers=True)
    if exe is None:
        pytest.skip("the HIP headers are not installed")
    assert host_program_support.run(exe) == {"cases": 64 * 3 * 6 + 10, "bad": 0}
