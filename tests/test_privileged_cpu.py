"""Privileged observations (include/dronenav.h dn_enable_privileged) without a GPU: the C struct and the row constants against their
Python twins, the exported symbols, the host-side validation of PrivilegedObservation and the loud failures that need no device."""
import ctypes as C
import dataclasses

import pytest

import abi_support as abi

NEW_SYMBOLS = ("dn_enable_privileged", "dn_get_privileged_config", "dn_bind_privileged")
INVALID, BAD_STATE = -1, -5


@pytest.fixture(scope="module")
def pkg():
    import drl_dronenavigation_amd as p
    return p


def test_privileged_config_layout_and_constants_match_header(pkg):
    from drl_dronenavigation_amd import privileged as P
    abi.check_layout(pkg._capi.DnPrivilegedConfig, 8, groups=0, reserved=4)          # the layout the header documents
    consts, G = abi.compiled().constants, P.PRIV_GROUPS
    assert [consts["DN_PRIV_" + k] for k in ("DIM", "OBS", "DYN", "WIND", "ACT", "SENS", "ALL")] == [
        P.PRIV_DIM, G["obs"], G["dyn"], G["wind"], G["act"], G["sens"], sum(G.values())]
    assert consts["DN_PRIV_DIM"] == 52
    abi.check_version()


def test_row_constants_are_consistent(pkg):
    from drl_dronenavigation_amd import privileged as P
    assert pkg.PRIV_DIM == 52 and pkg.PRIV_SLICES is P.PRIV_SLICES and pkg.PRIV_GROUPS is P.PRIV_GROUPS
    cols = [c for g in P.PRIV_GROUPS for c in P.PRIV_GROUP_COLUMNS[g]]
    assert sorted(cols) == list(range(52))                      # the five groups partition the row
    named = sorted(c for s in P.PRIV_SLICES.values() for c in range(s.start, s.stop))
    assert len(named) == len(set(named)) and set(range(52)) - set(named) == {13, 14, 15, 23, 27, 49, 50, 51}      # the rest is padding
    S = P.PRIV_SLICES
    assert (S["obs"], S["scales"], S["bias"]) == (slice(0, 13), slice(16, 20), slice(36, 49))
    assert [S[k].start for k in ("act_latency", "act_coeff", "sens_latency", "steps")] == [32, 33, 34, 35]
    owner = {c: g for g in P.PRIV_GROUPS for c in P.PRIV_GROUP_COLUMNS[g]}
    assert [owner[c] for c in (32, 33, 34, 35)] == ["act", "act", "sens", "obs"]       # the quad of scalars belongs to three groups


def test_privileged_symbols_are_exported_and_bound(pkg):
    lib = pkg._capi.load()
    P = pkg._capi.PROTOTYPES
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    cfg_p = C.POINTER(pkg._capi.DnPrivilegedConfig)
    want = {"dn_enable_privileged": (i32, [vp, cfg_p]), "dn_get_privileged_config": (i32, [vp, cfg_p]),
            "dn_bind_privileged": (i32, [vp, vp, vp, i64])}
    for name in NEW_SYMBOLS:
        assert name in P, name
        assert (P[name][0], list(P[name][1])) == want[name], name
        fn = getattr(lib, name)
        assert fn.restype == want[name][0] and list(fn.argtypes) == want[name][1], name
    abi.check_names(*NEW_SYMBOLS)


@pytest.mark.parametrize("bad", [(), [], ("obs", "body"), ("OBS",), "obs", ("obs", 3), (None,), 5, None])
def test_privileged_observation_rejects_bad_groups(pkg, bad):
    with pytest.raises(ValueError):
        pkg.PrivilegedObservation(groups=bad)


def test_privileged_observation_defaults_and_c_image(pkg):
    p = pkg.PrivilegedObservation()
    assert p.groups == ("obs", "dyn", "wind", "act", "sens") and p.mask == 31 and p.columns() == list(range(52))
    q = pkg.PrivilegedObservation(groups=["sens", "obs", "obs"])
    assert q.groups == ("obs", "sens") and q.mask == 17              # canonical order, no repeats
    assert q.columns() == list(range(16)) + [34, 35] + list(range(36, 52))
    c = q.to_c()
    assert (c.groups, c.reserved) == (17, 0)
    back = pkg.PrivilegedObservation.from_c(c)
    assert back == q and bytes(back.to_c()) == bytes(c)
    for m in range(1, 32):
        c.groups = m
        assert pkg.PrivilegedObservation.from_c(c).to_c().groups == m
    c.groups = 32
    with pytest.raises(ValueError):
        pkg.PrivilegedObservation.from_c(c)
    with pytest.raises(dataclasses.FrozenInstanceError):
        q.groups = ("obs",)
    assert "PrivilegedObservation" in pkg.__all__


def test_enable_privileged_fails_loudly_without_a_device(pkg):
    lib = pkg._capi.load()
    assert pkg._capi.STATUS_NAMES[INVALID] == "DN_ERR_INVALID_ARGUMENT"
    good = pkg.PrivilegedObservation().to_c()
    rc = lib.dn_enable_privileged(None, C.byref(good))
    assert rc == INVALID
    with pytest.raises(pkg.DroneNavError):
        pkg._capi.check(rc)
    assert b"env" in lib.dn_last_error()
    assert lib.dn_enable_privileged(None, None) == INVALID
    # the mask is judged before anything else: no env and no device are needed to refuse it
    for groups, reserved, word in ((0, 0, b"groups"), (32, 0, b"groups"), (-1, 0, b"groups"), (31 | 64, 0, b"groups"), (1, 7, b"reserved")):
        cfg = pkg._capi.DnPrivilegedConfig(groups, reserved)
        assert lib.dn_enable_privileged(None, C.byref(cfg)) == INVALID, (groups, reserved)
        assert word in lib.dn_last_error(), (groups, reserved, lib.dn_last_error())
    out = pkg._capi.DnPrivilegedConfig()
    assert lib.dn_get_privileged_config(None, C.byref(out)) == INVALID
    assert lib.dn_bind_privileged(None, None, None, 1) == INVALID


def test_column_runs_cover_exactly_the_written_columns():
    import itertools
    from drl_dronenavigation_amd.privileged import PRIV_GROUPS, PrivilegedObservation
    assert PrivilegedObservation().column_runs() == [(0, 52)]
    assert PrivilegedObservation(groups=("obs", "sens")).column_runs() == [(0, 16), (34, 52)]
    for r in range(1, 6):
        for groups in itertools.combinations(PRIV_GROUPS, r):
            p = PrivilegedObservation(groups=groups)
            runs = p.column_runs()
            assert [c for a, b in runs for c in range(a, b)] == p.columns() and len(runs) <= 3
