"""History rows (include/dronenav.h dn_stack_history) without a GPU: the NumPy reference of tests/history_support.py against a hand-written
case, HistoryObservation's validation and width rule, the refusals of the C ABI (dn_stack_history validates before its first device call),
the exported symbols, the inline width rule as a stand-alone host program, and the collectors' refusals."""
import ctypes as C
import types

import numpy as np
import pytest

import abi_support as abi
import history_support as H
import host_program_support

INVALID = -1
P = C.c_void_p(0x1000)           # a non-null, 16-byte aligned pointer that is never followed


@pytest.fixture(scope="module")
def pkg():
    import drl_dronenavigation_amd as p
    p.build.build_library()
    return p


# ---- the reference itself: F = 3, A = 2, E = 0, one drone, five steps, done at step 2 (W = 48: 39 + 8 columns and one of padding) ----
Z13, Z4 = [0.0] * 13, [0.0] * 4
PA = [-1.0, -2.0, -3.0, -4.0, -5.0, -6.0, -7.0, -8.0, -9.0, -10.0, -11.0, -12.0, -13.0]            # prev: oldest frame
PB = [-21.0, -22.0, -23.0, -24.0, -25.0, -26.0, -27.0, -28.0, -29.0, -30.0, -31.0, -32.0, -33.0]
PC = [-41.0, -42.0, -43.0, -44.0, -45.0, -46.0, -47.0, -48.0, -49.0, -50.0, -51.0, -52.0, -53.0]   # prev: newest frame
QA, QB = [-61.0, -62.0, -63.0, -64.0], [-71.0, -72.0, -73.0, -74.0]                                # prev: older, newer action
O0 = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0, 13.0]
O1 = [101.0, 102.0, 103.0, 104.0, 105.0, 106.0, 107.0, 108.0, 109.0, 110.0, 111.0, 112.0, 113.0]
O2 = [201.0, 202.0, 203.0, 204.0, 205.0, 206.0, 207.0, 208.0, 209.0, 210.0, 211.0, 212.0, 213.0]   # the reset row of the new episode
O3 = [301.0, 302.0, 303.0, 304.0, 305.0, 306.0, 307.0, 308.0, 309.0, 310.0, 311.0, 312.0, 313.0]
O4 = [401.0, 402.0, 403.0, 404.0, 405.0, 406.0, 407.0, 408.0, 409.0, 410.0, 411.0, 412.0, 413.0]
T2 = [291.0, 292.0, 293.0, 294.0, 295.0, 296.0, 297.0, 298.0, 299.0, 300.5, 301.5, 302.5, 303.5]   # the terminal row of step 2
A0, A1, A2 = [0.1, 0.2, 0.3, 0.4], [1.1, 1.2, 1.3, 1.4], [2.1, 2.2, 2.3, 2.4]
A3, A4 = [3.1, 3.2, 3.3, 3.4], [4.1, 4.2, 4.3, 4.4]
WANT_ROWS = [
    PB + PC + O0 + QB + A0 + [0.0],
    PC + O0 + O1 + A0 + A1 + [0.0],
    Z13 + Z13 + O2 + Z4 + Z4 + [0.0],           # the episode ended: a fresh stack, no action yet
    Z13 + O2 + O3 + Z4 + A3 + [0.0],
    O2 + O3 + O4 + A3 + A4 + [0.0],
]
WANT_TERMINAL_2 = O0 + O1 + T2 + A1 + A2 + [0.0]  # the old stack with the terminal row and the action that ended the episode


def test_reference_matches_the_hand_written_case():
    f = lambda rows: np.array(rows, np.float32)[:, None, :]             # noqa: E731  [K, 1, cols]
    obs = f([O0, O1, O2, O3, O4])
    acts = f([A0, A1, A2, A3, A4])
    term_obs = f([Z13, Z13, T2, Z13, Z13])
    done = np.array([[0], [0], [1], [0], [0]], np.uint8)
    prev = np.array([PA + PB + PC + QA + QB + [0.0]], np.float32)
    rows, term = H.stack_reference((3, 2, 0), prev, obs, acts, done, term_obs, None, None)
    assert rows.shape == term.shape == (5, 1, 48)
    assert np.array_equal(H.bits(rows[:, 0]), H.bits(np.array(WANT_ROWS, np.float32)))
    assert np.array_equal(H.bits(term[2, 0]), H.bits(np.array(WANT_TERMINAL_2, np.float32)))
    assert not term[[0, 1, 3, 4]].any()
    # the reset call: no prev, no actions, no done -- zero frames and the observation newest
    rows, _ = H.stack_reference((3, 2, 0), None, obs[:1], None, None, None, None, None)
    assert np.array_equal(rows[0, 0], np.array(Z13 + Z13 + O0 + Z4 + Z4 + [0.0], np.float32))
    # extras are copied through, the terminal ones into the terminal row
    x, xt = np.full((5, 1, 2), 7.0, np.float32), np.full((5, 1, 2), 9.0, np.float32)
    rows, term = H.stack_reference((1, 1, 2), None, obs, acts, done, term_obs, x, xt)
    assert rows.shape == (5, 1, 20)
    assert np.array_equal(rows[2, 0], np.array(O2 + Z4 + [7.0, 7.0, 0.0], np.float32))
    assert np.array_equal(term[2, 0], np.array(T2 + A2 + [9.0, 9.0, 0.0], np.float32))
    assert np.array_equal(rows[3, 0], np.array(O3 + A3 + [7.0, 7.0, 0.0], np.float32))


# ---- HistoryObservation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,a,e,w", [(1, 0, 0, 16), (4, 3, 0, 64), (3, 2, 8, 56), (2, 2, 8, 44)])
def test_width_of_the_named_rows(pkg, f, a, e, w):
    assert pkg.HistoryObservation(frames=f, actions=a).width(e) == w == H.width(f, a, e)


def test_history_observation_validates(pkg):
    h = pkg.HistoryObservation()
    assert (h.frames, h.actions, h.goal) == (3, 2, False) and h.width() == 48 and h.extra_dim == 0
    assert pkg.HistoryObservation(goal=True).width() == 56 and pkg.HistoryObservation(goal=True).extra_dim == 8
    with pytest.raises(ValueError, match="wider than 64"):
        pkg.HistoryObservation(frames=4, actions=4)
    with pytest.raises(ValueError, match="wider than 64"):
        pkg.HistoryObservation(frames=4, actions=3).width(4)
    with pytest.raises(ValueError, match="wider than 64"):
        pkg.HistoryObservation(frames=4, actions=3, goal=True)
    for bad in (dict(frames=0), dict(frames=5), dict(frames=2.0), dict(frames=True), dict(actions=-1), dict(actions=5), dict(actions=None),
                dict(goal=1), dict(goal="yes")):
        with pytest.raises(ValueError):
            pkg.HistoryObservation(**bad)
    with pytest.raises(ValueError, match="extra_dim"):
        h.width(-1)
    c = pkg.HistoryObservation(frames=2, actions=1, goal=True).to_c()
    assert (c.frames, c.actions, c.extra_dim, c.reserved) == (2, 1, 8, 0)
    assert "HistoryObservation" in pkg.__all__


def test_width_agrees_with_the_c_abi_over_the_grid(pkg):
    K = pkg._capi
    lib = K.load()
    seen = 0
    for f in range(0, 6):
        for a in range(-1, 6):
            for e in (0, 3, 8, 12, 40):
                got = lib.dn_history_width(C.byref(K.DnHistoryConfig(f, a, e, 0)))
                want = H.width(f, a, e)
                assert got == (INVALID if want is None else want), (f, a, e, got)
                if 1 <= f <= 4 and 0 <= a <= 4:
                    h = pkg.HistoryObservation(frames=f, actions=a) if H.width(f, a, 0) else None
                    if want is None:
                        if h is not None:
                            with pytest.raises(ValueError):
                                h.width(e)
                    else:
                        assert h.width(e) == want
                        seen += 1
    assert seen > 40
    assert lib.dn_history_width(None) == INVALID
    assert lib.dn_history_width(C.byref(K.DnHistoryConfig(3, 2, 0, 1))) == INVALID and b"reserved" in lib.dn_last_error()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_history_symbols_and_layout(pkg):
    abi.check_version()
    abi.check_names("dn_history_width", "dn_stack_history")
    for name in ("dn_history_width", "dn_stack_history"):
        assert f"int32_t {name}(" in abi.header_text(), name
    abi.check_layout(pkg._capi.DnHistoryConfig, 16, frames=0, actions=4, extra_dim=8, reserved=12)


def _call(lib, cfg, k=1, n=64, prev=P, obs=P, actions=P, done=P, terminal_obs=P, extra=None, terminal_extra=None, rows=P,
          terminal_rows=P):
    return lib.dn_stack_history(None if cfg is None else C.byref(cfg), k, n, prev, obs, actions, done, terminal_obs, extra,
                                terminal_extra, rows, terminal_rows, 0, None)


def test_dn_stack_history_validates_before_it_touches_a_device(pkg):
    """Dummy non-null pointers: every refusal returns before the first device call (this machine has no device to call)."""
    K = pkg._capi
    lib = K.load()
    good = K.DnHistoryConfig(3, 2, 0, 0)
    odd = C.c_void_p(0x1004)
    cases = [
        (dict(cfg=None), b"cfg"),
        (dict(cfg=K.DnHistoryConfig(0, 2, 0, 0)), b"frames"), (dict(cfg=K.DnHistoryConfig(5, 0, 0, 0)), b"frames"),
        (dict(cfg=K.DnHistoryConfig(3, -1, 0, 0)), b"actions"), (dict(cfg=K.DnHistoryConfig(3, 5, 0, 0)), b"actions"),
        (dict(cfg=K.DnHistoryConfig(3, 2, -1, 0)), b"extra_dim"),
        (dict(cfg=K.DnHistoryConfig(4, 4, 0, 0)), b"wider than 64"), (dict(cfg=K.DnHistoryConfig(4, 3, 4, 0)), b"wider than 64"),
        (dict(cfg=K.DnHistoryConfig(3, 2, 0, 7)), b"reserved"),
        (dict(cfg=good, k=0), b"k and n"), (dict(cfg=good, n=0), b"k and n"),
        (dict(cfg=good, rows=odd), b"16-byte"), (dict(cfg=good, terminal_rows=odd), b"16-byte"),
        (dict(cfg=good, rows=None), b"rows"), (dict(cfg=good, obs=None), b"obs"),
        (dict(cfg=good, terminal_obs=None), b"terminal_rows needs terminal_obs"),
        (dict(cfg=good, actions=None), b"done needs actions"),
    ]
    for kw, word in cases:
        assert _call(lib, **kw) == INVALID, kw
        assert word in lib.dn_last_error(), (kw, lib.dn_last_error())
    with pytest.raises(pkg.DroneNavError):
        K.check(_call(lib, cfg=None))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_width_rule_as_a_host_program(tmp_path, sanitize):
    """tests/tools/check_history_width.cpp walks F = -1 .. 6, A = -2 .. 6, E = -1 .. 70 against the rule written out independently of the
    function; built with the host compiler against the HIP headers, plainly and under the address and undefined-behaviour sanitizers,
    and run as its own process."""
    exe = host_program_support.build("check_history_width", tmp_path, sanitize=sanitize, hip_headers=True)
    if exe is None:
        pytest.skip("the HIP headers are not installed")
    assert host_program_support.run(exe) == {"cases": 8 * 9 * 72 + 3, "bad": 0}


# ---- the collectors ---------------------------------------------------------------------------------------------------------------------
def test_collectors_know_the_history_mode_and_refuse_history_envs(pkg):
    from drl_dronenavigation_amd import collector
    with pytest.raises(ValueError, match="'history'"):                    # the message for a misspelt mode lists the new one
        pkg.RolloutCollector(object(), None, 4, policy_input="histroy")
    with pytest.raises(TypeError, match="DroneVecEnv"):                   # the known mode gets as far as the env check
        pkg.RolloutCollector(object(), None, 4, policy_input="history")
    with pytest.raises(ValueError, match="FusedRolloutCollector does not carry history rows"):
        collector._refuse_extra_rows(types.SimpleNamespace(history=object()), "FusedRolloutCollector")
    collector._refuse_extra_rows(types.SimpleNamespace(history=None), "OffPolicyCollector")
    collector._refuse_extra_rows(object(), "OffPolicyCollector")
