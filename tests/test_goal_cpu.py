"""Goal observations (include/dronenav.h dn_enable_goal) without a GPU: the C struct and the row constants against their Python twins, the
exported symbols, the host-side validation of GoalObservation, the loud failures that need no device, and the NumPy reference of
tests/goal_support.py against hand-worked rows."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import abi_support as abi
import goal_support as G

NEW_SYMBOLS = ("dn_enable_goal", "dn_get_goal_config", "dn_bind_goal")
INVALID = -1


@pytest.fixture(scope="module")
def pkg():
    import drl_dronenavigation_amd as p
    return p


def test_goal_config_layout_and_constants_match_header(pkg):
    from drl_dronenavigation_amd import goal as M
    abi.check_layout(pkg._capi.DnGoalConfig, 8, frame=0, reserved=4)                 # the layout the header documents
    consts = abi.compiled().constants
    assert (consts["DN_GOAL_DIM"], consts["DN_GOAL_FRAME_WORLD"], consts["DN_GOAL_FRAME_BODY"]) == (M.GOAL_DIM, M.GOAL_FRAMES["world"],
                                                                                                  M.GOAL_FRAMES["body"]) == (8, 0, 1)
    abi.check_version()
    assert G.GOAL_DIM == M.GOAL_DIM == pkg.GOAL_DIM
    named = sorted(c for s in M.GOAL_SLICES.values() for c in range(s.start, s.stop))
    assert named == list(range(8))                              # the named slices partition the row


def test_goal_symbols_are_in_header_exports_and_ctypes_table(pkg):
    lib = pkg._capi.load()
    abi.check_version()
    P = pkg._capi.PROTOTYPES
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    cfg_p = C.POINTER(pkg._capi.DnGoalConfig)
    want = {"dn_enable_goal": (i32, [vp, cfg_p]), "dn_get_goal_config": (i32, [vp, cfg_p]), "dn_bind_goal": (i32, [vp, vp, vp, i64])}
    abi.check_names(*NEW_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert f"int32_t {name}(" in abi.header_text(), name
        assert name in P, name
        assert (P[name][0], list(P[name][1])) == want[name], name
        fn = getattr(lib, name)
        assert fn.restype == want[name][0] and list(fn.argtypes) == want[name][1], name


@pytest.mark.parametrize("bad", ["", "World", "inertial", 0, 1, None, ("world",), b"body"])
def test_goal_observation_rejects_bad_frames(pkg, bad):
    with pytest.raises(ValueError):
        pkg.GoalObservation(frame=bad)


def test_goal_observation_defaults_and_c_image(pkg):
    g = pkg.GoalObservation()
    assert g.frame == "world" and (g.to_c().frame, g.to_c().reserved) == (0, 0)
    b = pkg.GoalObservation(frame="body")
    c = b.to_c()
    assert (c.frame, c.reserved) == (1, 0)
    back = pkg.GoalObservation.from_c(c)
    assert back == b and bytes(back.to_c()) == bytes(c)
    assert pkg.GoalObservation.from_c(g.to_c()) == g
    c.frame = 2
    with pytest.raises(ValueError):
        pkg.GoalObservation.from_c(c)
    with pytest.raises(dataclasses.FrozenInstanceError):
        b.frame = "world"
    assert "GoalObservation" in pkg.__all__ and "GOAL_SLICES" in pkg.__all__


def test_enable_goal_fails_loudly_without_a_device(pkg):
    lib = pkg._capi.load()
    good = pkg.GoalObservation().to_c()
    rc = lib.dn_enable_goal(None, C.byref(good))
    assert rc == INVALID
    with pytest.raises(pkg.DroneNavError):
        pkg._capi.check(rc)
    assert b"env" in lib.dn_last_error()
    assert lib.dn_enable_goal(None, None) == INVALID
    # the frame is judged before anything else: no env and no device are needed to refuse it
    for frame, reserved, word in ((2, 0, b"frame"), (-1, 0, b"frame"), (0, 7, b"reserved"), (1, -1, b"reserved")):
        cfg = pkg._capi.DnGoalConfig(frame, reserved)
        assert lib.dn_enable_goal(None, C.byref(cfg)) == INVALID, (frame, reserved)
        assert word in lib.dn_last_error(), (frame, reserved, lib.dn_last_error())
    out = pkg._capi.DnGoalConfig()
    assert lib.dn_get_goal_config(None, C.byref(out)) == INVALID
    assert lib.dn_bind_goal(None, None, None, 1) == INVALID


def test_collectors_judge_policy_input_and_refuse_goal_envs_without_a_device(pkg):
    import types
    from drl_dronenavigation_amd import collector
    # an unknown mode is refused by name before the env is looked at
    for bad in ("goal", "observation+privileged", "", None):
        with pytest.raises(ValueError, match="policy_input"):
            pkg.RolloutCollector(object(), None, 4, policy_input=bad)
    with pytest.raises(TypeError, match="DroneVecEnv"):                   # a known mode gets as far as the env check
        pkg.RolloutCollector(object(), None, 4, policy_input="observation+goal")
    # what FusedRolloutCollector and OffPolicyCollector call first
    with pytest.raises(ValueError, match="FusedRolloutCollector does not carry goal observations"):
        collector._refuse_extra_rows(types.SimpleNamespace(goal=object()), "FusedRolloutCollector")
    collector._refuse_extra_rows(types.SimpleNamespace(goal=None), "OffPolicyCollector")
    collector._refuse_extra_rows(object(), "OffPolicyCollector")


# ---- the reference itself ------------------------------------------------------------------------------------------------------------
# Two waypoints in a box with x_high, y_high, z_high = 2, 4, 5 and x_low = y_low = -3: max_target_dist = max(3 + 2, 3 + 4, 5) = 7.
WP = [[1.0, 2.0, 3.0], [1.0, 4.0, 3.0]]
DIM = [-3.0, -3.0, 0.0, 2.0, 4.0, 5.0]


def test_reference_world_frame_hand_worked():
    assert G.max_target_dist(DIM) == 7.0
    y = np.zeros((2, 13), np.float32)
    y[:, 0:3] = [0.5, 0.25, 0.25]               # p_hat = (1, 1, 1.25), every factor exact in float32
    rows = G.goal_rows(y, np.array([0, 1]), WP, DIM, "world")
    # index 0: e = ((1, 2, 3) - (1, 1, 1.25)) / 7, n = ((1, 4, 3) - (1, 2, 3)) / 7, a next waypoint exists
    assert np.allclose(rows[0], [0.0, 1 / 7, 0.25, 0.0, 0.0, 2 / 7, 0.0, 1.0], rtol=0, atol=1e-15)
    # index 1, the last: e = ((1, 4, 3) - (1, 1, 1.25)) / 7, n = 0, no next waypoint
    assert np.allclose(rows[1], [0.0, 3 / 7, 0.25, 1.0, 0.0, 0.0, 0.0, 0.0], rtol=0, atol=1e-15)


def test_reference_body_frame_hand_worked():
    y = np.zeros((3, 13), np.float32)
    y[:, 0:3] = [0.5, 0.25, 0.25]
    y[0, 5] = 0.5       # yaw = 90 deg: the body x axis points along world +y, so a target along world +y lies along body +x
    y[1, 4] = 0.5       # pitch = 90 deg about y: the body x axis points along world -z, the body z axis along world +x
    y[2, 3] = 0.5       # roll = 90 deg about x: the body y axis points along world +z, the body z axis along world -y
    rows = G.goal_rows(y, np.zeros(3, np.int64), WP, DIM, "body")
    e = np.array([0.0, 1 / 7, 0.25])
    assert np.allclose(rows[0, 0:3], [e[1], -e[0], e[2]], rtol=0, atol=1e-15)
    assert np.allclose(rows[1, 0:3], [-e[2], e[1], e[0]], rtol=0, atol=1e-15)
    assert np.allclose(rows[2, 0:3], [e[0], e[2], -e[1]], rtol=0, atol=1e-15)
    assert np.allclose(rows[0, 4:7], [2 / 7, 0.0, 0.0], rtol=0, atol=1e-15)       # n = (0, 2, 0) / 7 along world +y -> body +x
    assert np.array_equal(rows[:, 3], [0, 0, 0]) and np.array_equal(rows[:, 7], [1, 1, 1])
    # the rotation convention: R = Rz Ry Rx carries the body axes to the world
    R = G.rotation(0.3, -0.4, 1.1)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(R) - 1) < 1e-15
    assert np.allclose(G.rotation(0.0, 0.0, math.pi / 2) @ [1, 0, 0], [0, 1, 0], atol=1e-15)


def test_reference_body_frame_with_identity_attitude_is_world_frame():
    rng = np.random.default_rng(1)
    y = rng.uniform(-1, 1, (64, 13)).astype(np.float32)
    y[:, 3:6] = 0.0
    idx = rng.integers(0, 2, 64)
    assert np.array_equal(G.goal_rows(y, idx, WP, DIM, "body"), G.goal_rows(y, idx, WP, DIM, "world"))


def test_reference_rotation_preserves_lengths():
    rng = np.random.default_rng(2)
    y = rng.uniform(-1, 1, (256, 13)).astype(np.float32)
    idx = rng.integers(0, 2, 256)
    w, b = G.goal_rows(y, idx, WP, DIM, "world"), G.goal_rows(y, idx, WP, DIM, "body")
    for s in (slice(0, 3), slice(4, 7)):
        assert np.allclose(np.linalg.norm(w[:, s], axis=1), np.linalg.norm(b[:, s], axis=1), rtol=0, atol=1e-14)
    assert np.array_equal(w[:, [3, 7]], b[:, [3, 7]])
    assert np.abs(b[:, 0:3] - w[:, 0:3]).max() > 0.1            # and it does rotate
