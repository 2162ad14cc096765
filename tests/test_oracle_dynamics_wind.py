"""The CPU oracle's restatement of per-drone dynamics randomisation and wind (oracle/dn_oracle.c orc_*_dw; include/dronenav.h
dn_enable_dynamics / dn_enable_wind), pinned on its own before the GPU tests lean on it
(tests/test_gpu_dynamics_wind_oracle.py):

- identity: scales of 1 and still air through the new entry points give the nominal oracle's bits, every physics x action type
  pair and random spawn;
- one step against the independent world-frame integrator tests/rigid_body_ref.py with M, J scaled, forces x s_kf (after the ground
  effect is added), the yaw torque x s_km and extra_world_force = k (.) w (+ the PYB_DRAG force), at the 1e-12 bar of
  tests/test_bullet_invariants.py;
- the draws of an episode start and the gust's step against a restatement of the header's formulas on orc_philox4x32 words,
  global ids past 2^32 and step counters on both sides of 2^32;
- the gust's stationary statistics over a long hover.
CPU only; tests/test_oracle_asan.py runs this file under AddressSanitizer / UBSan too."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import rigid_body_ref as RB
from oracle import oracle as O
from model_support import (CASES, CIRCLE6, DT, GUSTY_WIND, LOW, WIDE, WIDE_BODY, config, dyn, f32, ulps, want_gust_start,
                           want_gust_step, want_mean, want_scales, wind)

SIZEOF_ENV, SIZEOF_CONFIG = 696, 1704        # orc_env / orc_config before this extension: the golden replays' layout


# ---- identity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("physics,act,spawn", CASES)
def test_unit_scales_and_still_air_are_the_nominal_oracle(physics, act, spawn):
    """dynamics on with ranges [1, 1] (resample: every episode start draws exactly 1) and wind on with every range 0 and the gust
    off, through orc_vec_reset_dw / orc_vec_step_dw: outputs and state equal the nominal entry points', every step, auto-resets
    included."""
    n, T = 96, 80
    track = CIRCLE6 if spawn else LOW
    kw = dict(max_steps=30, normalize_obs=True, ground_contact=False, physics=physics, action_type=act, random_spawn=spawn,
              normalize_actions=act == 0, seed=7, f32_state=True, act_noise_sigma=0.01, obs_noise_sigma=0.01)
    a_env = O.OracleVecEnv(config(track, **kw), n)
    b_env = O.OracleVecEnv(config(track, **kw), n, dynamics=dyn(), wind=wind(azimuth=(0.0, 0.0)))
    assert bytes(a_env.reset().data) == bytes(b_env.reset().data)
    rng = np.random.default_rng(physics * 8 + act)
    n_done = 0
    for t in range(T):
        acts = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
        if act == 0:
            acts[1::2] = (0.0922 + 0.003 * rng.standard_normal((n // 2, 4))).astype(np.float32)
        ra, rb = a_env.step(acts), b_env.step(acts)
        for k in ra:
            assert ra[k].tobytes() == rb[k].tobytes(), (t, k)
        n_done += int(ra["done"].sum())
        assert np.array_equal(b_env.dw["dyn"], np.ones((n, 4), np.float32))
        assert not b_env.dw["wind_mean"].any() and not b_env.dw["wind_gust"].any()
    assert a_env.envs.tobytes() == b_env.envs.tobytes()
    assert n_done > n // 2


def test_layout_of_the_nominal_structs_is_unchanged():
    L = O.lib()
    assert (L.orc_sizeof_env(), L.orc_sizeof_config()) == (SIZEOF_ENV, SIZEOF_CONFIG)
    assert O.DW_DTYPE.itemsize == 48 and L.orc_sizeof_dw_state() == 48


# ---- one step against the independent integrator --------------------------------------------------------------------------
@pytest.mark.parametrize("physics", [0, 1, 2, 4])
def test_single_step_matches_independent_integrator(physics, monkeypatch):
    """Random tumbling states (some low enough for the ground effect), ActionType.RPM (float64 forces the test can restate bit
    for bit), scales in [0.7, 1.3] and random steady winds and gusts: the oracle's step against rigid_body_ref.step with M s_m,
    J s_I, forces (F + F_gnd) s_kf, yaw torque x s_km and extra_world_force = k (.) (wbar + g) + R F_drag (the drag force of
    BaseAviary._drag, orc_drag, from the nominal rpm and the ground velocity) -- wind read at step entry.  1e-12, the bar of
    test_bullet_step_matches_independent_world_frame_integrator."""
    rng = np.random.default_rng(100 + physics)
    n = 400
    quat = Rotation.random(n, random_state=physics + 3).as_quat()
    quat[: n // 4] = Rotation.from_euler("xyz", rng.uniform(-0.4, 0.4, (n // 4, 3))).as_quat()     # upright: the ground effect acts
    pos = rng.uniform(-2, 2, (n, 3)) + [0, 0, 3]
    pos[: n // 4, 2] = rng.uniform(0.02, 0.3, n // 4)
    vel, ang_v = rng.normal(0, 2.0, (n, 3)), rng.normal(0, 8.0, (n, 3))
    last = rng.uniform(12000, 22000, (n, 4))
    cfg = O.make_config([[5e3, 5e3, 5e3]], [0.0, 0.0, 1.0], WIDE, circle=False, cylinder=False, threshold=0.0, max_steps=1 << 20,
                        normalize_actions=False, normalize_obs=False, physics=physics, action_type=1, seed=3)
    ora = O.OracleVecEnv(cfg, n, dynamics=dyn(resample=False), wind=wind(gust_sigma=(0.8, 0.3), resample=False))
    ora.reset()
    for k, v in (("pos", pos), ("quat", quat), ("vel", vel), ("ang_v", ang_v), ("cur_pos", pos), ("last_clipped_action", last)):
        ora.envs[k] = v
    ora.refresh_rpy()
    ora.dw["dyn"] = rng.uniform(0.7, 1.3, (n, 4))
    ora.dw["wind_mean"][:, :3] = rng.normal(0, 6.0, (n, 3))
    ora.dw["wind_gust"][:, :3] = rng.normal(0, 1.0, (n, 3))
    w_entry = (ora.dw["wind_mean"][:, :3].astype(np.float64) + ora.dw["wind_gust"][:, :3].astype(np.float64))
    s = ora.dw["dyn"].astype(np.float64)
    rpy = ora.envs["rpy"].copy()
    acts = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
    out = ora.step(acts)
    assert not out["done"].any()
    assert not np.array_equal(ora.dw["wind_gust"][:, :3].astype(np.float64), w_entry - ora.dw["wind_mean"][:, :3])   # the gust moved
    k = np.array([f32(5.5626e-3), f32(5.5626e-3), f32(6.2490e-3)])
    hover = math.sqrt(RB.G * RB.M / (4 * RB.KF))
    u = (np.float32(1.0) + np.float32(0.05) * acts).astype(np.float64)
    rpm = hover * u
    f, tq = rpm * rpm * RB.KF, rpm * rpm * RB.KM
    zt = ((-tq[:, 0] + tq[:, 1]) - tq[:, 2]) + tq[:, 3]
    L = O.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))     # noqa: E731
    M0, J0 = RB.M, RB.J.copy()
    n_gnd = 0
    for i in range(n):
        fi = f[i].copy()
        extra = k * w_entry[i]
        if physics in (1, 4):
            g = np.zeros(4)
            L.orc_ground_effect(dp(np.ascontiguousarray(pos[i])), dp(np.ascontiguousarray(quat[i])), dp(np.ascontiguousarray(rpy[i])),
                                dp(np.ascontiguousarray(rpm[i])), 0, dp(g))
            fi = fi + g
            n_gnd += bool(g.any())
        if physics in (2, 4):
            d = np.zeros(3)
            L.orc_drag(dp(np.ascontiguousarray(quat[i])), dp(np.ascontiguousarray(vel[i])), dp(np.ascontiguousarray(last[i])), 0, dp(d))
            extra = extra + Rotation.from_quat(quat[i]).as_matrix() @ d
        monkeypatch.setattr(RB, "M", M0 * s[i, 0])
        monkeypatch.setattr(RB, "J", J0 * s[i, 1])
        ref = RB.step(pos[i], quat[i], vel[i], ang_v[i], fi * s[i, 2], zt[i] * s[i, 3], extra_world_force=extra)
        for name, r in zip(("pos", "quat", "vel", "ang_v"), ref):
            np.testing.assert_allclose(ora.envs[name][i], r, rtol=1e-12, atol=1e-12, err_msg=f"drone {i}: {name}")
    if physics in (1, 4):
        assert n_gnd > n // 8


# ---- draws ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset,step0", [(0, 5), ((1 << 32) - 20, (1 << 32) - 3), ((1 << 33) + 12345, (1 << 40) + 7)])
def test_episode_start_and_gust_draws_follow_the_header(offset, step0):
    """orc_vec_reset_dw draws at each drone's own step counter (here spread across 2^32), and every step of a fleet whose episodes
    all end (max_steps = 0) replaces the gust's update by the stationary draw; with episodes running the gust steps.  Every value
    against the header's formulas on orc_philox4x32 words: scales exact, steady wind and gusts within one float32 ulp (libm cos /
    sin / log on both sides: equal here)."""
    n, seed = 40, 0x1234_5678_9ABC
    d, w = WIDE_BODY, GUSTY_WIND
    for max_steps, T in ((0, 3), (1 << 20, 3)):
        cfg = O.make_config([[5e3, 5e3, 5e3]], [0.0, 0.0, 1.0], WIDE, circle=False, cylinder=False, threshold=0.0, max_steps=max_steps,
                            normalize_obs=False, seed=seed, env_id_offset=offset, action_type=1, normalize_actions=False)
        ora = O.OracleVecEnv(cfg, n, dynamics=d, wind=w)
        steps = np.array([step0 + (i % 7) - 3 for i in range(n)], np.uint64)
        ora.envs["step_count"] = steps
        ora.reset()
        for i in range(n):
            gid, sc = offset + i, int(steps[i])
            assert ora.dw["dyn"][i].tolist() == want_scales(d, gid, sc, seed), i
            assert ulps(ora.dw["wind_mean"][i], want_mean(w, gid, sc, seed)).max() <= 1, i
            assert ulps(ora.dw["wind_gust"][i], want_gust_start(w, gid, sc, seed)).max() <= 1, i
        for t in range(T):
            prev = ora.dw.copy()
            sc = ora.envs["step_count"].copy()
            out = ora.step(np.zeros((n, 4), np.float32))
            assert out["done"].all() == (max_steps == 0) and out["done"].any() == (max_steps == 0)
            for i in range(n):
                gid = offset + i
                if max_steps == 0:      # an episode start at sc: new body, new steady wind, the stationary gust (not the update)
                    assert ora.dw["dyn"][i].tolist() == want_scales(d, gid, int(sc[i]), seed), (t, i)
                    assert ulps(ora.dw["wind_mean"][i], want_mean(w, gid, int(sc[i]), seed)).max() <= 1, (t, i)
                    assert ulps(ora.dw["wind_gust"][i], want_gust_start(w, gid, int(sc[i]), seed)).max() <= 1, (t, i)
                else:
                    assert np.array_equal(ora.dw["dyn"][i], prev["dyn"][i]) and np.array_equal(ora.dw["wind_mean"][i], prev["wind_mean"][i])
                    assert ulps(ora.dw["wind_gust"][i], want_gust_step(w, prev["wind_gust"][i], gid, int(sc[i]), seed)).max() <= 1, (t, i)


def test_without_resample_the_body_and_steady_wind_stay_and_the_gust_restarts():
    n, seed = 32, 9
    cfg = O.make_config([[5e3, 5e3, 5e3]], [0.0, 0.0, 1.0], WIDE, circle=False, cylinder=False, threshold=0.0, max_steps=1,
                        normalize_obs=False, seed=seed, action_type=1, normalize_actions=False)
    ora = O.OracleVecEnv(cfg, n, dynamics=dyn(mass=(0.5, 2.0), resample=False), wind=wind(speed=(1, 5), gust_sigma=(0.0, 0.0), resample=False))
    ora.reset()
    assert np.array_equal(ora.dw["dyn"], np.ones((n, 4), np.float32)) and not ora.dw["wind_mean"].any()
    rng = np.random.default_rng(1)
    ora.dw["dyn"] = rng.uniform(0.5, 2.0, (n, 4))
    ora.dw["wind_mean"][:, :3] = rng.normal(0, 3, (n, 3))
    ora.dw["wind_gust"][:, :3] = rng.normal(0, 1, (n, 3))
    keep = ora.dw.copy()
    out = ora.step(np.zeros((n, 4), np.float32))
    assert not out["done"].any() and np.array_equal(ora.dw, keep)          # sigma = (0, 0): no draws, g keeps its value ...
    out = ora.step(np.zeros((n, 4), np.float32))
    assert out["done"].all()
    assert np.array_equal(ora.dw["dyn"], keep["dyn"]) and np.array_equal(ora.dw["wind_mean"], keep["wind_mean"])
    assert not ora.dw["wind_gust"].any()                                    # ... and becomes 0 at the next episode start


# ---- physics sanity -------------------------------------------------------------------------------------------------------
def test_scales_and_wind_change_the_flight_as_documented():
    """Level hover thrust from rest in zero damping: a body of mass M s_m with thrust x s_kf accelerates by g (s_kf / s_m - 1)
    vertically; a steady wind w adds k w / (M s_m) (5 m/s on the nominal body: about 1.03 m/s^2)."""
    n = 4
    cfg = O.make_config([[5e3, 5e3, 5e3]], [0.0, 0.0, 1.0], WIDE, circle=False, cylinder=False, threshold=0.0, max_steps=1 << 20,
                        normalize_obs=False, action_type=1, normalize_actions=False, zero_damping=True)
    ora = O.OracleVecEnv(cfg, n, dynamics=dyn(resample=False), wind=wind(resample=False))
    ora.reset()
    ora.dw["dyn"] = [[1.0, 1.0, 1.0, 1.0], [1.25, 1.0, 1.0, 1.0], [1.0, 0.5, 1.1, 1.0], [0.8, 1.0, 1.0, 1.0]]
    ora.dw["wind_mean"][:, 0] = 5.0
    ora.step(np.zeros((n, 4), np.float32))
    m = RB.M * ora.dw["dyn"][:, 0].astype(np.float64)
    kxy = f32(5.5626e-3)
    np.testing.assert_allclose(ora.envs["vel"][:, 0], DT * kxy * 5.0 / m, rtol=1e-12)
    np.testing.assert_allclose(ora.envs["vel"][:, 2], DT * RB.G * (ora.dw["dyn"][:, 2].astype(np.float64) * (RB.M / m) - 1.0), rtol=1e-9,
                               atol=1e-15)
    assert abs(kxy * 5.0 / RB.M - 1.03) < 0.01


def test_gust_statistics_over_a_long_hover():
    """Stationary OU law: mean 0, standard deviation sigma, lag-1 correlation a = exp(-dt / tau) after 120 steps from the
    stationary draw."""
    n, T, seed = 16384, 120, 5
    w = wind(gust_sigma=(0.8, 0.3), gust_tau=0.25)
    cfg = O.make_config([[5e3, 5e3, 5e3]], [0.0, 0.0, 1.0], WIDE, circle=False, cylinder=False, threshold=0.0, max_steps=1 << 20,
                        normalize_obs=False, seed=seed, action_type=1, normalize_actions=False)
    ora = O.OracleVecEnv(cfg, n, threads=8, wind=w)
    ora.reset()
    zero = np.zeros((n, 4), np.float32)
    for _ in range(T - 1):
        assert not ora.step(zero)["done"].any()
    g0 = ora.dw["wind_gust"][:, :3].astype(np.float64)
    ora.step(zero)
    g1 = ora.dw["wind_gust"][:, :3].astype(np.float64)
    a = math.exp(-DT / w.gust_tau)
    sig = np.array([0.8, 0.8, 0.3])
    for j in range(3):
        assert abs(g1[:, j].mean()) < 5 * sig[j] / math.sqrt(n), j
        assert abs(g1[:, j].std() / sig[j] - 1.0) < 0.03, j
        assert abs(np.corrcoef(g0[:, j], g1[:, j])[0, 1] - a) < 0.002, j
