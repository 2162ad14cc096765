"""The CPU oracle's restatement of the per-drone actuator model (oracle/dn_oracle.c orc_*_act; include/dronenav.h
dn_enable_actuator), pinned on its own before the GPU tests lean on it (tests/test_gpu_actuator_oracle.py):

- off is off: no actuator, and latency [0, 0] + motor_tau [0, 0], give orc_vec_step_dw's bits over the physics x action-type x spawn
  grid of tests/test_oracle_dynamics_wind.py, dynamics + wind on in some;
- latency: the oracle with latency = the oracle without it fed the shifted actions, bit for bit, with action noise and the normaliser,
  through episode ends; the shift is written here from the header sentence, as a look-up in the log of every command ever given;
- lag: a = 0 gives the nominal bits; a constant command follows c + (rpm_fill - c) a^k; one step of a lagged drone against
  tests/rigid_body_ref.py driven by forces formed from a numpy float64 filter (1e-12), with drag, ground effect and scaled bodies;
- episode starts: r = rpm_fill after every done; the new a acts from the first step of the new episode, the terminal step flew the old;
- draws: (d, a) against a restatement on orc_philox4x32 words, ids past 2^32 and step counters across 2^32; resample = 0 keeps values;
- coverage: the configurations, seeds and action streams of tests/test_gpu_actuator_oracle.py (defined once in tests/model_support.py) reach
  the cases that file claims to test -- episode ends, fills, latencies 0 and 8, history entries consumed across a launch boundary,
  episode restarts inside a launch, the ground effect acting -- shown on the oracle alone.
CPU only; tests/test_oracle_asan.py runs this file under AddressSanitizer / UBSan too."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import rigid_body_ref as RB
from oracle import oracle as O
from model_support import (ACT_FREE, ACT_OPT, ACT_SETV, ACTION_TYPES, BODY, CASES, CIRCLE6, DT, FREE_WHERE, FULL, GUSTY, GUSTY_WIND,
                           HOVER_FILL, INST, INST_CELLS, LAG_OPTION_CELLS, LAT_OPTION_CELLS, LOW, NOISE, PHYSICS, RAW_FILL, SHORT, WIDE,
                           WIDE_BODY, act, act_inst_oracle, act_track_oracle, actions_mixed, config, dyn, f32, free_body, option_actions,
                           option_setup, philox, same_step, short_set_values, stagger, ulps, unit, wind)

FP, DP = C.POINTER(C.c_float), C.POINTER(C.c_double)
ODD_FILL = (0.05, -0.3, 0.0922, 0.7)


class Coverage:
    """The counting asserts of the GPU file about its inputs, evaluated from (d, s) at the entry of step t of a launch."""

    def __init__(self):
        self.n_done = self.fills = self.crossed = self.restarted = self.delayed = 0
        self.seen = set()

    def entry(self, d, s, t):
        self.seen.update(np.unique(d).tolist())
        self.fills += int((s < d).sum())
        self.delayed += int(((d > 0) & (s >= d)).sum())
        self.crossed += int(((t < d) & (s >= d)).sum())          # consumed from the history of an earlier launch
        self.restarted += int(((t > 0) & (s < d)).sum())         # the episode restarted inside the launch and took `fill`

    def done(self, mask):
        self.n_done += int(np.asarray(mask).sum())


def run_oracle(ora, launches, cov, gnd_every=0):
    """`launches` = an iterable of [K, n, 4] action blocks; returns the number of (sampled) drone-steps on which the ground effect acted."""
    L = O.lib()
    n_gnd = 0
    for li, acts in enumerate(launches):
        for t in range(len(acts)):
            cov.entry(ora.act["latency"].copy(), ora.envs["steps"].copy(), t)
            if gnd_every and (li * len(acts) + t) % gnd_every == 0:
                e = ora.envs
                rpm = np.full(4, 14000.0)
                for i in range(0, ora.n, 8):
                    g = np.zeros(4)
                    L.orc_ground_effect(e["pos"][i].ctypes.data_as(DP), e["quat"][i].ctypes.data_as(DP), e["rpy"][i].ctypes.data_as(DP),
                                        rpm.ctypes.data_as(DP), 1, g.ctypes.data_as(DP))
                    n_gnd += bool(g.any())
            cov.done(ora.step(acts[t])["done"])
    return n_gnd


# ---- the pieces restated ---------------------------------------------------------------------------------------------------
def chain(actions, normalized):
    """The nominal float32 action chain's speeds (orc_rescale_action -> orc_preprocess_action, pinned by the golden vectors)."""
    L = O.lib()
    a = np.ascontiguousarray(actions, np.float32).reshape(-1, 4)
    rpm = np.zeros_like(a)
    for i in range(len(a)):
        src = a[i].copy()
        if normalized:
            r = np.zeros(4, np.float32)
            L.orc_rescale_action(src.ctypes.data_as(FP), r.ctypes.data_as(FP))
            src = r
        L.orc_preprocess_action(src.ctypes.data_as(FP), rpm[i].ctypes.data_as(FP))
    return rpm


def lag64(a, r, c):
    """r <- float32(a r + (1 - a) c), float64 in that nesting, numpy."""
    a = np.asarray(a, np.float32).astype(np.float64).reshape(-1, 1)
    return (a * np.asarray(r, np.float32).astype(np.float64) + (1.0 - a) * np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def want_draw(model, gid, step, seed):
    """ONE Philox call on stream 17: d = lo + floor((hi - lo + 1) u_0) clamped to hi; tau = lo + (hi - lo) u_1, a = float32(exp(-dt / tau))."""
    r = philox(gid, step, 17, seed)
    lo, hi = model.latency
    d = min(lo + int(math.floor((hi - lo + 1) * unit(r[0]))), hi)
    tau = f32(model.motor_tau[0]) + (f32(model.motor_tau[1]) - f32(model.motor_tau[0])) * unit(r[1])
    return d, (f32(math.exp(-DT / tau)) if tau > 0.0 else 0.0)


# ---- layout -----------------------------------------------------------------------------------------------------------------
def test_layouts():
    L = O.lib()
    assert (L.orc_sizeof_env(), L.orc_sizeof_config()) == (696, 1704)
    assert L.orc_sizeof_dw_state() == 48 and L.orc_sizeof_dw_config() == C.sizeof(O.OrcDwConfig)
    assert L.orc_sizeof_act_state() == O.ACT_DTYPE.itemsize == 152 and L.orc_sizeof_act_config() == C.sizeof(O.OrcActConfig)
    assert [O.ACT_DTYPE.fields[k][1] for k in ("latency", "coeff", "rpm", "history")] == [0, 4, 8, 24]
    ora = free_body(3, act(latency=(2, 5), motor_tau=(0.0, 0.1), fill=RAW_FILL))
    assert not ora.act["latency"].any() and not ora.act["coeff"].any()              # the first enable: d = 0, a = 0,
    assert np.array_equal(ora.act["rpm"], np.tile(chain([RAW_FILL], False), (3, 1)))  # r = rpm_fill,
    assert np.array_equal(ora.act["history"], np.tile(np.float32(RAW_FILL), (3, 8, 1)))   # history = fill
    norm = O.OracleVecEnv(config(LOW, normalize_actions=True), 2, actuator=act(fill=ODD_FILL))
    assert np.array_equal(norm.act["rpm"][0], chain([ODD_FILL], True)[0])           # rescaled first where the env normalises actions


# ---- off is off ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("physics,act_type,spawn", CASES)
def test_off_is_off_bit_for_bit(physics, act_type, spawn):
    """actuator=None and latency [0, 0] + motor_tau [0, 0] (resample on: every episode start draws d = 0, a = 0) against
    orc_vec_step_dw, dynamics + wind on where physics is even."""
    n, T = 96, 80
    track = CIRCLE6 if spawn else LOW
    kw = dict(max_steps=30, normalize_obs=True, ground_contact=False, physics=physics, action_type=act_type, random_spawn=spawn,
              normalize_actions=act_type == 0, seed=7, f32_state=True, act_noise_sigma=0.01, obs_noise_sigma=0.01)
    feat = dict(dynamics=WIDE_BODY, wind=GUSTY_WIND) if physics % 2 == 0 else {}
    base = O.OracleVecEnv(config(track, **kw), n, **feat)
    none = O.OracleVecEnv(config(track, **kw), n, actuator=None, **feat)
    zero = O.OracleVecEnv(config(track, **kw), n, actuator=act(fill=ODD_FILL), **feat)
    L = O.lib()
    obs = np.empty((n, O.OBS_DIM), np.float32)
    L.orc_vec_reset_dw(C.byref(base.cfg), *base._dw_args(), O._p(base.envs), n, O._p(obs), 1)      # the _dw entry point itself
    assert obs.tobytes() == none.reset().tobytes() == zero.reset().tobytes()
    rng = np.random.default_rng(physics * 8 + act_type)
    n_done = 0
    for t in range(T):
        acts = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
        if act_type == 0:
            acts[1::2] = (0.0922 + 0.003 * rng.standard_normal((n // 2, 4))).astype(np.float32)
        out = dict(obs=np.empty((n, O.OBS_DIM), np.float32), reward=np.empty(n, np.float32), done=np.empty(n, np.uint8),
                   truncated=np.empty(n, np.uint8), found_targets=np.empty(n, np.int32), terminal_obs=np.zeros((n, O.OBS_DIM), np.float32),
                   ep_ret=np.zeros(n, np.float32), ep_len=np.zeros(n, np.int32), terminated=np.empty(n, np.uint8))
        L.orc_vec_step_dw(C.byref(base.cfg), *base._dw_args(), O._p(base.envs), n, O._p(acts), *(O._p(out[k]) for k in (
            "obs", "reward", "done", "truncated", "found_targets", "terminal_obs", "ep_ret", "ep_len", "terminated")), 1)
        same_step(out, none.step(acts), t)
        same_step(out, zero.step(acts), t)
        n_done += int(out["done"].sum())
        assert not zero.act["latency"].any() and not zero.act["coeff"].any()
    assert base.envs.tobytes() == none.envs.tobytes() == zero.envs.tobytes() and base.dw.tobytes() == zero.dw.tobytes()
    assert n_done > n // 2
    # rpm only changes at episode starts (to rpm_fill: it never leaves it), the history holds the last 8 commands
    assert np.array_equal(zero.act["rpm"], np.tile(zero.act_cfg.rpm_fill[:], (n, 1)).astype(np.float32))
    assert np.array_equal(zero.act["history"][:, 0], acts)


# ---- latency --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "noise+norm", "dynamics+wind"])
def test_latency_equals_the_oracle_fed_shifted_actions(variant):
    """The header: "the action chain consumes the action commanded d vector steps ago if s >= d, and `fill` otherwise".  Here: log[k]
    = the commands of vector step k, and every command before the first step is `fill` (the first enable's history); drone i at vector
    step t with (d, s) read before the step flies log[t - d][i] if s >= d else fill.  B, without an actuator, is fed that."""
    n, T, seed = 300, 90, 31
    kw = dict(max_steps=40, seed=seed, normalize_obs=variant != "plain")
    if variant != "plain":
        kw.update(NOISE)
    dw = variant == "dynamics+wind"
    A = act_track_oracle("circle4", n, dict(latency=(0, 8), fill=ODD_FILL), dw, **kw)
    B = act_track_oracle("circle4", n, dict(), dw, **kw)
    B.enable_actuator(None)
    assert A.reset().tobytes() == B.reset().tobytes()
    rng = np.random.default_rng(5)
    stagger(A, rng)
    B.envs["steps"] = A.envs["steps"]
    fill = np.float32(ODD_FILL)
    log = {k: np.tile(fill, (n, 1)) for k in range(-8, 0)}
    cov = Coverage()
    idx = np.arange(n)
    for t in range(T):
        d, s = A.act["latency"].copy(), A.envs["steps"].copy()
        cov.entry(d, s, t)
        log[t] = actions_mixed(rng, n)
        ago = np.stack([log[t - k] for k in range(9)])                  # ago[k] = commanded k vector steps ago
        eff = np.where((s >= d)[:, None], ago[d, idx], fill)
        ra, rb = A.step(log[t]), B.step(eff)
        same_step(ra, rb, t)
        cov.done(ra["done"])
        assert np.array_equal(A.act["history"], ago[:8].transpose(1, 0, 2)), t      # takes the COMMANDED action, also on a done step
    assert A.envs.tobytes() == B.envs.tobytes() and A.dw.tobytes() == B.dw.tobytes()
    assert cov.n_done > n and cov.fills > 0 and cov.delayed > 0 and {0, 8} <= cov.seen, vars(cov)


# ---- lag --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalized", [True, False])
def test_zero_coefficient_is_the_nominal_path_bit_for_bit(normalized):
    """Lag ON (a nonzero motor_tau range, resample = 0) with every coeff = 0: float32(0 r + 1 c) = c, so every output is the
    nominal one; and rpm then holds c, the chain's speeds for the (noised) action."""
    n, T = 200, 70
    kw = dict(max_steps=25, normalize_obs=True, ground_contact=False, physics=4, seed=9, f32_state=True, normalize_actions=normalized,
              obs_noise_sigma=0.01)
    lagged = O.OracleVecEnv(config(LOW, **kw), n, dynamics=WIDE_BODY, wind=GUSTY_WIND,
                            actuator=act(motor_tau=(0.02, 0.15), fill=HOVER_FILL if normalized else RAW_FILL, resample=False))
    plain = O.OracleVecEnv(config(LOW, **kw), n, dynamics=WIDE_BODY, wind=GUSTY_WIND)
    assert lagged.reset().tobytes() == plain.reset().tobytes()
    rng = np.random.default_rng(2)
    n_done = 0
    for t in range(T):
        acts = option_actions(rng, n, "thrust", normalized)
        ra, rb = lagged.step(acts), plain.step(acts)
        same_step(ra, rb, t)
        c = chain(acts, normalized)
        dn = ra["done"].astype(bool)
        assert np.array_equal(lagged.act["rpm"][~dn], c[~dn]) and np.array_equal(lagged.act["rpm"][dn], np.tile(lagged.act_cfg.rpm_fill[:], (dn.sum(), 1)))
        n_done += int(dn.sum())
    assert lagged.envs.tobytes() == plain.envs.tobytes() and n_done > n and not lagged.act["coeff"].any()


def test_constant_command_follows_the_closed_form():
    """r_k = c + (rpm_fill - c) a^k; r is rounded to float32 every step: half an ulp enters per step and the earlier ones decay by a,
    so the distance stays below 0.5 / (1 - a) ulp, plus one for the cast of the closed form (the bound of the GPU test of this name):
    tau = 0.02 gives a = 0.812, 0.5 / (1 - a) = 2.7 -> 4 ulp."""
    n, steps = 64, 24
    ora = free_body(n, act(motor_tau=(0.02, 0.02), fill=(0.03, 0.03, 0.03, 0.03), resample=False))
    ora.reset()
    a = np.float32(math.exp(-DT / f32(0.02)))
    assert math.ceil(0.5 / (1.0 - float(a))) + 1 == 4
    ora.act["coeff"] = a
    thrust = np.random.default_rng(1).uniform(0.03, 0.15, (n, 4)).astype(np.float32)
    c = chain(thrust, False).astype(np.float64)
    r0 = ora.act["rpm"].astype(np.float64)
    assert np.abs(r0 - c).min() > 100.0
    for k in range(1, steps + 1):
        assert not ora.step(thrust)["done"].any()
        assert ulps(ora.act["rpm"], (c + (r0 - c) * float(a) ** k).astype(np.float32)).max() <= 4, k


@pytest.mark.parametrize("physics,normalized", [(0, False), (1, True), (2, False), (4, True)])
def test_lagged_step_matches_independent_integrator(physics, normalized, monkeypatch):
    """Random tumbling states (a quarter upright and low: the ground effect acts), ActionType.THRUST with the lag on, coefficients in
    [0.3, 0.98], previous speeds r anywhere in the commanded span, bodies with scales in [0.7, 1.3]: c from the chain, r' from the numpy
    float64 filter, forces KF r'^2 and the yaw torque from KM r'^2 in numpy float32 (BaseAviary._physics on a float32 array), the
    ground effect of r' (orc_ground_effect) added before x s_kf, the PYB_DRAG force of the PREVIOUS step's speeds
    (last_clipped_action), then rigid_body_ref.step with M s_m, J s_I.  1e-12, the bar of tests/test_oracle_dynamics_wind.py."""
    rng = np.random.default_rng(200 + physics)
    n = 400
    quat = Rotation.random(n, random_state=physics + 3).as_quat()
    quat[: n // 4] = Rotation.from_euler("xyz", rng.uniform(-0.4, 0.4, (n // 4, 3))).as_quat()
    pos = rng.uniform(-2, 2, (n, 3)) + [0, 0, 3]
    pos[: n // 4, 2] = rng.uniform(0.02, 0.3, n // 4)
    vel, ang_v = rng.normal(0, 2.0, (n, 3)), rng.normal(0, 8.0, (n, 3))
    last = rng.uniform(12000, 21000, (n, 4)).astype(np.float32)
    cfg = O.make_config([[5e3, 5e3, 5e3]], [0.0, 0.0, 1.0], WIDE, circle=False, cylinder=False, threshold=0.0, max_steps=1 << 20,
                        normalize_actions=normalized, normalize_obs=False, physics=physics, action_type=0, seed=3)
    ora = O.OracleVecEnv(cfg, n, dynamics=dyn(resample=False), actuator=act(motor_tau=(0.01, 0.2), fill=HOVER_FILL, resample=False))
    ora.reset()
    for k, v in (("pos", pos), ("quat", quat), ("vel", vel), ("ang_v", ang_v), ("cur_pos", pos), ("last_clipped_action", last)):
        ora.envs[k] = v
    ora.refresh_rpy()
    ora.dw["dyn"] = rng.uniform(0.7, 1.3, (n, 4))
    ora.act["coeff"] = rng.uniform(0.3, 0.98, n)
    ora.act["rpm"] = rng.uniform(9500, 21600, (n, 4))
    a, r_prev, s, rpy = ora.act["coeff"].copy(), ora.act["rpm"].copy(), ora.dw["dyn"].astype(np.float64), ora.envs["rpy"].copy()
    acts = option_actions(rng, n, "thrust", normalized)
    assert not ora.step(acts)["done"].any()
    r = lag64(a, r_prev, chain(acts, normalized))
    assert np.array_equal(ora.act["rpm"], r) and np.array_equal(ora.envs["last_clipped_action"], r.astype(np.float64))
    assert np.abs(r.astype(np.float64) - chain(acts, normalized)).min(axis=1).max() > 1000.0       # r is not c: the lag is seen
    sq = r * r
    f, tq = (sq * np.float32(RB.KF)).astype(np.float64), sq * np.float32(RB.KM)
    zt = (((-tq[:, 0] + tq[:, 1]) - tq[:, 2]) + tq[:, 3]).astype(np.float64)
    L = O.lib()
    M0, J0 = RB.M, RB.J.copy()
    n_gnd = 0
    for i in range(n):
        fi, extra = f[i].copy(), None
        p, q = np.ascontiguousarray(pos[i]), np.ascontiguousarray(quat[i])
        if physics in (1, 4):
            g = np.zeros(4)
            L.orc_ground_effect(p.ctypes.data_as(DP), q.ctypes.data_as(DP), np.ascontiguousarray(rpy[i]).ctypes.data_as(DP),
                                r[i].astype(np.float64).ctypes.data_as(DP), 1, g.ctypes.data_as(DP))
            fi = fi + g
            n_gnd += bool(g.any())
        if physics in (2, 4):
            d = np.zeros(3)
            L.orc_drag(q.ctypes.data_as(DP), np.ascontiguousarray(vel[i]).ctypes.data_as(DP), last[i].astype(np.float64).ctypes.data_as(DP), 1,
                       d.ctypes.data_as(DP))
            extra = Rotation.from_quat(quat[i]).as_matrix() @ d
        monkeypatch.setattr(RB, "M", M0 * s[i, 0])
        monkeypatch.setattr(RB, "J", J0 * s[i, 1])
        ref = RB.step(pos[i], quat[i], vel[i], ang_v[i], fi * s[i, 2], zt[i] * s[i, 3], extra_world_force=extra)
        for name, want in zip(("pos", "quat", "vel", "ang_v"), ref):
            np.testing.assert_allclose(ora.envs[name][i], want, rtol=1e-12, atol=1e-12, err_msg=f"drone {i}: {name}")
    if physics in (1, 4):
        assert n_gnd > n // 8


# ---- episode starts -----------------------------------------------------------------------------------------------------------------
def test_episode_start_sets_rpm_fill_and_the_new_coefficient_acts_from_the_first_step_only():
    """Free bodies, a constant command far from rpm_fill, episodes of up to 5 steps (staggered), (d, a) redrawn at every start with
    latency 0.  Not done: r' = the filter with the a read BEFORE the step.  Done: r' = rpm_fill exactly and a' = the draw, which differs
    from a; the terminal step flew the OLD a (its outputs equal a twin's that keeps a: resample = 0), and the next step's r is the
    filter from rpm_fill with the NEW a, which the old a would not have produced."""
    n, T, seed = 128, 18, 41
    model = act(motor_tau=(0.02, 0.15), fill=(0.03, 0.03, 0.03, 0.03))
    ora = free_body(n, model, seed=seed, max_steps=4, physics=4, obs_noise_sigma=0.01)
    twin = free_body(n, act(motor_tau=(0.02, 0.15), fill=(0.03, 0.03, 0.03, 0.03), resample=False), seed=seed, max_steps=4, physics=4,
                     obs_noise_sigma=0.01)
    ora.reset()
    twin.reset()
    stagger(ora, np.random.default_rng(0), hi=4)
    thrust = np.random.default_rng(1).uniform(0.10, 0.15, (n, 4)).astype(np.float32)
    c = chain(thrust, False)
    fill_rpm = np.tile(chain([model.fill], False), (n, 1))
    assert np.array_equal(ora.act["rpm"], fill_rpm) and np.abs(c - fill_rpm).min() > 3000.0
    was_done = np.zeros(n, bool)
    n_done = n_first = 0
    for t in range(T):
        a, r, sc = ora.act["coeff"].copy(), ora.act["rpm"].copy(), ora.envs["step_count"].copy()
        twin.envs[:], twin.act[:] = ora.envs, ora.act
        out, ref = ora.step(thrust), twin.step(thrust)
        same_step(out, ref, t)                                           # the step, terminal ones included, flew the a it entered with
        dn = out["done"].astype(bool)
        assert np.array_equal(ora.act["rpm"][~dn], lag64(a, r, c)[~dn]) and np.array_equal(ora.act["rpm"][dn], fill_rpm[dn]), t
        assert np.array_equal(r[was_done], fill_rpm[was_done])
        n_first += int((was_done & ~dn).sum())                           # first steps of an episode: r above is lag64(new a, rpm_fill, c)
        for i in np.flatnonzero(dn):
            d_new, a_new = want_draw(model, i, int(sc[i]), seed)
            assert d_new == 0 == ora.act["latency"][i] and ulps(ora.act["coeff"][i], a_new) <= 1 and ora.act["coeff"][i] != a[i]
            assert not np.array_equal(lag64([a[i]], fill_rpm[i], c[i]), lag64([ora.act["coeff"][i]], fill_rpm[i], c[i]))
        assert np.array_equal(ora.act["coeff"][~dn], a[~dn])
        was_done = dn
        n_done += int(dn.sum())
    assert n_done > 3 * n and n_first > n


# ---- draws ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset,step0", [(0, 5), ((1 << 32) - 20, (1 << 32) - 3), ((1 << 33) + 12345, (1 << 40) + 7)])
def test_draws_follow_the_header(offset, step0):
    """Reset draws at each drone's own step counter (spread across 2^32); with max_steps = 0 every step ends every episode and draws
    again keyed by that step; with episodes running nothing is drawn.  d exact, a within one float32 ulp (libm exp on both sides)."""
    n, seed = 400, 0x1234_5678_9ABC
    model = act(latency=(1, 8), motor_tau=(0.02, 0.15), fill=RAW_FILL)
    seen = set()
    for max_steps, T in ((0, 3), (1 << 20, 3)):
        ora = free_body(n, model, seed=seed, max_steps=max_steps, env_id_offset=offset)
        steps = np.array([step0 + (i % 7) - 3 for i in range(n)], np.uint64)
        ora.envs["step_count"] = steps
        ora.reset()
        want = [want_draw(model, offset + i, int(steps[i]), seed) for i in range(n)]
        assert ora.act["latency"].tolist() == [w[0] for w in want] and ulps(ora.act["coeff"], [w[1] for w in want]).max() <= 1
        for t in range(T):
            prev, sc = ora.act.copy(), ora.envs["step_count"].copy()
            out = ora.step(np.full((n, 4), 0.07, np.float32))
            assert out["done"].all() == (max_steps == 0) and out["done"].any() == (max_steps == 0)
            if max_steps == 0:
                want = [want_draw(model, offset + i, int(sc[i]), seed) for i in range(n)]
                assert ora.act["latency"].tolist() == [w[0] for w in want] and ulps(ora.act["coeff"], [w[1] for w in want]).max() <= 1
                assert t == 0 or ora.act["latency"].tolist() != prev["latency"].tolist()      # t = 0: the reset drew at this very step
            else:
                assert np.array_equal(ora.act["latency"], prev["latency"]) and np.array_equal(ora.act["coeff"], prev["coeff"])
            seen.update(ora.act["latency"].tolist())
            assert 1 <= ora.act["latency"].min() and ora.act["latency"].max() <= 8
            assert 0.81 < ora.act["coeff"].min() and ora.act["coeff"].max() < 0.973       # exp(-dt / 0.02) .. exp(-dt / 0.15)
    assert seen == set(range(1, 9))
    zero_tau = free_body(8, act(latency=(3, 3)), seed=seed)
    zero_tau.act["coeff"] = 0.5
    zero_tau.reset()
    assert (zero_tau.act["latency"] == 3).all() and not zero_tau.act["coeff"].any()            # a = 0 where tau = 0


def test_without_resample_written_values_survive_episode_starts():
    n = 256
    ora = free_body(n, act(latency=(0, 8), motor_tau=(0.02, 0.15), fill=RAW_FILL, resample=False), max_steps=2)
    ora.reset()
    assert not ora.act["latency"].any() and not ora.act["coeff"].any()
    vals = short_set_values(np.random.default_rng(4), n)
    for k, v in vals.items():
        ora.act[k] = v
    n_done = 0
    for t in range(7):
        n_done += int(ora.step(np.full((n, 4), 0.08, np.float32))["done"].sum())
    assert n_done == 2 * n and np.array_equal(ora.act["latency"], vals["latency"]) and np.array_equal(ora.act["coeff"], vals["coeff"])


# ---- coverage of the GPU configurations, on the reference alone --------------------------------------------------------------------
@pytest.mark.parametrize("dt,norm,noise,mode", INST_CELLS, ids=[f"{d}-norm{a}-noise{b}-{m}" for d, a, b, m in INST_CELLS])
def test_coverage_of_the_instantiation_cells(dt, norm, noise, mode):
    n, T, K = INST["n"], INST["T"], (1 if mode == "step" else INST["K"])
    ora = act_inst_oracle(dt, norm, noise)
    ora.reset()
    rng = np.random.default_rng(INST["rng"])
    stagger(ora, rng)
    cov = Coverage()
    run_oracle(ora, (np.stack([actions_mixed(rng, n) for _ in range(K)]) for _ in range(T // K)), cov)
    assert cov.n_done > n and cov.fills > 0 and {0, 8} <= cov.seen, vars(cov)
    a = ora.act["coeff"]
    assert 0.81 < a.min() and a.max() < 0.973 and len(np.unique(a)) > n // 2                   # the lag is on, drone by drone
    if mode == "rollout":
        assert cov.crossed > 0 and cov.restarted > 0, vars(cov)


@pytest.mark.parametrize("cell", range(len(LAG_OPTION_CELLS) + len(LAT_OPTION_CELLS)))
def test_coverage_of_the_option_cells(cell):
    n, T = ACT_OPT["n"], ACT_OPT["T"]
    if cell < len(LAG_OPTION_CELLS):
        physics, normalized, extra, feat = LAG_OPTION_CELLS[cell]
        act_name = "thrust"
    else:
        (physics, act_name), normalized, extra, feat = LAT_OPTION_CELLS[cell - len(LAG_OPTION_CELLS)], False, {}, "both"
    wp, spawn, dim, circle, kw, model = option_setup(physics, act_name, normalized, extra)
    cfg = O.make_config(wp, spawn.ravel(), dim, circle=circle, f32_state=True, physics=PHYSICS[physics], action_type=ACTION_TYPES[act_name], **kw)
    both = feat == "both"
    ora = O.OracleVecEnv(cfg, n, threads=8, dynamics=dyn(**BODY) if both else None, wind=wind(**GUSTY) if both else None,
                         actuator=act(**model))
    ora.reset()
    rng = np.random.default_rng(ACT_OPT["rng"])
    cov = Coverage()
    gnd = "gnd" in physics and not extra.get("random_spawn")
    n_gnd = run_oracle(ora, ([option_actions(rng, n, act_name, normalized)] for _ in range(T)), cov, gnd_every=5 if gnd else 0)
    assert cov.n_done > n // 2 and cov.fills > 0 and cov.delayed > 0 and {0, 8} <= cov.seen, vars(cov)
    if gnd:
        assert n_gnd > 0
    if act_name in ("pid", "vel", "one_d_pid"):          # delayed commands have been through the controller's state (integrals, last attitude)
        assert np.abs(ora.envs["pid"]).max() > 0 and cov.delayed > 10 * n
    if act_name == "thrust":
        assert len(np.unique(ora.act["coeff"])) > n // 2


@pytest.mark.parametrize("where", list(FREE_WHERE))
def test_coverage_of_the_free_running_launches(where):
    n, K = ACT_FREE["n"], ACT_FREE["K"]
    off, sc0 = FREE_WHERE[where]
    ora = act_track_oracle("race", n, FULL, True, max_steps=ACT_FREE["max_steps"], normalize_obs=False, seed=ACT_FREE["seed"], env_id_offset=off)
    ora.envs["step_count"] = sc0
    ora.reset()
    rng = np.random.default_rng(ACT_FREE["rng"])
    stagger(ora, rng)
    cov = Coverage()
    run_oracle(ora, (np.stack([rng.uniform(-1, 1, (n, 4)).astype(np.float32) for _ in range(K)]) for _ in range(ACT_FREE["launches"])), cov)
    assert cov.n_done > 2 * n and cov.restarted > 0 and cov.crossed > 0 and {0, 8} <= cov.seen, vars(cov)
    assert int(ora.envs["step_count"][0]) == sc0 + K * ACT_FREE["launches"]


def test_coverage_of_the_short_launches_and_set_values():
    n = SHORT["n"]
    ora = act_track_oracle("circle4", n, FULL, True, max_steps=SHORT["max_steps"], normalize_obs=False, seed=SHORT["seed"])
    ora.reset()
    rng = np.random.default_rng(SHORT["rng"])
    stagger(ora, rng, hi=SHORT["max_steps"])
    assert set(SHORT["Ks"]) == {1, 3, 7, 8, 9}
    per_k = {}
    for K in SHORT["Ks"]:
        ora.act["latency"][: n // 2] = 8                  # half the fleet at the full depth, whatever was drawn
        cov = per_k.setdefault(K, Coverage())
        run_oracle(ora, [np.stack([actions_mixed(rng, n) for _ in range(K)])], cov)
    for K, cov in per_k.items():
        assert cov.crossed > 0 and cov.n_done > 0 and 8 in cov.seen, (K, vars(cov))
        assert (cov.restarted > 0) == (K > 1), (K, vars(cov))
    ora = act_track_oracle("circle4", n, dict(FULL, resample=False), False, max_steps=ACT_SETV["max_steps"], normalize_obs=False, seed=ACT_SETV["seed"])
    ora.reset()
    rng = np.random.default_rng(ACT_SETV["rng"])
    for k, v in short_set_values(rng, n).items():
        ora.act[k] = v
    cov = Coverage()
    run_oracle(ora, (np.stack([actions_mixed(rng, n) for _ in range(ACT_SETV["K"])]) for _ in range(ACT_SETV["launches"])), cov)
    assert cov.n_done > 2 * n and cov.crossed > 0 and cov.restarted > 0 and cov.seen == set(range(9)), vars(cov)
