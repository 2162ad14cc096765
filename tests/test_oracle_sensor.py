"""The CPU oracle's restatement of the per-drone sensor model (oracle/dn_oracle.c orc_*_sens; include/dronenav.h dn_enable_sensor,
DESIGN.md section 4.1), pinned on its own before the GPU tests lean on it (tests/test_gpu_sensor_oracle.py).  The oracle keeps the
LOGICAL state dn_get_sensor returns -- d, b[13], hist[9][13] with hist[j] = o_{k - j}, shifted every step -- and no ring.

- layouts: orc_sens_state is 524 bytes, orc_sens_config starts with dn_sensor_config's 68; orc_config / orc_env keep their sizes;
- off is off: sensor=None, the defaults, and latency (0, 0) with zero amplitudes give orc_vec_step_act's bits over the physics x
  action-type x spawn grid of tests/test_oracle_actuator.py;
- transparency: reward, done, truncated, found_targets, ep_ret, ep_len and every state field outside the normaliser statistics are
  byte-equal to the same oracle without the sensor;
- the delivery rule, bit for bit, against tests/model_support.py's numpy Delivery on the sensor-less oracle's rows, terminal and
  reset rows included; the normaliser against the float64 Rms64 on the delivered stream at 1e-5 + 1e-5 |x|;
- draws against a restatement on orc_philox4x32 words, ids past 2^33 and step counters across 2^32;
- resample = 0: written d and b survive episode starts and are always applied, the reset row carries the written bias, and no row of
  the previous episode is delivered in the new one;
- coverage: the configurations, seeds and action streams of tests/test_gpu_sensor_oracle.py (defined once in tests/model_support.py) reach the
  cases that file claims to test, shown on the oracle alone.
CPU only; tests/test_oracle_asan.py runs this file under AddressSanitizer / UBSan too."""
import ctypes as C
import math

import numpy as np
import pytest

from model_support import (AMPS, CASES, CIRCLE6, FREE_WHERE, GUSTY_WIND, INST, INST_CELLS, LAT_FILL, LAUNCH_SHAPES, LOW, NOISE,
                           REENABLE, SENS_FREE, SENS_OPT, SENS_OPTION_CELLS, SENS_OPTION_IDS, SENS_SETV, SENSOR, SHAPE, SHAPES, WIDE_BODY,
                           Delivery, Rms64, act, actions_mixed, bits, config, free_body, option_actions, option_oracle, philox,
                           reenable_oracle, same_step, sens, sens_inst_oracle, sens_track_oracle, set_values, setv_oracle, setv_start,
                           shape_oracle, shape_plan, shape_values, stagger, unit)
from oracle import oracle as O

FP = C.POINTER(C.c_float)
OUT_KEYS = ("reward", "done", "truncated", "found_targets", "ep_ret", "ep_len", "terminated")
NOT_RMS = [k for k in O.ENV_DTYPE.names if not k.startswith("rms_")]


class Coverage:
    """The counting asserts of the GPU file about its inputs, from (d, s) at the entry of step t of a launch: the step is the
    episode's k-th, k = s + 1, and delivers the row of min(d, k) steps ago."""

    def __init__(self, n):
        self.n_done = self.young = self.delayed = self.crossed = self.after_restart = self.moved_spawn = self.last_done = 0
        self.seen = set()
        self.restarted = np.zeros(n, bool)

    def entry(self, d, s, t):
        k = s.astype(np.int64) + 1
        dd = np.minimum(d, k)
        if t == 0:
            self.restarted[:] = False
        self.seen.update(np.unique(d).tolist())
        self.young += int((k < d).sum())
        self.delayed += int(((d > 0) & (d <= k)).sum())
        self.crossed += int((dd > t).sum())                              # reaches back past the start of the launch
        self.after_restart += int((self.restarted & (dd > 0)).sum())    # an episode ended inside this launch, then a delayed delivery

    def done(self, mask, ora):
        mask = np.asarray(mask).astype(bool)
        self.n_done += int(mask.sum())
        self.restarted |= mask
        self.last_done += int(mask[-1])
        if ora.cfg.random_spawn:
            self.moved_spawn += int((ora.envs["spawn_pt"][mask] != np.array(ora.cfg.spawn[:])).any(axis=1).sum())


def run_oracle(ora, launches, cov):
    for acts in launches:
        for t in range(len(acts)):
            cov.entry(ora.sens["latency"].copy(), ora.envs["steps"].copy(), t)
            cov.done(ora.step(acts[t])["done"], ora)


# ---- layouts ---------------------------------------------------------------------------------------------------------------------
def test_layouts():
    L = O.lib()
    assert (L.orc_sizeof_env(), L.orc_sizeof_config()) == (696, 1704)
    assert L.orc_sizeof_act_state() == 152 and L.orc_sizeof_dw_state() == 48
    assert L.orc_sizeof_sens_state() == O.SENS_DTYPE.itemsize == 524 == 4 + 13 * 4 + 9 * 13 * 4
    assert L.orc_sizeof_sens_config() == C.sizeof(O.OrcSensConfig) == 68 + 8
    assert [O.SENS_DTYPE.fields[k][1] for k in ("latency", "bias", "history")] == [0, 4, 56]
    f = O.OrcSensConfig
    assert (f.latency.offset, f.bias_amp.offset, f.resample.offset, f.reserved.offset) == (0, 8, 60, 64)     # dn_sensor_config's
    ora = free_body(3, None)
    ora.enable_sensor(sens(latency=(2, 5), bias=AMPS))
    assert not ora.sens.tobytes().strip(b"\0")                           # the first enable: d = 0, b = 0, an all-zero history
    rule = {(lat, amp, rs): (c.lat_on, c.bias_on) for lat in ((0, 0), (0, 3), (2, 2)) for amp in (0.0, 0.1) for rs in (True, False)
            for c in [O.make_sens_config(sens(latency=lat, bias=amp, resample=rs))]}
    for (lat, amp, rs), got in rule.items():                            # the header's "off" paragraph
        assert got == ((1, 1) if not rs else (int(lat != (0, 0)), int(amp > 0))), (lat, amp, rs, got)


# ---- off is off ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("physics,act_type,spawn", CASES)
def test_off_is_off_bit_for_bit(physics, act_type, spawn):
    """sensor=None, SensorModel()'s defaults and latency (0, 0) with zero amplitudes against orc_vec_step_act itself, dynamics + wind +
    a latency-only actuator on where physics is even."""
    n, T = 96, 80
    track = CIRCLE6 if spawn else LOW
    kw = dict(max_steps=30, normalize_obs=True, ground_contact=False, physics=physics, action_type=act_type, random_spawn=spawn,
              normalize_actions=act_type == 0, seed=7, f32_state=True, act_noise_sigma=0.01, obs_noise_sigma=0.01)
    feat = dict(dynamics=WIDE_BODY, wind=GUSTY_WIND, actuator=act(latency=(0, 8), fill=LAT_FILL)) if physics % 2 == 0 else {}
    base = O.OracleVecEnv(config(track, **kw), n, **feat)
    others = [O.OracleVecEnv(config(track, **kw), n, sensor=s, **feat) for s in (None, sens(), sens(latency=(0, 0), bias=(0.0,) * 13))]
    L = O.lib()
    obs = np.empty((n, O.OBS_DIM), np.float32)
    L.orc_vec_reset_act(C.byref(base.cfg), *base._dw_args(), *base._act_args(), O._p(base.envs), n, O._p(obs), 1)   # the _act entry point
    for o in others:
        assert obs.tobytes() == o.reset().tobytes()
    rng = np.random.default_rng(physics * 8 + act_type)
    n_done = 0
    for t in range(T):
        acts = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
        if act_type == 0:
            acts[1::2] = (0.0922 + 0.003 * rng.standard_normal((n // 2, 4))).astype(np.float32)
        out = dict(obs=np.empty((n, O.OBS_DIM), np.float32), reward=np.empty(n, np.float32), done=np.empty(n, np.uint8),
                   truncated=np.empty(n, np.uint8), found_targets=np.empty(n, np.int32), terminal_obs=np.zeros((n, O.OBS_DIM), np.float32),
                   ep_ret=np.zeros(n, np.float32), ep_len=np.zeros(n, np.int32), terminated=np.empty(n, np.uint8))
        L.orc_vec_step_act(C.byref(base.cfg), *base._dw_args(), *base._act_args(), O._p(base.envs), n, O._p(acts), *(O._p(out[k]) for k in (
            "obs", "reward", "done", "truncated", "found_targets", "terminal_obs", "ep_ret", "ep_len", "terminated")), 1)
        for o in others:
            same_step(out, o.step(acts), t)
        n_done += int(out["done"].sum())
    for o in others:
        assert base.envs.tobytes() == o.envs.tobytes() and base.dw.tobytes() == o.dw.tobytes() and base.act.tobytes() == o.act.tobytes()
        assert not o.sens.tobytes().strip(b"\0")                         # off: nothing is drawn, nothing is stored
    assert n_done > n // 2


# ---- transparency, the delivery rule and the normaliser ----------------------------------------------------------------------------
def drive(S, P, model, T, rng, make_acts, norm, seed, gid0=0, sc0=0, stagger=True):
    """S (sensor on) beside P (the same oracle without it, normaliser OFF: its rows are the o_k).  Every row S writes against Delivery
    on P's rows: int32 views with S's normaliser off, Rms64 on the delivered stream at 1e-5 + 1e-5 |x| with it on.  Outputs and state
    outside the normaliser statistics byte-equal.  Returns (Delivery, worst fraction of the bar)."""
    n = S.n
    dl, rs, every = Delivery(model, n, seed, gid0), Rms64(n), np.arange(n)
    worst = [0.0]

    def check(got, y, rows, tag):
        if norm:
            want = rs(y, rows)
            frac = np.abs(got.astype(np.float64) - want) / (1e-5 + 1e-5 * np.abs(want))
            worst[0] = max(worst[0], float(frac.max(initial=0.0)))
            assert worst[0] <= 1.0, (tag, worst[0])
        else:
            assert np.array_equal(bits(got), bits(y)), tag

    o0 = P.reset()
    check(S.reset(), dl.start(every, o0, sc0), every, "reset")
    if stagger:
        k0 = rng.integers(0, 40, n)
        hist = rng.uniform(-1, 1, (n, 9, 13)).astype(np.float32)
        hist[:, 0] = o0
        S.envs["steps"] = P.envs["steps"] = k0
        S.sens["history"], dl.hist, dl.k = hist, hist.copy(), k0.astype(np.int64)
    for t in range(T):
        acts = make_acts(rng, n)
        sc = int(P.envs["step_count"][0])
        rS, rP = S.step(acts), P.step(acts)
        for k in OUT_KEYS:
            assert rS[k].tobytes() == rP[k].tobytes(), (k, t)
        done = rP["done"].astype(bool)
        rows, live = np.flatnonzero(done), np.flatnonzero(~done)
        y = dl.step(np.where(done[:, None], rP["terminal_obs"], rP["obs"]))
        check(rS["obs"][live], y[live], live, f"t={t} obs")                  # the normaliser: a finished drone's terminal row, then its reset row
        check(rS["terminal_obs"][rows], y[rows], rows, f"t={t} terminal_obs")
        check(rS["obs"][rows], dl.start(rows, rP["obs"][rows], sc), rows, f"t={t} reset rows")
        dl.ends += len(rows)
        for k in NOT_RMS:
            assert S.envs[k].tobytes() == P.envs[k].tobytes(), (k, t)
        assert np.array_equal(S.sens["latency"], dl.d) and np.array_equal(bits(S.sens["bias"]), bits(dl.b)), t
        valid = np.arange(9)[None, :] <= dl.k[:, None]
        assert not S.sens_cfg.lat_on or np.array_equal(bits(S.sens["history"])[valid], bits(dl.hist)[valid]), t
    assert S.dw.tobytes() == P.dw.tobytes() and S.act.tobytes() == P.act.tobytes()
    return dl, worst[0]


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "norm"])
@pytest.mark.parametrize("full", [False, True], ids=["alone", "dynamics+wind+actuator"])
def test_delivery_rule_transparency_and_normaliser(full, norm):
    n, T, seed = 300, 240, 31
    kw = dict(max_steps=40, seed=seed, **NOISE)
    S = sens_track_oracle("circle4", n, SENSOR, full, normalize_obs=norm, **kw)
    P = sens_track_oracle("circle4", n, None, full, normalize_obs=False, **kw)
    dl, worst = drive(S, P, sens(**SENSOR), T, np.random.default_rng(5), actions_mixed, norm, seed)
    assert dl.seen == set(range(9)) and dl.ends >= 3 * n and dl.young > 0, (dl.seen, dl.ends, dl.young)
    if norm:
        # each delivered row is fed once: the reset row, one row per step, and one more per episode end (terminal row, then reset row)
        assert int(np.rint(S.envs["rms_count"] - 1e-4).sum()) == n * (T + 1) + dl.ends
        print(f"normaliser against Rms64: worst fraction of the bar {worst:.3f}")


@pytest.mark.parametrize("which", ["latency-alone", "bias-alone"])
def test_each_half_alone(which):
    model = dict(latency=(0, 8), bias=0.0) if which == "latency-alone" else dict(latency=(0, 0), bias=AMPS)
    n, seed = 200, 33
    kw = dict(max_steps=25, seed=seed, normalize_obs=False, **NOISE)
    S, P = sens_track_oracle("circle4", n, model, False, **kw), sens_track_oracle("circle4", n, None, False, **kw)
    assert (S.sens_cfg.lat_on, S.sens_cfg.bias_on) == ((1, 0) if which == "latency-alone" else (0, 1))
    dl, _ = drive(S, P, sens(**model), 100, np.random.default_rng(6), actions_mixed, False, seed, stagger=which == "latency-alone")
    assert dl.ends > n
    if which == "bias-alone":
        assert not S.sens["latency"].any() and not S.sens["history"].any()      # the history is maintained only while the delay is on


# ---- draws -----------------------------------------------------------------------------------------------------------------------
def want_draw(model, gid, step, seed):
    """FOUR Philox calls on streams 18..21, u_m = (r_c + 0.5) / 2^32, m = 4 q + c: b_j = float32(amp_j (2 u_j - 1)) in float64,
    d = lo + floor((hi - lo + 1) u_13) clamped to hi."""
    u = [unit(r) for q in range(4) for r in philox(gid, step, 18 + q, seed)]
    lo, hi = model.latency
    b = [float(np.float32(float(np.float32(a)) * (2.0 * u[j] - 1.0))) for j, a in enumerate(model.bias)]
    return min(lo + int(math.floor((hi - lo + 1) * u[13])), hi), b


@pytest.mark.parametrize("offset,step0", [(0, 5), ((1 << 32) - 20, (1 << 32) - 3), ((1 << 33) + 12345, (1 << 40) + 7)])
def test_draws_follow_the_header(offset, step0):
    """Reset draws at each drone's own step counter (spread across 2^32); with max_steps = 0 every step ends every episode and draws
    again keyed by that step; with episodes running nothing is drawn.  d and b exact."""
    n, seed = 300, 0x1234_5678_9ABC
    model = sens(latency=(1, 8), bias=AMPS)
    seen = set()
    for max_steps, T in ((0, 3), (1 << 20, 3)):
        ora = free_body(n, None, seed=seed, max_steps=max_steps, env_id_offset=offset)
        ora.enable_sensor(model)
        steps = np.array([step0 + (i % 7) - 3 for i in range(n)], np.uint64)
        ora.envs["step_count"] = steps
        ora.reset()

        def same(sc):
            want = [want_draw(model, offset + i, int(sc[i]), seed) for i in range(n)]
            assert ora.sens["latency"].tolist() == [w[0] for w in want]
            assert np.array_equal(bits(ora.sens["bias"]), bits(np.array([w[1] for w in want], np.float32)))

        same(steps)
        for t in range(T):
            prev, sc = ora.sens.copy(), ora.envs["step_count"].copy()
            out = ora.step(np.full((n, 4), 0.07, np.float32))
            assert out["done"].all() == (max_steps == 0) and out["done"].any() == (max_steps == 0)
            if max_steps == 0:
                same(sc)
                assert t == 0 or ora.sens["latency"].tolist() != prev["latency"].tolist()
            else:
                assert np.array_equal(ora.sens["latency"], prev["latency"]) and np.array_equal(bits(ora.sens["bias"]), bits(prev["bias"]))
            seen.update(ora.sens["latency"].tolist())
            assert np.all(np.abs(ora.sens["bias"]) <= np.float32(AMPS)) and np.abs(ora.sens["bias"]).min(axis=0).max() > 0
    assert seen == set(range(1, 9))


# ---- resample = 0 ------------------------------------------------------------------------------------------------------------------
def test_without_resample_written_values_survive_and_are_always_applied():
    """The header: "resample = 0: d and b are what dn_set_sensor last wrote", "both are always applied".  Against the sensor-less
    oracle P: y_k = float32(o_{k - min(d, k)} + b) with the WRITTEN d and b in every episode, the reset row = float32(o_0 + b), and --
    the written history being a constant 1000 no observation reaches -- no row older than the episode is ever delivered."""
    n, T, seed = 256, 60, 12
    kw = dict(max_steps=7, seed=seed, normalize_obs=False, **NOISE)
    S, P = sens_track_oracle("circle4", n, dict(SENSOR, resample=False), False, **kw), sens_track_oracle("circle4", n, None, False, **kw)
    assert (S.sens_cfg.lat_on, S.sens_cfg.bias_on) == (1, 1)
    zero = sens_track_oracle("circle4", n, dict(latency=(0, 0), bias=0.0, resample=False), False, **kw)
    assert (zero.sens_cfg.lat_on, zero.sens_cfg.bias_on) == (1, 1)       # the values are the caller's: applied whatever the ranges say
    o0 = P.reset()
    assert np.array_equal(bits(S.reset()), bits(o0 + np.float32(0.0)))   # d = 0, b = 0 after the first enable
    vals = set_values(np.random.default_rng(4), n)
    vals["history"][:] = 1000.0
    vals["history"][:, 0] = o0
    for k, v in vals.items():
        S.sens[k] = v
    d, b = vals["latency"].astype(np.int64), vals["bias"]
    log = [[o0[i]] for i in range(n)]                                     # log[i] = the rows o_0 .. o_k of drone i's current episode
    n_done = young = 0
    for t in range(T):
        acts = actions_mixed(np.random.default_rng(100 + t), n)
        rS, rP = S.step(acts), P.step(acts)
        done = rP["done"].astype(bool)
        for i in range(n):
            log[i].append(rP["terminal_obs"][i] if done[i] else rP["obs"][i])
            k = len(log[i]) - 1
            young += k < d[i]
            y = log[i][k - min(d[i], k)] + b[i]
            got = rS["terminal_obs"][i] if done[i] else rS["obs"][i]
            assert np.array_equal(bits(got), bits(y)), (t, i)
            if done[i]:
                assert np.array_equal(bits(rS["obs"][i]), bits(rP["obs"][i] + b[i])), (t, i)      # the reset row carries the written bias
                log[i] = [rP["obs"][i]]
        assert np.abs(rS["obs"]).max() < 10.0 and np.abs(rS["terminal_obs"]).max() < 10.0          # the 1000s never leave
        assert np.array_equal(S.sens["latency"], vals["latency"]) and np.array_equal(bits(S.sens["bias"]), bits(b)), t
        n_done += int(done.sum())
    assert n_done > 5 * n and young > n and set(np.unique(d).tolist()) == set(range(9))


def test_a_second_enable_keeps_the_values_and_a_late_enable_waits_for_the_next_episode():
    n, seed = 200, 5
    kw = dict(max_steps=30, seed=seed, normalize_obs=False, **NOISE)
    S, P = sens_track_oracle("circle4", n, None, False, **kw), sens_track_oracle("circle4", n, None, False, **kw)
    S.reset(), P.reset()
    rng = np.random.default_rng(3)
    for t in range(12):
        a = actions_mixed(rng, n)
        same_step(S.step(a), P.step(a), t)
    S.enable_sensor(sens(**SENSOR))                                       # late: d = 0, b = 0 until each drone's next episode start
    started = np.zeros(n, bool)
    for t in range(40):
        a = actions_mixed(rng, n)
        rS, rP = S.step(a), P.step(a)
        quiet = ~started & ~rP["done"].astype(bool)
        assert np.array_equal(bits(rS["obs"][quiet]), bits(rP["obs"][quiet] + np.float32(0.0))), t
        started |= rP["done"].astype(bool)
        assert not S.sens["latency"][~started].any() and not S.sens["bias"][~started].any()
    assert started.all() and set(np.unique(S.sens["latency"]).tolist()) == set(range(9)) and np.abs(S.sens["bias"]).min() > 0
    before = S.sens.copy()
    S.enable_sensor(sens(**REENABLE["second"]))
    assert S.sens.tobytes() == before.tobytes()                           # "changes the configuration and keeps the current values"
    for t in range(40):
        dn = S.step(actions_mixed(rng, n))["done"].astype(bool)
        keep = ~dn if t == 0 else keep & ~dn
        assert np.array_equal(S.sens["latency"][keep], before["latency"][keep])
    assert not keep.any() and 2 <= S.sens["latency"].min() and S.sens["latency"].max() <= 5
    assert np.abs(S.sens["bias"]).max() > max(AMPS)


# ---- coverage of the GPU configurations, on the reference alone --------------------------------------------------------------------
@pytest.mark.parametrize("dt,norm,noise,mode", INST_CELLS, ids=[f"{d}-norm{a}-noise{b}-{m}" for d, a, b, m in INST_CELLS])
def test_coverage_of_the_instantiation_cells(dt, norm, noise, mode):
    n, T, K = INST["n"], INST["T"], (1 if mode == "step" else INST["K"])
    assert n % 64 != 0                                                   # a partial last tile
    ora = sens_inst_oracle(dt, norm, noise)
    assert (ora.act_cfg is None) == (ora.dw_cfg is None) == (not norm)   # the raw cells fly the sensor alone
    ora.reset()
    rng = np.random.default_rng(INST["rng"])
    stagger(ora, rng)
    cov = Coverage(n)
    run_oracle(ora, (np.stack([actions_mixed(rng, n) for _ in range(K)]) for _ in range(T // K)), cov)
    assert cov.n_done > n and cov.seen == set(range(9)) and cov.young > 0 and cov.delayed > 0 and cov.crossed > n, vars(cov)
    assert cov.last_done > 0                                             # ... on the last drone of the partial tile too
    if mode == "rollout":
        assert cov.after_restart > 0, vars(cov)


@pytest.mark.parametrize("cell", range(len(SENS_OPTION_CELLS)), ids=SENS_OPTION_IDS)
def test_coverage_of_the_option_cells(cell):
    n, T = SENS_OPT["n"], SENS_OPT["T"]
    physics, act_name, normalized, extra, feat = SENS_OPTION_CELLS[cell]
    ora = option_oracle(cell, n)
    assert (ora.act_cfg is None) == (feat == "sensor") and (ora.dw_cfg is None) == (feat != "both")
    ora.reset()
    rng = np.random.default_rng(SENS_OPT["rng"])
    cov = Coverage(n)
    run_oracle(ora, ([option_actions(rng, n, act_name, normalized)] for _ in range(T)), cov)
    assert cov.n_done >= n and cov.seen == set(range(9)) and cov.young > 0 and cov.delayed > 0, vars(cov)
    if extra.get("random_spawn"):
        assert cov.moved_spawn > n // 2, vars(cov)                        # reset rows whose columns 0-2 are not cfg.spawn's
    if act_name in ("pid", "vel", "one_d_pid"):
        assert np.abs(ora.envs["pid"]).max() > 0


@pytest.mark.parametrize("where", list(FREE_WHERE))
def test_coverage_of_the_free_running_launches(where):
    n, K = SENS_FREE["n"], SENS_FREE["K"]
    off, sc0 = FREE_WHERE[where]
    ora = sens_track_oracle("race", n, SENSOR, True, max_steps=SENS_FREE["max_steps"], normalize_obs=False, seed=SENS_FREE["seed"], env_id_offset=off)
    ora.envs["step_count"] = sc0
    ora.reset()
    rng = np.random.default_rng(SENS_FREE["rng"])
    stagger(ora, rng)
    cov = Coverage(n)
    run_oracle(ora, (np.stack([rng.uniform(-1, 1, (n, 4)).astype(np.float32) for _ in range(K)]) for _ in range(SENS_FREE["launches"])), cov)
    assert cov.n_done > 2 * n and cov.after_restart > n and cov.crossed > 0 and cov.seen == set(range(9)) and cov.young > 0, vars(cov)
    assert int(ora.envs["step_count"][0]) == sc0 + K * SENS_FREE["launches"] and K // 16 == 4       # the 16-slot ring wraps four times a launch


@pytest.mark.parametrize("n", SHAPES + LAUNCH_SHAPES)
def test_coverage_of_the_tile_shapes(n):
    ora = shape_oracle(n)
    ora.reset()
    for k, v in shape_values(n).items():
        ora.sens[k] = v
    rng = np.random.default_rng(SHAPE["rng"])
    cov = Coverage(n)
    starts = np.zeros(n, int)
    for K, single in shape_plan(n):
        c = Coverage(n) if K > 1 else cov
        run_oracle(ora, [np.stack([actions_mixed(rng, n) for _ in range(K)])], c)
        starts += c.restarted
        if K > 1:                                                        # every drone restarts inside every launch
            assert c.restarted.all() and c.last_done > 0 and c.after_restart > 0, vars(c)
    assert (n % 4 == 0) == (n in LAUNCH_SHAPES) and n % 64 != 0
    assert cov.last_done > 0 and cov.n_done >= 2 * n and (cov.young > 0 or n == 1), vars(cov)      # n = 1: the one drone has latency 0
    assert starts.min() >= 2 and cov.seen == set(range(min(n, 9))), (starts.min(), cov.seen)
    assert np.array_equal(ora.sens["latency"], np.arange(n) % 9)


def test_coverage_of_the_set_values_and_the_late_enable():
    n = SENS_SETV["n"]
    ora = setv_oracle()
    ora.reset()
    rng = np.random.default_rng(SENS_SETV["rng"])
    ora.envs["steps"], vals = setv_start(rng, n)
    for k, v in vals.items():
        ora.sens[k] = v
    cov = Coverage(n)
    run_oracle(ora, (np.stack([actions_mixed(rng, n) for _ in range(SENS_SETV["K"])]) for _ in range(SENS_SETV["launches"])), cov)
    assert cov.n_done > 4 * n and cov.crossed > 0 and cov.after_restart > 0 and cov.young > 0 and cov.seen == set(range(9)), vars(cov)
    assert np.array_equal(ora.sens["latency"], vals["latency"]) and n % 64 != 0
    n = REENABLE["n"]
    ora = reenable_oracle()
    ora.reset()
    rng = np.random.default_rng(REENABLE["rng"])
    run_oracle(ora, [np.stack([actions_mixed(rng, n) for _ in range(REENABLE["pre"])])], Coverage(n))
    mid = int((ora.envs["steps"] > 0).sum())
    assert mid > n // 2                                                   # the first enable lands in the middle of running episodes
    ora.enable_sensor(sens(**SENSOR))
    cov = Coverage(n)
    for _ in range(REENABLE["launches"]):
        run_oracle(ora, [np.stack([actions_mixed(rng, n) for _ in range(REENABLE["K"])])], cov)
    assert cov.n_done >= n and cov.seen == set(range(9)) and cov.young > 0
    ora.enable_sensor(sens(**REENABLE["second"]))
    cov = Coverage(n)
    for _ in range(REENABLE["launches"]):
        run_oracle(ora, [np.stack([actions_mixed(rng, n) for _ in range(REENABLE["K"])])], cov)
    assert cov.n_done >= n and {2, 3, 4, 5} <= cov.seen and cov.delayed > 0
