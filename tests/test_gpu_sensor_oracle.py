"""The per-drone sensor model (dn_enable_sensor: observation latency + per-episode bias) on the HIP path against the CPU oracle
(oracle/dn_oracle.c orc_vec_step_sens, written from include/dronenav.h as a shifted logical history, no ring, and itself pinned by
tests/test_oracle_sensor.py).  The configurations, seeds and action streams live in tests/model_support.py; tests/test_oracle_sensor.py shows on the
oracle alone that they reach the cases claimed here (every latency 0..8, deliveries with k < d and d <= k, episode ends inside a fused
launch followed by a delayed delivery, moved spawn points, an episode end on the last drone of a partial tile); every test here first
checks that its oracle has that file's configuration, byte for byte.

a. All 16 instantiations of dn_step_many_1w_kernel<R, NORM, NOISE, ONE, ..., M = DN_M_SENS> at n = 1000 (a partial last tile): dynamics +
   wind + actuator ride in the norm cells, the raw cells fly the sensor alone (the null-pointer paths of the family).  The oracle is
   loaded with the device's state AND its sensor state (latency, bias, logical history) before every step / 5-step launch.  Outputs
   at the existing bars.  Bit-exact part: a delivered row that reaches back past the start of the launch is float32(loaded history +
   bias) as int32 views (raw cells); after the launch latency, bias and every history entry that was already loaded are bit-equal;
   entries written during the launch are held at the observation bar.
b. The run-time options with the sensor on (22 cells), teacher-forced.
c. Free-running fused launches of 64 steps, ids past 2^33 / the step counter across 2^32, all four models on.
d. Tile shapes n in {1, 63, 65, 191} in single steps beside a fleet of n + 1 drones; dn_step_many refuses K > 1 unless num_envs % 4
   == 0, so the K = 20 launches fly at n in {4, 60, 68, 188} beside n + 4.
e. Values written by set_sensor with resample = 0.   f. A late first enable and a second enable.

No bar here is new: compare_step's 1e-5 (float64 compute), 5e-4 (float32 compute, over sqrt(min(var, 1)) under the normaliser), at most
1e-4 of the drone-steps with a flipped done flag, the lock-step discipline of the free-running tests, or exact equality.

Mutation evidence (one MI355X; each mutant changes values or ring-masked indices only; tests failed in this file of 50 | in
tests/test_gpu_sensor.py of 33):
 1. sx.k without the + 1: 49 (a-f, all tests but shape n = 1) | 22
 2. the reset row seeded into sens_slot(sc + 1): 49 | 22
 3. sens_restart adds the previous episode's bias: 41 (a, b, c, f) | 22
 4. SPAWN columns written after sens_restart: 2, the two random_spawn option cells | 0
 5. the resample = 0 branch does not reload the bias: 9, the eight shapes and the set-values test | 0
 6. the `active` guard on sens_deliver's store dropped: 0 | 0.  An equivalent mutant: an inactive lane shadows the last drone of its
    tile (same index, same registers), so the extra store writes that drone's own row to that drone's own address.
 7. dn_reset_kernel seeds sens_slot(sc): 45 (a, b, seven shapes) | 0
 8. the history kernel's - j turned into + j: 39 (a, b, set values) | 23
"""
import ctypes as C

import numpy as np
import pytest

import model_support as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gpu_support import (DEV, _features, _get_sens, _pair, _rollout_outs, _same_config, _stagger, check_act, check_dw,  # noqa: E402
                         check_sens, load_sens)
from gpu_support import pkg as _pkg  # noqa: E402
from model_support import NOISE, _step_mismatch, actions_mixed, bits, compare_step  # noqa: E402


def _launch(env, acts, single):
    dev = torch.device(DEV)
    if single:
        outs = [env.step_tensor(torch.from_numpy(acts[0]).to(dev))]
    else:
        outs = _rollout_outs(env.rollout_tensor(torch.from_numpy(acts).to(dev), want_terminal=True), len(acts))
    torch.cuda.synchronize()
    return [(o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy(), {k: v.cpu().numpy() for k, v in info.items() if k in (
        "truncated", "found_targets", "terminal_obs", "ep_length", "ep_return")}) for o, r, d, info in outs]


class _T:
    """compare_step / _step_mismatch call .cpu().numpy() on what they are given."""

    def __init__(self, a):
        self.a, self.shape = a, a.shape

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def _wrap(out):
    return _T(out[0]), _T(out[1]), _T(out[2]), {k: _T(v) for k, v in out[3].items()}


class Stats:
    def __init__(self):
        self.episodes = self.flips = self.delivered = self.exact = 0
        self.frac = 0.0

    def line(self, tag, dropped=0):
        share = self.exact / max(self.delivered, 1)
        return (f"SENS {tag}: {self.episodes} episodes compared, worst fraction of the observation bar {self.frac:.3f}, "
                f"{share:.4f} of the delivered rows bit for bit ({self.exact} / {self.delivered}), {self.flips} flags flipped, "
                f"{dropped} drones dropped at a branch cut")


def _exact_deliveries(outs, g0, k0, stats, tag, ncol=13):
    """A delivered row that reaches back past the start of the launch -- min(d, k) > t at step t -- was in the loaded history:
    float32(history[min(d, k) - t - 1] + bias), one float32 add per column, bit for bit.  The device's own done flags say which
    row is the delivered one (terminal_obs on an episode end) and which drones have restarted."""
    n = len(k0)
    idx = np.arange(n)
    restarted = np.zeros(n, bool)
    d0 = np.clip(g0["latency"].astype(np.int64), 0, 8)
    for t, (obs, _, done, info) in enumerate(outs):
        dd = np.minimum(d0, k0.astype(np.int64) + t + 1)
        back = (dd > t) & ~restarted
        row = np.where(done.astype(bool)[:, None], info["terminal_obs"], obs)[:, :ncol]
        want = (g0["history"][idx, np.maximum(dd - t - 1, 0)] + g0["bias"])[:, :ncol]
        assert np.array_equal(bits(row[back]), bits(want[back])), f"{tag} t={t}: a row of the loaded history left changed"
        stats.delivered += n
        stats.exact += int(back.sum())
        restarted |= done.astype(bool)
    return restarted


def _outputs(out, ref, f32, norm_var, fused, stats, tag):
    """The existing output bars.  Returns the mask of drones whose done flag agrees (all of them in float64 compute)."""
    obs, _, done, info = out
    k = obs.shape[1]
    dn = ref["done"].astype(bool)
    if f32:
        same = done == ref["done"]
        stats.flips += int((~same).sum())
        bar = 5e-4 / np.sqrt(np.minimum(norm_var, 1.0))[:, :k] if norm_var is not None else np.full((len(dn), k), 5e-4)
        err = np.abs(obs.astype(np.float64) - ref["obs"][:, :k]) / bar
        term = np.abs(info["terminal_obs"].astype(np.float64) - ref["terminal_obs"][:, :k]) / bar
        frac = max(float(err[same].max(initial=0.0)), float(term[same & dn].max(initial=0.0)))
        assert frac <= 1.0, f"{tag}: obs / terminal_obs at {frac:.3f} of the 5e-4 bar"
    else:
        same = np.ones(len(dn), bool)
        compare_step(_wrap(out), ref, tag, rew_atol=1e-4 if fused else 1e-5)
        frac = max(float(np.abs(obs.astype(np.float64) - ref["obs"][:, :k]).max()),
                   float(np.abs(info["terminal_obs"].astype(np.float64) - ref["terminal_obs"][:, :k])[dn].max(initial=0.0))) / 1e-5
    stats.frac = max(stats.frac, frac)
    stats.episodes += int((dn & same).sum())
    return same


# ---- a. every instantiation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,norm,noise,mode", M.INST_CELLS, ids=[f"{d}-norm{a}-noise{b}-{m}" for d, a, b, m in M.INST_CELLS])
def test_every_sensor_instantiation_matches_oracle(dt, norm, noise, mode, monkeypatch):
    """n = 1000 (15 full tiles and one of 40 lanes), 150 steps, max_steps = 40, staggered step counters, latency [0, 8] + bias AMPS.
    Measured on one MI355X against the oracle (every run prints the line): 3661 episodes compared in each of the 16 cells, no done
    flag flipped, no drone dropped.  Worst fraction of the observation bar (1e-5 float64 compute, 5e-4 float32 compute, over
    sqrt(min(var, 1)) under the normaliser), step | rollout:
      f64 raw 0.024 | 0.024, f64 raw+noise 0.024 | 0.024, f64 norm 0.143 | 0.167, f64 norm+noise 0.143 | 0.143,
      f32 raw 0.125 | 0.132, f32 raw+noise 0.126 | 0.170, f32 norm 0.046 | 0.046, f32 norm+noise 0.133 | 0.158.
    Share of the 150 000 delivered rows per raw cell that reached back past the launch start and were checked bit for bit, step |
    rollout: f64 0.8912 | 0.6452, f64 noise 0.8836 | 0.6370, f32 0.8919 | 0.6438, f32 noise 0.9014 | 0.6549 (a single step checks
    every delayed delivery: 8 of 9 latencies; the rest are undelayed rows or rows measured inside the launch, held at the bar)."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, T, K = M.INST["n"], M.INST["T"], (1 if mode == "step" else M.INST["K"])
    f32 = dt == "f32"
    if norm and noise and not f32:
        # the reason written in tests/test_gpu_actuator_oracle.py: the default noise draws are float32 transcendentals, one ulp of
        # obs + noise over a running std of 0.01 is 1.2e-5; DN_EXACT_OBS_NOISE=1 is the same kernel with the float64 form of the draws
        monkeypatch.setenv("DN_EXACT_OBS_NOISE", "1")
    dynamics, wind = _features(pkg, bool(norm), bool(norm))
    kw = dict(max_steps=M.INST["max_steps"], normalize_obs=bool(norm), seed=M.sens_inst_seed(dt, norm, noise),
              compute_dtype="float32" if f32 else "float64", sensor=pkg.SensorModel(**M.SENSOR), **(NOISE if noise else {}))
    if norm:
        kw.update(actuator=pkg.ActuatorModel(**M.FULL))
    env, ora = _pair(tracks.circle(1, 4, 1), n, dynamics, wind, **kw)
    ora.enable_actuator(M.act(**M.FULL) if norm else None)
    ora.enable_sensor(M.sens(**M.SENSOR))
    _same_config(ora, M.sens_inst_oracle(dt, norm, noise, n=1))
    assert env.kernel_waves(fused=True) == env.kernel_waves(fused=False) == 1
    r0 = env.reset_tensor().cpu().numpy()
    want0 = ora.reset()
    if not norm:
        np.testing.assert_allclose(r0, want0, rtol=0, atol=5e-4 if f32 else 1e-5, err_msg="reset rows")
    every = np.ones(n, bool)
    check_sens(env, ora, every, None, np.zeros(n, np.int64), 9, np.ones(n, bool), 5e-4 if f32 else 1e-5, "reset")
    rng = np.random.default_rng(M.INST["rng"])
    _stagger(env, rng)
    stats = Stats()
    bar = 5e-4 if f32 else 1e-5
    tag0 = f"{dt}/norm{norm}/noise{noise}/{mode}"
    for launch in range(T // K):
        g0 = load_sens(env, ora)
        k0 = ora.envs["steps"].astype(np.int64)
        acts = np.stack([actions_mixed(rng, n) for _ in range(K)])
        outs = _launch(env, acts, mode == "step")
        tag = f"{tag0} launch {launch}"
        restarted = np.zeros(n, bool)
        if not norm:
            restarted = _exact_deliveries(outs, g0, k0, stats, tag)
        agree = np.ones(n, bool)
        for t, out in enumerate(outs):
            ref = ora.step(acts[t])
            agree &= _outputs(out, ref, f32, ora.envs["rms_var"] if norm else None, mode == "rollout", stats, f"{tag} t={t}")
            if norm:
                restarted |= ref["done"].astype(bool)
        if norm:
            check_dw(env, ora, agree, f32, mode == "rollout", tag)
            check_act(env, ora, agree, f32, mode == "rollout", tag)
        check_sens(env, ora, agree, g0, k0, K, restarted, bar, tag)
    assert stats.episodes > n
    assert stats.flips <= n * T * 1e-4, f"{stats.flips} done flags differ"
    assert norm or stats.exact > n, "no delivered row reached back past a launch start"
    print(stats.line(tag0))
    env.close()


# ---- b. options ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", range(len(M.SENS_OPTION_CELLS)), ids=M.SENS_OPTION_IDS)
def test_options_with_the_sensor_match_oracle(cell):
    """Teacher-forced single steps, 100 steps at 1024 drones, compare_step's 1e-5, float64 compute.  The 18 cells of
    tests/test_gpu_actuator_oracle.py with the sensor on top, three with the sensor and nothing else (thrust, PID, random_spawn) and
    one with the normaliser.  random_spawn: the rows of dn_reset and of the in-kernel auto-resets are spawn-point columns + noise + the
    NEW bias.  With a single step per launch every delayed delivery reaches back past the launch start: all of them are checked bit
    for bit against float32(loaded history + bias) in the cells without the normaliser.
    Measured on one MI355X against the oracle: 1024 episodes compared per cell (3072 in the two random_spawn cells, max_steps = 25),
    no done flag flipped; worst fraction of the 1e-5 bar 0.012 in 17 cells, 0.024 in three (pyb_gnd thrust, one_d_pid, the
    sensor-only pyb_gnd_drag_dw pid), 0.003 for one_d_rpm, 0.167 in the normaliser cell; 91 454 of 102 400 delivered
    rows (0.8931) checked bit for bit in every raw cell, 91 800 (0.8965) in the random_spawn cells, none in the normaliser cell."""
    pkg = _pkg()
    n, T = M.SENS_OPT["n"], M.SENS_OPT["T"]
    physics, act, normalized, extra, feat = M.SENS_OPTION_CELLS[cell]
    wp, spawn, dim, circle, kw, model, both = M.option_cell(cell)
    dynamics, wind = _features(pkg, both, both)
    env = pkg.DroneVecEnv(None, n, target_points=wp, initial_xyzs=spawn, aviary_dim=dim, circle=circle, device=DEV, physics=physics,
                          act=act, dynamics=dynamics, wind=wind, actuator=None if model is None else pkg.ActuatorModel(**model),
                          sensor=pkg.SensorModel(**M.SENSOR), **kw)
    assert env.kernel_waves(fused=True) == env.kernel_waves(fused=False) == 1
    assert pkg.vec_env.PHYSICS == M.PHYSICS and pkg.vec_env.ACTION_TYPES == M.ACTION_TYPES
    ora = M.option_oracle(cell, n, ground_contact=env.ground_contact)
    ora.dw_cfg = O.make_dw_config(dynamics, wind)
    _same_config(ora, M.option_oracle(cell, 1))
    norm = bool(kw["normalize_obs"])
    ncol = env.obs_dim
    assert ncol == (13 if kw.get("include_distance", True) else 12)
    r0 = env.reset_tensor().cpu().numpy()
    want0 = ora.reset()
    if not norm:
        np.testing.assert_allclose(r0, want0[:, :ncol], rtol=0, atol=1e-5, err_msg="dn_reset rows")
    every = np.ones(n, bool)
    check_sens(env, ora, every, None, np.zeros(n, np.int64), 9, every, 1e-5, "reset", ncol)
    rng = np.random.default_rng(M.SENS_OPT["rng"])
    stats = Stats()
    tag0 = M.SENS_OPTION_IDS[cell]
    for t in range(T):
        g0 = load_sens(env, ora)
        k0 = ora.envs["steps"].astype(np.int64)
        a = M.option_actions(rng, n, act, normalized)
        outs = _launch(env, a[None], True)
        restarted = outs[0][2].astype(bool)
        if not norm:
            _exact_deliveries(outs, g0, k0, stats, f"{tag0} t={t}", ncol)
        _outputs(outs[0], ora.step(a), False, None, False, stats, f"{tag0} t={t}")
        if both:
            check_dw(env, ora, every, False, False, f"{tag0} t={t}")
        if model is not None:
            check_act(env, ora, every, False, False, f"{tag0} t={t}")
        check_sens(env, ora, every, g0, k0, 1, restarted, 1e-5, f"{tag0} t={t}", ncol)
    assert stats.episodes >= n and (norm or stats.exact > n)
    print(stats.line(tag0))
    env.close()


# ---- c. - f. free-running launches ---------------------------------------------------------------------------------------------------
def _lockstep(env, ora, acts, lock, tag, single=False):
    """One launch (single: one dn_step) against the free-running oracle with the discipline of test_gpu_actuator_oracle._lockstep_launch:
    a drone may leave ONLY at an atan2 branch cut, at most 8 of them.  Returns (episodes compared, the device's outputs)."""
    outs = _launch(env, acts, single)
    n_done = 0
    for t, o in enumerate(outs):
        bias = ora.sens["bias"].astype(np.float64) if ora.sens_cfg is not None else np.zeros((ora.n, 13))
        ref = ora.step(acts[t])
        bad = _step_mismatch(_wrap(o), ref, obs_atol=1e-4, rew_atol=2e-4)
        first = bad & lock
        if first.any():
            # the delivered row less the bias it left with: the row as it was measured, min(d, k) steps ago
            row = np.where(ref["done"].astype(bool)[:, None], ref["terminal_obs"], ref["obs"])[first].astype(np.float64) - bias[first]
            at_cut = (np.abs(np.abs(row[:, 3]) - 1.0) <= 1e-5) | (np.abs(np.abs(row[:, 5]) - 1.0) <= 1e-5) | \
                     (np.abs(np.abs(row[:, 4]) - 0.5) <= 1e-2)
            assert at_cut.all(), (f"{tag} t={t}: drones {np.flatnonzero(first)[~at_cut][:8]} left lockstep away from an atan2 branch "
                                  f"cut (raw roll / pitch / yaw columns {row[~at_cut][:4, 3:6]})")
        lock &= ~bad
        assert (~lock).sum() <= 8, f"{tag} t={t}: {int((~lock).sum())} drones out of lockstep"
        n_done += int((ref["done"].astype(bool) & lock).sum())
    return n_done, outs


def _exact_state(env, ora, lock, tag):
    got = _get_sens(env)
    assert np.array_equal(got["latency"][lock], ora.sens["latency"][lock]), f"{tag}: latency"
    assert np.array_equal(bits(got["bias"][lock]), bits(ora.sens["bias"][lock])), f"{tag}: bias"
    return got


@pytest.mark.parametrize("where", list(M.FREE_WHERE))
def test_free_running_fused_launches_with_the_sensor_match_oracle(where):
    """K = 64 (the 16-slot ring wraps four times per launch), 4096 drones, 256 steps of U(-1, 1) commands on the race track,
    max_steps = 100, dynamics + wind + actuator + sensor; both sides keep their own state.  Sensor latency and bias of the drones in
    lockstep exact after every launch.  The staggered step counters reach behind the reset row, so after the stagger the oracle's
    history is copied from the device once, as an initial condition: the rows delivered from behind the reset row in the first launch
    (at most 8 per drone) are the device's own and prove nothing; every later row is measured by each side for itself.
    Measured on one MI355X: 8200 (ids past 2^33) and 8195 (step counter across 2^32) episodes compared, 0 drones dropped."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, K = M.SENS_FREE["n"], M.SENS_FREE["K"]
    off, sc0 = M.FREE_WHERE[where]
    dynamics, wind = _features(pkg, True, True)
    kw = dict(max_steps=M.SENS_FREE["max_steps"], normalize_obs=False, seed=M.SENS_FREE["seed"], env_id_offset=off)
    env, ora = _pair(tracks.reaching(), n, dynamics, wind, actuator=pkg.ActuatorModel(**M.FULL), sensor=pkg.SensorModel(**M.SENSOR), **kw)
    ora.enable_actuator(M.act(**M.FULL))
    ora.enable_sensor(M.sens(**M.SENSOR))
    _same_config(ora, M.sens_track_oracle("race", 1, M.SENSOR, True, **kw))
    env.step_count = sc0
    ora.envs["step_count"] = sc0
    np.testing.assert_allclose(env.reset_tensor().cpu().numpy(), ora.reset(), rtol=0, atol=1e-6)
    rng = np.random.default_rng(M.SENS_FREE["rng"])
    _stagger(env, rng, ora)
    ora.sens["history"] = _get_sens(env)["history"]      # the staggered counters reach behind the reset row: both sides find the same rows there
    lock = np.ones(n, bool)
    n_done = 0
    for rep in range(M.SENS_FREE["launches"]):
        acts = np.stack([rng.uniform(-1, 1, (n, 4)).astype(np.float32) for _ in range(K)])
        n_done += _lockstep(env, ora, acts, lock, f"{where} launch {rep}")[0]
        check_dw(env, ora, lock, False, True, f"{where} launch {rep}")
        check_act(env, ora, lock, False, True, f"{where} launch {rep}")
        _exact_state(env, ora, lock, f"{where} launch {rep}")
    assert n_done > 2 * n and env.step_count == sc0 + K * M.SENS_FREE["launches"]
    print(f"SENS {where}: {n_done} episodes compared, {int((~lock).sum())} drones dropped at a branch cut")
    env.close()


@pytest.mark.parametrize("n", M.SHAPES + M.LAUNCH_SHAPES)
def test_tile_shapes_match_oracle_and_shadow_lanes_store_nothing(n):
    """resample = 0, latency i mod 9 and a bias row per drone written by set_sensor, max_steps = 6, against the free-running oracle:
    14 single steps, then two launches of 20 in which every drone restarts.  dn_step_many refuses K > 1 unless num_envs % 4 == 0, so at
    n in {1, 63, 65, 191} the 40 steps of the launches are single steps too (asserted: the refusal is the documented one), and the
    launches fly at the nearest sizes the entry point takes, n in {4, 60, 68, 188}, each still one partial tile.  A wider fleet (n + 1
    drones; n + 4 where launches run) with the same ids and values flies beside it: the rows of drones 0 .. n - 1 are the same bits,
    so the lanes beyond n (and the [slot][4][N] stride) play no part.
    Measured on one MI355X, episodes compared at n = 1 / 63 / 65 / 191: 7 / 441 / 455 / 1337; at n = 4 / 60 / 68 / 188: 28 / 420 /
    476 / 1316; 0 drones dropped in all eight."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    kw = dict(max_steps=M.SHAPE["max_steps"], normalize_obs=False, seed=M.SHAPE["seed"], **NOISE)
    model = dict(M.SENSOR, resample=False)
    env, ora = _pair(tracks.circle(1, 4, 1), n, None, None, sensor=pkg.SensorModel(**model), **kw)
    ora.enable_sensor(M.sens(**model))
    _same_config(ora, M.shape_oracle(1))
    extra = 4 if n % 4 == 0 else 1
    big = pkg.DroneVecEnv(tracks.circle(1, 4, 1), n + extra, device=DEV, sensor=pkg.SensorModel(**model), **kw)
    r_env = env.reset_tensor().cpu().numpy()
    np.testing.assert_allclose(r_env, ora.reset(), rtol=0, atol=1e-6)
    assert np.array_equal(bits(big.reset_tensor().cpu().numpy()[:n]), bits(r_env))
    vals, vbig = M.shape_values(n), M.shape_values(n + extra)
    assert all(np.array_equal(vals[k], vbig[k][:n]) for k in vals)
    env.set_sensor(**{k: torch.from_numpy(v).to(DEV) for k, v in vals.items()})
    big.set_sensor(**{k: torch.from_numpy(v).to(DEV) for k, v in vbig.items()})
    for k, v in vals.items():
        ora.sens[k] = v
    rng = np.random.default_rng(M.SHAPE["rng"])
    lock = np.ones(n, bool)
    n_done = last_done = 0
    if n % 4:
        with pytest.raises(pkg._capi.DroneNavError, match="num_envs % 4 == 0"):
            env.rollout_tensor(torch.zeros((M.SHAPE["K"], n, 4), device=DEV))
    for li, (K, single) in enumerate(M.shape_plan(n)):
        acts = np.stack([actions_mixed(rng, n) for _ in range(K)])
        tag = f"n={n} launch {li} K={K}"
        done_n, outs = _lockstep(env, ora, acts, lock, tag, single)
        n_done += done_n
        last_done += int(lock[-1] and any(o[2][-1] for o in outs))
        wide = _launch(big, np.concatenate([acts, np.zeros((K, extra, 4), np.float32)], axis=1), single)
        for t, (a, b) in enumerate(zip(outs, wide)):
            dn = a[2].astype(bool)
            assert np.array_equal(bits(a[0]), bits(b[0][:n])) and np.array_equal(bits(a[1]), bits(b[1][:n])), f"{tag} t={t}"
            assert np.array_equal(a[2], b[2][:n]) and np.array_equal(bits(a[3]["terminal_obs"][dn]), bits(b[3]["terminal_obs"][:n][dn])), f"{tag} t={t}"
        got = _exact_state(env, ora, lock, tag)
        assert np.array_equal(got["latency"], vals["latency"]) and np.array_equal(bits(got["bias"]), bits(vals["bias"])), tag
        gb = _get_sens(big)
        kk = ora.envs["steps"].astype(np.int64)
        valid = (np.arange(9)[None, :] <= kk[:, None]) & lock[:, None]
        assert np.array_equal(bits(got["history"])[valid], bits(gb["history"][:n])[valid]), tag
    assert n_done >= 2 * n - 8 and last_done > 0, (n_done, last_done)      # ... an episode end on the last drone of the partial tile
    print(f"SENS shape n={n}: {n_done} episodes compared, {int((~lock).sum())} drones dropped at a branch cut")
    env.close()
    big.close()


def test_values_written_by_set_sensor_are_flown_as_the_oracle_flies_them():
    """resample = 0: random valid latency / bias / history written by set_sensor on staggered episodes (n = 1500), then four free-running
    launches of 20 steps with max_steps = 15: every drone starts more than one episode; d and b must read back unchanged.
    Measured on one MI355X: 7500 episodes compared, 0 drones dropped."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, K = M.SENS_SETV["n"], M.SENS_SETV["K"]
    model = dict(M.SENSOR, resample=False)
    kw = dict(max_steps=M.SENS_SETV["max_steps"], normalize_obs=False, seed=M.SENS_SETV["seed"])
    env, ora = _pair(tracks.circle(1, 4, 1), n, None, None, sensor=pkg.SensorModel(**model), **kw)
    ora.enable_sensor(M.sens(**model))
    _same_config(ora, M.setv_oracle(1))
    np.testing.assert_allclose(env.reset_tensor().cpu().numpy(), ora.reset(), rtol=0, atol=1e-6)
    rng = np.random.default_rng(M.SENS_SETV["rng"])
    steps, vals = M.setv_start(rng, n)
    st = env.get_state()
    st["steps"] = steps.astype(st["steps"].dtype)
    env.set_state(st)
    ora.envs["steps"] = steps
    env.set_sensor(**{k: torch.from_numpy(v).to(DEV) for k, v in vals.items()})
    for k, v in vals.items():
        ora.sens[k] = v
    lock = np.ones(n, bool)
    n_done = 0
    for rep in range(M.SENS_SETV["launches"]):
        acts = np.stack([actions_mixed(rng, n) for _ in range(K)])
        n_done += _lockstep(env, ora, acts, lock, f"set values launch {rep}")[0]
        got = _exact_state(env, ora, lock, f"set values launch {rep}")
        assert np.array_equal(got["latency"], vals["latency"]) and np.array_equal(bits(got["bias"]), bits(vals["bias"]))
    assert n_done > 4 * n - 40
    print(f"SENS set values: {n_done} episodes compared, {int((~lock).sum())} drones dropped at a branch cut")
    env.close()


def test_late_enable_and_second_enable_match_oracle():
    """dn_enable_sensor on an env that has flown 30 steps (dynamics + wind + actuator on, episodes running): undelayed, unbiased rows
    until each drone's next episode start, the drawn values afterwards; then a second enable with latency [2, 5] and doubled
    amplitudes, which keeps d, b and the history.  Free-running against an oracle treated the same way.
    Measured on one MI355X: 3000 episodes compared, 0 drones dropped."""
    pkg = _pkg()
    from drl_dronenavigation_amd import _capi, tracks
    R = M.REENABLE
    n, K = R["n"], R["K"]
    dynamics, wind = _features(pkg, True, True)
    kw = dict(max_steps=R["max_steps"], normalize_obs=False, seed=R["seed"], **NOISE)
    env, ora = _pair(tracks.circle(1, 4, 1), n, dynamics, wind, actuator=pkg.ActuatorModel(**M.FULL), **kw)
    ora.enable_actuator(M.act(**M.FULL))
    _same_config(ora, M.reenable_oracle(1))
    np.testing.assert_allclose(env.reset_tensor().cpu().numpy(), ora.reset(), rtol=0, atol=1e-6)
    rng = np.random.default_rng(R["rng"])
    lock = np.ones(n, bool)
    lib = _capi.load()
    n_done = _lockstep(env, ora, np.stack([actions_mixed(rng, n) for _ in range(R["pre"])]), lock, "before the enable")[0]

    def enable(model_kw):
        model = pkg.SensorModel(**model_kw)
        _capi.check(lib.dn_enable_sensor(env._handle, C.byref(model.to_c())))
        env.sensor = model
        ora.enable_sensor(M.sens(**model_kw))
        assert bytes(env.sensor_config().to_c()) == bytes(model.to_c())

    enable(M.SENSOR)
    assert env.kernel_waves(fused=True) == env.kernel_waves(fused=False) == 1
    first = _get_sens(env)
    assert not first["latency"].any() and not first["bias"].any()
    started = np.zeros(n, bool)
    for rep in range(R["launches"]):
        done_n, outs = _lockstep(env, ora, np.stack([actions_mixed(rng, n) for _ in range(K)]), lock, f"late enable launch {rep}")
        n_done += done_n
        for o in outs:
            started |= o[2].astype(bool)
        got = _exact_state(env, ora, lock, f"late enable launch {rep}")
        assert not got["latency"][~started].any() and not got["bias"][~started].any()      # d = 0, b = 0 until the next episode start
    assert started.sum() > n // 2 and set(np.unique(got["latency"]).tolist()) == set(range(9))
    before = _get_sens(env)
    enable(R["second"])
    after = _get_sens(env)
    kk = env.get_state()["steps"].astype(np.int64)
    valid = np.arange(9)[None, :] <= kk[:, None]
    assert np.array_equal(after["latency"], before["latency"]) and np.array_equal(bits(after["bias"]), bits(before["bias"]))
    assert np.array_equal(bits(after["history"])[valid], bits(before["history"])[valid])
    for rep in range(R["launches"]):
        n_done += _lockstep(env, ora, np.stack([actions_mixed(rng, n) for _ in range(K)]), lock, f"second enable launch {rep}")[0]
        got = _exact_state(env, ora, lock, f"second enable launch {rep}")
    assert n_done > 2 * n and {2, 3, 4, 5} <= set(np.unique(got["latency"]).tolist())
    print(f"SENS late + second enable: {n_done} episodes compared, {int((~lock).sum())} drones dropped at a branch cut")
    env.close()
