"""The per-drone actuator model (dn_enable_actuator: command latency + motor lag) on the HIP path against the CPU oracle
(oracle/dn_oracle.c orc_vec_step_act, written from include/dronenav.h and itself pinned by tests/test_oracle_actuator.py).  The
configurations, seeds and action streams live in tests/model_support.py; tests/test_oracle_actuator.py shows on the oracle alone that they reach the
cases claimed here (episode ends, fills, latencies 0 and 8, history entries consumed across a launch boundary, restarts inside a
launch, the ground effect acting); every test here first checks that its oracle has that file's configuration, byte for byte.

a. All 16 instantiations of dn_step_many_1w_kernel<R, NORM, NOISE, ONE, ..., M = DN_M_ACT> with latency [0, 8] AND lag
   (motor_tau [0.02, 0.15]) on together, dynamics + wind riding in the norm cells; the oracle is loaded with the device's state,
   scales, wind and actuator state before every step (step) or 5-step launch (rollout).  Outputs at the bars of
   tests/test_gpu_dynamics_wind_oracle.py.  Actuator state afterwards: latency and history exact, coeff <= 1 float32 ulp (device exp
   against libm, as test_gpu_actuator.test_draws_follow_their_definition), rpm in float64 compute <= 1 ulp and >= 99.9 % bit-equal,
   in float32 compute within LAG_F32_STEP (one step) / LAG_F32_LAUNCH (5-step launch) of RPM_SPAN.
b. The run-time options with the lag on (THRUST) and latency alone for every other action type, teacher-forced.
c. Free-running fused launches of 64 steps with drone ids past 2^33 / the step counter crossing 2^32.
d. Short launches (K around the history's depth, interleaved) and an env whose actuator state was written by set_actuator.
"""
import numpy as np
import pytest

import model_support as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gpu_support import (DEV, _features, _get_act, _pair, _rollout_outs, _same_config, _stagger, check_act, check_dw,  # noqa: E402
                         load_act)
from gpu_support import pkg as _pkg  # noqa: E402
from model_support import (LAG_F32_BOUND, LAG_F32_LAUNCH, LAG_F32_LAUNCH_BOUND, LAG_F32_STEP, NOISE, _step_mismatch,  # noqa: E402
                           actions_mixed, compare_step)


# ---- a. every instantiation, latency and lag together ------------------------------------------------------------------------
@pytest.mark.parametrize("dt,norm,noise,mode", M.INST_CELLS, ids=[f"{d}-norm{a}-noise{b}-{m}" for d, a, b, m in M.INST_CELLS])
def test_every_instantiation_with_latency_and_lag_matches_oracle(dt, norm, noise, mode, monkeypatch):
    """n = 1000, 150 steps, max_steps = 40, staggered step counters.  Measured on one MI355X (3661 episodes per cell): float64
    compute, rpm bit-equal to the oracle in 100 % of the compared values in all eight cells (0 ulp); float32 compute, max
    |rpm - oracle| = 1.597e-7 RPM_SPAN after a teacher-forced step in all four step cells (bar LAG_F32_STEP = 3.0e-7) and 3.994e-7 /
    4.792e-7 / 4.792e-7 / 3.994e-7 after a 5-step launch in the four rollout cells (bar LAG_F32_LAUNCH = 1.0e-6, about 2x the
    largest, a priori 2.15e-6); no done flag flipped."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, T, K = M.INST["n"], M.INST["T"], (1 if mode == "step" else M.INST["K"])
    f32 = dt == "f32"
    if norm and noise and not f32:
        # The default observation-noise draws use the hardware's float32 transcendentals, within 1.2e-6 of the float64 definition
        # (dronenav.h, dn_get_kernel_waves): the noise term moves by up to 0.01 x 1.2e-6 = 1.2e-8, which flips the float32 sum
        # obs + noise by one ulp (1.19e-7 in [1, 2)) in a fair share of the draws.  A lagged drone fed hover commands holds its
        # spawn point (1, 0, 1) +- millimetres, so the running std of its x and z columns is the noise's 0.01 and the normaliser turns
        # that one ulp into 1.19e-7 / 0.01 = 1.2e-5: above compare_step's 1e-5 by the formats alone (seen with the default draws:
        # 6e-6 somewhere in every step where the column is below 1, 1.013e-5 in one value of 1.95 million where it is above).
        # DN_EXACT_OBS_NOISE=1 is the switch the header offers for comparisons with a CPU evaluation: the same kernel, the draws
        # in the float64 form (a run-time flag).  The float32 cells scale their bar by the std and keep the default draws.
        monkeypatch.setenv("DN_EXACT_OBS_NOISE", "1")
    dynamics, wind = _features(pkg, bool(norm), bool(norm))
    kw = dict(max_steps=M.INST["max_steps"], normalize_obs=bool(norm), seed=M.act_inst_seed(dt, norm, noise),
              compute_dtype="float32" if f32 else "float64", actuator=pkg.ActuatorModel(**M.FULL), **(NOISE if noise else {}))
    env, ora = _pair(tracks.circle(1, 4, 1), n, dynamics, wind, **kw)
    ora.enable_actuator(M.act(**M.FULL))
    _same_config(ora, M.act_inst_oracle(dt, norm, noise))
    assert env.kernel_waves(fused=True) == env.kernel_waves(fused=False) == 1
    assert LAG_F32_LAUNCH <= LAG_F32_LAUNCH_BOUND and LAG_F32_STEP <= LAG_F32_BOUND
    env.reset_tensor()
    ora.reset()
    check_act(env, ora, np.ones(n, bool), False, False, "reset")
    rng = np.random.default_rng(M.INST["rng"])
    _stagger(env, rng)
    dev = torch.device(DEV)
    n_done = flips = 0
    stats = {}
    tag0 = f"{dt}/norm{norm}/noise{noise}/{mode}"
    for launch in range(T // K):
        load_act(env, ora)
        acts = np.stack([actions_mixed(rng, n) for _ in range(K)])
        if mode == "step":
            outs = [env.step_tensor(torch.from_numpy(acts[0]).to(dev))]
        else:
            outs = _rollout_outs(env.rollout_tensor(torch.from_numpy(acts).to(dev), want_terminal=True), K)
        torch.cuda.synchronize()
        agree = np.ones(n, bool)
        for t, out in enumerate(outs):
            ref = ora.step(acts[t])
            tag = f"{tag0} launch {launch} t={t}"
            if f32:
                same = out[2].cpu().numpy() == ref["done"]
                flips += int((~same).sum())
                agree &= same
                bar = 5e-4 / np.sqrt(np.minimum(ora.envs["rms_var"], 1.0)) if norm else 5e-4
                err = np.abs(out[0].cpu().numpy().astype(np.float64) - ref["obs"]) - bar
                assert (err[same] <= 0).all(), f"{tag}: obs off the 5e-4 bar by {err[same].max():.3e}"
                n_done += int(ref["done"].sum())
            else:
                n_done += compare_step(out, ref, tag, rew_atol=1e-5 if mode == "step" else 1e-4)
        check_dw(env, ora, agree, f32, mode == "rollout", f"{tag0} launch {launch}")
        check_act(env, ora, agree, f32, mode == "rollout", f"{tag0} launch {launch}", stats)
    assert n_done > n
    assert flips <= n * T * 1e-4, f"{flips} done flags differ"
    print(f"ACT {tag0}: {n_done} episodes, rpm max {stats['dist']:.3e} span from the oracle, {stats['eq']:.5f} bit-equal, {flips} flags flipped")
    env.close()


# ---- b. options -------------------------------------------------------------------------------------------------------------
OPTION_CELLS = ([(p, "thrust", na, e, f) for p, na, e, f in M.LAG_OPTION_CELLS] + [(p, a, False, {}, "both") for p, a in M.LAT_OPTION_CELLS])


@pytest.mark.parametrize("physics,act,normalized,extra,feat", OPTION_CELLS,
                         ids=[f"{p}-{a}-{'norm' if na else 'raw'}-{'-'.join(e) or 'plain'}-{f}" for p, a, na, e, f in OPTION_CELLS])
def test_options_with_the_actuator_match_oracle(physics, act, normalized, extra, feat):
    """Teacher-forced, 100 steps at 1024 drones, low spawn with ground contact off (the clipped ground effect acts), compare_step's
    1e-5.  THRUST cells: latency [0, 8] + lag [0.02, 0.15] s (the lagged speeds feed the ground effect, PYB_DRAG's last_rpm, s_kf,
    s_km), normalised and raw actions.  Other action types: latency [0, 8] alone -- the delayed command goes through HOVER_RPM (1 +
    0.05 a) or the PID loop, whose integrals and last attitude the teacher forcing carries along."""
    pkg = _pkg()
    n, T = M.ACT_OPT["n"], M.ACT_OPT["T"]
    wp, spawn, dim, circle, kw, model = M.option_setup(physics, act, normalized, extra)
    dynamics, wind = _features(pkg, feat == "both", feat == "both")
    env = pkg.DroneVecEnv(None, n, target_points=wp, initial_xyzs=spawn, aviary_dim=dim, circle=circle, device=DEV, physics=physics,
                          act=act, dynamics=dynamics, wind=wind, actuator=pkg.ActuatorModel(**model), **kw)
    assert env.kernel_waves(fused=True) == env.kernel_waves(fused=False) == 1
    assert pkg.vec_env.PHYSICS == M.PHYSICS and pkg.vec_env.ACTION_TYPES == M.ACTION_TYPES
    cfg = O.make_config(wp, spawn.ravel(), dim, circle=circle, f32_state=True, physics=M.PHYSICS[physics], action_type=M.ACTION_TYPES[act], **kw)
    assert bool(cfg.ground_contact) == env.ground_contact
    ora = O.OracleVecEnv(cfg, n, threads=8, dynamics=dynamics, wind=wind, actuator=M.act(**model))
    ora.dw_cfg = O.make_dw_config(dynamics, wind)
    env.reset_tensor()
    ora.reset()
    check_act(env, ora, np.ones(n, bool), False, False, "reset")
    rng = np.random.default_rng(M.ACT_OPT["rng"])
    dev = torch.device(DEV)
    n_done = 0
    every = np.ones(n, bool)
    tag0 = f"{physics}/{act}/{'norm' if normalized else 'raw'}/{extra}/{feat}"
    for t in range(T):
        load_act(env, ora)
        a = M.option_actions(rng, n, act, normalized)
        out = env.step_tensor(torch.from_numpy(a).to(dev))
        torch.cuda.synchronize()
        n_done += compare_step(out, ora.step(a), f"{tag0} t={t}")
        check_dw(env, ora, every, False, False, f"{tag0} t={t}")
        check_act(env, ora, every, False, False, f"{tag0} t={t}")
    assert n_done > n // 2
    env.close()


# ---- c. / d. free-running launches -----------------------------------------------------------------------------------------------
def _lockstep_launch(env, ora, acts, lock, tag):
    """One fused launch against the free-running oracle with the discipline of test_free_running_fused_launches_match_oracle: a drone
    may leave ONLY at an atan2 branch cut, at most 8 of them.  Returns the number of episodes compared."""
    K = len(acts)
    out = env.rollout_tensor(torch.from_numpy(acts).to(torch.device(DEV)), want_terminal=True)
    torch.cuda.synchronize()
    n_done = 0
    for t, o in enumerate(_rollout_outs(out, K)):
        ref = ora.step(acts[t])
        bad = _step_mismatch(o, ref, obs_atol=1e-4, rew_atol=2e-4)
        first = bad & lock
        if first.any():
            row = np.where(ref["done"].astype(bool)[:, None], ref["terminal_obs"], ref["obs"])[first].astype(np.float64)
            at_cut = (np.abs(np.abs(row[:, 3]) - 1.0) <= 1e-5) | (np.abs(np.abs(row[:, 5]) - 1.0) <= 1e-5) | \
                     (np.abs(np.abs(row[:, 4]) - 0.5) <= 1e-2)
            assert at_cut.all(), (f"{tag} t={t}: drones {np.flatnonzero(first)[~at_cut][:8]} left lockstep away from an atan2 branch "
                                  f"cut (raw roll / pitch / yaw columns {row[~at_cut][:4, 3:6]})")
        lock &= ~bad
        assert (~lock).sum() <= 8, f"{tag} t={t}: {int((~lock).sum())} drones out of lockstep"
        n_done += int((ref["done"].astype(bool) & lock).sum())
    return n_done


@pytest.mark.parametrize("where", list(M.FREE_WHERE))
def test_free_running_fused_launches_with_the_actuator_match_oracle(where):
    """K = 64, 4096 drones, 256 steps of U(-1, 1) commands on the race track, max_steps = 100, dynamics + wind + latency + lag; both
    sides keep their own state.  Actuator state of the drones in lockstep after every launch at (a)'s float64 bars."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, K = M.ACT_FREE["n"], M.ACT_FREE["K"]
    off, sc0 = M.FREE_WHERE[where]
    dynamics, wind = _features(pkg, True, True)
    env, ora = _pair(tracks.reaching(), n, dynamics, wind, max_steps=M.ACT_FREE["max_steps"], normalize_obs=False, seed=M.ACT_FREE["seed"],
                     env_id_offset=off, actuator=pkg.ActuatorModel(**M.FULL))
    ora.enable_actuator(M.act(**M.FULL))
    _same_config(ora, M.act_track_oracle("race", 1, M.FULL, True, max_steps=M.ACT_FREE["max_steps"], normalize_obs=False,
                                       seed=M.ACT_FREE["seed"], env_id_offset=off))
    env.step_count = sc0
    ora.envs["step_count"] = sc0
    np.testing.assert_allclose(env.reset_tensor().cpu().numpy(), ora.reset(), rtol=0, atol=1e-6)
    check_act(env, ora, np.ones(n, bool), False, False, "reset")
    rng = np.random.default_rng(M.ACT_FREE["rng"])
    _stagger(env, rng, ora)
    lock = np.ones(n, bool)
    n_done = 0
    stats = {}
    for rep in range(M.ACT_FREE["launches"]):
        acts = np.stack([rng.uniform(-1, 1, (n, 4)).astype(np.float32) for _ in range(K)])
        n_done += _lockstep_launch(env, ora, acts, lock, f"{where} launch {rep}")
        check_dw(env, ora, lock, False, True, f"{where} launch {rep}")
        check_act(env, ora, lock, False, True, f"{where} launch {rep}", stats)
    assert n_done > 2 * n and env.step_count == sc0 + K * M.ACT_FREE["launches"]
    print(f"ACT {where}: {n_done} episodes compared, {int((~lock).sum())} drones dropped at a branch cut, rpm {stats['eq']:.5f} bit-equal")
    env.close()


def test_short_launches_around_the_history_depth_match_oracle():
    """Free-running float64, K in {1, 3, 7, 8, 9} interleaved in one run (the end-of-launch history shift sees K below, at and above
    its depth, each after each), half the drones held at latency 8 by set_actuator before every launch."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n = M.SHORT["n"]
    dynamics, wind = _features(pkg, True, True)
    kw = dict(max_steps=M.SHORT["max_steps"], normalize_obs=False, seed=M.SHORT["seed"])
    env, ora = _pair(tracks.circle(1, 4, 1), n, dynamics, wind, actuator=pkg.ActuatorModel(**M.FULL), **kw)
    ora.enable_actuator(M.act(**M.FULL))
    _same_config(ora, M.act_track_oracle("circle4", 1, M.FULL, True, **kw))
    np.testing.assert_allclose(env.reset_tensor().cpu().numpy(), ora.reset(), rtol=0, atol=1e-6)
    rng = np.random.default_rng(M.SHORT["rng"])
    st = env.get_state()
    st["steps"] = rng.integers(0, M.SHORT["max_steps"], n).astype(st["steps"].dtype)
    env.set_state(st)
    ora.envs["steps"] = st["steps"]
    lock = np.ones(n, bool)
    n_done = 0
    for li, K in enumerate(M.SHORT["Ks"]):
        lat = env.get_actuator()["latency"].clone()
        lat[: n // 2] = 8
        env.set_actuator(latency=lat)
        ora.act["latency"][: n // 2] = 8
        acts = np.stack([actions_mixed(rng, n) for _ in range(K)])
        n_done += _lockstep_launch(env, ora, acts, lock, f"short launch {li} K={K}")
        check_act(env, ora, lock, False, True, f"short launch {li} K={K}")
    assert n_done > n
    env.close()


def test_values_written_by_set_actuator_are_flown_as_the_oracle_flies_them():
    """resample = False: latency, coeff, rpm and history written by set_actuator (random valid values, every latency 0..8), then four
    free-running launches of 20 steps with max_steps = 15: every drone starts more than one episode; d and a must hold."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, K = M.ACT_SETV["n"], M.ACT_SETV["K"]
    model = dict(M.FULL, resample=False)
    kw = dict(max_steps=M.ACT_SETV["max_steps"], normalize_obs=False, seed=M.ACT_SETV["seed"])
    env, ora = _pair(tracks.circle(1, 4, 1), n, None, None, actuator=pkg.ActuatorModel(**model), **kw)
    ora.enable_actuator(M.act(**model))
    _same_config(ora, M.act_track_oracle("circle4", 1, model, False, **kw))
    np.testing.assert_allclose(env.reset_tensor().cpu().numpy(), ora.reset(), rtol=0, atol=1e-6)
    rng = np.random.default_rng(M.ACT_SETV["rng"])
    vals = M.short_set_values(rng, n)
    env.set_actuator(**{k: torch.from_numpy(v).to(DEV) for k, v in vals.items()})
    for k, v in vals.items():
        ora.act[k] = v
    lock = np.ones(n, bool)
    n_done = 0
    for rep in range(M.ACT_SETV["launches"]):
        acts = np.stack([actions_mixed(rng, n) for _ in range(K)])
        n_done += _lockstep_launch(env, ora, acts, lock, f"set values launch {rep}")
        check_act(env, ora, lock, False, True, f"set values launch {rep}")
        got = _get_act(env)
        assert np.array_equal(got["latency"], vals["latency"]) and np.array_equal(got["coeff"], vals["coeff"])
    assert n_done > 2 * n - 16
    env.close()
