"""Per-drone dynamics randomisation and wind (dn_enable_dynamics / dn_enable_wind) on the HIP path against the CPU oracle
(oracle/dn_oracle.c orc_vec_step_dw, itself pinned by tests/test_oracle_dynamics_wind.py): every kernel instantiation of the two
families, the run-time options inside them, and free-running fused launches through many in-launch episode starts.

a. Every instantiation: both families are dn_step_many_1w_kernel<R, NORM, NOISE, ONE, XOPT = true, SAMPLE = false, M = DN_M_DYN | DN_M_WIND>
   (dn_launch_step_many, launch_models), one test ID per cell:

       test ID cell [family-dtype-norm-noise-mode]   R       NORM   NOISE  ONE    WIND   dynamics scales
       dyn-f64-norm0-noise0-step / -rollout           double  false  false  true / false  false  on
       dyn-f64-norm0-noise1-step / -rollout           double  false  true   true / false  false  on
       dyn-f64-norm1-noise0-step / -rollout           double  true   false  true / false  false  on
       dyn-f64-norm1-noise1-step / -rollout           double  true   true   true / false  false  on
       dyn-f32-norm0-noise0-step / -rollout           float   false  false  true / false  false  on
       dyn-f32-norm0-noise1-step / -rollout           float   false  true   true / false  false  on
       dyn-f32-norm1-noise0-step / -rollout           float   true   false  true / false  false  on
       dyn-f32-norm1-noise1-step / -rollout           float   true   true   true / false  false  on
       wind-f64-norm0-noise0-step / -rollout          double  false  false  true / false  true   off (null scale pointer)
       wind-f64-norm0-noise1-step / -rollout          double  false  true   true / false  true   off (null scale pointer)
       wind-f64-norm1-noise0-step / -rollout          double  true   false  true / false  true   on
       wind-f64-norm1-noise1-step / -rollout          double  true   true   true / false  true   on
       wind-f32-norm0-noise0-step / -rollout          float   false  false  true / false  true   off (null scale pointer)
       wind-f32-norm0-noise1-step / -rollout          float   false  true   true / false  true   off (null scale pointer)
       wind-f32-norm1-noise0-step / -rollout          float   true   false  true / false  true   on
       wind-f32-norm1-noise1-step / -rollout          float   true   true   true / false  true   on

   step = step_tensor (ONE = true), rollout = rollout_tensor with K = 5 (ONE = false).  n = 1000 (a ragged last tile), 150 steps on a
   short circle with max_steps = 40, noise = obs 0.01 / act 0.001.  The oracle is loaded with the device's state, scales and wind
   before every step (step) or every launch (rollout: the oracle runs the launch's 5 steps on its own, float32 state like the
   registers).  Outputs: float64 compute at compare_step's 1e-5 bars (rollout: rewards 1e-4, a free-running distance may differ by an
   ulp, as in test_free_running_vs_f32_state_oracle); float32 compute at test_float32_compute_mode_tolerance's 5e-4 on the observations
   with at most 1e-4 of the done flags flipped.  Post-step scales and steady wind (redraws included, float64 draws in either dtype):
   <= 1 float32 ulp; the gust <= 1 ulp and >= 99.9 % bit-equal in float64 compute.  In float32 compute the gust's step runs in
   R = float (a and b cast to float): measured on one MI355X, its distance from the float64 definition is at most 3.97e-7 sigma
   after one step and 1.19e-6 sigma after a 5-step launch; the bars GUST_F32_STEP = 8e-7 and GUST_F32_LAUNCH = 2.5e-6 sigma hold it
   with about 2x margin.  With the normaliser on, the float32 observation bar is 5e-4 divided by the column's running std (where
   that is below 1): the normaliser scales an arithmetic difference by 1 / std.  The drones' episode step counters start spread
   over [0, 40), so that in every wave some lanes start an episode (redraw) while others fly on.
b. The option matrix of test_physics_options_match_oracle with both features on (mass 0.7-1.3, the gusts of model_support.GUSTY),
   plus random spawn, the reward wrappers, zero damping and include_distance = False, and a few cells with one feature alone.
c. Free-running fused launches, K = 64, n = 4096, 256 steps, with the lockstep discipline of
   test_baseline_full_size_fused_launch_matches_oracle: once with env_id_offset = 2^33 + 12345, once with the step counter just
   below 2^32 so that the draws cross the word boundary.
"""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gpu_support import DEV, _features, _pair, _stagger, check_dw, load_dw  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402
from model_support import NOISE, _step_mismatch, actions_mixed, compare_step  # noqa: E402


# ---- a. every instantiation ----------------------------------------------------------------------------------------------
CELLS = [(fam, dt, norm, noise, mode) for fam in ("dyn", "wind") for dt in ("f64", "f32") for norm in (0, 1) for noise in (0, 1)
         for mode in ("step", "rollout")]


@pytest.mark.parametrize("fam,dt,norm,noise,mode", CELLS, ids=[f"{f}-{d}-norm{a}-noise{b}-{m}" for f, d, a, b, m in CELLS])
def test_every_instantiation_matches_oracle(fam, dt, norm, noise, mode):
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, T, K = 1000, 150, (1 if mode == "step" else 5)
    f32 = dt == "f32"
    dynamics, wind = _features(pkg, fam == "dyn" or bool(norm), fam == "wind")
    kw = dict(max_steps=40, normalize_obs=bool(norm), seed=1000 + len(fam) * 16 + norm * 4 + noise * 2 + f32,
              compute_dtype="float32" if f32 else "float64", **(NOISE if noise else {}))
    env, ora = _pair(tracks.circle(1, 4, 1), n, dynamics, wind, **kw)
    assert env.kernel_waves(fused=True) == env.kernel_waves(fused=False) == 1
    env.reset_tensor()
    ora.reset()
    rng = np.random.default_rng(7)
    _stagger(env, rng)
    dev = torch.device(DEV)
    n_done = flips = 0
    worst = 0.0
    for launch in range(T // K):
        load_dw(env, ora)
        acts = np.stack([actions_mixed(rng, n) for _ in range(K)])
        if mode == "step":
            outs = [env.step_tensor(torch.from_numpy(acts[0]).to(dev))]
        else:
            r = env.rollout_tensor(torch.from_numpy(acts).to(dev), want_terminal=True)
            outs = [(r["obs"][t], r["reward"][t], r["done"][t],
                     dict(truncated=r["truncated"][t], found_targets=r["found_targets"][t], terminal_obs=r["terminal_obs"][t],
                          ep_length=r["ep_length"][t], ep_return=r["ep_return"][t])) for t in range(K)]
        torch.cuda.synchronize()
        agree = np.ones(n, bool)
        for t, out in enumerate(outs):
            ref = ora.step(acts[t])
            tag = f"{fam}/{dt}/norm{norm}/noise{noise}/{mode} launch {launch} t={t}"
            if f32:
                same = out[2].cpu().numpy() == ref["done"]
                flips += int((~same).sum())
                agree &= same
                # the normaliser divides a float32-arithmetic difference by the running std of its column: the bar follows it
                bar = 5e-4 / np.sqrt(np.minimum(ora.envs["rms_var"], 1.0)) if norm else 5e-4
                err = np.abs(out[0].cpu().numpy().astype(np.float64) - ref["obs"]) - bar
                assert (err[same] <= 0).all(), f"{tag}: obs off the 5e-4 bar by {err[same].max():.3e}"
                n_done += int(ref["done"].sum())
            else:
                n_done += compare_step(out, ref, tag, rew_atol=1e-5 if mode == "step" else 1e-4)
        worst = max(worst, check_dw(env, ora, agree, f32, mode == "rollout", f"{fam}/{dt}/norm{norm}/noise{noise}/{mode} launch {launch}"))
    assert n_done > n                                           # episodes ended and redrew (inside launches in the rollout cells)
    assert flips <= n * T * 1e-4, f"{flips} done flags differ"
    print(f"{fam}/{dt}/norm{norm}/noise{noise}/{mode}: {n_done} episodes, gust max {worst:.3e} sigma, {flips} flags flipped")
    env.close()


# ---- b. run-time options with the features on ------------------------------------------------------------------------------
OPTION_PAIRS = [("pyb_gnd", "thrust"), ("pyb_drag", "thrust"), ("pyb_gnd_drag_dw", "thrust"), ("pyb_gnd_drag_dw", "rpm"), ("pyb", "rpm"),
                ("pyb_dw", "thrust"), ("pyb", "pid"), ("pyb", "vel"), ("pyb_drag", "one_d_rpm"), ("pyb", "one_d_pid"),
                ("pyb_gnd_drag_dw", "pid")]
OPTION_CELLS = ([(p, a, {}, "both") for p, a in OPTION_PAIRS]
                + [("pyb", "thrust", dict(random_spawn=True), "both"), ("pyb", "thrust", dict(clip_rew=True, norm_rew=True), "both"),
                   ("pyb_drag", "thrust", dict(zero_damping=True), "both"), ("pyb", "thrust", dict(include_distance=False), "both"),
                   ("pyb_gnd_drag_dw", "thrust", {}, "dyn"), ("pyb_gnd_drag_dw", "pid", {}, "dyn"), ("pyb_drag", "rpm", {}, "wind"),
                   ("pyb_gnd", "vel", {}, "wind"), ("pyb", "thrust", dict(random_spawn=True), "dyn")])


@pytest.mark.parametrize("physics,act,extra,feat", OPTION_CELLS,
                         ids=[f"{p}-{a}-{'-'.join(e) or 'plain'}-{f}" for p, a, e, f in OPTION_CELLS])
def test_options_with_dynamics_and_wind_match_oracle(physics, act, extra, feat):
    """Teacher-forced, 100 steps at 1024 drones: the physics x action-type pairs of test_physics_options_match_oracle (low spawn,
    ground contact off: the clipped ground effect acts) with the body scales and the wind on, then random spawn (circle6), the
    reward wrappers, zero damping and include_distance = False; `feat` names the features on.  compare_step's 1e-5 bars."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, T = 1024, 100
    dynamics, wind = _features(pkg, feat in ("both", "dyn"), feat in ("both", "wind"))
    kw = dict(max_steps=60, normalize_obs=False, seed=31, **extra)
    if extra.get("random_spawn"):
        track = tracks.REGISTRY["circle6"]()              # distinct gates: every line has a length
        wp, spawn, dim, circle = track.targets(), track.initial_xyzs, track.aviary_dim, track.is_circle
        kw.update(max_steps=25, cylinder=False)
    else:
        wp, spawn, dim, circle = (np.array([[0.0, 1.0, 0.4], [-1.0, 0.0, 0.8], [0.0, -1.0, 0.4]]), np.array([[1.0, 0.0, 0.05]]),
                                  np.array([-2.0, -2.0, 0.0, 2.0, 2.0, 2.0]), False)
        kw.update(ground_contact=False, cylinder=False, normalize_actions=act == "thrust")
    env = pkg.DroneVecEnv(None, n, target_points=wp, initial_xyzs=spawn, aviary_dim=dim, circle=circle, device=DEV, physics=physics,
                          act=act, dynamics=dynamics, wind=wind, **kw)
    assert env.kernel_waves(fused=True) == env.kernel_waves(fused=False) == 1
    cfg = O.make_config(wp, np.asarray(spawn).ravel()[:3], dim, circle=circle, f32_state=True, physics=pkg.vec_env.PHYSICS[physics],
                        action_type=pkg.vec_env.ACTION_TYPES[act], **kw)
    ora = O.OracleVecEnv(cfg, n, threads=8, dynamics=dynamics, wind=wind)
    env.reset_tensor()
    ora.reset()
    check_dw(env, ora, np.ones(n, bool), False, False, "reset")
    rng = np.random.default_rng(5)
    dev = torch.device(DEV)
    n_done = 0
    for t in range(T):
        load_dw(env, ora)
        a = actions_mixed(rng, n) if act == "thrust" else rng.uniform(-1, 1, (n, 4)).astype(np.float32)
        out = env.step_tensor(torch.from_numpy(a).to(dev))
        torch.cuda.synchronize()
        n_done += compare_step(out, ora.step(a), f"{physics}/{act}/{extra}/{feat} t={t}")
        check_dw(env, ora, np.ones(n, bool), False, False, f"{physics}/{act}/{extra}/{feat} t={t}")
    assert n_done > n // 2
    env.close()


# ---- c. free-running fused launches -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["gid-past-2^33", "step-across-2^32"])
def test_free_running_fused_launches_match_oracle(where):
    """K = 64 steps per dn_step_many, 4096 drones, 256 steps of U(-1, 1) actions on the race track with max_steps = 100 (crashes and
    time limits, the step counters spread): every drone starts several episodes inside launches, each redrawing its body and wind.  Both sides keep their own float32 state; a drone may
    leave the lockstep comparison ONLY at an atan2 branch cut (its raw roll or yaw column within 1e-5 of +-1, or the pitch column
    within 1e-2 of +-1/2), at most 8 of them (test_baseline_full_size_fused_launch_matches_oracle's discipline).  Scales and wind
    of the drones in lockstep after every launch: <= 1 float32 ulp, the gust >= 99.9 % bit-equal."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, K, launches = 4096, 64, 4
    dynamics, wind = _features(pkg, True, True)
    off, sc0 = ((1 << 33) + 12345, 0) if where == "gid-past-2^33" else (0, (1 << 32) - 100)
    env, ora = _pair(tracks.reaching(), n, dynamics, wind, max_steps=100, normalize_obs=False, seed=0xD1CE, env_id_offset=off)
    env.step_count = sc0
    ora.envs["step_count"] = sc0
    np.testing.assert_allclose(env.reset_tensor().cpu().numpy(), ora.reset(), rtol=0, atol=1e-6)
    check_dw(env, ora, np.ones(n, bool), False, False, "reset")
    rng = np.random.default_rng(64)
    _stagger(env, rng, ora)
    dev = torch.device(DEV)
    lock = np.ones(n, bool)
    n_done = 0
    for rep in range(launches):
        acts = np.stack([rng.uniform(-1, 1, (n, 4)).astype(np.float32) for _ in range(K)])
        out = env.rollout_tensor(torch.from_numpy(acts).to(dev), want_terminal=True)
        torch.cuda.synchronize()
        for t in range(K):
            info = dict(truncated=out["truncated"][t], found_targets=out["found_targets"][t], terminal_obs=out["terminal_obs"][t],
                        ep_length=out["ep_length"][t], ep_return=out["ep_return"][t])
            ref = ora.step(acts[t])
            bad = _step_mismatch((out["obs"][t], out["reward"][t], out["done"][t], info), ref, obs_atol=1e-4, rew_atol=2e-4)
            first = bad & lock
            if first.any():
                row = np.where(ref["done"].astype(bool)[:, None], ref["terminal_obs"], ref["obs"])[first].astype(np.float64)
                at_cut = (np.abs(np.abs(row[:, 3]) - 1.0) <= 1e-5) | (np.abs(np.abs(row[:, 5]) - 1.0) <= 1e-5) | \
                         (np.abs(np.abs(row[:, 4]) - 0.5) <= 1e-2)
                assert at_cut.all(), (f"{where} launch {rep} t={t}: drones {np.flatnonzero(first)[~at_cut][:8]} left lockstep away "
                                      f"from an atan2 branch cut (raw roll / pitch / yaw columns {row[~at_cut][:4, 3:6]})")
            lock &= ~bad
            assert (~lock).sum() <= 8, f"{where} launch {rep} t={t}: {int((~lock).sum())} drones out of lockstep"
            n_done += int((ref["done"].astype(bool) & lock).sum())
        check_dw(env, ora, lock, False, True, f"{where} launch {rep}")
    assert n_done > 2 * n
    assert env.step_count == sc0 + K * launches
    print(f"{where}: {n_done} episodes compared, {int((~lock).sum())} drones dropped at a branch cut")
    env.close()
