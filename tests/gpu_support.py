"""What the GPU tests share and what needs torch and the package: the package loader, env builders, bit-for-bit comparisons of envs,
and the loaders / checkers that hold the device's per-drone model state against the CPU oracle's.  A plain module like
tests/rigid_body_ref.py -- pytest does not collect it and does not rewrite its asserts, so every assert here carries its own message.
What needs numpy and the oracle alone is in tests/model_support.py."""
import numpy as np
import pytest
import torch

from model_support import (BODY, GUST_F32_LAUNCH, GUST_F32_STEP, GUSTY, LAG_F32_LAUNCH, LAG_F32_STEP, RPM_SPAN, STATE_KEYS, WIDE, _mixed,
                           bits, gpu_state_to_oracle, ulps)
from oracle import oracle as O

DEV = "cuda:0"


def pkg():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no CPU fallback")
    import drl_dronenavigation_amd as pkg
    return pkg


# ---- envs and bit-for-bit comparisons ----------------------------------------------------------------------------------------------
def _acts(rng, n, K):
    return torch.from_numpy(np.stack([_mixed(rng, n) for _ in range(K)])).to(DEV)


def _same_state(a, b):
    for k in STATE_KEYS:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k


def _same_wind(a, b):
    for j, (x, y) in enumerate(zip(a.get_wind(), b.get_wind())):
        assert torch.equal(x, y), ("mean", "gust")[j]


def _same_actuator(a, b):
    x, y = a.get_actuator(), b.get_actuator()
    for k in x:
        assert torch.equal(x[k], y[k]), k


def _same_sensor(a, b):
    x, y = a.get_sensor(), b.get_sensor()
    for k in x:
        assert torch.equal(x[k], y[k]), k


def _run_pair(envs, rng, n, launches=3, K=20):
    """Reset, one dn_step and `launches` fused launches of K steps on every env with the same actions: the outputs, bit for bit."""
    outs = [e.reset_tensor().clone() for e in envs]
    for i, o in enumerate(outs[1:]):
        assert torch.equal(outs[0], o), f"reset: env {i + 1} differs from env 0"
    a = torch.from_numpy(_mixed(rng, n)).to(DEV)
    res = [tuple(x.clone() for x in e.step_tensor(a)[:3]) for e in envs]
    for i, r in enumerate(res[1:]):
        for name, x, y in zip(("obs", "reward", "done"), res[0], r):
            assert torch.equal(x, y), f"single step: {name} of env {i + 1} differs from env 0"
    n_done = 0
    for launch in range(launches):
        acts = _acts(rng, n, K)
        rs = [{k: v.clone() for k, v in e.rollout_tensor(acts, want_terminal=True).items()} for e in envs]
        for r in rs[1:]:
            for k in rs[0]:
                assert torch.equal(rs[0][k], r[k]), (launch, k)
        n_done += int(rs[0]["done"].sum())
    sts = [e.get_state() for e in envs]
    for s in sts[1:]:
        _same_state(sts[0], s)
    return n_done


def _bullet_env(pkg, n, **kw):
    """A free body far from every target and wall: no episode ends, actions are the four rotor thrusts."""
    opts = dict(target_points=np.array([[5e3, 5e3, 5e3]]), initial_xyzs=np.array([[0.0, 0.0, 1.0]]), aviary_dim=WIDE,
                circle=False, cylinder=False, ground_contact=False, normalize_actions=False, normalize_obs=False,
                threshold=0.0, max_steps=1 << 20, device=DEV)
    opts.update(kw)
    return pkg.DroneVecEnv(None, n, **opts)


def _advance(env, acts):
    """K = len(acts) control steps (dn_step for K = 1, else one fused launch): step-major numpy copies, the privileged rows included
    where the env writes them."""
    keys = ("obs", "reward", "done", "truncated", "found_targets", "terminal_obs", "ep_return", "ep_length", "privileged", "terminal_privileged")
    if acts.shape[0] == 1:
        o, r, d, info = env.step_tensor(acts[0])
        out = dict(info, obs=o, reward=r, done=d)
        return {k: out[k].cpu().numpy()[None] for k in keys if k in out}
    out = env.rollout_tensor(acts, want_terminal=True)
    return {k: out[k].cpu().numpy() for k in keys if k in out}


def _rollout_outs(r, K):
    return [(r["obs"][t], r["reward"][t], r["done"][t],
             dict(truncated=r["truncated"][t], found_targets=r["found_targets"][t], terminal_obs=r["terminal_obs"][t],
                  ep_length=r["ep_length"][t], ep_return=r["ep_return"][t])) for t in range(K)]


# ---- the env beside its oracle ---------------------------------------------------------------------------------------------------
def make_pair(track, n, *, f32_state, max_steps=4096, **kw):
    env = pkg().DroneVecEnv(track, n, max_steps=max_steps, device="cuda:0", **kw)
    okw = {k: v for k, v in kw.items() if k in ("normalize_obs", "include_distance", "normalize_actions",
                                                "act_noise_sigma", "obs_noise_sigma", "seed", "env_id_offset",
                                                "ground_contact", "threshold", "cylinder", "clip_rew", "norm_rew", "random_spawn")}
    okw.setdefault("normalize_obs", True)
    okw["ground_contact"] = env.ground_contact     # DroneVecEnv's default is DN_GROUND_CONTACT_AUTO: the oracle gets what dn_create resolved
    cfg = O.make_config(track.targets(), track.initial_xyzs, track.aviary_dim, circle=track.is_circle,
                        max_steps=max_steps, f32_state=f32_state, **okw)
    return env, O.OracleVecEnv(cfg, n, threads=8)


def _features(pkg, dynamics, wind):
    d = pkg.DynamicsRandomization(**BODY) if dynamics is True else dynamics
    w = pkg.WindDisturbance(**GUSTY) if wind is True else wind
    return d or None, w or None


def _pair(track, n, dynamics, wind, **kw):
    """make_pair with the features on both sides (float32 state in the oracle)."""
    env, ora = make_pair(track, n, f32_state=True, dynamics=dynamics, wind=wind, **kw)
    ora.dw_cfg = O.make_dw_config(dynamics, wind)
    return env, ora


def _stagger(env, rng, ora=None):
    """Spread the drones' episode step counters over [0, 40) so that time limits end episodes at different steps: waves in which
    some lanes start an episode and others fly on, inside launches too."""
    st = env.get_state()
    st["steps"] = rng.integers(0, 40, len(st)).astype(st["steps"].dtype)
    env.set_state(st)
    if ora is not None:
        ora.envs["steps"] = st["steps"]


def _same_config(ora, ref):
    """The oracle of a GPU test is the one the CPU file of its model ran its coverage on, byte for byte."""
    def same(a, b):
        return (a is None and b is None) or (a is not None and b is not None and bytes(a) == bytes(b))
    assert bytes(ora.cfg) == bytes(ref.cfg) and same(ora.act_cfg, ref.act_cfg) and same(ora.sens_cfg, ref.sens_cfg), \
        "oracle configuration drifted from the CPU file"
    assert (ora.dw_cfg is None and ref.dw_cfg is None) or bytes(ora.dw_cfg) == bytes(ref.dw_cfg if ref.dw_cfg is not None else O.make_dw_config()), \
        "oracle dynamics / wind configuration drifted from the CPU file"


# ---- teacher forcing (load_*) and the models' state after a step or launch (check_*), model by model ---------------------------------
def _get_act(env):
    return {k: v.cpu().numpy() for k, v in env.get_actuator().items()}


def _get_sens(env):
    return {k: v.cpu().numpy() for k, v in env.get_sensor().items()}


def load_dw(env, ora):
    """Teacher forcing: the device's state, scales and wind into the oracle."""
    gpu_state_to_oracle(env.get_state(), ora.envs, env.step_count)
    ora.refresh_rpy()
    if ora.dw_cfg.dynamics:
        ora.dw["dyn"] = env.get_dynamics().cpu().numpy()
    if ora.dw_cfg.wind:
        m, g = env.get_wind()
        ora.dw["wind_mean"], ora.dw["wind_gust"] = m.cpu().numpy(), g.cpu().numpy()


def load_act(env, ora):
    """Teacher forcing: the device's state, scales, wind and the four actuator arrays into the oracle."""
    load_dw(env, ora)
    for k, v in _get_act(env).items():
        ora.act[k] = v


def load_sens(env, ora):
    """Teacher forcing: the device's state, scales, wind, actuator arrays and get_sensor() (latency, bias, history) into the oracle.
    Returns the loaded sensor arrays."""
    if ora.act_cfg is not None:
        load_act(env, ora)
    else:
        load_dw(env, ora)
    g = _get_sens(env)
    for k, v in g.items():
        ora.sens[k] = v
    return g


def _dw_distance(env, ora, rows):
    """(scale ulps, steady-wind ulps, gust ulps, gust |diff| / sigma, gust bit-equal fraction) over `rows`."""
    z = np.zeros(0)
    s_u = m_u = g_u = g_rel = z
    g_eq = 1.0
    if ora.dw_cfg.dynamics:
        s_u = ulps(env.get_dynamics().cpu().numpy()[rows], ora.dw["dyn"][rows])
    if ora.dw_cfg.wind:
        m, g = (x.cpu().numpy()[rows] for x in env.get_wind())
        m_u = ulps(m, ora.dw["wind_mean"][rows])
        g_u = ulps(g[:, :3], ora.dw["wind_gust"][rows, :3])
        sig = np.array([ora.dw_cfg.gust_sigma[0], ora.dw_cfg.gust_sigma[0], ora.dw_cfg.gust_sigma[1]], np.float64)
        g_rel = np.abs(g[:, :3].astype(np.float64) - ora.dw["wind_gust"][rows, :3]) / sig
        g_eq = float(np.mean(g[:, :3] == ora.dw["wind_gust"][rows, :3])) if len(g) else 1.0
    mx = lambda a: float(a.max(initial=0))      # noqa: E731
    return mx(s_u), mx(m_u), mx(g_u), mx(g_rel), g_eq


def check_dw(env, ora, rows, f32, fused, tag):
    s_u, m_u, g_u, g_rel, g_eq = _dw_distance(env, ora, rows)
    assert s_u <= 1 and m_u <= 1, f"{tag}: scales {s_u} / steady wind {m_u} ulps"
    if f32:
        bar = GUST_F32_LAUNCH if fused else GUST_F32_STEP
        assert g_rel <= bar, f"{tag}: float32-compute gust {g_rel:.3e} sigma from the float64 definition (bar {bar:.0e})"
    else:
        assert g_u <= 1 and g_eq >= 0.999, f"{tag}: gust {g_u} ulps, {g_eq:.5f} bit-equal"
    return g_rel


def check_act(env, ora, rows, f32, fused, tag, stats=None):
    got = _get_act(env)
    assert np.array_equal(got["latency"][rows], ora.act["latency"][rows]), f"{tag}: latency"
    assert np.array_equal(got["history"][rows], ora.act["history"][rows]), f"{tag}: history"
    c_u = ulps(got["coeff"][rows], ora.act["coeff"][rows]).max(initial=0)
    assert c_u <= 1, f"{tag}: coeff {c_u} ulps"
    r, want = got["rpm"][rows], ora.act["rpm"][rows]
    dist = float(np.abs(r.astype(np.float64) - want).max(initial=0) / RPM_SPAN)
    eq = float(np.mean(r == want)) if len(r) else 1.0
    if f32:
        bar = LAG_F32_LAUNCH if fused else LAG_F32_STEP
        assert dist <= bar, f"{tag}: float32-compute rpm {dist:.3e} span from the oracle (bar {bar:.1e})"
    else:
        r_u = ulps(r, want).max(initial=0)
        assert r_u <= 1 and eq >= 0.999, f"{tag}: rpm {r_u} ulps, {eq:.5f} bit-equal"
    if stats is not None:
        stats["dist"], stats["eq"] = max(stats.get("dist", 0.0), dist), min(stats.get("eq", 1.0), eq)


def check_sens(env, ora, rows, g0, k0, K, restarted, bar, tag, ncol=13):
    """After a launch of K steps: latency and bias exact (draws included), history entries that were already loaded -- entry j >= K of
    a drone that did not restart -- bit-equal to the loaded entry j - K, entries written during the launch at the observation bar."""
    got = _get_sens(env)
    assert np.array_equal(got["latency"][rows], ora.sens["latency"][rows]), f"{tag}: latency"
    assert np.array_equal(bits(got["bias"][rows]), bits(ora.sens["bias"][rows])), f"{tag}: bias"
    if not ora.sens_cfg.lat_on:
        return got
    k = ora.envs["steps"].astype(np.int64)
    j = np.arange(9)[None, :]
    valid = (j <= k[:, None]) & rows[:, None]
    old = valid & (j >= K) & ~restarted[:, None] & (j - K <= k0[:, None])
    if K < 9:
        assert np.array_equal(bits(got["history"][:, K:, :ncol])[old[:, K:]], bits(g0["history"][:, : 9 - K, :ncol])[old[:, K:]]), \
            f"{tag}: a loaded history entry changed"
    new = valid & ~old
    err = np.abs(got["history"].astype(np.float64) - ora.sens["history"])[:, :, :ncol][new]
    assert (err <= bar).all(), f"{tag}: history entries written in the launch off the oracle by {err.max():.3e} (bar {bar:.0e})"
    return got
