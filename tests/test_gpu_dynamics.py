"""Per-drone dynamics randomisation (include/dronenav.h dn_enable_dynamics) on the HIP path: scales of 1 are the nominal body bit for
bit, power-of-two scales leave every acceleration unchanged, the scaled step against the independent integrator of
tests/rigid_body_ref.py, the Philox draws against their definition, sharding, the refusals of the sampling-fused entry points, and
checkpointing through get_state + get_dynamics."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats
from scipy.spatial.transform import Rotation

import rigid_body_ref as RB

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gpu_support import DEV, _bullet_env, _run_pair, _same_state  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402
from model_support import _dyn_draw, _mixed  # noqa: E402


# ---- (a) identity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["zero_damping_one_wave", "reference_norm_on", "reference_norm_off"])
def test_unit_scales_are_the_nominal_body_bit_for_bit(case, monkeypatch):
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n = 2048
    kw = dict(max_steps=15, seed=11, device=DEV)
    if case == "zero_damping_one_wave":
        monkeypatch.setenv("DN_WAVES", "1")           # both envs on the one-wave option kernel, with and without the scales
        kw.update(zero_damping=True, normalize_obs=True)
    else:
        monkeypatch.delenv("DN_WAVES", raising=False)  # the DR-off env runs dn_create's own pick
        kw.update(normalize_obs=case == "reference_norm_on")
    track = tracks.reaching()
    dr = pkg.DroneVecEnv(track, n, dynamics=pkg.DynamicsRandomization(), **kw)
    plain = pkg.DroneVecEnv(track, n, **kw)
    assert dr.kernel_waves(fused=True) == dr.kernel_waves(fused=False) == 1
    n_done = _run_pair([dr, plain], np.random.default_rng(3), n)
    assert n_done > n                                   # episodes ended and restarted inside the fused launches
    assert torch.equal(dr.get_dynamics(), torch.ones((n, 4), device=DEV))
    dr.close()
    plain.close()


# ---- (b) similarity -----------------------------------------------------------------------------------------------
def test_power_of_two_scales_leave_every_acceleration_unchanged():
    """Mass, inertia, KF and KM scaled by the same power of two: F/m, tau/I and the gyroscopic term over I are the same numbers in
    floating point, so the fleet flies the nominal trajectory exactly (this does not rest on the recalled Bullet constants)."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n = 4096
    kw = dict(max_steps=15, seed=5, normalize_obs=True, physics="pyb", device=DEV)
    track = tracks.reaching()
    dr = pkg.DroneVecEnv(track, n, dynamics=pkg.DynamicsRandomization(resample=False), **kw)
    plain = pkg.DroneVecEnv(track, n, **kw)
    s = torch.tensor([0.5, 1.0, 2.0], device=DEV)[torch.arange(n, device=DEV) % 3]
    scales = s[:, None].expand(n, 4).contiguous()
    dr.set_dynamics(scales)
    assert _run_pair([dr, plain], np.random.default_rng(9), n) > n
    assert torch.equal(dr.get_dynamics(), scales)      # resample = 0: the resets kept them
    dr.close()
    plain.close()


# ---- (c) physics against references --------------------------------------------------------------------------------
def _scaled_step(pos, quat, vel, ang_v, thrust, scales):
    pkg = _pkg()
    n = len(pos)
    env = _bullet_env(pkg, n, dynamics=pkg.DynamicsRandomization(resample=False))
    env.reset_tensor()
    st = env.get_state()
    st["pos"], st["quat"], st["vel"], st["ang_v"], st["cur_pos"] = pos, quat, vel, ang_v, pos
    env.set_state(st)
    env.set_dynamics(torch.from_numpy(np.ascontiguousarray(scales, dtype=np.float32)).to(DEV))
    _, _, done, _ = env.step_tensor(torch.from_numpy(np.ascontiguousarray(thrust, dtype=np.float32)).to(DEV))
    torch.cuda.synchronize()
    assert not done.any().item()
    out = env.get_state()
    env.close()
    return out


def test_heavier_body_hover_closed_form():
    hover = RB.M * RB.G / 4.0
    rest = np.array([[0.3, -0.2, 1.0]], np.float32)
    st = _scaled_step(rest, np.array([[0, 0, 0, 1]], np.float32), np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32),
                      np.full((1, 4), hover, np.float32), np.array([[1.25, 1.0, 1.0, 1.0]]))
    f, _ = RB.thrust_to_force(np.full(4, hover, np.float32).astype(np.float64))
    vz = (f.sum() / (1.25 * RB.M) - RB.G) / 240.0
    assert vz < -0.008                                  # (1/1.25 - 1) g / 240
    np.testing.assert_allclose(st["vel"][0], [0, 0, vz], rtol=1e-6, atol=1e-7)
    np.testing.assert_array_equal(st["ang_v"][0], 0.0)
    np.testing.assert_allclose(st["pos"][0][2], 1.0 + vz / 240.0, rtol=1e-7)


@pytest.mark.parametrize("which", ["all_four", "kf_km_only"])
def test_scaled_step_matches_independent_integrator(which, monkeypatch):
    """Random tumbling states and random non-power-of-two scales in [0.7, 1.3]: the HIP step against tests/rigid_body_ref.py with its
    M and J set per drone and the chain's forces x s_kf, z-torque x s_km.  1e-5 absolute + 1e-6 relative (the north-star bar)."""
    rng = np.random.default_rng(31)
    n = 512
    quat = Rotation.random(n, random_state=6).as_quat().astype(np.float32)
    quat /= np.linalg.norm(quat.astype(np.float64), axis=1, keepdims=True).astype(np.float32)
    pos = (rng.uniform(-2, 2, (n, 3)) + [0, 0, 3]).astype(np.float32)
    vel = rng.normal(0, 2.0, (n, 3)).astype(np.float32)
    ang_v = rng.normal(0, 8.0, (n, 3)).astype(np.float32)
    thrust = rng.uniform(0.02, 0.16, (n, 4)).astype(np.float32)
    scales = rng.uniform(0.7, 1.3, (n, 4)).astype(np.float32)
    if which == "kf_km_only":
        scales[:, :2] = 1.0
    st = _scaled_step(pos, quat, vel, ang_v, thrust, scales)
    f, tq = RB.thrust_to_force(thrust.astype(np.float64))
    zt = (tq * RB.YAW_SIGN).sum(-1)
    M0, J0 = RB.M, RB.J.copy()
    s = scales.astype(np.float64)
    for k in range(n):
        monkeypatch.setattr(RB, "M", M0 * s[k, 0])
        monkeypatch.setattr(RB, "J", J0 * s[k, 1])
        ref = RB.step(pos[k], quat[k].astype(np.float64), vel[k], ang_v[k], f[k] * s[k, 2], zt[k] * s[k, 3])
        for name, r in zip(("pos", "quat", "vel", "ang_v"), ref):
            got = st[name][k].astype(np.float64)
            if name == "quat" and np.dot(got, r) < 0:
                r = -r
            assert np.all(np.abs(got - r) <= 1e-5 + 1e-6 * np.abs(r)), f"drone {k}: {name} {got} vs {r}"


# ---- (d) draws ------------------------------------------------------------------------------------------------------
RANGES = dict(mass=(0.8, 1.2), inertia=(0.5, 1.5), kf=(0.9, 1.1), km=(0.7, 1.05))


def test_reset_draws_follow_their_definition_and_are_uniform():
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, seed = 262144, 0x1234_5678_9ABC
    d = pkg.DynamicsRandomization(**RANGES)
    env = pkg.DroneVecEnv(tracks.reaching(), n, dynamics=d, seed=seed, normalize_obs=False, device=DEV)
    assert bytes(env.dynamics_config().to_c()) == bytes(d.to_c())
    sc = env.step_count
    env.reset_tensor()
    got = env.get_dynamics().cpu().numpy()
    for gid in list(range(512)) + list(range(n - 512, n)):
        assert np.array_equal(got[gid], _dyn_draw(d, gid, sc, seed)), gid
    for j, name in enumerate(("mass", "inertia", "kf", "km")):
        lo, hi = (float(np.float32(v)) for v in RANGES[name])
        col = got[:, j].astype(np.float64)
        assert col.min() >= lo and col.max() <= hi, name
        p = stats.kstest((col - lo) / (hi - lo), "uniform").pvalue
        assert p > 1e-3, (name, p)
    env.close()


def test_episode_ends_redraw_and_the_others_keep_their_body():
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, seed = 1024, 77
    d = pkg.DynamicsRandomization(**RANGES)
    env = pkg.DroneVecEnv(tracks.reaching(), n, dynamics=d, seed=seed, max_steps=6, normalize_obs=False, device=DEV)
    env.reset_tensor()
    rng = np.random.default_rng(2)
    cur = env.get_dynamics().cpu().numpy()
    redrawn = 0
    for t in range(9):
        sc = env.step_count
        _, _, done, _ = env.step_tensor(torch.from_numpy(_mixed(rng, n)).to(DEV))
        done = done.cpu().numpy().astype(bool)
        got = env.get_dynamics().cpu().numpy()
        for i in np.flatnonzero(done):
            cur[i] = _dyn_draw(d, i, sc, seed)             # the draw of the step the new episode starts on
        redrawn += int(done.sum())
        assert np.array_equal(got, cur), t
    assert redrawn >= n                                 # max_steps = 6: every drone's episode ended at least once
    env.close()


# ---- (e) sharding ---------------------------------------------------------------------------------------------------
def test_eight_shards_equal_the_whole_fleet():
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, R, K = 32768, 8, 20
    m = n // R
    kw = dict(normalize_obs=False, max_steps=12, seed=2026, device=DEV, dynamics=pkg.DynamicsRandomization(**RANGES))
    track = tracks.reaching()
    whole = pkg.DroneVecEnv(track, n, **kw)
    parts = [pkg.DroneVecEnv(track, m, env_id_offset=r * m, **kw) for r in range(R)]
    assert torch.equal(whole.reset_tensor(), torch.cat([p.reset_tensor() for p in parts]))
    assert torch.equal(whole.get_dynamics(), torch.cat([p.get_dynamics() for p in parts]))
    rng = np.random.default_rng(5)
    n_done = 0
    for rep in range(3):
        acts = torch.from_numpy(np.stack([_mixed(rng, n) for _ in range(K)])).to(DEV)
        a = whole.rollout_tensor(acts)
        bs = [p.rollout_tensor(acts[:, r * m:(r + 1) * m].contiguous()) for r, p in enumerate(parts)]
        for k in ("obs", "reward", "done", "truncated", "found_targets"):
            assert torch.equal(a[k], torch.cat([b[k] for b in bs], dim=1)), (k, rep)
        n_done += int(a["done"].sum())
        assert torch.equal(whole.get_dynamics(), torch.cat([p.get_dynamics() for p in parts])), rep
    assert n_done >= n
    _same_state(whole.get_state(), np.concatenate([p.get_state() for p in parts]))
    for e in [whole] + parts:
        e.close()


# ---- (f) refusals and fallback ----------------------------------------------------------------------------------------
def test_sampling_fused_entry_points_refuse_and_the_collectors_fall_back():
    pkg = _pkg()
    from drl_dronenavigation_amd import _capi, tracks
    from drl_dronenavigation_amd.collector import FusedRolloutCollector, OffPolicyCollector
    from drl_dronenavigation_amd.policy_mfma import mlp_forward
    lib = _capi.load()
    dev = torch.device(DEV)
    track = tracks.reaching()
    n, T, seed = 512, 10, 17
    kw = dict(normalize_obs=True, max_steps=6, seed=3, device=dev)
    d = pkg.DynamicsRandomization(**RANGES)
    env, twin = pkg.DroneVecEnv(track, n, dynamics=d, **kw), pkg.DroneVecEnv(track, n, dynamics=d, **kw)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    z4, z1 = torch.zeros((n, 4), device=dev), torch.zeros(n, device=dev)
    z13, zb, zi = torch.zeros((n, 13), device=dev), torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    z8, zk = torch.zeros((n, 8), device=dev), torch.zeros((n, 13), dtype=torch.float64, device=dev)
    log_std = (C.c_float * 4)(-5.0, -5.0, -5.0, -5.0)
    env.reset_tensor()
    sc0 = env.step_count
    def refused(name, rc):
        assert rc == -1 and b"dynamics" in lib.dn_last_error(), (name, rc, lib.dn_last_error())

    calls = {
        "dn_step_sampled": lambda: lib.dn_step_sampled(env._handle, z4.data_ptr(), log_std, seed, 0, z4.data_ptr(), z1.data_ptr(), z13.data_ptr(),
                                               z1.data_ptr(), zb.data_ptr(), zb.data_ptr(), zi.data_ptr(), None, None, None, None, stream),
        "dn_step_squashed": lambda: lib.dn_step_squashed(env._handle, z8.data_ptr(), seed, 0, z4.data_ptr(), None, z13.data_ptr(), z1.data_ptr(),
                                                 zb.data_ptr(), zb.data_ptr(), zi.data_ptr(), None, None, None, None, stream),
        "dn_mlp_step_sampled": lambda: lib.dn_mlp_step_sampled(env._handle, C.byref(_capi.DnMlpNet()), 1, z13.data_ptr(), 13, log_std, seed, 0,
                                                       z4.data_ptr(), z1.data_ptr(), z13.data_ptr(), z1.data_ptr(), zb.data_ptr(), zb.data_ptr(),
                                                       zi.data_ptr(), None, None, None, None, stream),
        "dn_eval_kinematics": lambda: lib.dn_eval_kinematics(env._handle, zk.data_ptr(), z13.data_ptr(), z1.data_ptr(), zb.data_ptr(), zb.data_ptr(),
                                                     zi.data_ptr(), None, None, None, stream),
    }
    for name, call in calls.items():
        refused(name, call())
    torch.cuda.synchronize()
    assert env.step_count == sc0                         # the refused calls launched nothing

    torch.manual_seed(4)
    net = pkg.MlpActorCritic(log_std_init=-5.0).to(dev)
    with torch.no_grad():
        net.action_net.bias.fill_(0.0922)
    pol = pkg.FusedMlpPolicy(net, n, dev)
    env2 = pkg.DroneVecEnv(track, n, dynamics=d, **kw)
    col = FusedRolloutCollector(env2, pol, T, bootstrap_truncated=False, use_graph=False, seed=seed)
    assert not col._sampled_step
    out = {k: v.clone() for k, v in col.collect().items()}
    obs = twin.reset_tensor().clone()
    assert torch.equal(obs, out["obs"][0])
    act, clipped, logp = torch.zeros((n, 4), device=dev), torch.zeros((n, 4), device=dev), torch.zeros(n, device=dev)
    mean, val = torch.zeros((n, 4), device=dev), torch.zeros((n, 1), device=dev)
    for t in range(T):
        mlp_forward([pol.pi, pol.vf], obs, [mean, val])
        _capi.check(lib.dn_policy_sample(twin._handle, mean.data_ptr(), log_std, seed, 0, act.data_ptr(), clipped.data_ptr(), logp.data_ptr(), stream))
        nobs, rew, done, _ = twin.step_tensor(clipped, want_terminal=False)
        assert torch.equal(act, out["actions"][t]) and torch.equal(logp, out["log_probs"][t]) and torch.equal(rew, out["rewards"][t]), t
        assert torch.equal(nobs, out["next_obs"] if t == T - 1 else out["obs"][t + 1]), t
        obs = nobs.clone()
    assert int(out["episode_starts"].sum()) > n
    assert torch.equal(env2.get_dynamics(), twin.get_dynamics())
    # ... and the scales are live: the same rollout on the nominal body goes elsewhere
    plain = pkg.DroneVecEnv(track, n, **kw)
    colp = FusedRolloutCollector(plain, pol, T, bootstrap_truncated=False, use_graph=False, seed=seed)
    assert colp._sampled_step
    outp = colp.collect()
    assert not torch.equal(outp["obs"][T - 1], out["obs"][T - 1])
    torch.manual_seed(8)
    sac = pkg.FusedSacActor(pkg.SacActor().to(dev), n, dev, grade="bf16")
    assert not OffPolicyCollector(twin, sac, buffer_size=4)._fused_sample and OffPolicyCollector(plain, sac, buffer_size=4)._fused_sample
    for e in (env, env2, twin, plain):
        e.close()


# ---- (g) round trip and checkpoint ------------------------------------------------------------------------------------
# normalize_obs: the blob also carries the normaliser's statistics -- mean, count and, since ABI 10, the second moment itself (rms_m2) --
# and _same_state compares them byte for byte
@pytest.mark.parametrize("normalize_obs", [False, True], ids=["raw", "norm"])
def test_set_get_round_trip_and_checkpoint_continuation(normalize_obs):
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, K = 4096, 20
    kw = dict(normalize_obs=normalize_obs, max_steps=15, seed=9, device=DEV, dynamics=pkg.DynamicsRandomization(**RANGES))
    track = tracks.reaching()
    a = pkg.DroneVecEnv(track, n, **kw)
    a.reset_tensor()
    x = torch.rand((n, 4), device=DEV) + 0.5
    a.set_dynamics(x)
    assert torch.equal(a.get_dynamics(), x)
    for bad in (x.double(), x[:-1], -x, x * float("inf"), x.cpu()):
        with pytest.raises((TypeError, ValueError)):
            a.set_dynamics(bad)
    rng = np.random.default_rng(12)
    a.rollout_tensor(torch.from_numpy(np.stack([_mixed(rng, n) for _ in range(K)])).to(DEV))
    st, dyn, sc = a.get_state(), a.get_dynamics(), a.step_count
    b = pkg.DroneVecEnv(track, n, **kw)
    b.reset_tensor()
    b.set_state(st)
    b.set_dynamics(dyn)
    b.step_count = sc
    acts = torch.from_numpy(np.stack([_mixed(rng, n) for _ in range(K)])).to(DEV)
    ra = {k: v.clone() for k, v in a.rollout_tensor(acts, want_terminal=True).items()}
    rb = b.rollout_tensor(acts, want_terminal=True)
    assert int(ra["done"].sum()) > 0
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k
    assert torch.equal(a.get_dynamics(), b.get_dynamics())
    _same_state(a.get_state(), b.get_state())
    a.close()
    b.close()
