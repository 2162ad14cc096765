"""Per-drone sensor model (include/dronenav.h dn_enable_sensor) on the HIP path: observation latency and per-episode bias.

The contract makes the feature a pure function of the PLAIN env's outputs, so the reference is the env without the sensor model plus a
few lines of numpy (model_support.Delivery): o_k is the plain env's pre-normaliser row, y_k = float32(o_{k - min(d, k)} + b).

 1. off is off, bit for bit, alone and on top of dynamics + wind + actuator;
 2. transparency: nothing feeds back into reward, episode ends, Monitor outputs or the body state over 300 steps;
 3. the delivery rule, bit exact, every row of every drone (normaliser off; noise on and off);
 4. the normaliser is fed the delivered rows: a float64 numpy RunningMeanStd on the delivered stream, itself pinned against the plain
    env with the normaliser on, at the project's observation bar (1e-5 relative + 1e-5 absolute);
 5. all 16 instantiations: float64 / float32 compute x normaliser x noise x single / fused;
 6. one fused launch = single steps, K in {5, 20, 64}, history included;
 7. the draws against their Philox definition (d and b of every episode of every run come from the definition, never from the device),
    at env_id_offset 0 and past 2^33 and at a step counter past 2^32;
 8. two shards = the whole fleet;  9. set / get round trip and checkpoint continuation;  10. refusals, collectors, kernel shape.

Every run through _drive asserts that it met the boundaries: every latency 0..8, >= 100 episode ends, a delivery with k < d.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gpu_support import DEV, _acts, _advance, _run_pair, _same_sensor, _same_state  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402
from model_support import (AMPS, BODY, BODY_KEYS, FULL, GUSTY, NOISE, Delivery, Rms64, Worst, bits)  # noqa: E402


def _model(pkg, **kw):
    opts = dict(latency=(0, 8), bias=AMPS)
    opts.update(kw)
    return pkg.SensorModel(**opts)


def _envs(pkg, n, model, *, f32=False, norm=False, noise=False, full=False, seed=31, offset=0, pinned=False):
    """The env with the sensor model, the plain env with the normaliser OFF (its rows are the o_k) and, on request, the plain env with
    the normaliser on (pins the numpy normaliser)."""
    from drl_dronenavigation_amd import tracks
    kw = dict(max_steps=40, seed=seed, device=DEV, compute_dtype="float32" if f32 else "float64", env_id_offset=offset)
    if noise:
        kw.update(NOISE)
    if full:
        kw.update(dynamics=pkg.DynamicsRandomization(**BODY), wind=pkg.WindDisturbance(**GUSTY), actuator=pkg.ActuatorModel(**FULL))
    track = tracks.circle(1, 4, 1)
    S = pkg.DroneVecEnv(track, n, sensor=model, normalize_obs=norm, **kw)
    P = pkg.DroneVecEnv(track, n, normalize_obs=False, **kw)
    PN = pkg.DroneVecEnv(track, n, normalize_obs=True, **kw) if pinned else None
    return S, P, PN


def _drive(pkg, model, *, n=2048, K=1, steps=60, norm=False, sc0=0, seed=31, offset=0, rng_seed=5, **kw):
    """Runs S beside P over `steps` control steps in launches of K and holds every row S writes against Delivery on P's rows: int32
    views with the normaliser off, the observation bar against Rms64 with it on.  Returns (episode ends, worst figure)."""
    S, P, PN = _envs(pkg, n, model, norm=norm, seed=seed, offset=offset, pinned=norm, **kw)
    envs = [e for e in (S, P, PN) if e is not None]
    assert S.kernel_waves(fused=True) == S.kernel_waves(fused=False) == 1
    if sc0:
        for e in envs:
            e.step_count = sc0
    rng = np.random.default_rng(rng_seed)
    dl = Delivery(model, n, seed, offset)
    rs, rp, worst = Rms64(n), Rms64(n), Worst()
    allrows = np.arange(n)

    def check(got, y, rows, tag, ref=rs):
        if norm:
            worst.close(got, ref(y, rows), tag)
        else:
            assert np.array_equal(bits(got), bits(y)), tag

    o0 = P.reset_tensor().cpu().numpy()
    check(S.reset_tensor().cpu().numpy(), dl.start(allrows, o0, sc0), allrows, "reset")
    if PN is not None:
        check(PN.reset_tensor().cpu().numpy(), o0, allrows, "reset (plain, normaliser on)", rp)
    # staggered episode starts: the step counters spread over [0, 40) and a history to go with them
    st = S.get_state()
    steps0 = rng.integers(0, 40, n)
    dl.k = steps0.astype(np.int64)
    dl.hist[:, 1:] = rng.uniform(-1, 1, (n, 8, 13)).astype(np.float32)
    for e in envs:
        s = e.get_state()
        s["steps"] = steps0.astype(st["steps"].dtype)
        e.set_state(s)
    S.set_sensor(history=torch.from_numpy(dl.hist).to(DEV))
    sc = sc0
    for launch in range(steps // K):
        acts = _acts(rng, n, K)
        rS, rP = _advance(S, acts), _advance(P, acts)
        rN = _advance(PN, acts) if PN is not None else None
        for k in ("reward", "done", "truncated", "found_targets"):
            assert np.array_equal(rS[k], rP[k]), (k, launch)
        for t in range(K):
            tag = f"launch {launch} t={t}"
            done = rP["done"][t].astype(bool)
            rows = np.flatnonzero(done)
            o = np.where(done[:, None], rP["terminal_obs"][t], rP["obs"][t])
            y = dl.step(o)
            live = np.flatnonzero(~done)
            # the normaliser sees a finished drone's terminal row first, then its reset row: the order the statistics are updated in
            check(rS["obs"][t][live], y[live], live, tag + " obs")
            check(rS["terminal_obs"][t][rows], y[rows], rows, tag + " terminal_obs")
            y0 = dl.start(rows, rP["obs"][t][rows], sc + t)
            check(rS["obs"][t][rows], y0, rows, tag + " reset rows")
            assert np.array_equal(rS["ep_return"][t][rows], rP["ep_return"][t][rows]) and np.array_equal(rS["ep_length"][t][rows], rP["ep_length"][t][rows])
            if rN is not None:
                check(rN["obs"][t][live], o[live], live, tag + " obs (plain, normaliser on)", rp)
                check(rN["terminal_obs"][t][rows], o[rows], rows, tag + " terminal_obs (plain, normaliser on)", rp)
                check(rN["obs"][t][rows], rP["obs"][t][rows], rows, tag + " reset rows (plain, normaliser on)", rp)
            dl.ends += len(rows)
        sc += K
    assert S.step_count == sc
    a, b = S.get_state(), P.get_state()
    for k in BODY_KEYS:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k
    assert np.array_equal(a["steps"], dl.k)
    g = {k: v.cpu().numpy() for k, v in S.get_sensor().items()}
    assert np.array_equal(g["latency"], dl.d) and np.array_equal(bits(g["bias"]), bits(dl.b))
    valid = np.arange(9)[None, :] <= dl.k[:, None]                      # entries older than the episode are unspecified
    assert np.array_equal(bits(g["history"])[valid], bits(dl.hist)[valid])
    if norm:
        print(f"normaliser: worst |diff| {worst.abs:.3e}, worst fraction of the bar {worst.excess:.3f}")
    for e in envs:
        e.close()
    # a run that met no boundary proves nothing
    assert dl.seen == set(range(model.latency[0], model.latency[1] + 1)) and dl.ends >= 100 and dl.young > 0, (dl.seen, dl.ends, dl.young)
    return dl.ends, worst


# ---- 1. off is off --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True], ids=["alone", "dynamics+wind+actuator"])
def test_sensor_off_is_off_bit_for_bit(full, monkeypatch):
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    monkeypatch.delenv("DN_WAVES", raising=False)
    n = 2048
    kw = dict(max_steps=15, seed=21, device=DEV, normalize_obs=True, **NOISE)
    if full:
        kw.update(dynamics=pkg.DynamicsRandomization(**BODY), wind=pkg.WindDisturbance(**GUSTY), actuator=pkg.ActuatorModel(**FULL))
    track = tracks.reaching()
    sens = pkg.DroneVecEnv(track, n, sensor=pkg.SensorModel(), **kw)
    plain = pkg.DroneVecEnv(track, n, **kw)
    assert sens.kernel_waves(fused=True) == sens.kernel_waves(fused=False) == 1
    assert _run_pair([sens, plain], np.random.default_rng(3), n) > n     # every output; episodes ended and restarted inside the launches
    _same_state(sens.get_state(), plain.get_state())                     # the normaliser statistics included
    g = sens.get_sensor()
    assert not bool(g["latency"].any()) and not bool(g["bias"].any())
    sens.close()
    plain.close()


# ---- 2. transparency ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True], ids=["alone", "dynamics+wind+actuator"])
def test_sensor_model_feeds_nothing_back(full):
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, K, launches = 2048, 20, 16                                        # 320 control steps
    kw = dict(max_steps=40, seed=8, device=DEV, normalize_obs=True, **NOISE)
    if full:
        kw.update(dynamics=pkg.DynamicsRandomization(**BODY), wind=pkg.WindDisturbance(**GUSTY), actuator=pkg.ActuatorModel(**FULL))
    track = tracks.circle(1, 4, 1)
    S, P = pkg.DroneVecEnv(track, n, sensor=_model(pkg), **kw), pkg.DroneVecEnv(track, n, **kw)
    S.reset_tensor()
    P.reset_tensor()
    rng = np.random.default_rng(2)
    n_done = differs = 0
    for launch in range(launches):
        acts = _acts(rng, n, K)
        a = {k: v.clone() for k, v in S.rollout_tensor(acts, want_terminal=True).items()}
        b = P.rollout_tensor(acts, want_terminal=True)
        for k in ("reward", "done", "truncated", "found_targets"):
            assert torch.equal(a[k], b[k]), (k, launch)
        m = a["done"].bool()
        for k in ("ep_return", "ep_length"):
            assert torch.equal(a[k][m], b[k][m]), (k, launch)
        n_done += int(m.sum())
        differs += int((a["obs"] != b["obs"]).any(dim=2).sum())
        sa, sb = S.get_state(), P.get_state()
        for k in BODY_KEYS:
            assert np.ascontiguousarray(sa[k]).tobytes() == np.ascontiguousarray(sb[k]).tobytes(), (k, launch)
    lat = S.get_sensor()["latency"].cpu().numpy()
    assert n_done >= 100 and set(np.unique(lat).tolist()) == set(range(9)) and differs > n * K, (n_done, differs)   # ... and the model is live
    S.close()
    P.close()


# ---- 3. / 4. / 5. the delivery rule and the normaliser, over all 16 instantiations ----------------------------------------------
@pytest.mark.parametrize("K", [1, 20], ids=["single", "fused"])
@pytest.mark.parametrize("noise", [False, True], ids=["quiet", "noise"])
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "norm"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_delivery_rule_in_every_instantiation(f32, norm, noise, K):
    """Normaliser off: every obs / terminal_obs / reset row equals float32(o_{k - min(d, k)} + b) as int32 views, no exclusions.
    Normaliser on: the float64 numpy normaliser on the delivered stream at 1e-5 + 1e-5 |x|, no drone excluded; the same numpy
    statement is held against the plain env with the normaliser on in the same run, which pins the reference itself."""
    ends, _ = _drive(_pkg(), _model(_pkg()), K=K, steps=60, f32=f32, norm=norm, noise=noise)
    assert ends >= 100


def test_delivery_rule_on_top_of_dynamics_wind_and_actuator():
    _drive(_pkg(), _model(_pkg()), K=20, steps=60, noise=True, full=True)
    _drive(_pkg(), _model(_pkg()), K=1, steps=40, norm=True, noise=True, full=True)


def test_latency_alone_and_bias_alone():
    pkg = _pkg()
    _drive(pkg, _model(pkg, bias=0.0), K=20, steps=60, noise=True)
    S, P, _ = _envs(pkg, 1024, _model(pkg, latency=(0, 0)), noise=True)
    o0 = P.reset_tensor().cpu().numpy()
    g = S.reset_tensor().cpu().numpy()
    dl = Delivery(S.sensor, 1024, 31, 0)
    assert np.array_equal(bits(g), bits(dl.start(np.arange(1024), o0, 0)))
    acts = _acts(np.random.default_rng(1), 1024, 50)
    rS, rP = _advance(S, acts), _advance(P, acts)
    ends = 0
    for t in range(50):
        done = rP["done"][t].astype(bool)
        rows = np.flatnonzero(done)
        y = dl.step(np.where(done[:, None], rP["terminal_obs"][t], rP["obs"][t]))
        assert np.array_equal(bits(rS["obs"][t][~done]), bits(y[~done])) and np.array_equal(bits(rS["terminal_obs"][t][rows]), bits(y[rows]))
        assert np.array_equal(bits(rS["obs"][t][rows]), bits(dl.start(rows, rP["obs"][t][rows], t)))
        ends += len(rows)
    assert ends >= 100 and not bool(S.get_sensor()["latency"].any())
    S.close()
    P.close()


# ---- 6. fused = single ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 20, 64])
def test_one_fused_launch_equals_single_steps(K):
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, launches = 2048, 3 if K > 5 else 8
    kw = dict(max_steps=40, seed=77, device=DEV, normalize_obs=True, sensor=_model(pkg), actuator=pkg.ActuatorModel(**FULL),
              dynamics=pkg.DynamicsRandomization(**BODY), wind=pkg.WindDisturbance(**GUSTY), **NOISE)
    track = tracks.circle(1, 4, 1)
    F, S = pkg.DroneVecEnv(track, n, **kw), pkg.DroneVecEnv(track, n, **kw)
    assert torch.equal(F.reset_tensor(), S.reset_tensor())
    rng = np.random.default_rng(9)
    st = F.get_state()
    st["steps"] = rng.integers(0, 40, n).astype(st["steps"].dtype)
    hist = torch.from_numpy(rng.uniform(-1, 1, (n, 9, 13)).astype(np.float32)).to(DEV)
    for e in (F, S):
        e.set_state(st)
        e.set_sensor(history=hist)
    n_done = young = 0
    seen = set()
    for launch in range(launches):
        acts = _acts(rng, n, K)
        r = {k: v.clone() for k, v in F.rollout_tensor(acts, want_terminal=True).items()}
        for t in range(K):
            d = S.get_sensor()["latency"].cpu().numpy()
            seen.update(np.unique(d).tolist())
            young += int((S.get_state()["steps"] + 1 < d).sum())
            o, rew, done, info = S.step_tensor(acts[t])
            tag = f"K={K} launch {launch} t={t}"
            assert torch.equal(o, r["obs"][t]) and torch.equal(rew, r["reward"][t]) and torch.equal(done, r["done"][t]), tag
            assert torch.equal(info["truncated"], r["truncated"][t]) and torch.equal(info["found_targets"], r["found_targets"][t]), tag
            m = done.bool()
            for k in ("terminal_obs", "ep_return", "ep_length"):
                assert torch.equal(info[k][m], r[k][t][m]), (tag, k)
            n_done += int(m.sum())
        _same_sensor(F, S)
        _same_state(F.get_state(), S.get_state())
    assert n_done >= 100 and seen == set(range(9)) and young > 0, (n_done, seen, young)
    F.close()
    S.close()


# ---- 7. the draws -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset, sc0", [(0, 0), ((1 << 33) + 5, 0), (0, (1 << 32) + 7), ((1 << 33) + 5, (1 << 32) + 7)])
def test_draws_follow_their_definition(offset, sc0):
    """Delivery takes d and b of every episode from the Philox definition; _drive holds the device's latency and bias (get_sensor)
    and every delivered row against it, reset draws and in-kernel draws alike."""
    _drive(_pkg(), _model(_pkg()), K=20, steps=60, noise=True, offset=offset, sc0=sc0, seed=0x2468_ACE0_1357)


# ---- 8. sharding ------------------------------------------------------------------------------------------------------------
def test_two_shards_equal_the_whole_fleet():
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, K = 4096, 20
    m = n // 2
    kw = dict(normalize_obs=True, max_steps=12, seed=2027, device=DEV, sensor=_model(pkg), **NOISE)
    track = tracks.reaching()
    whole = pkg.DroneVecEnv(track, n, **kw)
    parts = [pkg.DroneVecEnv(track, m, env_id_offset=r * m, **kw) for r in range(2)]
    assert torch.equal(whole.reset_tensor(), torch.cat([p.reset_tensor() for p in parts]))
    rng = np.random.default_rng(5)
    n_done = 0
    for rep in range(3):
        acts = _acts(rng, n, K)
        a = whole.rollout_tensor(acts)
        bs = [p.rollout_tensor(acts[:, r * m:(r + 1) * m].contiguous()) for r, p in enumerate(parts)]
        for k in ("obs", "reward", "done", "truncated", "found_targets"):
            assert torch.equal(a[k], torch.cat([b[k] for b in bs], dim=1)), (k, rep)
        n_done += int(a["done"].sum())
        wa, pa = whole.get_sensor(), [p.get_sensor() for p in parts]
        for k in wa:
            assert torch.equal(wa[k], torch.cat([x[k] for x in pa])), (k, rep)
    assert n_done >= n and set(np.unique(wa["latency"].cpu().numpy()).tolist()) == set(range(9))
    _same_state(whole.get_state(), np.concatenate([p.get_state() for p in parts]))
    for e in [whole] + parts:
        e.close()


# ---- 9. set / get, checkpoint -----------------------------------------------------------------------------------------------
# normalize_obs: the blob also carries the normaliser's statistics -- mean, count and, since ABI 10, the second moment itself (rms_m2) --
# and _same_state compares them byte for byte
@pytest.mark.parametrize("normalize_obs", [False, True], ids=["raw", "norm"])
def test_set_get_round_trip_and_checkpoint_continuation(normalize_obs):
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    n, K = 2048, 20
    kw = dict(normalize_obs=normalize_obs, max_steps=15, seed=9, device=DEV, sensor=_model(pkg), actuator=pkg.ActuatorModel(**FULL),
              dynamics=pkg.DynamicsRandomization(**BODY), wind=pkg.WindDisturbance(**GUSTY), **NOISE)
    track = tracks.reaching()
    a = pkg.DroneVecEnv(track, n, **kw)
    a.reset_tensor()
    assert bytes(a.sensor_config().to_c()) == bytes(a.sensor.to_c())
    lat = torch.randint(0, 9, (n,), dtype=torch.int32, device=DEV)
    bi, hi = torch.randn((n, 13), device=DEV) * 0.05, torch.randn((n, 9, 13), device=DEV)
    a.set_sensor(latency=lat, bias=bi, history=hi)
    g = a.get_sensor()
    assert torch.equal(g["latency"], lat) and torch.equal(g["bias"], bi) and torch.equal(g["history"], hi)
    a.set_sensor(bias=bi * 0.5)
    g = a.get_sensor()
    assert torch.equal(g["bias"], bi * 0.5) and torch.equal(g["history"], hi) and torch.equal(g["latency"], lat)
    a.step_count = 1000 + 16 * 3 + 5                                     # the logical history does not move with the step counter
    assert torch.equal(a.get_sensor()["history"], hi)
    a.step_count = 0
    for bad in (dict(latency=lat.long()), dict(latency=lat + 9), dict(bias=bi[:-1]), dict(bias=bi * float("nan")), dict(history=hi[:, :8]),
                dict(bias=bi.cpu())):
        with pytest.raises((TypeError, ValueError)):
            a.set_sensor(**bad)
    rng = np.random.default_rng(12)
    a.rollout_tensor(_acts(rng, n, K))
    a.step_tensor(_acts(rng, n, 1)[0])                                   # 21 steps: the ring has wrapped
    st, sens, sc = a.get_state(), a.get_sensor(), a.step_count
    others = dict(dyn=a.get_dynamics(), wind=a.get_wind(), act=a.get_actuator())

    def restore(detour):
        b = pkg.DroneVecEnv(track, n, **kw)
        b.reset_tensor()
        b.set_state(st)
        b.set_dynamics(others["dyn"])
        b.set_wind(*others["wind"])
        b.set_actuator(**others["act"])
        if detour:               # the history is written at another step counter, which is then moved: the rows keep their meaning
            b.step_count = sc + 11
            b.set_sensor(**sens)
        b.step_count = sc
        if not detour:
            b.set_sensor(**sens)
        return b

    b, c = restore(False), restore(True)
    _same_sensor(a, b)
    _same_sensor(a, c)
    n_done = 0
    for _ in range(2):
        acts = _acts(rng, n, K)
        ra = {k: v.clone() for k, v in a.rollout_tensor(acts, want_terminal=True).items()}
        n_done += int(ra["done"].sum())
        for e in (b, c):
            re = e.rollout_tensor(acts, want_terminal=True)
            for k in ra:
                assert torch.equal(ra[k], re[k]), k
    assert n_done >= 100
    for e in (b, c):
        _same_sensor(a, e)
        _same_state(a.get_state(), e.get_state())
    off = pkg.DroneVecEnv(track, 64, device=DEV)
    assert off.sensor_config() is None and off.sensor is None
    with pytest.raises(RuntimeError):
        off.get_sensor()
    off.close()
    for e in (a, b, c):
        e.close()


def test_observation_scale_matches_the_kernels_columns():
    """A body at a known state: the observation columns are the physical values times observation_scale()."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    env = pkg.DroneVecEnv(tracks.circle(1, 4, 1), 64, device=DEV, normalize_obs=False)
    sc = env.observation_scale()
    assert sc.shape == (13,) and np.allclose(sc[3:12], [1 / np.pi] * 3 + [1 / 3] * 3 + [1.0] * 3)
    o = env.reset_tensor().cpu().numpy().astype(np.float64)
    st = env.get_state()
    np.testing.assert_allclose(o[:, :3], st["pos"].astype(np.float64) * sc[:3], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(o[:, 12], st["d"].astype(np.float64) * sc[12], rtol=1e-6, atol=1e-7)
    env.close()


# ---- 10. refusals, collectors, kernel shape -------------------------------------------------------------------------------------
def test_sampling_fused_entry_points_refuse_and_the_collectors_fall_back():
    pkg = _pkg()
    from drl_dronenavigation_amd import _capi, tracks
    from drl_dronenavigation_amd.collector import FusedRolloutCollector, OffPolicyCollector
    lib = _capi.load()
    dev = torch.device(DEV)
    track = tracks.reaching()
    n, T, seed = 512, 10, 17
    kw = dict(normalize_obs=True, max_steps=6, seed=3, device=dev)
    model = _model(pkg, latency=(1, 8))
    plain = pkg.DroneVecEnv(track, n, **kw)
    w0 = (plain.kernel_waves(fused=True), plain.kernel_waves(fused=False))
    late = pkg.DroneVecEnv(track, n, **kw)
    assert (late.kernel_waves(fused=True), late.kernel_waves(fused=False)) == w0        # the previous value without the sensor
    _capi.check(lib.dn_enable_sensor(late._handle, C.byref(model.to_c())))
    assert late.kernel_waves(fused=True) == late.kernel_waves(fused=False) == 1
    late.close()
    env = pkg.DroneVecEnv(track, n, sensor=model, **kw)
    assert env.kernel_waves(fused=True) == env.kernel_waves(fused=False) == 1
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    z4, z1 = torch.zeros((n, 4), device=dev), torch.zeros(n, device=dev)
    z13, zb, zi = torch.zeros((n, 13), device=dev), torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    z8, zk = torch.zeros((n, 8), device=dev), torch.zeros((n, 13), dtype=torch.float64, device=dev)
    log_std = (C.c_float * 4)(-5.0, -5.0, -5.0, -5.0)
    env.reset_tensor()
    sc0 = env.step_count
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
        rc = call()
        assert rc == -1 and b"sensor" in lib.dn_last_error(), (name, rc, lib.dn_last_error())
    torch.cuda.synchronize()
    assert env.step_count == sc0                         # the refused calls launched nothing

    torch.manual_seed(4)
    net = pkg.MlpActorCritic(log_std_init=-5.0).to(dev)
    pol = pkg.FusedMlpPolicy(net, n, dev)
    env2 = pkg.DroneVecEnv(track, n, sensor=model, **kw)
    col = FusedRolloutCollector(env2, pol, T, bootstrap_truncated=False, use_graph=False, seed=seed)
    assert not col._sampled_step
    out = {k: v.clone() for k, v in col.collect().items()}
    colp = FusedRolloutCollector(plain, pol, T, bootstrap_truncated=False, use_graph=False, seed=seed)
    assert colp._sampled_step
    outp = colp.collect()
    assert int(out["episode_starts"].sum()) > n and bool(torch.isfinite(out["obs"]).all())
    assert not torch.equal(outp["obs"][T - 1], out["obs"][T - 1])         # the sensor model is live in the collected rollout
    torch.manual_seed(8)
    sac = pkg.FusedSacActor(pkg.SacActor().to(dev), n, dev, grade="bf16")
    oc = OffPolicyCollector(env, sac, buffer_size=4, seed=5)
    assert not oc._fused_sample and OffPolicyCollector(pkg.DroneVecEnv(track, n, **kw), sac, buffer_size=4)._fused_sample
    ba = oc.collect(3).actions[:3].clone()
    assert bool(torch.isfinite(ba).all()) and bool((ba.abs() <= 1).all()) and bool(ba.abs().sum() > 0)
    for e in (env, env2, plain):
        e.close()
