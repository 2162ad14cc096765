"""Privileged observations (include/dronenav.h dn_enable_privileged) on the HIP path: the true observation and the drawn model
parameters, per drone and step.

The reference is the env itself: a twin without observation noise, sensor model and normaliser states the true observation, and the
existing getters (dn_get_dynamics / wind / actuator / sensor, dn_get_state) state the parameter columns.

 1. nothing feeds back: every output, the state and the four getters, bit for bit, with and without the feature over 304 steps;
 2. the true observation against the twin's obs / terminal_obs, float64 and float32 compute, single steps and fused launches;
 3. the parameter columns against the getters before and after every single step (terminal rows: before, step rows: after);
 4. one fused launch = single steps, K in {5, 20, 64}, both buffers;
 5. all 16 instantiations at a fleet with a partial last tile, some models off: the neutral columns hold exactly 1 / 0;
 6. the group mask: unselected columns keep the caller's bytes;
 7. dn_reset, two shards, hipGraph replay, capacity_steps, unbind, the refusing entry points;
 8. RolloutCollector(value_input="privileged") against a host recomputation, and "observation" unchanged by the feature.

Every driving run asserts that it met its boundaries (episode ends, latencies 0..8 of both models, ends inside a fused launch).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gpu_support import DEV, _acts, _advance, _same_state  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402
from model_support import AMPS, BODY, FULL, GUSTY, NOISE  # noqa: E402
from model_support import bits as _bits  # noqa: E402  (a test here has a local called bits)

PARAM_COLS = np.arange(16, 52)
PATTERN = 0x7FC12345                    # a quiet NaN no kernel produces
ALL_LAT = set(range(9))


def _models(pkg, which=("dynamics", "wind", "actuator", "sensor")):
    full = dict(dynamics=pkg.DynamicsRandomization(**BODY), wind=pkg.WindDisturbance(**GUSTY), actuator=pkg.ActuatorModel(**FULL),
                sensor=pkg.SensorModel(latency=(0, 8), bias=AMPS))
    return {k: v for k, v in full.items() if k in which}


def _env(pkg, n, *, priv=True, groups=None, which=("dynamics", "wind", "actuator", "sensor"), track=None, **kw):
    from drl_dronenavigation_amd import tracks
    opts = dict(max_steps=40, seed=17, device=DEV, normalize_obs=False)
    opts.update(kw)
    opts.update(_models(pkg, which))
    if priv:
        opts["privileged"] = pkg.PrivilegedObservation() if groups is None else pkg.PrivilegedObservation(groups=groups)
    return pkg.DroneVecEnv(track or tracks.circle(1, 4, 1), n, **opts)


def _twin(pkg, n, **kw):
    """The env whose obs IS the true observation: same seed, bodies, wind, actuator and action noise; no observation noise, no sensor
    model, no normaliser, no privileged rows."""
    kw = dict(kw)
    kw.pop("obs_noise_sigma", None)
    which = tuple(m for m in kw.pop("which", ("dynamics", "wind", "actuator", "sensor")) if m != "sensor")
    return _env(pkg, n, priv=False, which=which, **dict(kw, normalize_obs=False))


def _params(env):
    """Columns 16..51 as the getters state them right now (a model that is off: its neutral value); column 35 = dn_env_state.steps."""
    x = np.zeros((env.num_envs, 52), np.float32)
    x[:, 16:20] = env.get_dynamics().cpu().numpy() if env.dynamics is not None else 1.0
    if env.wind is not None:
        mean, gust = env.get_wind()
        x[:, 20:23], x[:, 24:27] = mean.cpu().numpy()[:, :3], gust.cpu().numpy()[:, :3]
    if env.actuator is not None:
        a = {k: v.cpu().numpy() for k, v in env.get_actuator().items()}
        x[:, 28:32], x[:, 32], x[:, 33] = a["rpm"], a["latency"], a["coeff"]
    if env.sensor is not None:
        s = {k: v.cpu().numpy() for k, v in env.get_sensor().items()}
        x[:, 34], x[:, 36:49] = s["latency"], s["bias"]
    x[:, 35] = env.get_state()["steps"]
    return x


def _same_bits(got, want, tag):
    a, b = _bits(got), _bits(want)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError((tag, len(bad), bad[:5].tolist(), np.asarray(got)[tuple(bad[0])], np.asarray(want)[tuple(bad[0])]))


class Seen:
    """The boundaries a driving run must meet."""

    def __init__(self):
        self.ends = self.inside = self.truncations = 0
        self.act_lat, self.sens_lat = set(), set()

    def rows(self, res, priv_key="privileged"):
        done = res["done"].astype(bool)
        self.ends += int(done.sum())
        self.inside += int(done[:-1].sum()) if done.shape[0] > 1 else 0
        self.truncations += int(res["truncated"].sum())
        if priv_key in res:
            self.act_lat.update(np.unique(res[priv_key][..., 32]).astype(int).tolist())
            self.sens_lat.update(np.unique(res[priv_key][..., 34]).astype(int).tolist())

    def step(self, done, info):
        """One single step's device tensors (step_tensor's done and info dict)."""
        self.rows({k: v.cpu().numpy()[None] for k, v in dict(done=done, truncated=info["truncated"], privileged=info["privileged"]).items()})

    def check(self, fused=True, latencies=True):
        assert self.ends >= 100, self.ends
        assert not fused or self.inside > 0, "no episode ended inside a fused launch"
        assert not latencies or (self.act_lat == ALL_LAT and self.sens_lat == ALL_LAT), (self.act_lat, self.sens_lat)


# ---- 1. nothing feeds back -----------------------------------------------------------------------------------------------
def test_privileged_rows_feed_nothing_back():
    pkg = _pkg()
    n = 2048
    kw = dict(normalize_obs=True, **NOISE)
    A, B = _env(pkg, n, **kw), _env(pkg, n, priv=False, **kw)
    assert A.kernel_waves(fused=True) == A.kernel_waves(fused=False) == 1
    assert torch.equal(A.reset_tensor(), B.reset_tensor())
    rng, seen = np.random.default_rng(4), Seen()
    plan = [1] * 4 + [20] * 15                                            # 304 control steps
    for launch, K in enumerate(plan):
        acts = _acts(rng, n, K)
        ra, rb = _advance(A, acts), _advance(B, acts)
        for k in rb:
            if k in ("terminal_obs", "ep_return", "ep_length"):
                m = rb["done"].astype(bool)
                assert np.array_equal(_bits(ra[k][m]) if ra[k].dtype == np.float32 else ra[k][m],
                                      _bits(rb[k][m]) if rb[k].dtype == np.float32 else rb[k][m]), (k, launch)
            elif ra[k].dtype == np.float32:
                _same_bits(ra[k], rb[k], (k, launch))
            else:
                assert np.array_equal(ra[k], rb[k]), (k, launch)
        seen.rows(ra)
        _same_state(A.get_state(), B.get_state())                         # the normaliser statistics included
        assert torch.equal(A.get_dynamics(), B.get_dynamics())
        for x, y in zip(A.get_wind(), B.get_wind()):
            assert torch.equal(x, y)
        for ga, gb in ((A.get_actuator(), B.get_actuator()), (A.get_sensor(), B.get_sensor())):
            for k in ga:
                assert torch.equal(ga[k], gb[k]), (k, launch)
    assert A.step_count == B.step_count == sum(plan)
    seen.check()
    A.close()
    B.close()


# ---- 2. the true observation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_true_observation_equals_the_twin_without_noise_sensor_and_normaliser(f32):
    pkg = _pkg()
    n = 2048
    kw = dict(compute_dtype="float32" if f32 else "float64", **NOISE)
    A, T = _env(pkg, n, normalize_obs=True, **kw), _twin(pkg, n, **kw)
    A.reset_tensor()
    _same_bits(A.privileged.cpu().numpy()[:, :13], T.reset_tensor().cpu().numpy(), "reset")
    rng, seen, differs = np.random.default_rng(9), Seen(), 0
    for launch, K in enumerate([1] * 6 + [20] * 4 + [1] * 3 + [5] * 2):
        acts = _acts(rng, n, K)
        ra, rt = _advance(A, acts), _advance(T, acts)
        assert np.array_equal(ra["done"], rt["done"]) and np.array_equal(ra["reward"], rt["reward"]), launch
        done = rt["done"].astype(bool)
        _same_bits(ra["privileged"][..., :13], rt["obs"], ("obs", launch))                      # every drone, every step
        _same_bits(ra["terminal_privileged"][..., :13][done], rt["terminal_obs"][done], ("terminal_obs", launch))
        assert not ra["privileged"][..., 13:16].view(np.int32).any() and not ra["terminal_privileged"][..., 13:16][done].view(np.int32).any()
        differs += int((ra["obs"] != rt["obs"]).any(axis=2).sum())
        seen.rows(ra)
    seen.check()
    assert differs > n * 50, differs            # ... and what the policy sees IS degraded
    A.close()
    T.close()


# ---- 3. the parameter columns, single steps ----------------------------------------------------------------------------------
def test_parameter_columns_equal_the_getters_before_and_after_every_step():
    pkg = _pkg()
    n = 2048
    A = _env(pkg, n, normalize_obs=True, **NOISE)
    A.reset_tensor()
    _same_bits(A.privileged.cpu().numpy()[:, PARAM_COLS], _params(A)[:, PARAM_COLS], "reset")
    rng, seen = np.random.default_rng(12), Seen()
    for t in range(90):
        before = _params(A)
        r = _advance(A, _acts(rng, n, 1))
        after = _params(A)
        done = r["done"][0].astype(bool)
        _same_bits(r["privileged"][0][:, PARAM_COLS], after[:, PARAM_COLS], ("step row", t))
        before[:, 35] = r["ep_length"][0]                                 # the finished episode's length (valid where done)
        _same_bits(r["terminal_privileged"][0][done][:, PARAM_COLS], before[done][:, PARAM_COLS], ("terminal row", t))
        assert (before[done][:, 35] >= 1).all() and (before[done][:, 35] == r["terminal_privileged"][0][done][:, 35]).all()
        # a restarted drone: the new episode's draws, r = rpm_fill, step counter 0
        assert not after[done][:, 35].any()
        seen.rows(r)
        seen.act_lat.update(np.unique(r["terminal_privileged"][0][done][:, 32]).astype(int).tolist())
    seen.check(fused=False)
    assert seen.truncations > 0
    A.close()


# ---- 4. fused = single ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 20, 64])
def test_one_fused_launch_equals_single_steps(K):
    pkg = _pkg()
    n = 2048
    kw = dict(max_steps=12, normalize_obs=True, **NOISE)
    F, S = _env(pkg, n, **kw), _env(pkg, n, **kw)
    assert torch.equal(F.reset_tensor(), S.reset_tensor()) and torch.equal(F.privileged, S.privileged)
    rng, seen = np.random.default_rng(K), Seen()
    for launch in range(4):
        acts = _acts(rng, n, K)
        rf = _advance(F, acts)
        for t in range(K):
            rs = _advance(S, acts[t:t + 1])
            done = rs["done"][0].astype(bool)
            assert np.array_equal(rf["done"][t], rs["done"][0])
            _same_bits(rf["obs"][t], rs["obs"][0], ("obs", launch, t))
            _same_bits(rf["privileged"][t], rs["privileged"][0], ("privileged", launch, t))
            _same_bits(rf["terminal_privileged"][t][done], rs["terminal_privileged"][0][done], ("terminal_privileged", launch, t))
        seen.rows(rf)
        assert torch.equal(F.privileged, S.privileged)                   # env.privileged follows the launch's last step
    _same_state(F.get_state(), S.get_state())
    _same_bits(_params(F), _params(S), "getters")
    seen.check()
    F.close()
    S.close()


# ---- 5. all 16 instantiations, a partial last tile, some models off ----------------------------------------------------------
@pytest.mark.parametrize("K", [1, 20], ids=["single", "fused"])
@pytest.mark.parametrize("noise", [False, True], ids=["quiet", "noise"])
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "norm"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_every_instantiation_with_some_models_off(f32, norm, noise, K):
    pkg = _pkg()
    n = 1000                                                              # 15 whole tiles and one of 40 drones
    which = ("wind", "sensor") if f32 == norm else ("dynamics", "actuator")
    kw = dict(max_steps=15, compute_dtype="float32" if f32 else "float64", which=which, **(NOISE if noise else {}))
    A, T = _env(pkg, n, normalize_obs=norm, **kw), _twin(pkg, n, **kw)
    A.reset_tensor()
    T.reset_tensor()
    rng, seen = np.random.default_rng(3), Seen()
    for launch in range(60 // K):
        acts = _acts(rng, n, K)
        ra, rt = _advance(A, acts), _advance(T, acts)
        done = rt["done"].astype(bool)
        assert np.array_equal(ra["done"], rt["done"])
        _same_bits(ra["privileged"][..., :13], rt["obs"], ("obs", launch))
        _same_bits(ra["terminal_privileged"][..., :13][done], rt["terminal_obs"][done], ("terminal_obs", launch))
        _same_bits(ra["privileged"][-1][:, PARAM_COLS], _params(A)[:, PARAM_COLS], ("last step row", launch))
        for rows in (ra["privileged"].reshape(-1, 52), ra["terminal_privileged"][done]):
            if "dynamics" not in which:
                assert (rows[:, 16:20].view(np.int32) == np.float32(1.0).view(np.int32)).all()
            for model, cols in (("wind", slice(20, 28)), ("actuator", slice(28, 34)), ("sensor", slice(36, 52))):
                if model not in which:
                    assert not rows[:, cols].view(np.int32).any(), model
            if "sensor" not in which:
                assert not rows[:, 34].view(np.int32).any()
            assert not rows[:, [13, 14, 15, 23, 27, 49, 50, 51]].view(np.int32).any()
        seen.rows(ra)
    seen.check(fused=K > 1, latencies=False)
    lat = seen.sens_lat if "sensor" in which else seen.act_lat
    assert lat == ALL_LAT and (seen.act_lat if "sensor" in which else seen.sens_lat) == {0}
    A.close()
    T.close()


# ---- 6. the group mask ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [("obs",), ("dyn",), ("wind",), ("act",), ("sens",), ("obs", "sens"), ("act", "sens"), ("act", "obs"),
                                    ("dyn", "wind", "act"), ("obs", "dyn", "wind", "act", "sens")], ids="+".join)
def test_unselected_groups_keep_the_callers_bytes(groups):
    """A flies beside F, the same env with every group selected: A's selected columns are F's, its other columns keep the NaN pattern
    the buffers were filled with before every call -- reset, single steps, fused launches, step rows and terminal rows."""
    pkg = _pkg()
    n, K = 1000, 20
    A, F = _env(pkg, n, groups=groups, max_steps=15, **NOISE), _env(pkg, n, max_steps=15, **NOISE)
    sel = np.zeros(52, bool)
    sel[A.privileged_obs.columns()] = True
    assert A.privileged_config() == A.privileged_obs and A.privileged_config().mask == A.privileged_obs.mask

    def fill(*tensors):
        for x in tensors:
            x.view(torch.int32).fill_(PATTERN)

    def judge(rows, full_rows, tag):
        bits = _bits(rows)
        assert (bits[..., ~sel] == PATTERN).all(), (tag, "an unselected column was written")
        assert np.array_equal(bits[..., sel], _bits(full_rows)[..., sel]), (tag, "the selected columns are not those of the full row")
        assert not (bits[..., sel] == PATTERN).any(), (tag, "a selected column was not written")

    fill(A.privileged)
    A.reset_tensor()
    F.reset_tensor()
    judge(A.privileged.cpu().numpy(), F.privileged.cpu().numpy(), "reset")
    rng, seen = np.random.default_rng(6), Seen()                          # F's rows carry the latencies A's mask may leave out
    for t in range(18):                                                   # single steps across the first truncations
        a = _acts(rng, n, 1)
        fill(A.privileged, A._term_priv)
        ra, rf = _advance(A, a), _advance(F, a)
        done = rf["done"][0].astype(bool)
        judge(ra["privileged"][0], rf["privileged"][0], ("step", t))
        judge(ra["terminal_privileged"][0][done], rf["terminal_privileged"][0][done], ("terminal", t))
        assert (_bits(ra["terminal_privileged"][0][~done]) == PATTERN).all(), "a terminal row was written for a drone that flies on"
        seen.rows(rf)
    out = None
    for launch in range(4):                                               # fused launches into the caller's prefilled buffers
        acts = _acts(rng, n, K)
        if out is None:
            out = A.rollout_tensor(acts, want_terminal=True)              # the first launch hands out the buffers
        else:
            fill(out["privileged"], out["terminal_privileged"], A.privileged)
            A.rollout_tensor(acts, out=out, want_terminal=True)
            judge(A.privileged.cpu().numpy(), out["privileged"][-1].cpu().numpy(), ("env.privileged after a fused launch", launch))
        rf = _advance(F, acts)
        if launch == 0:
            continue
        done = rf["done"].astype(bool)
        judge(out["privileged"].cpu().numpy(), rf["privileged"], ("fused step rows", launch))
        term = out["terminal_privileged"].cpu().numpy()
        judge(term[done], rf["terminal_privileged"][done], ("fused terminal rows", launch))
        assert (_bits(term[~done]) == PATTERN).all()
        seen.rows(rf)
    seen.check()
    A.close()
    F.close()


# ---- 7. dn_reset, shards, hipGraph, capacity, unbind, refusals -----------------------------------------------------------------
def test_reset_writes_the_fresh_rows():
    pkg = _pkg()
    n = 1000
    A, T = _env(pkg, n, normalize_obs=True, random_spawn=True, **NOISE), _twin(pkg, n, random_spawn=True, **NOISE)
    for _ in range(2):                                                    # the second reset redraws: fresh rows again
        A.reset_tensor()
        rows = A.privileged.cpu().numpy()
        _same_bits(rows[:, :13], T.reset_tensor().cpu().numpy(), "true reset observation")
        _same_bits(rows[:, PARAM_COLS], _params(A)[:, PARAM_COLS], "parameters")
        assert not rows[:, 35].any() and not rows[:, 13:16].view(np.int32).any()
        rpm_fill = A.get_actuator()["rpm"].cpu().numpy()
        assert np.array_equal(rows[:, 28:32], rpm_fill) and (rpm_fill == rpm_fill[0]).all() and rpm_fill.all()
        acts = _acts(np.random.default_rng(1), n, 7)
        A.rollout_tensor(acts)
        T.rollout_tensor(acts)
    # without want_terminal there are no terminal rows: none handed out, none written
    A._term_priv.view(torch.int32).fill_(PATTERN)
    info = A.step_tensor(acts[0], want_terminal=False)[3]
    assert info["terminal_privileged"] is None and info["privileged"] is A.privileged
    assert bool((A._term_priv.view(torch.int32) == PATTERN).all())
    A.close()
    T.close()


def test_two_shards_equal_the_whole_fleet():
    pkg = _pkg()
    n, K = 2048, 20
    kw = dict(max_steps=15, normalize_obs=True, **NOISE)
    W = _env(pkg, n, **kw)
    halves = [_env(pkg, n // 2, env_id_offset=off, **kw) for off in (0, n // 2)]
    W.reset_tensor()
    for h in halves:
        h.reset_tensor()
    assert torch.equal(W.privileged, torch.cat([h.privileged for h in halves]))
    rng, seen = np.random.default_rng(2), Seen()
    for launch in range(3):
        acts = _acts(rng, n, K)
        rw = _advance(W, acts)
        rh = [_advance(h, acts[:, i * n // 2:(i + 1) * n // 2].contiguous()) for i, h in enumerate(halves)]
        done = rw["done"].astype(bool)
        for k in ("privileged", "terminal_privileged"):
            both = np.concatenate([r[k] for r in rh], axis=1)
            _same_bits(rw[k][done] if k.startswith("terminal") else rw[k], both[done] if k.startswith("terminal") else both, (k, launch))
        seen.rows(rw)
    seen.check()
    for e in [W] + halves:
        e.close()


def test_a_captured_graph_keeps_writing():
    pkg = _pkg()
    n = 1024
    kw = dict(max_steps=15, normalize_obs=True, **NOISE)
    G, E = _env(pkg, n, **kw), _env(pkg, n, **kw)
    G.reset_tensor()
    E.reset_tensor()
    rng = np.random.default_rng(5)
    static = torch.zeros((n, 4), dtype=torch.float32, device=DEV)
    for _ in range(3):                                                    # warm-up, eager
        a = _acts(rng, n, 1)[0]
        static.copy_(a)
        G.step_tensor(static)
        E.step_tensor(a)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    a = _acts(rng, n, 1)[0]
    static.copy_(a)
    with torch.cuda.graph(graph):
        G.step_tensor(static)
    graph.replay()
    E.step_tensor(a)
    seen = Seen()
    for t in range(30):
        a = _acts(rng, n, 1)[0]
        static.copy_(a)
        for x in (G.privileged, G._term_priv):
            x.view(torch.int32).fill_(PATTERN)
        graph.replay()
        _, _, done, info = E.step_tensor(a)
        m = done.bool()
        assert torch.equal(G.privileged.view(torch.int32), info["privileged"].view(torch.int32)), t
        assert torch.equal(G._term_priv.view(torch.int32)[m], info["terminal_privileged"].view(torch.int32)[m]), t
        assert bool((G._term_priv.view(torch.int32)[~m] == PATTERN).all())
        seen.step(done, info)
    seen.check(fused=False)
    _same_state(G.get_state(), E.get_state())
    G.close()
    E.close()


def test_capacity_unbind_and_refusals():
    pkg = _pkg()
    from drl_dronenavigation_amd import collector
    n = 1024
    A, P = _env(pkg, n, **NOISE), _env(pkg, n, priv=False, **NOISE)
    lib, h = A._lib, A._handle
    A.reset_tensor()
    P.reset_tensor()
    rng = np.random.default_rng(7)
    # capacity_steps: k beyond it is refused before anything is launched
    rows = torch.zeros((4, n, 52), dtype=torch.float32, device=DEV)
    rows.view(torch.int32).fill_(PATTERN)
    pkg._capi.check(lib.dn_bind_privileged(h, rows.data_ptr(), None, 4))
    A._priv_bound = None
    acts = _acts(rng, n, 5)
    o = dict(obs=torch.zeros((5, n, 13), device=DEV), reward=torch.zeros((5, n), device=DEV), done=torch.zeros((5, n), dtype=torch.uint8, device=DEV),
             truncated=torch.zeros((5, n), dtype=torch.uint8, device=DEV), found=torch.zeros((5, n), dtype=torch.int32, device=DEV))

    def many(k):
        return lib.dn_step_many(h, k, acts.data_ptr(), o["obs"].data_ptr(), o["reward"].data_ptr(), o["done"].data_ptr(), o["truncated"].data_ptr(),
                                o["found"].data_ptr(), None, None, None, None, None)
    assert many(5) == -1 and b"capacity_steps" in lib.dn_last_error()
    torch.cuda.synchronize()
    assert bool((rows.view(torch.int32) == PATTERN).all()) and A.step_count == 0
    assert many(4) == 0
    torch.cuda.synchronize()
    assert not bool((rows.view(torch.int32) == PATTERN).any()) and A.step_count == 4
    P.rollout_tensor(acts[:4].contiguous())
    # misuse of the binding
    assert lib.dn_bind_privileged(h, rows.data_ptr() + 4, None, 4) == -1 and b"aligned" in lib.dn_last_error()
    assert lib.dn_bind_privileged(h, rows.data_ptr(), None, 0) == -1
    assert lib.dn_bind_privileged(h, None, rows.data_ptr(), 4) == -1
    assert lib.dn_bind_privileged(P._handle, rows.data_ptr(), None, 4) == -5          # DN_ERR_BAD_STATE: not enabled
    # unbind: enabled but unbound writes nothing, and flies the same steps
    pkg._capi.check(lib.dn_bind_privileged(h, None, None, 0))
    rows.view(torch.int32).fill_(PATTERN)
    A.privileged.view(torch.int32).fill_(PATTERN)
    a = _acts(rng, n, 1)[0]
    A._launch(a)
    ref = P.step_tensor(a)
    torch.cuda.synchronize()
    assert bool((rows.view(torch.int32) == PATTERN).all()) and bool((A.privileged.view(torch.int32) == PATTERN).all())
    assert torch.equal(A._obs, P._obs) and torch.equal(A._reward, ref[1])
    assert many(5) == 0                                                   # no binding, no capacity to exceed
    P.rollout_tensor(acts)
    # the next step_tensor binds the env's own buffers again
    a = _acts(rng, n, 1)[0]
    _, _, _, info = A.step_tensor(a)
    P.step_tensor(a)
    assert not bool((info["privileged"].view(torch.int32) == PATTERN).any())
    _same_state(A.get_state(), P.get_state())
    # the entry points whose kernels carry no rows
    B = _env(pkg, n, which=())
    with pytest.raises(pkg.DroneNavError, match="privileged"):
        B.eval_kinematics_tensor(torch.zeros((n, 13), dtype=torch.float64, device=DEV))
    mean, out4, lp = torch.zeros((n, 4), device=DEV), torch.zeros((n, 4), device=DEV), torch.zeros(n, device=DEV)
    log_std = (C.c_float * 4)(0, 0, 0, 0)
    rc = lib.dn_step_sampled(B._handle, mean.data_ptr(), log_std, 1, 0, out4.data_ptr(), lp.data_ptr(), *B._ptrs[0], None, None, None, None, None)
    assert rc == -1 and b"dn_enable_privileged" in lib.dn_last_error()
    rc = lib.dn_step_squashed(B._handle, torch.zeros((n, 8), device=DEV).data_ptr(), 1, 0, out4.data_ptr(), lp.data_ptr(), *B._ptrs[0],
                              None, None, None, None, None)
    assert rc == -1 and b"dn_enable_privileged" in lib.dn_last_error()
    assert B.kernel_waves(fused=True) == B.kernel_waves(fused=False) == 1
    for cls in (collector.FusedRolloutCollector, collector.OffPolicyCollector):
        with pytest.raises(ValueError, match="privileged"):
            cls(B, None, 8)
    with pytest.raises(ValueError, match="privileged"):
        collector.RolloutCollector(P, lambda o: None, 8, value_fn=lambda x: x, value_input="privileged")      # the env has no rows
    with pytest.raises(ValueError, match="value_fn"):
        collector.RolloutCollector(B, lambda o: None, 8, value_input="privileged")
    with pytest.raises(ValueError, match="value_input"):
        collector.RolloutCollector(B, lambda o: None, 8, value_input="both")
    for e in (A, P, B):
        e.close()


# ---- 8. the collector ----------------------------------------------------------------------------------------------------
def _policy(n):
    g = torch.Generator(device="cpu").manual_seed(3)
    W = (0.05 * torch.randn((13, 4), generator=g)).to(DEV)
    Wv = (0.1 * torch.randn((13,), generator=g)).to(DEV)

    def policy(obs):
        x = torch.nan_to_num(obs).clamp(-5, 5)
        return 0.0922 + 0.01 * torch.tanh(x @ W), x @ Wv, -(x * x).sum(dim=1)
    return policy


def _critic():
    g = torch.Generator(device="cpu").manual_seed(4)
    W1, W2 = (0.2 * torch.randn((52, 32), generator=g)).to(DEV), (0.2 * torch.randn((32,), generator=g)).to(DEV)
    return lambda rows: torch.tanh(rows * 0.01 @ W1) @ W2


def test_collector_values_come_from_the_privileged_rows():
    pkg = _pkg()
    from drl_dronenavigation_amd.collector import RolloutCollector
    n, T, gamma = 1024, 48, 0.99
    kw = dict(max_steps=40, normalize_obs=True, **NOISE)
    A, R = _env(pkg, n, **kw), _env(pkg, n, **kw)
    value_fn = _critic()
    col = RolloutCollector(A, _policy(n), T, value_fn=value_fn, value_input="privileged", gamma=gamma)
    first = R.reset_tensor()
    assert torch.equal(col._last_obs, first)
    priv = R.privileged.clone()
    seen = Seen()
    for rollout in range(2):                                              # the second rollout starts mid-episode
        buf = col.collect()
        assert tuple(buf["privileged"].shape) == (T, n, 52)
        trunc = 0
        for t in range(T):
            assert torch.equal(buf["privileged"][t], priv), (rollout, t)
            assert torch.equal(buf["values"][t], value_fn(priv).reshape(-1)), (rollout, t)
            _, reward, done, info = R.step_tensor(buf["actions"][t].clamp(-1.0, 1.0))
            rows = torch.where(done.bool()[:, None], info["terminal_privileged"], info["privileged"])
            want = reward + gamma * value_fn(rows).reshape(-1) * info["truncated"].to(reward.dtype)
            assert torch.equal(buf["rewards"][t], want), (rollout, t)
            # the bootstrap reads the TERMINAL rows: the finished episode's parameters, not the new draws
            m = info["truncated"].bool()
            if bool(m.any()):
                assert torch.equal(info["terminal_privileged"][m][:, 35], info["ep_length"][m].float()) and not bool(info["privileged"][m][:, 35].any())
                assert not torch.equal(info["terminal_privileged"][m][:, 16:20], info["privileged"][m][:, 16:20])
            trunc += int(m.sum())
            seen.step(done, info)
            priv = info["privileged"].clone()
        assert torch.equal(buf["last_values"], value_fn(priv).reshape(-1))
        assert trunc > 0, "no truncation: the bootstrap was not exercised"
    seen.check(fused=False)
    A.close()
    R.close()


def test_collector_on_observations_is_unchanged_by_the_feature():
    pkg = _pkg()
    from drl_dronenavigation_amd.collector import RolloutCollector
    n, T = 1024, 48
    kw = dict(max_steps=40, normalize_obs=True, **NOISE)
    A, P = _env(pkg, n, **kw), _env(pkg, n, priv=False, **kw)
    ca, cp = RolloutCollector(A, _policy(n), T), RolloutCollector(P, _policy(n), T)
    seen = Seen()
    for rollout in range(2):
        ba, bp = ca.collect(), cp.collect()
        assert set(ba) == set(bp)
        # the ends of this rollout's steps (episode_starts[0] belongs to the step before it), the latencies of the fleet after it
        seen.ends += int(bp["episode_starts"][1:].sum()) + int(bp["last_dones"].sum())
        seen.act_lat.update(np.unique(P.get_actuator()["latency"].cpu().numpy()).astype(int).tolist())
        seen.sens_lat.update(np.unique(P.get_sensor()["latency"].cpu().numpy()).astype(int).tolist())
        for k in bp:
            assert torch.equal(ba[k].view(torch.int32) if ba[k].dtype == torch.float32 else ba[k],
                               bp[k].view(torch.int32) if bp[k].dtype == torch.float32 else bp[k]), (k, rollout)
    seen.check(fused=False)
    _same_state(A.get_state(), P.get_state())
    A.close()
    P.close()
