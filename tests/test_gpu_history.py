"""History rows (include/dronenav.h dn_stack_history, csrc/dn_history.hip) on the HIP path.  Every comparison of rows is exact, on the
int32 views: the kernel only copies words.

 1. synthetic inputs (random bit patterns) against the NumPy loop of tests/history_support.py: six configurations, fleets around the
    tile edges, launches shorter and longer than the stack, six done fields; terminal rows only where done, stores end at the fleet;
 2. NULL inputs equal explicit zeros; `prev` aliased to `rows`; K steps in one launch = K chained calls; two halves = the whole;
 3. through DroneVecEnv: env.history / info["history"] / rollout_tensor against the reference applied to the env's own outputs, goal
    columns, nothing else changes (outputs, state, kernel shape), hipGraph replay;
 4. RolloutCollector(policy_input="history") with a torch policy and with FusedMlpPolicy at W = 64, eager and graph-replayed, and the
    collector on plain observations unchanged by the option."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import history_support as H  # noqa: E402
import mlp_support as S  # noqa: E402
from gpu_support import DEV, _acts, _same_state  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402
from model_support import NOISE  # noqa: E402
from test_gpu_mlp_wide import ABS_BARS  # noqa: E402

PATTERN = 0x7FC12345                    # a quiet NaN nothing here produces
WP = np.array([[0.0, 1.0, 0.6], [-1.0, 0.0, 1.0], [0.0, -1.0, 0.6]])
SPAWN = np.array([[1.0, 0.0, 0.5]])
DIM = [-2.0, -2.0, 0.0, 2.0, 2.0, 2.0]
SHAPES = [(1, n) for n in (1, 63, 64, 65, 191)] + [(k, n) for k in (2, 5, 7) for n in (4, 64, 68, 192)]


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _stack(pkg, cfg, K, N, prev, obs, actions, done, terminal_obs, extra, terminal_extra, rows, terminal_rows):
    """dn_stack_history on device tensors (or None)."""
    K_ = pkg._capi
    ptr = [None if x is None else x.data_ptr() for x in (prev, obs, actions, done, terminal_obs, extra, terminal_extra, rows, terminal_rows)]
    K_.check(K_.load().dn_stack_history(C.byref(K_.DnHistoryConfig(*cfg, 0)), K, N, *ptr, 0,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def _inputs(rng, cfg, K, N):
    E, W = cfg[2], H.width(*cfg)
    d = dict(prev=H.random_words(rng, (N, W)), obs=H.random_words(rng, (K, N, 13)), actions=H.random_words(rng, (K, N, 4)),
             terminal_obs=H.random_words(rng, (K, N, 13)))
    d["extra"] = H.random_words(rng, (K, N, E)) if E else None
    d["terminal_extra"] = H.random_words(rng, (K, N, E)) if E else None
    return d


def _same(got, want, tag):
    a, b = H.bits(got), H.bits(want)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError((tag, len(bad), bad[:5].tolist(), hex(a[tuple(bad[0])] & 0xFFFFFFFF), hex(b[tuple(bad[0])] & 0xFFFFFFFF)))


def _run(pkg, cfg, K, N, inp, done, *, prev=True, actions=True, extra=True, terminal=True):
    """One launch into sentinel-filled buffers with one guard row in front of the first slice and one behind the last.
    Returns (rows [K, N, W], terminal_rows [K, N, W] or None) as numpy, after checking the guards."""
    W = H.width(*cfg)
    g = lambda name, on=True: _dev(inp[name]) if on and inp[name] is not None else None      # noqa: E731
    bufs = []
    for _ in range(2 if terminal else 1):
        b = torch.empty((K * N + 2, W), dtype=torch.float32, device=DEV)
        b.view(torch.int32).fill_(PATTERN)
        bufs.append(b)
    rows = bufs[0][1:-1]
    trows = bufs[1][1:-1] if terminal else None
    _stack(pkg, cfg, K, N, g("prev", prev), g("obs"), g("actions", actions), _dev(done), g("terminal_obs", terminal), g("extra", extra),
           g("terminal_extra", extra and terminal), rows, trows)
    torch.cuda.synchronize()
    for b in bufs:
        guard = b.view(torch.int32)[[0, -1]]
        assert bool((guard == PATTERN).all()), "a store left the fleet's rows"
    out = [b[1:-1].cpu().numpy().reshape(K, N, W) for b in bufs]
    return out[0], (out[1] if terminal else None)


@pytest.mark.parametrize("cfg", H.CONFIGS, ids=lambda c: "F%dA%dE%d" % c)
def test_synthetic_inputs_match_the_reference(cfg):
    """The guard rows: the step slices of a launch are contiguous, so the rows that belong to no slice are the one in front of slice 0
    and the one behind slice K - 1 (for K = 1 that is the (N + 1)-row buffer); both keep their sentinel."""
    pkg = _pkg()
    used = 13 * cfg[0] + 4 * cfg[1] + cfg[2]
    rng = np.random.default_rng(1000 + 100 * cfg[0] + 10 * cfg[1] + cfg[2])
    ends = 0
    for K, N in SHAPES:
        inp = _inputs(rng, cfg, K, N)
        for name, done in H.done_patterns(rng, K, N).items():
            want, want_t = H.stack_reference(cfg, inp["prev"], inp["obs"], inp["actions"], done, inp["terminal_obs"], inp["extra"],
                                             inp["terminal_extra"])
            got, got_t = _run(pkg, cfg, K, N, inp, done)
            tag = (cfg, K, N, name)
            _same(got, want, tag + ("rows",))
            assert not H.bits(got[..., used:]).any(), tag + ("padding",)
            m = done.astype(bool)
            _same(got_t[m], want_t[m], tag + ("terminal rows",))
            assert (H.bits(got_t[~m]) == PATTERN).all(), tag + ("a terminal row was written where no episode ended",)
            ends += int(m.sum())
            # without a terminal buffer the rows are the same
            got2, _ = _run(pkg, cfg, K, N, inp, done, terminal=False)
            _same(got2, want, tag + ("rows without terminal",))
    assert ends > 1000


@pytest.mark.parametrize("cfg", [(4, 3, 0), (3, 2, 8)], ids=lambda c: "F%dA%dE%d" % c)
def test_null_inputs_equal_explicit_zeros(cfg):
    pkg = _pkg()
    rng = np.random.default_rng(7)
    for K, N in ((1, 65), (5, 68)):
        inp = _inputs(rng, cfg, K, N)
        done = (rng.random((K, N)) < 0.3).astype(np.uint8)
        zero = lambda name: dict(inp, **{name: np.zeros_like(inp[name])})      # noqa: E731
        for name, kw in (("prev", dict(prev=False)), ("actions", dict(actions=False)), ("extra", dict(extra=False))):
            if inp[name] is None:
                continue
            d = None if name == "actions" else done                # the ABI refuses done without actions: the reset call ends no episode
            got = _run(pkg, cfg, K, N, inp, d, **kw)
            want = _run(pkg, cfg, K, N, dict(zero(name), **({"terminal_extra": np.zeros_like(inp["terminal_extra"])} if name == "extra" else {})),
                        np.zeros((K, N), np.uint8) if d is None else d)
            _same(got[0], want[0], (cfg, K, N, name, "rows"))
            m = (np.zeros((K, N), bool) if d is None else d.astype(bool))
            _same(got[1][m], want[1][m], (cfg, K, N, name, "terminal"))
        got = _run(pkg, cfg, K, N, inp, None)
        want = _run(pkg, cfg, K, N, inp, np.zeros((K, N), np.uint8))
        _same(got[0], want[0], (cfg, K, N, "done", "rows"))
        assert (H.bits(got[1]) == PATTERN).all()


@pytest.mark.parametrize("cfg", [(4, 3, 0), (3, 2, 8), (1, 0, 0)], ids=lambda c: "F%dA%dE%d" % c)
def test_in_place(cfg):
    """`prev` aliased to `rows` (K = 1) and to the last slot of `rows` (the env's own use after a K-step launch) gives the bits of a
    separate `prev`."""
    pkg = _pkg()
    rng = np.random.default_rng(11)
    W = H.width(*cfg)
    for K, N in ((1, 191), (1, 64), (5, 192), (2, 68)):
        inp = _inputs(rng, cfg, K, N)
        done = (rng.random((K, N)) < 0.3).astype(np.uint8)
        want, want_t = _run(pkg, cfg, K, N, inp, done)
        rows = torch.zeros((K, N, W), dtype=torch.float32, device=DEV)
        trows = torch.zeros((K, N, W), dtype=torch.float32, device=DEV)
        rows[K - 1].copy_(_dev(inp["prev"]))
        _stack(pkg, cfg, K, N, rows[K - 1], _dev(inp["obs"]), _dev(inp["actions"]), _dev(done), _dev(inp["terminal_obs"]), _dev(inp["extra"]),
               _dev(inp["terminal_extra"]), rows, trows)
        _same(rows.cpu().numpy(), want, (cfg, K, N, "rows"))
        m = done.astype(bool)
        _same(trows.cpu().numpy()[m], want_t[m], (cfg, K, N, "terminal"))


@pytest.mark.parametrize("K", [5, 20])
def test_one_launch_equals_chained_single_steps(K):
    pkg = _pkg()
    rng = np.random.default_rng(K)
    for cfg in ((4, 3, 0), (3, 2, 8)):
        N, W = 68, H.width(*cfg)
        inp = _inputs(rng, cfg, K, N)
        done = (rng.random((K, N)) < 0.3).astype(np.uint8)
        want, want_t = _run(pkg, cfg, K, N, inp, done)
        prev = inp["prev"]
        for t in range(K):
            one = {k: (v if v is None or k == "prev" else v[t:t + 1]) for k, v in inp.items()}
            one["prev"] = prev
            got, got_t = _run(pkg, cfg, 1, N, one, done[t:t + 1])
            _same(got[0], want[t], (cfg, K, t, "rows"))
            m = done[t].astype(bool)
            _same(got_t[0][m], want_t[t][m], (cfg, K, t, "terminal"))
            prev = got[0]
        assert prev.shape == (N, W)


def test_two_halves_equal_the_whole():
    pkg = _pkg()
    rng = np.random.default_rng(3)
    cfg, K, N = (3, 2, 8), 5, 128
    inp = _inputs(rng, cfg, K, N)
    done = (rng.random((K, N)) < 0.3).astype(np.uint8)
    want, want_t = _run(pkg, cfg, K, N, inp, done)
    for lo in (0, 64):
        half = {k: (None if v is None else v[lo:lo + 64] if k == "prev" else v[:, lo:lo + 64]) for k, v in inp.items()}
        got, got_t = _run(pkg, cfg, K, 64, half, done[:, lo:lo + 64])
        _same(got, want[:, lo:lo + 64], (lo, "rows"))
        m = done[:, lo:lo + 64].astype(bool)
        _same(got_t[m], want_t[:, lo:lo + 64][m], (lo, "terminal"))


# ---- through the env ---------------------------------------------------------------------------------------------------------------------
def _env(pkg, n, history, goal=False, **kw):
    opts = dict(target_points=WP, initial_xyzs=SPAWN, aviary_dim=DIM, circle=False, cylinder=False, max_steps=15, seed=17, device=DEV,
                normalize_obs=True, **NOISE)
    opts.update(kw)
    if goal:
        opts["goal"] = pkg.GoalObservation(frame="body")
    if history is not None:
        opts["history"] = history
    return pkg.DroneVecEnv(None, n, **opts)


def _spread(envs, rng):
    """Episode step counters over [0, 15): the time limit ends episodes at different steps, inside launches too."""
    steps = rng.integers(0, 15, envs[0].num_envs)
    for e in envs:
        st = e.get_state()
        st["steps"] = steps.astype(st["steps"].dtype)
        e.set_state(st)


@pytest.mark.parametrize("goal", [False, True], ids=["plain", "goal"])
def test_env_history_matches_the_reference_and_changes_nothing_else(goal):
    pkg = _pkg()
    n = 192
    hist = pkg.HistoryObservation(frames=3, actions=2, goal=goal)
    cfg = (3, 2, 8 if goal else 0)
    W = H.width(*cfg)
    used = 39 + 8
    A, B = _env(pkg, n, hist, goal), _env(pkg, n, None, goal)           # with and without the option
    assert tuple(A.reset_tensor().shape) == (n, 13) and B.history is None
    B.reset_tensor()
    assert tuple(A.history.shape) == (n, W)
    rng = np.random.default_rng(23)
    _spread((A, B), rng)
    x0 = A.goal.cpu().numpy()[None] if goal else None
    prev, _ = H.stack_reference(cfg, None, A._obs.cpu().numpy()[None], None, None, None, x0, None)
    prev = prev[0]
    _same(A.history.cpu().numpy(), prev, "reset")
    ends = 0
    for t in range(40):
        a = _acts(rng, n, 1)[0]
        want_terminal = t % 4 != 3
        oa, ra, da, ia = A.step_tensor(a, want_terminal=want_terminal)
        ob, rb, db, ib = B.step_tensor(a, want_terminal=want_terminal)
        assert ia["history"] is A.history
        for k in ib:
            if torch.is_tensor(ib[k]):
                assert torch.equal(ia[k].view(torch.uint8) if ia[k].dtype.is_floating_point else ia[k],
                                   ib[k].view(torch.uint8) if ib[k].dtype.is_floating_point else ib[k]), (t, k)
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)) and torch.equal(ra.view(torch.int32), rb.view(torch.int32))
        assert torch.equal(da, db)
        done = da.cpu().numpy()[None]
        x = ia["goal"].cpu().numpy()[None] if goal else None
        xt = ia["terminal_goal"].cpu().numpy()[None] if goal and want_terminal else None
        want, want_t = H.stack_reference(cfg, prev, A._obs.cpu().numpy()[None], a.cpu().numpy()[None], done,
                                         ia["terminal_obs"].cpu().numpy()[None] if want_terminal else None, x, xt)
        _same(A.history.cpu().numpy(), want[0], (t, "rows"))
        m = done[0].astype(bool)
        if want_terminal:
            _same(ia["terminal_history"].cpu().numpy()[m], want_t[0][m], (t, "terminal"))
        else:
            assert ia["terminal_history"] is None
        if goal:
            _same(A.history.cpu().numpy()[:, used:used + 8], ia["goal"].cpu().numpy(), (t, "goal columns"))
            if want_terminal:
                _same(ia["terminal_history"].cpu().numpy()[m][:, used:used + 8], ia["terminal_goal"].cpu().numpy()[m], (t, "terminal goal"))
        prev = want[0]
        ends += int(m.sum())
    assert ends > n
    # fused launches: three in a row, terminal rows on and off, the dict passed back
    for want_terminal in (True, False):
        outs = [None, None]
        inside = 0
        for launch in range(3):
            acts = _acts(rng, n, 20)
            for j, e in enumerate((A, B)):
                outs[j] = e.rollout_tensor(acts, out=outs[j], want_terminal=want_terminal)
            ra, rb = outs
            for k in rb:
                assert torch.equal(ra[k].view(torch.uint8) if ra[k].dtype.is_floating_point else ra[k],
                                   rb[k].view(torch.uint8) if rb[k].dtype.is_floating_point else rb[k]), (launch, k)
            assert ("terminal_history" in ra) == want_terminal and tuple(ra["history"].shape) == (20, n, W)
            g = lambda k: ra[k].cpu().numpy() if k in ra else None      # noqa: E731
            want, want_t = H.stack_reference(cfg, prev, g("obs"), acts.cpu().numpy(), g("done"), g("terminal_obs"),
                                             g("goal") if goal else None, g("terminal_goal") if goal else None)
            _same(g("history"), want, (launch, want_terminal, "rows"))
            _same(A.history.cpu().numpy(), want[-1], (launch, want_terminal, "env.history"))
            m = g("done").astype(bool)
            if want_terminal:
                _same(g("terminal_history")[m], want_t[m], (launch, "terminal"))
            inside += int(m[:-1].sum())
            prev = want[-1]
        assert inside > n
    _same_state(A.get_state(), B.get_state())
    with pytest.raises(ValueError, match="history"):
        A.rollout_tensor(_acts(rng, n, 2), out={k: v for k, v in outs[0].items() if k != "history"})
    A.close()
    B.close()


def test_option_needs_its_goal_env_and_leaves_the_kernel_shape_alone():
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    with pytest.raises(ValueError, match="GoalObservation"):
        _env(pkg, 64, pkg.HistoryObservation(goal=True), goal=False)
    with pytest.raises(TypeError, match="HistoryObservation"):
        _env(pkg, 64, (3, 2))
    n = 32768
    shapes = []
    for hist in (None, pkg.HistoryObservation(frames=4, actions=3)):
        kw = {} if hist is None else dict(history=hist)
        env = pkg.DroneVecEnv(tracks.circle(1, 4, 1), n, device=DEV, **kw)
        env.reset_tensor()
        a = torch.zeros((2, n, 4), dtype=torch.float32, device=DEV)
        env.step_tensor(a[0])
        env.rollout_tensor(a)
        torch.cuda.synchronize()
        shapes.append((env.kernel_waves(False), env.kernel_waves(True)))
        env.close()
    assert shapes[0] == shapes[1] and min(shapes[0]) > 1, shapes


def test_captured_graph_matches_eager_steps():
    pkg = _pkg()
    n = 192
    hist = pkg.HistoryObservation(frames=4, actions=3)
    Gr, E = _env(pkg, n, hist), _env(pkg, n, hist)
    Gr.reset_tensor()
    E.reset_tensor()
    rng = np.random.default_rng(5)
    _spread((Gr, E), rng)
    static = torch.zeros((n, 4), dtype=torch.float32, device=DEV)
    for _ in range(3):                                                    # warm-up, eager
        a = _acts(rng, n, 1)[0]
        static.copy_(a)
        Gr.step_tensor(static)
        E.step_tensor(a)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    a = _acts(rng, n, 1)[0]
    static.copy_(a)
    with torch.cuda.graph(graph):
        Gr.step_tensor(static)
    graph.replay()
    E.step_tensor(a)
    ends = 0
    for t in range(20):
        a = _acts(rng, n, 1)[0]
        static.copy_(a)
        Gr._term_hist.view(torch.int32).fill_(PATTERN)
        graph.replay()
        _, _, done, info = E.step_tensor(a)
        m = done.bool()
        assert torch.equal(Gr.history.view(torch.int32), info["history"].view(torch.int32)), t
        assert torch.equal(Gr._term_hist.view(torch.int32)[m], info["terminal_history"].view(torch.int32)[m]), t
        assert bool((Gr._term_hist.view(torch.int32)[~m] == PATTERN).all())
        ends += int(m.sum())
    assert ends > 0
    _same_state(Gr.get_state(), E.get_state())
    Gr.close()
    E.close()


# ---- the collector -----------------------------------------------------------------------------------------------------------------------
def _hover(net):
    with torch.no_grad():
        net.action_net.bias.fill_(0.0922)                                       # hover: flights last until the time limit
    return net


def _reference_buffer_rows(cfg, buf):
    """buf["history"] from buf["obs"], the episode-start flags and the clipped actions: slot 0 is a fresh stack (the first rollout after
    the reset), slot t + 1 follows from slot t by the step rule (terminal rows are not part of the buffer)."""
    obs, acts = buf["obs"].cpu().numpy(), buf["actions"].clamp(-1.0, 1.0).cpu().numpy()
    starts = buf["episode_starts"].cpu().numpy()
    first, _ = H.stack_reference(cfg, None, obs[:1], None, None, None, None, None)
    rest, _ = H.stack_reference(cfg, first[0], obs[1:], acts[:-1], starts[1:], None, None, None)
    return np.concatenate((first, rest))


def test_collector_feeds_the_policy_the_history_rows():
    pkg = _pkg()
    from drl_dronenavigation_amd.collector import FusedRolloutCollector, OffPolicyCollector, RolloutCollector
    n, T, dev, gamma = 192, 20, torch.device(DEV), 0.99
    hist = pkg.HistoryObservation(frames=3, actions=2)
    W = hist.width()
    torch.manual_seed(3)
    net = _hover(pkg.MlpActorCritic(obs_dim=W).to(dev))
    with pytest.raises(ValueError, match="needs an env built with history"):
        e = _env(pkg, n, None)
        try:
            RolloutCollector(e, net, T, policy_input="history")
        finally:
            e.close()
    env = _env(pkg, n, hist)
    for refuse in (lambda: FusedRolloutCollector(env, None, T), lambda: OffPolicyCollector(env, None, T)):
        with pytest.raises(ValueError, match="does not carry history rows"):
            refuse()
    calls = []

    def policy(x):
        calls.append(x.clone())
        return net(x, deterministic=True)

    with torch.no_grad():
        buf = RolloutCollector(env, policy, T, value_fn=net.predict_values, gamma=gamma, policy_input="history").collect()
        assert tuple(buf["history"].shape) == (T, n, W) and tuple(buf["obs"].shape) == (T, n, 13) and len(calls) == T
        for t in range(T):
            assert torch.equal(calls[t].view(torch.int32), buf["history"][t].view(torch.int32)), t
        _same(buf["history"].cpu().numpy(), _reference_buffer_rows((3, 2, 0), buf), "buffer rows")
        # the bootstrap: a twin env flown with the buffer's clipped actions gives the terminal rows and the truncation flags
        twin = _env(pkg, n, hist)
        twin.reset_tensor()
        truncated = 0
        for t in range(T):
            _, reward, done, info = twin.step_tensor(buf["actions"][t].clamp(-1.0, 1.0))
            seen = torch.where(done.bool()[:, None], info["terminal_history"], info["history"])
            want = reward + gamma * net.predict_values(seen) * info["truncated"].to(reward.dtype)
            assert torch.equal(buf["rewards"][t], want), t
            tr = info["truncated"].bool()
            boot = (buf["rewards"][t] - reward)[tr]
            assert torch.equal(boot, ((reward + gamma * net.predict_values(info["terminal_history"]))[tr] - reward[tr])), t
            truncated += int(tr.sum())
        assert truncated > 0
        twin.close()
    env.close()


def test_collector_runs_the_fused_policy_on_full_width_rows():
    """FusedMlpPolicy at W = 64 in the float32 grade against the torch network on the same rows: the bar tests/test_gpu_mlp_wide.py holds
    that grade to (ABS_BARS["fp32"]: action mean, value).  Then a replayed hipGraph of the rollout against an eager twin."""
    pkg = _pkg()
    from drl_dronenavigation_amd import policy_mfma as pm
    from drl_dronenavigation_amd.collector import RolloutCollector
    n, T, dev = 256, 4, torch.device(DEV)
    hist = pkg.HistoryObservation(frames=4, actions=3)
    assert hist.width() == 64
    net = _hover(S.perturbed_net(pkg, 64, 564, dev))
    runs = []
    for use_graph in (False, True):
        env = _env(pkg, n, hist, max_steps=4, normalize_obs=False)   # inputs in [-1, 1], the range the bar was set on
        pol = pm.FusedMlpPolicy(net, n, dev, grade="fp32")
        col = RolloutCollector(env, lambda x, pol=pol: pol(x, deterministic=True), T, policy_input="history", use_graph=use_graph)
        for _ in range(3):
            out = col.collect()
        torch.cuda.synchronize()
        assert (col._graph is not None) == use_graph
        runs.append({k: v.clone() for k, v in out.items()})
        env.close()
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    buf = runs[0]
    assert float(buf["rewards"].abs().sum()) > 0 and int(buf["episode_starts"].sum()) > 0
    with torch.no_grad():
        for t in range(T):
            mean, value, _ = net(buf["history"][t], deterministic=True)
            e_pi, e_vf = float((buf["actions"][t] - mean).abs().max()), float((buf["values"][t] - value).abs().max())
            print(f"t={t}: max |err| action mean {e_pi:.3e} value {e_vf:.3e}; bars {ABS_BARS['fp32']}")
            assert e_pi <= ABS_BARS["fp32"][0] and e_vf <= ABS_BARS["fp32"][1], (t, e_pi, e_vf)


def test_collector_on_plain_observations_is_unchanged_by_the_option():
    pkg = _pkg()
    from drl_dronenavigation_amd.collector import RolloutCollector
    n, T, dev = 192, 20, torch.device(DEV)
    torch.manual_seed(5)
    net = _hover(pkg.MlpActorCritic(obs_dim=13).to(dev))
    runs = []
    with torch.no_grad():
        for hist in (None, pkg.HistoryObservation()):
            env = _env(pkg, n, hist)
            out = RolloutCollector(env, lambda x: net(x, deterministic=True), T).collect()
            assert "history" not in out
            runs.append({k: v.clone() for k, v in out.items()})
            env.close()
    for k in runs[0]:
        assert torch.equal(runs[0][k].view(torch.uint8), runs[1][k].view(torch.uint8)), k
    assert int(runs[0]["episode_starts"][1:].sum()) > 0
