"""Every extra row family at once (privileged rows, goal rows, history rows and the track of each drone) on the HIP path.  The other GPU
files build an env with one or two of them; here env `A` has all four, and four twins have one family each -- the history twin also has
the goal rows its rows end with.  All five fly the same bank, sensor model, seed and actions: the bank and the sensor decide the flights,
the rows feed nothing back, so every output of `A` equals every twin's and each family's rows equal the matching twin's, bit for bit
(int32 views).  The "track" twin is the bank alone.

 1. reset_tensor and 12 step_tensor calls, want_terminal on the even steps: the terminal rows where done, None in `info` without;
 2. rollout_tensor with K = 5 (a fresh `out` with terminal rows, the same `out` again, one single step after it, a fresh `out` without
    terminal rows): the K-step buffers, the env's current rows = the last slot, the caller's buffers no longer bound afterwards;
 3. RolloutCollector(value_input="privileged", policy_input="history") over two rollouts against a twin env driven by hand.

N = 65 is one full tile and a tail of one drone; dn_step_many takes whole groups of four drones only (it refuses num_envs % 4 != 0), so
the K-step drive flies N_MANY = 68, the shortest tail it accepts.  max_steps = 5 puts the first time limit on step 4, which asks for
terminal rows, and the second on step 9, which does not; the bank's short tracks and the mixed actions end episodes in between."""
import functools

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import track_support as S  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402
from model_support import AMPS  # noqa: E402

N, N_MANY, MAX_STEPS, STEPS, K, T = 65, 68, 5, 12, 5, 8
ROWS = ("privileged", "goal", "history")                # the row families; the fourth, "track", is two int32 vectors
OUTPUTS = ("obs", "reward", "done", "truncated")


def _family_kw(pkg):
    goal = pkg.GoalObservation("body")
    return {"privileged": dict(privileged=pkg.PrivilegedObservation()), "goal": dict(goal=goal),
            "history": dict(goal=goal, history=pkg.HistoryObservation(frames=3, actions=2, goal=True)), "track": {}}


def _env(pkg, n, *families):
    kw = {}
    for f in families:
        kw.update(_family_kw(pkg)[f])
    return S.bank_env(pkg, n, max_steps=MAX_STEPS, sensor=pkg.SensorModel(latency=(0, 8), bias=AMPS), **kw)


def _envs(pkg, n):
    """`A` and its four twins, by the family the twin has."""
    return _env(pkg, n, *_family_kw(pkg)), {f: _env(pkg, n, f) for f in _family_kw(pkg)}


def _current(env):
    """The env's current rows by their info key."""
    rows = {k: getattr(env, k) for k in ROWS}
    rows["track"] = env.track_ids
    return {k: v.clone() for k, v in rows.items() if v is not None}


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(got, want, tag, where=None):
    a, b = _bits(got), _bits(want)
    assert a.shape == b.shape and a.dtype == b.dtype, (tag, a.shape, b.shape, a.dtype, b.dtype)
    ne = a != b
    if where is not None:
        ne = ne & (where.bool()[..., None] if ne.dim() > where.dim() else where.bool())
    assert not bool(ne.any()), (tag, int(ne.sum()), ne.nonzero()[:4].tolist())


def _same_record(a, twin, keys, tag):
    """The outputs, and `keys` of the twin's record: terminal rows where done, the rest everywhere."""
    for k in OUTPUTS + tuple(keys):
        if k not in twin:
            assert k not in a, (tag, k)
            continue
        rows_where_done = k.startswith("terminal_") and k != "terminal_track"
        _same(a[k], twin[k], (tag, k), where=a["done"] if rows_where_done else None)


def _keys(family):
    return (family, "terminal_" + family)


def _step_log(env, acts):
    """Reset, then one step_tensor per action batch with want_terminal on the even steps: one record per call."""
    log = [dict(obs=env.reset_tensor().clone(), **_current(env))]
    for t, a in enumerate(acts):
        want = t % 2 == 0
        obs, reward, done, info = env.step_tensor(a, want_terminal=want)
        for k in ROWS:
            if getattr(env, k) is None:
                assert k not in info and "terminal_" + k not in info, (t, k)
            else:
                assert info[k] is getattr(env, k) and (info["terminal_" + k] is None) == (not want), (t, k)
        assert info["track"] is env.track_ids and info["terminal_track"] is not None, t     # the finished tracks come with every step
        rec = dict(info, obs=obs, reward=reward, done=done)
        log.append({k: v.clone() for k, v in rec.items() if v is not None})
    return log


def _launch_log(env, acts):
    """From a fresh reset: rollout_tensor into a fresh `out` with terminal rows, into the same `out` again, one step_tensor, and
    rollout_tensor into a fresh `out` without terminal rows.  One record per call."""
    log = [dict(obs=env.reset_tensor().clone(), **_current(env))]
    out = None
    for j in range(2):
        got = env.rollout_tensor(acts[j * K:(j + 1) * K], out=out, want_terminal=j == 0)
        assert out is None or got is out, j
        out = got
        log.append({k: v.clone() for k, v in out.items()})
        _last_slot_is_current(env, out, j)
    kept = {k: out[k].clone() for k in ROWS if k in out}
    obs, reward, done, info = env.step_tensor(acts[2 * K])
    log.append({k: v.clone() for k, v in dict(info, obs=obs, reward=reward, done=done).items()})
    for k, v in kept.items():                                   # the single step wrote the env's rows, not the caller's
        _same(out[k], v, ("still bound after the launch", k))
    out = env.rollout_tensor(acts[2 * K + 1:], want_terminal=False)
    for k in ROWS:
        assert (k in out) == (getattr(env, k) is not None) and "terminal_" + k not in out, k
    log.append({k: v.clone() for k, v in out.items()})
    _last_slot_is_current(env, out, 2)
    return log


def _last_slot_is_current(env, out, tag):
    if env.privileged is not None:
        cols = env.privileged_obs.columns()
        _same(env.privileged[:, cols], out["privileged"][K - 1][:, cols], (tag, "env.privileged"))
    if env.goal is not None:
        _same(env.goal, out["goal"][K - 1], (tag, "env.goal"))
    if env.history is not None:
        _same(env.history, out["history"][K - 1], (tag, "env.history"))


@functools.lru_cache(maxsize=None)
def _logs():
    """Both drives on all five envs, once for the file: (step logs, launch logs), each `A`'s and then the twins' by family."""
    pkg = _pkg()
    logs = []
    for n, drive, acts in ((N, _step_log, S.action_stream(N, STEPS, seed=11)), (N_MANY, _launch_log, S.action_stream(N_MANY, 3 * K + 1, seed=12))):
        a, twins = _envs(pkg, n)
        logs.append((drive(a, acts), {f: drive(e, acts) for f, e in twins.items()}))
        for e in (a, *twins.values()):
            e.close()
    return logs


def test_single_steps_with_every_family_equal_each_family_alone():
    mine, twins = _logs()[0]
    done = torch.stack([r["done"] for r in mine[1:]]).bool()
    asked = torch.arange(STEPS, device=done.device) % 2 == 0
    assert bool(done[asked].any()) and bool(done[~asked].any()), "episodes must end on steps with and without terminal rows"
    assert bool((~done).any(dim=1).any()), "some step must leave a drone in flight"
    assert not torch.equal(mine[1]["privileged"][:, :13], mine[1]["obs"]), "the sensor model must part the true observation from the delivered one"
    for f, log in twins.items():
        assert set(log[0]) == {"obs", "track", f}.union({"goal"} if f == "history" else ()), (f, sorted(log[0]))
        _same(mine[0]["obs"], log[0]["obs"], (f, "reset", "obs"))
        _same(mine[0][f], log[0][f], (f, "reset", f))
        for t, (a, b) in enumerate(zip(mine[1:], log[1:])):
            assert ("terminal_" + f in b) == (t % 2 == 0 or f == "track"), (f, t)
            _same_record(a, b, _keys(f), (f, t))


def test_k_step_launches_with_every_family_equal_each_family_alone():
    mine, twins = _logs()[1]
    assert bool(mine[1]["done"].any()) and not bool(mine[1]["done"].all())
    for f, log in twins.items():
        _same(mine[0][f], log[0][f], (f, "reset", f))
        for j, (a, b) in enumerate(zip(mine[1:], log[1:])):
            assert f in b and ("terminal_" + f in b) == (j < 3 or f == "track"), (f, j, sorted(b))
            _same_record(a, b, _keys(f), (f, "call", j))


def test_collector_carries_every_family_it_is_asked_for():
    """RolloutCollector on an env like `A`: the buffer's rows are those of a twin env flown by hand with the buffer's actions, the policy
    is shown the history rows and the value function the privileged rows (of the step, of the truncation bootstrap, of the last values),
    and a second collect() goes on from the carried rows."""
    pkg = _pkg()
    from drl_dronenavigation_amd.collector import RolloutCollector
    env, twin = _env(pkg, N, *_family_kw(pkg)), _env(pkg, N, *_family_kw(pkg))
    stream = S.action_stream(N, 2 * T, seed=13)
    shown, valued = [], []

    def policy(x):
        shown.append(x.clone())
        return stream[len(shown) - 1], torch.zeros(N, device=x.device), torch.zeros(N, device=x.device)

    def value_fn(x):
        valued.append(x.clone())
        return torch.zeros(N, device=x.device)

    col = RolloutCollector(env, policy, T, value_fn=value_fn, value_input="privileged", policy_input="history", bootstrap_truncated=True)
    cur = dict(obs=twin.reset_tensor().clone(), **_current(twin))
    ends = 0
    for rollout in range(2):
        buf = {k: v.clone() for k, v in col.collect().items()}
        assert "goal" not in buf and buf["track"].dtype == torch.int32
        assert len(shown) == T * (rollout + 1) and len(valued) == (2 * T + 1) * (rollout + 1)
        calls, seen = valued[(2 * T + 1) * rollout:], shown[T * rollout:]
        for t in range(T):
            tag = (rollout, t)
            for k in ("obs", "privileged", "history", "track"):
                _same(buf[k][t], cur[k], tag + (k,))
            _same(seen[t], cur["history"], tag + ("policy input",))
            _same(calls[2 * t], cur["privileged"], tag + ("value input",))
            obs, reward, done, info = twin.step_tensor(buf["actions"][t].clamp(-1.0, 1.0))
            _same(calls[2 * t + 1], torch.where(done.bool()[:, None], info["terminal_privileged"], info["privileged"]), tag + ("bootstrap input",))
            assert torch.equal(buf["rewards"][t], reward), tag          # the value function answers 0: the bootstrap adds nothing
            ends += int(done.sum())
            cur = dict(obs=obs.clone(), **_current(twin))
        _same(calls[2 * T], cur["privileged"], (rollout, "last values input"))
        _same(col._last_obs, cur["obs"], (rollout, "carried obs"))
    assert ends > 0
    env.close()
    twin.close()
