"""What the track bank's GPU tests share (tests/test_gpu_tracks.py): the test bank, env builders, a driver that logs every output of a
run on the device, the coverage a driving run must show, and the documented draw restated in NumPy.  A plain module like
tests/model_support.py -- pytest does not collect it and does not rewrite its asserts, so every assert here carries its own message.

The reference for a bank drone on track t is the SAME drone of a single-track env of this library configured with t (same N, seed,
env_id_offset and actions): those kernels are held to the CPU oracle by the other GPU files, and every draw is keyed by (seed, drone,
step), so the comparison is bit for bit."""
import numpy as np
import torch

import goal_support as G  # noqa: F401  (the collector test's reference)
from gpu_support import DEV
from model_support import AMPS, BODY, FULL, GUSTY, NOISE, actions_mixed, philox

from drl_dronenavigation_amd import tracks as T

SPAWN = [[0.0, 0.0, 0.1]]
BOX = (-2, -2, 0, 2, 2, 2)
# the four long tracks, then two short ones that complete at once / every second step: 28 table rows in all
BANK = [T.up(), T.half_up_forward(), T.up_sharp_back_turn(), T.up_circle(), T.Track([[0, 0, .3]], SPAWN, BOX),
        T.Track([[0, 0, .2], [0, 0, .35]], SPAWN, BOX)]
W = np.array([len(t.waypoints) for t in BANK])
LONG, SHORT = (0, 1, 2, 3), (4, 5)
WEIGHTS = (1, 0, 2, 1, 3, 1)
MAX_STEPS, STEPS, K = 120, 400, 20
SEED = 23
OUT_KEYS = ("obs", "reward", "done", "truncated", "found_targets", "terminal_obs", "ep_return", "ep_length")
assert W.tolist() == [5, 3, 5, 12, 1, 2] and W.sum() == 28, W

# the option grid of tests 1 and 2: (compute dtype, normaliser, noise, goal frame or None = unbound, models + privileged rows on)
GRID = [("float64", False, False, None, False), ("float32", True, True, "world", False), ("float64", True, False, "body", True),
        ("float32", False, True, None, True)]
GRID_IDS = ["f64-raw-quiet-unbound-plain", "f32-norm-noise-world-plain", "f64-norm-quiet-body-models", "f32-raw-noise-unbound-models"]


def grid_kw(pkg, cell):
    dtype, norm, noise, goal, models = cell
    kw = dict(compute_dtype=dtype, normalize_obs=norm)
    if noise:
        kw.update(NOISE)
    if goal:
        kw["goal"] = pkg.GoalObservation(frame=goal)
    if models:
        kw.update(dynamics=pkg.DynamicsRandomization(**BODY), wind=pkg.WindDisturbance(**GUSTY), actuator=pkg.ActuatorModel(**FULL),
                  sensor=pkg.SensorModel(latency=(0, 8), bias=AMPS), privileged=pkg.PrivilegedObservation())
    return kw


def base_kw(**kw):
    # ground_contact is given explicitly: DN_GROUND_CONTACT_AUTO could resolve differently for a bank and for one of its tracks
    opts = dict(ground_contact=True, max_steps=MAX_STEPS, threshold=0.3, seed=SEED, device=DEV, normalize_obs=False)
    opts.update(kw)
    return opts


def bank_env(pkg, n, which=None, weights=None, resample=True, **kw):
    ts = BANK if which is None else [BANK[t] for t in which]
    return pkg.DroneVecEnv(None, n, tracks=pkg.TrackBank(ts, weights=weights, resample=resample), **base_kw(**kw))


def single_env(pkg, n, t, **kw):
    return pkg.DroneVecEnv(BANK[t], n, **base_kw(**kw))


def action_stream(n, steps=STEPS, seed=5):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([actions_mixed(rng, n) for _ in range(steps)])).to(DEV)


def drive(env, acts, fused):
    """Flies acts [S, n, 4] on `env` (after its reset): S single steps, or S / K launches of K.  Returns step-major device tensors of
    every output, the goal / privileged rows where the env writes them, `reset_obs`, and -- with a bank -- `track0` (after the reset),
    `track` / `finished` [S or S / K, n] after every call."""
    S, n = acts.shape[0], env.num_envs
    log = dict(reset_obs=env.reset_tensor().clone())
    if env.goal is not None:
        log["reset_goal"] = env.goal.clone()
    if env.track_ids is not None:
        log["track0"] = env.track_ids.clone()
    rows = []
    if fused:
        assert S % K == 0, "whole launches only"
        for j in range(S // K):
            out = env.rollout_tensor(acts[j * K:(j + 1) * K], want_terminal=True)
            rows.append({k: v.clone() for k, v in out.items() if k != "done_mask"})
    else:
        for t in range(S):
            o, r, d, info = env.step_tensor(acts[t])
            out = dict(info, obs=o, reward=r, done=d)
            rows.append({k: v.clone() for k, v in out.items() if k != "done_mask" and v is not None})
    for k in rows[0]:
        per_call = k in ("track", "terminal_track")
        log["finished" if k == "terminal_track" else k] = torch.stack([r[k] for r in rows]) if (per_call or not fused) \
            else torch.cat([r[k] for r in rows])
    return log


TERMINAL = ("terminal_obs", "ep_return", "ep_length", "terminal_goal", "terminal_privileged")


def same_log(got, want, cols, tag, keys=None):
    """Every logged output of the drones `cols` (a bool mask or None = all), bit for bit; rows that are written only where done are
    compared where done."""
    done = got["done"].bool()
    for k in (keys or [k for k in want if k in got]):
        a, b = got[k], want[k]
        if a.dtype in (torch.float32, torch.float64):
            a, b = a.view(torch.int32 if a.dtype == torch.float32 else torch.int64), b.view(torch.int32 if b.dtype == torch.float32 else torch.int64)
        ne = a != b
        if ne.dim() > done.dim() and k not in ("reset_obs", "reset_goal"):
            ne = ne.any(dim=-1)
        elif k in ("reset_obs", "reset_goal"):
            ne = ne.any(dim=-1)
        if k in TERMINAL:
            ne = ne & done
        if cols is not None:
            ne = ne[..., cols]
        assert not bool(ne.any()), (tag, k, int(ne.sum()), ne.nonzero()[:4].tolist())


def same_state(a, b, rows, tag, keys=None):
    for k in (keys or a.dtype.names):
        assert np.ascontiguousarray(a[k][rows]).tobytes() == np.ascontiguousarray(b[k][rows]).tobytes(), (tag, "state", k)


def entry_tracks(log):
    """The track every single step was entered with: [S, n] (the logged `track` is the track AFTER the step)."""
    return torch.cat([log["track0"][None], log["track"][:-1]]).cpu().numpy()


def coverage(done, truncated, found, entry, which_long=LONG, which_short=SHORT, restarts=None, advances_on=None):
    """What a driving run must show (numpy [S, n] arrays; `entry` = the track each step was entered with, in bank numbering): at least one
    truncation, one termination short of the last gate and one gate advance on each long track, one completion on each short track, and
    -- `restarts` = the track after each step, for resample = 1 -- a restart that changed track and one that kept it.  `advances_on`
    (the small fleets): the long tracks a gate advance is asked of, None = all.  Returns the counts."""
    done, truncated = done.astype(bool), truncated.astype(bool)
    prev = np.concatenate([np.zeros_like(found[:1]), np.where(done[:-1], 0, found[:-1])])
    advance = found > prev
    counts = {}
    for t in which_long:
        m = entry == t
        c = dict(truncated=int((done & truncated & m).sum()), crashed=int((done & ~truncated & (found < W[t]) & m).sum()),
                 advances=int((advance & m).sum()), ends=int((done & m).sum()))
        need_advance = advances_on is None or t in advances_on
        assert c["truncated"] >= 1 and c["crashed"] >= 1 and (c["advances"] >= 1 or not need_advance), ("long track without coverage", t, c)
        counts[t] = c
    for t in which_short:
        m = entry == t
        c = dict(completed=int((done & (found == W[t]) & m).sum()), ends=int((done & m).sum()))
        assert c["completed"] >= 1, ("short track never completed", t, c)
        counts[t] = c
    if restarts is not None:
        counts["changed"], counts["kept"] = int((done & (restarts != entry)).sum()), int((done & (restarts == entry)).sum())
        assert counts["changed"] >= 1 and counts["kept"] >= 1, ("restarts", counts)
    return counts


def draw(cdf, gid, step, seed):
    """The documented draw: ONE Philox4x32-10 call on (seed; gid, step, stream 22), u = (r_0 + 0.5) / 2^32 in float64,
    t = the number of k in 0..T-2 with u >= cdf_k."""
    u = (philox(int(gid), int(step), 22, seed)[0] + 0.5) / 4294967296.0
    return int(sum(1 for k in range(len(cdf) - 1) if u >= cdf[k]))


def cdf_of(weights):
    s = np.cumsum(np.asarray(weights, np.float32).astype(np.float64))
    return s / s[-1]
