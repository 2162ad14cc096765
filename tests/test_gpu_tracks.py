"""The per-drone track bank (include/dronenav.h dn_enable_tracks) on the HIP path.

The reference for a bank drone on track t is the SAME drone of a single-track env of this library configured with t (tests/track_support.py):
bit for bit, not to a tolerance.  The test bank: up (5 waypoints), half_up_forward (3), up_sharp_back_turn (5), up_circle (12), one
waypoint above the spawn (completes at once) and two (completes every second step); max_steps = 120, model_support.actions_mixed, 400
single steps or 20 launches of K = 20.  Every test that drives a bank asserts the coverage of track_support.coverage.

 1. a bank of one is no bank;
 2. fixed assignment: drone i on track i mod 6 equals drone i of the single-track env of its track;
 3. draws: track and finished after the reset and after every step against the documented draw;
 4. trajectories under redraw against single-track envs teacher-forced with the bank env's state;
 5. twenty K = 20 launches equal 400 single steps;
 6. 188 drones equal shards of 96 + 92;
 7. the per-track counters against the single-step outputs and dn_stats;
 8. refusals and the Python surface.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import track_support as S  # noqa: E402
from gpu_support import DEV  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402
from track_support import G  # noqa: E402


def _np(log, *keys):
    return [log[k].cpu().numpy() for k in keys]


# ---- 1 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resample", [True, False], ids=["redraw", "keep"])
@pytest.mark.parametrize("fused", [False, True], ids=["single", "k20"])
@pytest.mark.parametrize("cell", S.GRID, ids=S.GRID_IDS)
def test_a_bank_of_one_is_no_bank(cell, fused, resample):
    """T = 1 with the config's track (`up`), under either resample: outputs, state, statistics, goal / privileged rows and terminal rows
    equal the env without a bank.  191 drones in single steps, 188 in launches.  (The counts do not depend on resample: the plain env's.)
    Measured on one MI355X over the eight cells: 726-805 episode ends, 119-179 of them truncated and 593-653 short of the last gate,
    1 845-2 171 gate advances."""
    pkg = _pkg()
    n = 188 if fused else 191
    kw = S.grid_kw(pkg, cell)
    plain, bank = S.single_env(pkg, n, 0, **kw), S.bank_env(pkg, n, which=[0], resample=resample, **kw)
    acts = S.action_stream(n)
    want, got = S.drive(plain, acts, fused), S.drive(bank, acts, fused)
    S.same_log(got, want, None, "bank of one")
    S.same_state(bank.get_state(), plain.get_state(), slice(None), "bank of one")
    assert bank.stats() == plain.stats()
    assert int(got["track"].abs().sum()) == 0 and int(got["track0"].abs().sum()) == 0
    done, trunc, found = _np(want, "done", "truncated", "found_targets")
    print("counts", S.coverage(done, trunc, found, np.zeros_like(found), which_long=(0,), which_short=()))
    plain.close(), bank.close()


# ---- 2 --------------------------------------------------------------------------------------------------------------------------------
def _fixed(pkg, n, cell, fused, steps=S.STEPS, cover="full"):
    kw = S.grid_kw(pkg, cell)
    ids = np.arange(n) % 6
    bank = S.bank_env(pkg, n, resample=False, **kw)
    bank.set_tracks(ids.astype(np.int32))
    # dn_set_tracks does not touch the state: the created state still holds the distance to waypoint 0 of track 0, which the first reset
    # row shows in column 12 (the reference's stale-distance quirk).  The single-track envs start from the same state.
    st0 = bank.get_state()
    acts = S.action_stream(n, steps)
    got = S.drive(bank, acts, fused)
    assert np.array_equal(got["track"].cpu().numpy(), np.broadcast_to(ids, got["track"].shape)), "resample = 0 keeps the assignment"
    st = bank.get_state()
    for t in range(6):
        if not (ids == t).any():
            continue
        one = S.single_env(pkg, n, t, **kw)
        one.set_state(st0)
        want = S.drive(one, acts, fused)
        cols = torch.from_numpy(ids == t).to(DEV)
        S.same_log(got, want, cols, f"track {t}")
        S.same_state(st, one.get_state(), ids == t, f"track {t}")
        one.close()
    fin, done = got["finished"].cpu().numpy(), got["done"].cpu().numpy().astype(bool)
    ended = np.maximum.accumulate(done if not fused else done.reshape(-1, S.K, n).any(axis=1), axis=0)
    assert np.array_equal(fin, np.where(ended, ids[None], -1)), "finished = the drone's track once an episode of it ended, -1 before"
    d, tr, f = _np(got, "done", "truncated", "found_targets")
    if cover == "full":
        print("counts", S.coverage(d, tr, f, np.broadcast_to(ids, f.shape)))
    elif cover == "small":
        # eleven drones a track: gate advances are asked of the two tracks whose first gates lie within the threshold of the spawn (up,
        # up_circle); half_up_forward and up_sharp_back_turn see a handful among 32 drones and may see none among eleven
        print("counts", S.coverage(d, tr, f, np.broadcast_to(ids, f.shape), advances_on=(0, 3)))
    else:
        # one drone flies one track (track 0, `up`): its episodes end, and it passes the gates beside the spawn
        assert d.sum() >= 1 and (f > 0).any(), "the one drone neither ended an episode nor passed a gate"
        print("counts", dict(ends=int(d.sum()), truncated=int((d.astype(bool) & tr.astype(bool)).sum()), best=int(f.max())))
    bank.close()


@pytest.mark.parametrize("fused", [False, True], ids=["single", "k20"])
@pytest.mark.parametrize("cell", S.GRID, ids=S.GRID_IDS)
def test_fixed_assignment_flies_each_drone_on_its_own_track(cell, fused):
    """resample = 0, drone i on track i mod 6 (dn_set_tracks, then dn_reset): every output, dn_get_state, the goal and terminal goal
    rows (both frames over the grid) and the privileged rows of every drone equal the same drone of the single-track env of its track.
    191 drones in single steps, 188 in K = 20 launches.
    Measured on one MI355X over the eight cells, per long track: 13-38 truncations and 81-116 terminations short of the last gate;
    gate advances 319-374 (up), 1-36 (half_up_forward), 6-40 (up_sharp_back_turn), 292-334 (up_circle); completions of the two short
    tracks 12 400-12 800 and 6 200."""
    _fixed(_pkg(), 188 if fused else 191, cell, fused)


@pytest.mark.parametrize("n,fused", [(65, False), (1, False), (68, True)], ids=["65-single", "1-single", "68-k20"])
@pytest.mark.parametrize("cell", S.GRID, ids=S.GRID_IDS)
def test_fixed_assignment_at_the_fleet_edges(cell, n, fused):
    """The partial-tile fleets over the same option grid: 65 and 1 drones in single steps, 68 in K = 20 launches.  Coverage: 65 and 68
    drones (eleven a track) assert what the full fleets assert except gate advances on the two tracks whose first gate is out of reach
    of the spawn; the one drone flies `up` alone and asserts that its episodes end and that it passes a gate.
    Measured on one MI355X: the 65- and 68-drone fleets over the four cells, per long track, 2-12 truncations and 30-44 terminations
    short of the last gate; gate advances 112-140 (up), 0-13 (half_up_forward), 2-14 (up_sharp_back_turn), 102-122 (up_circle);
    completions 4 400 and 2 000-2 200.  The one drone: 3-5 episode ends (0-2 of them truncated), found_targets up to 2."""
    _fixed(_pkg(), n, cell, fused, cover="one" if n == 1 else "small")


# ---- 3, 7: one run with redraws, shared ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def redraw_run():
    pkg = _pkg()
    n = 191
    env = S.bank_env(pkg, n, weights=S.WEIGHTS, resample=True, goal=pkg.GoalObservation("world"), env_id_offset=1000)
    base = env.stats()
    sc0 = env.step_count
    log = S.drive(env, S.action_stream(n), False)
    run = dict(n=n, log=log, sc0=sc0, stats0=base, stats1=env.stats(), counters=env.track_stats(), env=env, offset=1000)
    yield run
    env.close()


def test_tracks_follow_the_documented_draw(redraw_run):
    """resample = 1, weights (1, 0, 2, 1, 3, 1): after dn_reset and after every single step, `track` is the documented draw for every
    drone whose episode started there and unchanged elsewhere; `finished` is the entry track where done and unchanged elsewhere; track 1
    (weight 0) never appears.
    Measured on one MI355X (191 drones, 400 steps; truncated / short of the last gate / gate advances): up 42 / 140 / 462,
    up_sharp_back_turn 75 / 294 / 28, up_circle 21 / 153 / 452; completions of the short tracks 736 and 225; 1 224 restarts changed track
    and 462 kept it.  half_up_forward has weight 0 and is never flown here."""
    r = redraw_run
    n, log, cdf = r["n"], r["log"], S.cdf_of(S.WEIGHTS)
    track0, track, fin, done = _np(log, "track0", "track", "finished", "done")
    want = np.array([S.draw(cdf, r["offset"] + i, r["sc0"], S.SEED) for i in range(n)])
    assert np.array_equal(track0, want), "dn_reset's draw"
    cur, last = track0.copy(), np.full(n, -1)
    for t in range(S.STEPS):
        d = done[t].astype(bool)
        last = np.where(d, cur, last)
        for i in np.flatnonzero(d):
            cur[i] = S.draw(cdf, r["offset"] + i, r["sc0"] + t, S.SEED)
        assert np.array_equal(track[t], cur), f"step {t}: track"
        assert np.array_equal(fin[t], last), f"step {t}: finished"
    assert not (track == 1).any() and not (track0 == 1).any(), "a zero weight was drawn"
    entry = S.entry_tracks(log)
    d, tr, f = _np(log, "done", "truncated", "found_targets")
    print("counts", S.coverage(d, tr, f, entry, which_long=(0, 2, 3), restarts=track))


def test_counters_equal_the_counts_of_the_outputs(redraw_run):
    """The per-track counters equal the counts recomputed from the single-step outputs under the entry tracks; their sums over the
    tracks equal the deltas of dn_stats; reset = 1 zeroes them."""
    r = redraw_run
    log, env = r["log"], r["env"]
    entry = S.entry_tracks(log)
    done, trunc, found, eplen = _np(log, "done", "truncated", "found_targets", "ep_length")
    done = done.astype(bool)
    want = np.zeros((6, 5), np.int64)
    for t in range(6):
        m = done & (entry == t)
        want[t] = [m.sum(), (m & (found == S.W[t])).sum(), (m & trunc.astype(bool)).sum(), found[m].sum(), eplen[m].sum()]
    assert np.array_equal(r["counters"], want), (r["counters"], want)
    delta = {k: r["stats1"][k] - r["stats0"][k] for k in r["stats1"]}
    tot = want.sum(axis=0)
    assert [delta["episodes"], delta["completed"], delta["truncated"], delta["sum_found_targets"], delta["sum_ep_len"]] == tot.tolist(), (delta, tot)
    assert want[1].sum() == 0 and want[:, 0].min(initial=1 << 30, where=np.array(S.WEIGHTS) > 0) > 0
    assert np.array_equal(env.track_stats(reset=True), want) and not env.track_stats().any(), "reset = 1 returns, then zeroes"


# ---- 4 --------------------------------------------------------------------------------------------------------------------------------
def test_trajectories_under_redraw_follow_the_entry_track_and_restart_on_the_new_one():
    """resample = 1, goal rows bound, normaliser, noise and sensor off (dn_set_state then round trips exactly).  Before each single step
    the bank env's state is copied into the six single-track envs (each takes the drones that are on its track).  Where an episode goes
    on, everything equals the entry track's env; where it ends, reward, flags, found_targets, terminal_obs, the Monitor values and the
    terminal goal row equal the entry track's env, the reset observation equals it too (the spawn is shared, and column 12 shows the
    ended episode's distance), and the new pose, idx, steps and the reset goal row are those of a freshly reset env of the NEW track.
    The fresh d = d_prev is the distance from the kept _current_position to waypoint 0 of the NEW track (the auto-reset does not reset
    that position -- the reference's quirk, which every single-track kernel has -- so it is NOT the freshly reset env's distance from the
    spawn; it is checked against the state's own cur_pos to 5e-7, and d_prev = d bit for bit).
    Measured on one MI355X (191 drones, 400 steps; truncated / short of the last gate / gate advances): up 40 / 126 / 440,
    up_sharp_back_turn 54 / 315 / 25, up_circle 38 / 157 / 486; completions of the short tracks 740 and 233; 1 208 restarts changed track
    and 495 kept it."""
    pkg = _pkg()
    n = 191
    goal = dict(goal=pkg.GoalObservation("world"))
    bank = S.bank_env(pkg, n, weights=S.WEIGHTS, resample=True, **goal)
    ones = [S.single_env(pkg, n, t, **goal) for t in range(6)]
    fresh = []
    for e in ones:
        e.reset_tensor()
        fresh.append((e.goal[0].clone(), e.get_state()[0]))
    bank.reset_tensor()
    acts = S.action_stream(n)
    keys = ("obs", "reward", "done", "truncated", "found_targets", "terminal_obs", "ep_return", "ep_length", "terminal_goal")
    pose = ("pos", "quat", "vel", "ang_v", "idx", "steps", "just_found")
    # d of a restart: three float32 coordinates of `cur_pos`, each within half an ulp of a value below 2 (6e-8), move the distance by at
    # most sqrt(3) x 6e-8; the float32 rounding of a distance below 4 adds 2.4e-7; the float64 evaluation itself is exact at this scale
    D_ATOL = 5e-7
    log = dict(done=[], truncated=[], found_targets=[], entry=[], after=[])
    for t in range(S.STEPS):
        st = bank.get_state()
        entry = bank.track_ids.cpu().numpy().copy()
        for s, e in enumerate(ones):
            mine = e.get_state()
            mine[entry == s] = st[entry == s]
            e.set_state(mine)
        o, r, d, info = bank.step_tensor(acts[t])
        got = {k: v.clone() for k, v in dict(info, obs=o, reward=r, done=d).items() if k in keys + ("goal", "track")}
        done = got["done"].bool()
        done_h, after = done.cpu().numpy(), got["track"].cpu().numpy()
        st1 = bank.get_state()
        flags = []
        for s, e in enumerate(ones):
            o, r, d, info = e.step_tensor(acts[t])
            want = dict(info, obs=o, reward=r, done=d)
            on = torch.from_numpy(entry == s).to(DEV)
            for k in keys:
                ne = (got[k] != want[k]) if got[k].dim() == 1 else (got[k] != want[k]).any(dim=1)
                if k in S.TERMINAL:
                    ne = ne & done
                flags.append(((s, k), (ne & on).any()))
            going = on & ~done
            flags.append(((s, "goal"), ((got["goal"] != want["goal"]).any(dim=1) & going).any()))
            S.same_state(st1, e.get_state(), (entry == s) & ~done_h, f"step {t} track {s}")
            starts = (after == s) & done_h                                 # episodes that start on track s here, whatever they ended on
            flags.append(((s, "reset goal row"), ((got["goal"] != fresh[s][0]).any(dim=1) & torch.from_numpy(starts).to(DEV)).any()))
            for k in pose:
                rows = st1[k][starts]
                assert rows.tobytes() == np.broadcast_to(fresh[s][1][k], rows.shape).tobytes(), (t, s, k)
            # the auto-reset keeps _current_position (the reference's quirk, as in every single-track kernel), so the fresh d is measured
            # from THERE to waypoint 0 of the new track, not from the spawn: d = d_prev = |cur_pos - wp0_new|
            d_want = np.linalg.norm(st1["cur_pos"][starts].astype(np.float64) - S.BANK[s].waypoints[0], axis=1)
            assert np.abs(st1["d"][starts] - d_want).max(initial=0.0) <= D_ATOL, (t, s, "d", np.abs(st1["d"][starts] - d_want).max())
            assert st1["d"][starts].tobytes() == st1["d_prev"][starts].tobytes(), (t, s, "d_prev")
        bad = torch.stack([f for _, f in flags]).cpu().numpy()                 # one synchronisation per step
        assert not bad.any(), (t, [name for (name, _), x in zip(flags, bad) if x])
        log["done"].append(done_h), log["truncated"].append(got["truncated"].cpu().numpy())
        log["found_targets"].append(got["found_targets"].cpu().numpy()), log["entry"].append(entry), log["after"].append(after)
    L = {k: np.stack(v) for k, v in log.items()}
    print("counts", S.coverage(L["done"], L["truncated"], L["found_targets"], L["entry"], which_long=(0, 2, 3), restarts=L["after"]))
    for e in ones + [bank]:
        e.close()


# ---- 5, 6 -----------------------------------------------------------------------------------------------------------------------------
def _redraw_env(pkg, n, **kw):
    return S.bank_env(pkg, n, weights=S.WEIGHTS, resample=True, goal=pkg.GoalObservation("body"), normalize_obs=True, **S.NOISE, **kw)


def test_twenty_launches_of_twenty_equal_400_single_steps():
    """resample = 1, goal rows (body frame), normaliser and noise on, 188 drones: every output, the state, `track`, `finished` at every
    launch boundary and the counters, bit for bit.
    Measured on one MI355X (truncated / short of the last gate / gate advances): up 37 / 144 / 473, up_sharp_back_turn 63 / 276 / 17,
    up_circle 34 / 164 / 474; completions of the short tracks 692 and 204; 1 159 restarts changed track and 455 kept it."""
    pkg = _pkg()
    n = 188
    a, b = _redraw_env(pkg, n), _redraw_env(pkg, n)
    acts = S.action_stream(n)
    one, many = S.drive(a, acts, False), S.drive(b, acts, True)
    S.same_log(many, one, None, "fused", keys=[k for k in one if k not in ("track", "finished")])
    assert torch.equal(many["track"], one["track"][S.K - 1::S.K]) and torch.equal(many["finished"], one["finished"][S.K - 1::S.K])
    S.same_state(b.get_state(), a.get_state(), slice(None), "fused")
    assert np.array_equal(a.track_stats(), b.track_stats()) and a.stats() == b.stats()
    d, tr, f = _np(one, "done", "truncated", "found_targets")
    print("counts", S.coverage(d, tr, f, S.entry_tracks(one), which_long=(0, 2, 3), restarts=one["track"].cpu().numpy()))
    a.close(), b.close()


def test_two_shards_equal_the_whole_fleet():
    """188 drones equal shards of 96 + 92 with env_id_offset, in 400 single steps with redraws (goal rows, normaliser and noise on):
    outputs, tracks after every step, state; the shards' counters add up to the fleet's.
    Measured on one MI355X (the fleet of the test above: the same counts): up 37 / 144 / 473, up_sharp_back_turn 63 / 276 / 17, up_circle
    34 / 164 / 474 (truncated / short of the last gate / gate advances); completions 692 and 204; 1 159 restarts changed track, 455 kept it."""
    pkg = _pkg()
    whole, lo, hi = _redraw_env(pkg, 188), _redraw_env(pkg, 96), _redraw_env(pkg, 92, env_id_offset=96)
    acts = S.action_stream(188)
    w, a, b = S.drive(whole, acts, False), S.drive(lo, acts[:, :96].contiguous(), False), S.drive(hi, acts[:, 96:].contiguous(), False)
    per_drone = ("reset_obs", "reset_goal", "track0")                 # [n, ...]: every other entry is [steps or launches, n, ...]
    both = {k: torch.cat([a[k], b[k]], dim=0 if k in per_drone else 1) for k in w}
    S.same_log(both, w, None, "shards")
    sw, sa, sb = whole.get_state(), lo.get_state(), hi.get_state()
    S.same_state(np.concatenate([sa, sb]), sw, slice(None), "shards")
    assert np.array_equal(lo.track_stats() + hi.track_stats(), whole.track_stats())
    d, tr, f = _np(w, "done", "truncated", "found_targets")
    print("counts", S.coverage(d, tr, f, S.entry_tracks(w), which_long=(0, 2, 3), restarts=w["track"].cpu().numpy()))
    for e in (whole, lo, hi):
        e.close()


# ---- checkpoint -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize_obs", [False, True], ids=["raw", "norm"])
def test_a_bank_fleet_round_trips_through_set_state_mid_flight(normalize_obs):
    """A checkpoint of a bank fleet is get_state + track_ids, restored as set_tracks THEN set_state (include/dronenav.h).  The bank here
    puts the one-waypoint track first, so that every drone on a longer track that passed a gate holds an idx >= W_0: dn_set_state holds
    idx to the drone's OWN track.  After 100 single steps with redraws the fleet is restored into a second env, and both fly 100 more
    steps bit for bit (outputs, goal rows, tracks, state).  In the other direction an idx inside a longer track's count but beyond the
    drone's own is refused.  Noise and the sensor are off; with the normaliser on the blob carries its second moment verbatim (rms_m2,
    ABI 10), so dn_set_state round trips exactly either way (the flight does not depend on the normaliser: the figures below hold for both).
    Measured on one MI355X: at the checkpoint 179 of 191 drones hold an idx >= W_0 = 1 (the largest is 3), after 508 episode ends; 350
    more end after the restore."""
    pkg = _pkg()
    n, order = 191, [4, 3, 0, 5]                                  # bank track 0 = the one-waypoint track, 1 = up_circle, 2 = up, 3 = two waypoints
    Wb = S.W[order]
    make = lambda: S.bank_env(pkg, n, which=order, resample=True, goal=pkg.GoalObservation("world"), normalize_obs=normalize_obs)      # noqa: E731
    acts = S.action_stream(n, 200)
    keys = ("obs", "reward", "done", "truncated", "found_targets", "terminal_obs", "ep_return", "ep_length", "goal", "terminal_goal", "track")

    def fly(env, a):
        rows = []
        for t in range(a.shape[0]):
            o, r, d, info = env.step_tensor(a[t])
            rows.append({k: v.clone() for k, v in dict(info, obs=o, reward=r, done=d).items() if k in keys})
        return {k: torch.stack([r[k] for r in rows]) for k in keys}

    first = make()
    first.reset_tensor()
    before = fly(first, acts[:100])
    st, ids, sc = first.get_state(), first.track_ids.clone(), first.step_count
    tr = ids.cpu().numpy()
    beyond = st["idx"] >= Wb[0]
    assert beyond.sum() >= 10 and (tr == 0).any() and len(set(tr.tolist())) == 4, (int(beyond.sum()), set(tr.tolist()))
    assert (st["idx"] < Wb[tr]).all(), "idx is the index within the drone's own track"
    second = make()
    second.reset_tensor()
    second.set_tracks(ids)
    second.set_state(st)
    second.step_count = sc
    S.same_state(second.get_state(), st, slice(None), "restored")
    want, got = fly(first, acts[100:]), fly(second, acts[100:])
    S.same_log(got, want, None, "after the restore")
    S.same_state(second.get_state(), first.get_state(), slice(None), "after the restore")
    restarts = int(want["done"].sum())
    assert restarts >= 100 and bool((want["track"][1:] != want["track"][:-1]).any()), "no redraw after the restore"
    # the other direction: a drone on the one-waypoint track with idx 1 (inside up_circle's 12) is refused, and nothing is written
    bad = st.copy()
    i = int(np.flatnonzero(tr == 0)[0])
    bad["idx"][i] = 1
    with pytest.raises(pkg.DroneNavError, match="idx/steps out of range"):
        second.set_state(bad)
    S.same_state(second.get_state(), first.get_state(), slice(None), "after the refused write")
    print("counts", dict(idx_beyond_w0=int(beyond.sum()), max_idx=int(st["idx"].max()), restarts_after=restarts,
                         done_before=int(before["done"].sum())))
    first.close(), second.close()


# ---- 8 --------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    pkg = _pkg()
    K = pkg._capi
    lib = K.load()
    n = 64

    def refused(env, cfg, word, status=-1):
        rc = lib.dn_enable_tracks(env._handle, C.byref(cfg))
        assert rc == status and word in lib.dn_last_error().decode(), (rc, word, lib.dn_last_error())

    plain = S.single_env(pkg, n, 0)
    buf = torch.zeros(n, dtype=torch.int32, device=DEV)
    out = np.zeros((6, 5), np.int64)
    cfg = K.DnTrackBankConfig()
    for rc in (lib.dn_set_tracks(plain._handle, buf.data_ptr(), None), lib.dn_get_tracks(plain._handle, buf.data_ptr(), None, None),
               lib.dn_get_track_stats(plain._handle, out.ctypes.data, 0), lib.dn_get_track_bank_config(plain._handle, C.byref(cfg))):
        assert rc == -5, rc                                              # DN_ERR_BAD_STATE before enabling
    assert plain.track_ids is None and plain.track_bank_config() is None
    with pytest.raises(RuntimeError, match="TrackBank"):
        plain.set_tracks(np.zeros(n, np.int32))
    with pytest.raises(RuntimeError, match="TrackBank"):
        plain.track_stats()
    good = pkg.TrackBank(S.BANK, weights=S.WEIGHTS)

    def edited(**kw):
        c = good.to_c()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c

    refused(plain, edited(num_tracks=0), "num_tracks")
    refused(plain, edited(num_tracks=65), "num_tracks")
    refused(plain, edited(num_waypoints=(2, 0)), "track 2")
    refused(plain, edited(num_waypoints=(3, 65)), "track 3")
    refused(plain, edited(num_waypoints=(3, 49)), "at most 64")                              # 28 - 12 + 49 = 65 rows
    refused(plain, edited(waypoints=(40, float("nan"))), "not finite")
    refused(plain, edited(waypoints=(41, float("inf"))), "not finite")
    refused(plain, edited(weight=(2, -1.0)), "weight[2]")
    refused(plain, edited(weight=(0, float("nan"))), "weight[0]")
    c = edited()
    for k in range(6):
        c.weight[k] = 0.0
    refused(plain, c, "every weight is zero")
    refused(plain, edited(reserved=1), "reserved")
    refused(plain, edited(resample=2), "resample")
    refused(plain, edited(waypoints=(2, 0.1000001)), "track 0")                               # not bit-equal to the config's
    refused(plain, edited(num_waypoints=(0, 4)), "track 0")
    assert plain.track_ids is None and lib.dn_get_tracks(plain._handle, buf.data_ptr(), None, None) == -5, "a refusal enables nothing"
    circle = pkg.DroneVecEnv(pkg.tracks.circle(1, 4, 1), n, device=DEV)
    refused(circle, good.to_c(), "circle")
    spawn = S.single_env(pkg, n, 0, random_spawn=True)
    refused(spawn, good.to_c(), "random_spawn")
    for kw in (dict(circle=True), dict(random_spawn=True)):
        with pytest.raises(ValueError):
            S.bank_env(pkg, n, **kw)
    with pytest.raises(ValueError, match="track 0"):
        pkg.DroneVecEnv(S.BANK[1], n, tracks=good, device=DEV)
    with pytest.raises(TypeError):
        pkg.DroneVecEnv(S.BANK[0], n, tracks=S.BANK, device=DEV)
    # a later call: the same geometry changes weights and resample and keeps the assignment; another geometry is refused
    bank = S.bank_env(pkg, n, weights=S.WEIGHTS, resample=False)
    ids = (np.arange(n) % 6).astype(np.int32)
    bank.set_tracks(ids)
    assert lib.dn_enable_tracks(bank._handle, C.byref(pkg.TrackBank(S.BANK, weights=(0, 0, 0, 0, 0, 1), resample=True).to_c())) == 0
    lib.dn_get_tracks(bank._handle, buf.data_ptr(), None, None)
    assert np.array_equal(buf.cpu().numpy(), ids), "the assignment survives a second dn_enable_tracks"
    bank.reset_tensor()
    assert (bank.track_ids == 5).all(), "the new weights are in force"
    got = bank.track_bank_config()
    assert got.resample and np.array_equal(got.weights, [0, 0, 0, 0, 0, 1]) and got.num_waypoints == S.W.tolist()
    refused(bank, pkg.TrackBank(S.BANK[:5]).to_c(), "geometry")
    refused(bank, pkg.TrackBank([S.BANK[0], S.BANK[2], S.BANK[1]] + S.BANK[3:]).to_c(), "geometry")
    # the entry points whose kernels carry no model refuse the bank through the same walk
    a = torch.zeros((n, 4), device=DEV)
    with pytest.raises(pkg.DroneNavError, match="track bank"):
        bank.eval_kinematics_tensor(torch.zeros((n, 13), dtype=torch.float64, device=DEV))
    p = bank._ptrs
    ls = (C.c_float * 4)()
    assert lib.dn_step_sampled(bank._handle, a.data_ptr(), ls, 1, 0, a.data_ptr(), buf.data_ptr(), *p[0], *p[1], p[2], None) == -1
    assert b"track bank" in lib.dn_last_error()
    assert bank.kernel_waves(False) == 1 and bank.kernel_waves(True) == 1
    for e in (plain, circle, spawn, bank):
        e.close()


def test_ground_contact_auto_is_resolved_over_the_bank():
    """A config created with DN_GROUND_CONTACT_AUTO on a track that does not need the term (a gate at z = 1.5 reached from a spawn at
    z = 1.5) turns it on when a track of the bank reaches down to the floor."""
    pkg = _pkg()
    box, spawn = (-2, -2, 0, 2, 2, 2), [[0, 0, 1.5]]
    high = pkg.Track([[1, 0, 1.5]], spawn, box)
    low = pkg.Track([[1, 0, 0.2]], spawn, box)
    alone = pkg.DroneVecEnv(high, 8, device=DEV)
    assert not alone.ground_contact
    both = pkg.DroneVecEnv(high, 8, tracks=pkg.TrackBank([high, low]), device=DEV)
    assert both.ground_contact and both.cfg.ground_contact == 1
    same = pkg.DroneVecEnv(high, 8, tracks=pkg.TrackBank([high, high]), device=DEV)
    assert not same.ground_contact
    fixed = pkg.DroneVecEnv(high, 8, tracks=pkg.TrackBank([high, low]), ground_contact=False, device=DEV)
    assert not fixed.ground_contact, "an explicit setting stays"
    for e in (alone, both, same, fixed):
        e.close()


def test_python_surface_and_collector():
    """The info keys, rollout_tensor's tracks, the collector buffer's `track`, the refusing collectors, and
    RolloutCollector(policy_input="observation+goal") on a bank env: one rollout whose goal rows equal goal_support.goal_rows with each
    drone's OWN waypoints at that file's bar."""
    pkg = _pkg()
    n, T = 128, 16
    env = S.bank_env(pkg, n, weights=S.WEIGHTS, goal=pkg.GoalObservation("world"))
    env.reset_tensor()
    assert env.track_ids.dtype == torch.int32 and tuple(env.track_ids.shape) == (n,) and env.track_ids.device.type == "cuda"
    o, r, d, info = env.step_tensor(torch.zeros((n, 4), device=DEV))
    assert info["track"] is env.track_ids and tuple(info["terminal_track"].shape) == (n,)
    out = env.rollout_tensor(S.action_stream(n, 20))
    assert out["track"] is env.track_ids and "terminal_track" in out
    bare = S.bank_env(pkg, 64)                                          # without goal rows: the bank alone is what they refuse
    with pytest.raises(ValueError, match="track bank"):
        pkg.FusedRolloutCollector(bare, None, 4)
    with pytest.raises(ValueError, match="track bank"):
        pkg.OffPolicyCollector(bare, None, 1024)
    bare.close()
    rng = np.random.default_rng(3)
    stream = [torch.from_numpy(S.actions_mixed(rng, n)).to(DEV) for _ in range(T)]
    seen, calls = [], [0]

    def policy(x):
        a = stream[min(calls[0], T - 1)]
        calls[0] += 1
        seen.append(x.clone())
        return a, torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)

    col = pkg.RolloutCollector(env, policy, T, policy_input="observation+goal", bootstrap_truncated=False)
    buf = col.collect()
    assert buf["track"].dtype == torch.int32 and tuple(buf["track"].shape) == (T, n)
    track, obs, goal = buf["track"].cpu().numpy(), buf["obs"].cpu().numpy(), buf["goal"].cpu().numpy()
    assert torch.equal(seen[0], torch.cat((buf["obs"][0], buf["goal"][0]), dim=1))
    assert len(set(track.ravel().tolist())) >= 4 and (track != track[0]).any(), "the rollout saw redraws"
    checked = 0
    for t in set(track.ravel().tolist()):
        m = track == t
        idx = goal[..., 3][m].astype(np.int64)
        want = G.goal_rows(obs[m], idx, S.BANK[t].waypoints, S.BOX)
        assert np.abs(want[:, [0, 1, 2, 4, 5, 6]]).max() < G.MAG
        np.testing.assert_allclose(goal[m], want, rtol=0, atol=G.ATOL, err_msg=f"track {t}")
        checked += int(m.sum())
    assert checked == T * n
    env.close()
