"""dn_get_state / dn_set_state with the observation normaliser ON: the blob is this project's checkpoint, reshard and set_attr path, and
since ABI 10 it carries the normaliser's second moment M2 = var x count verbatim (dn_env_state.rms_m2) beside var = M2 / count.

Before, dn_set_state rebuilt M2 from var and count (csrc/dn_second_moment.h second_moment): the m nearest var x count that divides back
to var.  That reads back as the same var, but neighbouring M2 divide to the same var, and about one word in eleven came back one ulp off
(tests/test_state_moments_cpu.py walks the rule on the CPU).  Here the device words themselves are compared: a restored fleet, a fleet
one drone of which went through set_attr, the halves of a resharded fleet and a checkpoint with every per-drone model on must continue
with the bits of the fleet that was never interrupted, and an edited var or count must still be honoured.

Fleets: 132 drones for launches (two tiles and a ragged one, a multiple of four as dn_step_many wants), 130 for single steps; max_steps
is small enough that every drone ends episodes inside the flown steps, before and after the blob is taken.  `_old_rule` restates second_moment in NumPy: each test that
restores a blob counts the words that rule would have moved and requires some, or it would pass without the field."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import track_support as S  # noqa: E402
from gpu_support import DEV, _acts  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402
from model_support import AMPS, BODY, FULL, GUSTY, NOISE  # noqa: E402

N_LAUNCH, N_SINGLE = 132, 130
MAX_STEPS = 10          # an episode is over at its 11th step at the latest: every drone ends three in FLOWN steps, most one in 7 more
FLOWN = 40


def _old_rule(var, count):
    """csrc/dn_second_moment.h second_moment, element-wise: var x count, or the neighbour that divides back to var."""
    var, count = np.broadcast_arrays(np.asarray(var, np.float64), np.asarray(count, np.float64))
    with np.errstate(all="ignore"):
        m = var * count
        lo, hi = np.nextafter(m, -np.inf), np.nextafter(m, np.inf)
        keep = ~(count > 0.0) | ~np.isfinite(m) | (m / count == var)
        return np.where(keep, m, np.where(lo / count == var, lo, np.where(hi / count == var, hi, m)))


def _lossy_words(st):
    """How many second moments of the blob the rule before ABI 10 would not have restored."""
    return int((_old_rule(st["rms_var"], st["rms_count"][:, None]) != st["rms_m2"]).sum())


def _same_blob(a, b, tag, rows=slice(None)):
    for k in a.dtype.names:
        assert np.array_equal(a[k][rows], b[k][rows]), (tag, "state", k, int((a[k][rows] != b[k][rows]).sum()))


def _env(pkg, n, seed=3, **kw):
    from drl_dronenavigation_amd import tracks
    opts = dict(normalize_obs=True, max_steps=MAX_STEPS, seed=seed, device=DEV)
    opts.update(kw)
    return pkg.DroneVecEnv(tracks.reaching(), n, **opts)


def _fly(env, rng, steps, fused):
    """`steps` control steps after a reset: launches of 20 or single steps.  Returns the episodes that ended.  The episode step counters
    are spread over [0, MAX_STEPS) first, so that the time limit ends episodes at every step: waves in which some lanes start an episode
    while others fly on."""
    env.reset_tensor()
    st = env.get_state()
    st["steps"] = rng.integers(0, MAX_STEPS, len(st)).astype(st["steps"].dtype)
    env.set_state(st)
    ends = 0
    if fused:
        for _ in range(steps // 20):
            ends += int(env.rollout_tensor(_acts(rng, env.num_envs, 20))["done"].sum())
    else:
        for a in _acts(rng, env.num_envs, steps):
            ends += int(env.step_tensor(a)[2].sum())
    return ends


def _restore(twin, st, step_count):
    twin.reset_tensor()
    twin.set_state(st)
    twin.step_count = step_count


def _step(env, a):
    """One dn_step: clones of everything step_tensor returns."""
    o, r, d, info = env.step_tensor(a)
    return {k: v.clone() for k, v in dict(info, obs=o, reward=r, done=d).items() if v is not None}


EPISODE_END = ("ep_return", "ep_length")      # with the terminal_* rows: written only where the step ended an episode


def _same_step(x, y, tag, rows=None):
    """Every tensor of two single steps bit for bit, over the drones `rows` (None = all): the rows that are written only where done are
    compared where done (elsewhere each env's buffer holds what its own earlier steps left)."""
    assert x.keys() == y.keys(), (tag, sorted(x), sorted(y))
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])
    done = pick(x["done"]).bool()
    for k in x:
        if k == "done_mask" and rows is not None:
            continue                                   # one ballot word per 64 drones: not separable by drone
        a, b = (x[k], y[k]) if k == "done_mask" else (pick(x[k]), pick(y[k]))
        if k.startswith("terminal_") or k in EPISODE_END:
            a, b = a[done], b[done]
        assert torch.equal(a, b), (tag, k)


def _same_launch(x, y, tag, skip=()):
    """Every tensor of two fused launches bit for bit (rollout_tensor hands out zeroed buffers, so unwritten rows agree too)."""
    assert x.keys() == y.keys(), (tag, sorted(x), sorted(y))
    for k in x:
        assert k in skip or torch.equal(x[k], y[k]), (tag, k)


COUNTERS = ("episodes", "truncated", "completed", "sum_ep_len", "sum_found_targets")


def _same_stats_since(a, a0, b, b0, tag):
    """dn_stats of two envs since their marks a0 / b0: the counters as integers, the return sum in its device unit of 1e-6, and the
    step total outright (it is the step counter times the fleet)."""
    for k in COUNTERS:
        assert a[k] - a0[k] == b[k] - b0[k], (tag, k)
    assert round((a["sum_ep_return"] - a0["sum_ep_return"]) * 1e6) == round((b["sum_ep_return"] - b0["sum_ep_return"]) * 1e6), tag
    assert a["env_steps"] == b["env_steps"], tag


# ---- a. the round trip is the identity on the device words ------------------------------------------------------------------------------
@pytest.mark.parametrize("norm_rew", [True, False], ids=["norm_rew", "plain"])
@pytest.mark.parametrize("waves", [("1", "5"), ("5", "1")], ids=["one_wave_to_five", "five_waves_to_one"])
def test_round_trip_is_the_identity_on_the_device_words(waves, norm_rew, monkeypatch):
    """A normalised fleet flies 40 steps (every drone ends at least two episodes), its blob goes into a twin created with another seed
    (no noise here: the seed keys nothing) after the twin's own reset, and the twin's get_state must equal the blob in every field,
    rms_m2 included.  Then both continue -- one launch of K = 1, one of K = 7, and 7 single steps, each from a fleet of its own -- and
    every returned tensor, the final state and the statistics must agree bit for bit.  The source runs under DN_WAVES = 1 and the twin
    under DN_WAVES = 5 and the other way round: the blob does not know the kernel shape.  DN_WAVES = 5 is the five-wave kernel in the
    plain configuration and falls back to three waves with the reward normaliser on (csrc/dn_shapes.h): both are flown, the first for
    the kernel, the second for the rr_* words of the blob."""
    pkg = _pkg()
    want_shape = {"1": 1, "5": 3 if norm_rew else 5}
    for mode, K, n in (("launch", 1, N_LAUNCH), ("launch", 7, N_LAUNCH), ("single", 7, N_SINGLE)):
        tag = f"{mode} K={K}"
        rng = np.random.default_rng(100 + K + n)
        monkeypatch.setenv("DN_WAVES", waves[0])
        src = _env(pkg, n, seed=3, norm_rew=norm_rew)
        monkeypatch.setenv("DN_WAVES", waves[1])
        twin = _env(pkg, n, seed=99, norm_rew=norm_rew)
        assert (src.kernel_waves(fused=True), twin.kernel_waves(fused=True)) == (want_shape[waves[0]], want_shape[waves[1]])
        ends = _fly(src, rng, FLOWN, fused=mode == "launch")
        assert ends >= 2 * n, (tag, ends)
        st, sc = src.get_state(), src.step_count
        assert sc == FLOWN and (st["rms_count"] > FLOWN).all() and (st["rms_m2"] > 0).all()
        assert np.array_equal(st["rms_var"], st["rms_m2"] / st["rms_count"][:, None])
        if norm_rew:
            assert (st["rr_count"] > FLOWN).all() and float(np.abs(st["rr_var"] - 1.0).min()) > 0.0
        lossy = _lossy_words(st)
        print(f"{tag} {waves[0]}->{waves[1]} norm_rew={norm_rew}: {lossy} of {st['rms_m2'].size} second moments are not what the rule before ABI 10 restores")
        assert lossy > 0, tag
        _restore(twin, st, sc)
        _same_blob(twin.get_state(), st, tag + ": restored")
        s0, t0 = src.stats(), twin.stats()
        acts = _acts(rng, n, K)
        if mode == "launch":
            a = {k: v.clone() for k, v in src.rollout_tensor(acts, want_terminal=True).items()}
            _same_launch(a, twin.rollout_tensor(acts, want_terminal=True), tag)
            ends = int(a["done"].sum())
        else:
            ends = 0
            for t in range(K):
                a = _step(src, acts[t])
                _same_step(a, _step(twin, acts[t]), f"{tag} t={t}")
                ends += int(a["done"].sum())
        assert ends > 0 or K == 1, tag
        _same_blob(twin.get_state(), src.get_state(), tag + ": continued")
        _same_stats_since(src.stats(), s0, twin.stats(), t0, tag)
        src.close(), twin.close()


# ---- b. set_attr on one drone is local ----------------------------------------------------------------------------------------------------
def test_set_attr_on_one_drone_leaves_every_other_drone_alone(monkeypatch):
    """DroneVecEnv.set_attr is a get_state / set_state round trip of the whole fleet.  Two fleets are restored from one blob; on one,
    drone 17's `_steps` is set to 3.  The state bytes of every other drone must be those of the blob, and over 7 more steps every other
    drone's outputs and final state must be the untouched fleet's."""
    monkeypatch.delenv("DN_WAVES", raising=False)
    pkg = _pkg()
    n, who = N_LAUNCH, 17
    rng = np.random.default_rng(21)
    src = _env(pkg, n, norm_rew=True)
    assert _fly(src, rng, FLOWN, fused=True) >= 2 * n
    st, sc = src.get_state(), src.step_count
    lossy = _lossy_words(st[np.arange(n) != who])
    assert lossy > 0
    one, twin = _env(pkg, n, seed=7, norm_rew=True), _env(pkg, n, seed=8, norm_rew=True)
    _restore(one, st, sc)
    _restore(twin, st, sc)
    assert int(st["steps"][who]) != 3
    one.set_attr("_steps", 3, indices=[who])
    others = np.arange(n) != who
    after = one.get_state()
    _same_blob(after, st, "after set_attr", rows=others)
    assert int(after["steps"][who]) == 3 and one.get_attr("_steps", indices=[who]) == [3]
    for k in st.dtype.names:
        if k != "steps":
            assert np.array_equal(after[k][who], st[k][who]), k
    rows = torch.from_numpy(others).to(DEV)
    ends = 0
    for t, a in enumerate(_acts(rng, n, 7)):
        x = _step(one, a)
        _same_step(x, _step(twin, a), f"t={t}", rows=rows)
        ends += int(x["done"][rows].sum())
    assert ends > 0
    _same_blob(one.get_state(), twin.get_state(), "7 steps on", rows=others)
    for e in (src, one, twin):
        e.close()


# ---- c. edits are honoured ----------------------------------------------------------------------------------------------------------------
def test_edited_statistics_are_honoured_and_bad_counts_refused(monkeypatch):
    """rms_m2 is a hint: it is taken while it divides to the var beside it.  An edited var (hint left stale) reads back exactly and is
    what the next observation is normalised with -- the same bits as a fleet whose rms_m2 was set to second_moment(0.25, count) by hand;
    a doubled count keeps every var as given (2 count x var has the bits of count x var: an M2 that divides back exists; for an
    arbitrary new count none may, csrc/dn_second_moment.h); a zeroed rms_m2 (a producer from before ABI 10) restores statistics that
    read back the same; a count that is zero, negative, NaN or infinite is refused and nothing is written."""
    monkeypatch.delenv("DN_WAVES", raising=False)
    pkg = _pkg()
    n = N_SINGLE
    rng = np.random.default_rng(33)
    src = _env(pkg, n)
    assert _fly(src, rng, FLOWN, fused=False) >= 2 * n
    st, sc = src.get_state(), src.step_count
    count = st["rms_count"]
    one, two = _env(pkg, n, seed=5), _env(pkg, n, seed=6)
    # an edited var
    edited = st.copy()
    edited["rms_var"][:, 3] = 0.25
    assert not (edited["rms_m2"][:, 3] / count == 0.25).any()
    by_hand = edited.copy()
    by_hand["rms_m2"][:, 3] = _old_rule(0.25, count)
    _restore(one, edited, sc)
    _restore(two, by_hand, sc)
    back = one.get_state()
    assert np.array_equal(back["rms_var"][:, 3], np.full(n, 0.25)) and np.array_equal(back["rms_m2"][:, 3], by_hand["rms_m2"][:, 3])
    _same_blob(back, two.get_state(), "edited var")
    keep = np.arange(13) != 3
    assert np.array_equal(back["rms_m2"][:, keep], st["rms_m2"][:, keep]), "the other columns keep their own words"
    keep = torch.from_numpy(keep).to(DEV)
    a = _acts(rng, n, 1)[0]
    x, y, z = _step(one, a), _step(two, a), _step(src, a)
    _same_step(x, y, "edited var: the next observation")
    assert torch.equal(x["obs"][:, keep], z["obs"][:, keep]) and not torch.equal(x["obs"][:, 3], z["obs"][:, 3])
    # an edited count
    doubled = st.copy()
    doubled["rms_count"] = 2.0 * count
    one.set_state(doubled)
    back = one.get_state()
    assert np.array_equal(back["rms_count"], 2.0 * count) and np.array_equal(back["rms_var"], st["rms_var"])
    assert np.array_equal(back["rms_m2"], _old_rule(st["rms_var"], 2.0 * count[:, None]))
    # a producer that does not fill the hint
    old = st.copy()
    old["rms_m2"] = 0.0
    one.set_state(old)
    back = one.get_state()
    assert np.array_equal(back["rms_var"], st["rms_var"]) and np.array_equal(back["rms_m2"], _old_rule(st["rms_var"], count[:, None]))
    lossy = int((back["rms_m2"] != st["rms_m2"]).sum())
    print(f"zeroed hint: {lossy} of {back['rms_m2'].size} second moments come back as a neighbour of the device's word")
    assert lossy > 0, "the blob has no word for which the hint matters"
    # counts that are no counts
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        wrong = st.copy()
        wrong["rms_count"][5] = bad
        with pytest.raises(pkg.DroneNavError, match="rms_count"):
            one.set_state(wrong)
        _same_blob(one.get_state(), back, f"after the refused count {bad}")
    for e in (src, one, two):
        e.close()


# ---- d. reshard ---------------------------------------------------------------------------------------------------------------------------
def test_a_resharded_fleet_continues_with_the_whole_fleets_bits(monkeypatch):
    """The blob of a 132-drone normalised fleet with action and observation noise goes, in halves, to two 66-drone environments with
    env_id_offset 0 and 66 (the same Philox key: the noise is keyed by seed, global drone id and step) and the same step counter.  Over
    7 steps -- single steps: dn_step_many wants a multiple of four drones -- the halves must continue with the whole fleet's bits."""
    monkeypatch.delenv("DN_WAVES", raising=False)
    pkg = _pkg()
    n, half = N_LAUNCH, N_LAUNCH // 2
    rng = np.random.default_rng(44)
    whole = _env(pkg, n, seed=11, norm_rew=True, **NOISE)
    assert _fly(whole, rng, FLOWN, fused=True) >= 2 * n
    st, sc = whole.get_state(), whole.step_count
    assert _lossy_words(st[:half]) > 0 and _lossy_words(st[half:]) > 0
    parts = [_env(pkg, half, seed=11, norm_rew=True, env_id_offset=off, **NOISE) for off in (0, half)]
    for e, rows in zip(parts, (slice(0, half), slice(half, n))):
        _restore(e, st[rows], sc)
    _same_blob(np.concatenate([e.get_state() for e in parts]), st, "restored halves")
    w0 = whole.stats()
    ends = 0
    for t, a in enumerate(_acts(rng, n, 7)):
        w = _step(whole, a)
        ends += int(w["done"].sum())
        for e, rows in zip(parts, (slice(0, half), slice(half, n))):
            got = _step(e, a[rows].contiguous())
            _same_step(got, {k: (v if k == "done_mask" else v[rows]) for k, v in w.items()}, f"t={t} rows {rows.start}..", rows=slice(None))
    assert ends > 0
    _same_blob(np.concatenate([e.get_state() for e in parts]), whole.get_state(), "7 steps on")
    w1, p = whole.stats(), [e.stats() for e in parts]
    for k in COUNTERS:
        assert w1[k] - w0[k] == p[0][k] + p[1][k], k
    for e in [whole] + parts:
        e.close()


# ---- e. one whole checkpoint ----------------------------------------------------------------------------------------------------------------
def _everything(pkg, n, seed):
    """Every per-drone model and every row family on one env, with the normalisers: a track bank (tests/track_support.py BANK),
    dynamics, gusty wind, actuator, sensor, both noise streams, goal + privileged + history rows."""
    return S.bank_env(pkg, n, resample=True, max_steps=12, seed=seed, normalize_obs=True, norm_rew=True, clip_rew=True,
                      dynamics=pkg.DynamicsRandomization(**BODY), wind=pkg.WindDisturbance(**GUSTY), actuator=pkg.ActuatorModel(**FULL),
                      sensor=pkg.SensorModel(latency=(0, 8), bias=AMPS), goal=pkg.GoalObservation("world"),
                      privileged=pkg.PrivilegedObservation(), history=pkg.HistoryObservation(frames=2, actions=2, goal=True), **NOISE)


def _models(env):
    out = dict(dynamics=env.get_dynamics().clone(), tracks=env.track_ids.clone(), history=env.history.clone())
    out.update({"wind_" + k: v.clone() for k, v in zip(("mean", "gust"), env.get_wind())})
    out.update({"actuator_" + k: v.clone() for k, v in env.get_actuator().items()})
    out.update({"sensor_" + k: v.clone() for k, v in env.get_sensor().items()})
    return out


def test_a_checkpoint_with_every_model_and_the_normaliser_on_continues_bit_for_bit(monkeypatch):
    """ONE environment takes everything at once -- track bank, DynamicsRandomization, gusty WindDisturbance, ActuatorModel, SensorModel,
    action and observation noise, goal, privileged and history rows, observation and reward normalisers, reward clipping -- so there is
    no split.  25 steps (a launch of 20 and one of 5: the actuator's ring of 8 and the sensor's of 9 have wrapped), then the checkpoint:
    get_state, step_count, get_dynamics / get_wind / get_actuator / get_sensor, track_ids and env.history (a plain tensor the caller
    saves, DroneVecEnv.step_tensor).  It is restored in the order include/dronenav.h prescribes -- set_tracks before set_state, the step
    counter before set_sensor -- into a second env that has already flown three steps of its own.  That env has the SAME seed: the seed
    is configuration (dn_config.seed), the key of every draw after the restore, not state a blob could carry.  Two launches of K = 7
    follow on both: every returned tensor, the final state, every model's arrays, the tracks and the statistics bit for bit."""
    monkeypatch.delenv("DN_WAVES", raising=False)
    pkg = _pkg()
    n = N_LAUNCH
    rng = np.random.default_rng(55)
    src = _everything(pkg, n, seed=S.SEED)
    src.reset_tensor()
    ends = sum(int(src.rollout_tensor(_acts(rng, n, K))["done"].sum()) for K in (20, 5))
    assert ends >= n
    st, sc, saved = src.get_state(), src.step_count, _models(src)
    assert sc == 25 and _lossy_words(st) > 0
    assert len(set(saved["tracks"].cpu().tolist())) >= 4, "the fleet is spread over the bank at the checkpoint"
    twin = _everything(pkg, n, seed=S.SEED)
    twin.reset_tensor()
    twin.rollout_tensor(_acts(np.random.default_rng(56), n, 3))
    twin.set_tracks(saved["tracks"])
    twin.set_state(st)
    twin.set_dynamics(saved["dynamics"])
    twin.set_wind(mean=saved["wind_mean"], gust=saved["wind_gust"])
    twin.set_actuator(**{k[len("actuator_"):]: v for k, v in saved.items() if k.startswith("actuator_")})
    twin.step_count = sc
    twin.set_sensor(**{k[len("sensor_"):]: v for k, v in saved.items() if k.startswith("sensor_")})
    twin.history.copy_(saved["history"])
    _same_blob(twin.get_state(), st, "restored")
    for k, v in _models(twin).items():
        assert torch.equal(v, saved[k]), ("restored", k)
    s0, t0, ts0, tt0 = src.stats(), twin.stats(), src.track_stats(), twin.track_stats()
    ended = torch.zeros(n, dtype=torch.bool, device=DEV)
    for launch in range(2):
        acts = _acts(rng, n, 7)
        a = {k: v.clone() for k, v in src.rollout_tensor(acts, want_terminal=True).items()}
        assert {"privileged", "goal", "history", "terminal_history", "track", "terminal_track"} <= a.keys()
        b = twin.rollout_tensor(acts, want_terminal=True)
        # terminal_track is the track of the drone's most recently ended episode: no checkpoint carries it (dn_set_tracks takes the
        # current tracks only), so it is compared for the drones that have ended an episode since the restore
        _same_launch(a, b, f"launch {launch}", skip=("terminal_track",))
        ended |= a["done"].bool().any(dim=0)
        assert torch.equal(a["terminal_track"][ended], b["terminal_track"][ended]), f"launch {launch}: terminal_track"
    assert bool(ended.all())
    _same_blob(twin.get_state(), src.get_state(), "14 steps on")
    got = _models(twin)
    for k, v in _models(src).items():
        assert torch.equal(got[k], v), ("14 steps on", k)
    _same_stats_since(src.stats(), s0, twin.stats(), t0, "14 steps on")
    assert np.array_equal(src.track_stats() - ts0, twin.track_stats() - tt0)
    src.close(), twin.close()
