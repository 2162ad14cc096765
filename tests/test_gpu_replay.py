"""SAC replay minibatches on the device (include/dronenav.h dn_replay_sample, csrc/dn_replay.hip, replay.py) on the HIP path.  Every
comparison is exact, through int32 views; the reference is NumPy indexing on the host (tests/replay_support.py), so there is no tolerance.

 1. both layouts over a covering selection of edge shapes -- T in {1, 2, 3, 5}, N in {1, 63, 64, 65}, D in {1, 13, 64}, A in {1, 4, 8},
    batch in {1, 63, 64, 65, 257, 1025}: 63 / 65 rows leave a last block of 15 / 1 rows, 257 and 1025 span many blocks -- and every
    window: not full at pos 1 and T - 1, full at pos 0, full at pos 1, mid and T - 1.  On each: `indices` equals dn_replay_indices and
    never names the skipped slot, a done row takes terminal_obs, a row at slot T - 1 that is not done takes the ring's spare row T, a
    timeout row has dones == 0;
 2. fewer rows than batch_size leave the rest of every static output untouched;
 3. the caller's indices reproduce torch indexing; out-of-range values read the clamped transition;
 4. the output equals RingReplayBuffer.sample / ReplayBuffer.sample with the sampler's (t, e) substituted for torch's draws;
 5. on buffers the OffPolicyCollector filled, with a torch callable and with a FusedSacActor;
 6. under graph replay with draw_offset;
 7. source offsets beyond 2^31 words.

The sources are random int32 bit patterns viewed as float32 (NaN payloads included) and the flags hold every combination of done and
timeout, so a wrong row, a wrong branch or a touched bit cannot pass."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import replay_support as R  # noqa: E402
from gpu_support import DEV  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402

SEED, DRAW = 11, 5
LAYOUTS = pytest.mark.parametrize("layout", [R.PLAIN, R.RING], ids=["plain", "ring"])
# T, N, D, A, batch: every value of every list above appears, with both layouts
SHAPES = [(1, 1, 1, 1, 1), (2, 63, 13, 4, 63), (3, 64, 64, 8, 64), (5, 65, 13, 1, 65), (3, 63, 1, 8, 257), (5, 64, 13, 4, 1025),
          (2, 65, 64, 4, 257), (1, 64, 13, 8, 1025), (5, 1, 64, 1, 63), (2, 1, 13, 4, 1)]
PATTERN = 0x7FC12345                    # what the untouched rows of an output hold


def _windows(t):
    """(pos, full): not full at pos 1 and T - 1; full at pos 0; full at pos 1, mid and T - 1."""
    inside = lambda ps: sorted({p for p in ps if 1 <= p < t})      # noqa: E731
    return [(p, False) for p in inside((1, t - 1))] + [(0, True)] + [(p, True) for p in inside((1, t // 2, t - 1))]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _same(got, want, tag):
    """got: a device tensor; want: a NumPy array of the same words."""
    w = _dev(want)
    assert got.shape == w.shape and got.dtype == w.dtype and torch.equal(_bits(got), _bits(w)), tag


@functools.lru_cache(maxsize=None)
def _buffer(layout, t, n, d, a):
    """(the NumPy sources, the collector's buffer object holding the same words on the device), made once per shape."""
    pkg = _pkg()
    host = R.build(layout, t, n, d, a)
    buf = (pkg.RingReplayBuffer if layout == R.RING else pkg.ReplayBuffer)(t, n, d, a, DEV)
    for name, x in host.items():
        getattr(buf, name).copy_(_dev(x))
    return host, buf


def _check(got, layout, host, flat, n, tag):
    """The six outputs against plain indexing at the flat indices `flat`."""
    flat = np.asarray(flat, np.int64)
    want = R.sample(layout, host, flat // n, flat % n)
    for k in R.FIELDS:
        _same(got[k], want[k], (tag, k))
    _same(got["indices"], flat, (tag, "indices"))


# ---- 1. edge shapes and windows -----------------------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("t,n,d,a,batch", SHAPES)
def test_every_window_is_the_reference(layout, t, n, d, a, batch):
    pkg = _pkg()
    host, buf = _buffer(layout, t, n, d, a)
    s = pkg.ReplaySampler(buf, batch, seed=SEED)
    for pos, full in _windows(t):
        buf.pos, buf.full = pos, full
        valid, skip = R.window(layout, t, pos, full)
        tag = (layout, t, n, d, a, batch, pos, full)
        for draw in (DRAW, (1 << 64) - 1):
            got = s.sample(draw=draw)
            flat = R.flat(SEED, draw, valid, n, skip, 0, batch)
            assert np.array_equal(s.indices(draw).numpy(), flat), tag
            _check(got, layout, host, flat, n, tag)
            slot, env = flat // n, flat % n
            assert 0 <= slot.min() and slot.max() < valid + (skip >= 0) and not (slot == skip).any(), tag
            if layout == R.RING:                                # the rules by name, from the sources themselves
                nxt, dn = got["next_obs"].cpu().numpy().view(np.int32), got["dones"].cpu().numpy()
                done, late = host["done_flags"][slot, env] != 0, host["timeout_flags"][slot, env] != 0
                assert np.array_equal(nxt[done], host["terminal_obs"][slot, env].view(np.int32)[done]), (tag, "a done row takes terminal_obs")
                last = ~done & (slot == t - 1)
                assert np.array_equal(nxt[last], host["obs_ring"][t, env].view(np.int32)[last]), (tag, "slot T - 1 takes the spare row")
                assert (dn[late] == 0).all() and (dn[done & ~late] == 1).all() and (dn[~done] == 0).all(), (tag, "dones")
    buf.pos, buf.full = 0, False
    with pytest.raises(RuntimeError, match="the replay buffer is empty"):
        s.sample()


def test_every_kind_of_row_was_seen():
    """1025 rows from a full ring of 3 x 65 mid-cycle hold done rows, rows at slot T - 1 that are not done, timeout rows that are done, and
    rows that are neither: the rules checked above are exercised, not vacuous."""
    pkg = _pkg()
    t, n = 3, 65
    host, buf = _buffer(R.RING, t, n, 13, 4)
    buf.pos, buf.full = 1, True
    s = pkg.ReplaySampler(buf, 1025, seed=SEED)
    flat = s.sample(draw=DRAW)["indices"].cpu().numpy()
    slot, env = flat // n, flat % n
    done, late = host["done_flags"][slot, env] != 0, host["timeout_flags"][slot, env] != 0
    for name, rows in (("done", done), ("done and timeout", done & late), ("last slot, not done", ~done & (slot == t - 1)), ("plain", ~done & ~late)):
        assert rows.sum() >= 16, name
    assert set(slot.tolist()) == {0, 2}


# ---- 2. fewer rows than batch_size --------------------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("count", [1, 15, 16, 17, 256])
def test_rows_beyond_count_are_left_untouched(layout, count):
    pkg = _pkg()
    t, n, d, a = 3, 65, 13, 4
    host, buf = _buffer(layout, t, n, d, a)
    buf.pos, buf.full = 2, True
    valid, skip = R.window(layout, t, 2, True)
    s = pkg.ReplaySampler(buf, 257, seed=SEED)
    for v in s.out.values():
        (v.view(torch.int32) if v.dtype == torch.float32 else v).fill_(PATTERN)
    got = s.sample(count, draw=DRAW)
    assert all(v.shape[0] == count for v in got.values())
    _check(got, layout, host, R.flat(SEED, DRAW, valid, n, skip, 0, count), n, (layout, count))
    torch.cuda.synchronize()
    for k, v in s.out.items():
        rest = v[count:]
        assert bool(((rest.view(torch.int32) if rest.dtype == torch.float32 else rest) == PATTERN).all()), (layout, count, k)


# ---- 3. the caller's indices ----------------------------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("t,n,d,a", [(1, 1, 1, 1), (3, 65, 13, 4), (5, 64, 64, 8)])
def test_the_callers_indices_reproduce_torch_indexing(layout, t, n, d, a):
    pkg = _pkg()
    host, buf = _buffer(layout, t, n, d, a)
    buf.pos, buf.full = 0, True
    s = pkg.ReplaySampler(buf, 1025, seed=SEED)
    picked = np.random.default_rng(t * n).integers(0, t * n, 1025)                 # with repeats
    idx = _dev(picked)
    got = s.sample(indices=idx)
    _check(got, layout, host, picked, n, (layout, t, n, "indices"))
    ti, ei = idx // n, idx % n
    ring = layout == R.RING
    obs = (buf.obs_ring if ring else buf.obs)[ti, ei]
    nxt = torch.where(buf.done_flags[ti, ei].bool()[:, None], buf.terminal_obs[ti, ei], buf.obs_ring[ti + 1, ei]) if ring else buf.next_obs[ti, ei]
    for k, want in (("obs", obs), ("next_obs", nxt), ("actions", buf.actions[ti, ei]), ("rewards", buf.rewards[ti, ei])):
        assert torch.equal(_bits(got[k]), _bits(want)), (layout, t, n, k)
    with pytest.raises(ValueError, match="with indices, draw must be None"):
        s.sample(indices=idx, draw=3)
    with pytest.raises(ValueError, match="indices must be a dense int64 tensor"):
        s.sample(indices=idx.int())


@LAYOUTS
@pytest.mark.parametrize("t,n", [(1, 1), (3, 65), (5, 64)])
def test_out_of_range_indices_read_the_clamped_transition(layout, t, n):
    pkg = _pkg()
    host, buf = _buffer(layout, t, n, 13, 4)
    buf.pos, buf.full = 0, True
    m = t * n
    asked = np.array([-5, m, m + 3, 1 << 40, -(1 << 62), (1 << 63) - 1, -(1 << 63), 0, m - 1, -1], np.int64)
    slot, env = R.clamp(asked, t, n)
    assert slot.tolist()[:2] == [0, t - 1] and env.tolist()[:3] == [0, 0, 3 % n] and (slot < t).all() and (env < n).all()
    got = pkg.ReplaySampler(buf, 16).sample(indices=_dev(asked))
    _check(got, layout, host, slot * n + env, n, (layout, t, n))


# ---- 4. equivalence with the existing methods ---------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("pos,full", [(2, False), (0, True), (2, True)])
def test_the_output_is_the_buffers_own_sample_at_the_same_draws(layout, pos, full, monkeypatch):
    """RingReplayBuffer.sample / ReplayBuffer.sample, unchanged, with the sampler's (t, e) in place of their torch.randint draws."""
    pkg = _pkg()
    n, batch = 65, 257
    _, buf = _buffer(layout, 3, n, 13, 4)
    buf.pos, buf.full = pos, full
    got = {k: v.clone() for k, v in pkg.ReplaySampler(buf, batch, seed=SEED).sample(draw=DRAW).items()}
    ti, ei = got["indices"] // n, got["indices"] % n
    if layout == R.RING:
        monkeypatch.setattr(buf, "_sample_slots", lambda batch_size, generator=None: (ti, ei), raising=True)
    else:
        draws = [ti, ei]
        monkeypatch.setattr(torch, "randint", lambda *args, **kw: draws.pop(0))
    want = buf.sample(batch)
    monkeypatch.undo()
    assert set(want) == set(R.FIELDS)
    for k in R.FIELDS:
        assert torch.equal(_bits(got[k]), _bits(want[k])), (layout, pos, full, k)


# ---- 5. on collected buffers ----------------------------------------------------------------------------------------------------------------
def _check_collected(pkg, buf, tag):
    n = buf.num_envs
    s = pkg.ReplaySampler(buf, 257, seed=SEED)
    got = s.sample(draw=DRAW)
    assert np.array_equal(got["indices"].cpu().numpy(), s.indices(DRAW).numpy()), tag
    ti, ei = got["indices"] // n, got["indices"] % n
    skipped = buf.pos if hasattr(buf, "obs_ring") and buf.pos else -1           # every slot of a ReplayBuffer is whole
    assert buf.full and not bool((ti == skipped).any()) and int(ti.max()) == buf.buffer_size - 1, tag
    want = dict(obs=buf.obs[ti, ei], next_obs=buf.next_obs[ti, ei], actions=buf.actions[ti, ei], rewards=buf.rewards[ti, ei],
                dones=buf.dones[ti, ei] * (1.0 - buf.timeouts[ti, ei]))
    for k in R.FIELDS:
        assert torch.equal(_bits(got[k]), _bits(want[k])), (tag, k)
    return got


def test_on_the_buffers_the_off_policy_collector_fills():
    """A ring of 4 slots: one and a half cycles with a torch callable (ReplayBuffer, full, mid-cycle), then collect_cycle with a
    FusedSacActor (RingReplayBuffer, full at a cycle boundary) and two more steps (mid-cycle: slot 2 is being replaced)."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    from drl_dronenavigation_amd.collector import OffPolicyCollector, ReplayBuffer, RingReplayBuffer
    n, T = 256, 4
    kw = dict(max_steps=3, normalize_obs=False, act_noise_sigma=0.002, obs_noise_sigma=0.01, seed=9)
    env = pkg.DroneVecEnv(tracks.reaching(), n, device=DEV, **kw)
    w = (torch.randn(13, 4, generator=torch.Generator(device="cpu").manual_seed(5)) * 0.02).to(DEV)
    col = OffPolicyCollector(env, lambda obs: 0.0922 + obs @ w * 0.001, buffer_size=T)
    buf = col.collect(T + T // 2)
    assert isinstance(buf, ReplayBuffer) and buf.full and buf.pos == 2
    got = _check_collected(pkg, buf, "torch callable")
    assert float(got["dones"].sum()) + float(buf.timeouts.sum()) > 0                # episodes of 3 steps ended inside the ring
    env.close()

    env = pkg.DroneVecEnv(tracks.reaching(), n, device=DEV, **kw)
    torch.manual_seed(0)
    col = OffPolicyCollector(env, pkg.FusedSacActor(pkg.SacActor().to(DEV), n, DEV, grade="fp32"), buffer_size=T, seed=2)
    buf = col.collect_cycle()
    assert isinstance(buf, RingReplayBuffer) and buf.full and buf.pos == 0
    _check_collected(pkg, buf, "FusedSacActor, cycle boundary")
    col.collect(2)
    assert buf.pos == 2
    _check_collected(pkg, buf, "FusedSacActor, mid-cycle")
    env.close()


# ---- 6. graph -----------------------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_graph_replay_draws_afresh_with_the_draw_offset(layout):
    """One eager call, then sample() captured on one stream and replayed twice with draw_offset incremented in between: each replay is
    the eager call of draw BASE + offset, in the same static tensors."""
    pkg = _pkg()
    t, n, batch, base = 3, 65, 257, 40
    host, buf = _buffer(layout, t, n, 13, 4)
    buf.pos, buf.full = 1, True
    valid, skip = R.window(layout, t, 1, True)
    s, eager = pkg.ReplaySampler(buf, batch, seed=SEED), pkg.ReplaySampler(buf, batch, seed=SEED)
    s.sample(draw=base)
    where = {k: v.data_ptr() for k, v in s.out.items()}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = s.sample(draw=base)
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert int(s.draw_offset) == replay
        _check(captured, layout, host, R.flat(SEED, base + replay, valid, n, skip, 0, batch), n, (layout, "replay", replay))
        want = eager.sample(draw=base + replay)
        for k in want:
            assert torch.equal(_bits(captured[k]), _bits(want[k])), (layout, replay, k)
        s.draw_offset.add_(1)
    assert {k: v.data_ptr() for k, v in s.out.items()} == where and all(captured[k].data_ptr() == where[k] for k in where)


def test_the_default_draw_is_a_host_counter():
    pkg = _pkg()
    host, buf = _buffer(R.RING, 3, 65, 13, 4)
    buf.pos, buf.full = 0, True
    s = pkg.ReplaySampler(buf, 64, seed=SEED)
    for draw in range(3):
        assert s.draw == draw
        _check(s.sample(), R.RING, host, R.flat(SEED, draw, 3, 65, -1, 0, 64), 65, draw)
    s.sample(draw=77)
    assert s.draw == 3                                          # an explicit draw leaves the counter alone


# ---- 7. beyond 2^31 words -----------------------------------------------------------------------------------------------------------------
def test_source_offsets_beyond_2_to_31_words():
    """A ring of 5 slots x 2^23 drones x 64 columns: slot 4 and the spare row lie beyond word 2^31 of the ring (about 26 GB in all).  Word
    i of a row is a function of its (row, drone, column), filled row by row; the reference is torch indexing on the device."""
    pkg = _pkg()
    t, n, d, a, batch = 5, 1 << 23, 64, 1, 1025
    assert t * n * d > 1 << 31
    buf = pkg.RingReplayBuffer(t, n, d, a, DEV)
    cell = torch.arange(n * d, dtype=torch.int32, device=DEV).view(n, d)
    for row in range(t + 1):
        buf.obs_ring[row].view(torch.int32).copy_(cell).add_(row << 27)
    for row in range(t):
        buf.terminal_obs[row].view(torch.int32).copy_(cell).add_((row << 27) + 0x40000000)
        buf.actions[row].view(torch.int32).copy_(cell[:, :1]).add_(row << 27)
        buf.rewards[row].view(torch.int32).copy_(cell[:, 0]).add_(row << 27).neg_()
    buf.done_flags.copy_((torch.arange(n, device=DEV) % 3 == 0).to(torch.uint8))
    buf.pos, buf.full = 0, True
    got = pkg.ReplaySampler(buf, batch, seed=SEED).sample(draw=DRAW)
    flat = R.flat(SEED, DRAW, t, n, -1, 0, batch)
    _same(got["indices"], flat, "indices")
    ti, ei = got["indices"] // n, got["indices"] % n
    assert int((ti == t - 1).sum()) > 100
    done = buf.done_flags[ti, ei].bool()
    want = dict(obs=buf.obs_ring[ti, ei], next_obs=torch.where(done[:, None], buf.terminal_obs[ti, ei], buf.obs_ring[ti + 1, ei]),
                actions=buf.actions[ti, ei], rewards=buf.rewards[ti, ei], dones=done.float())
    for k in R.FIELDS:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
    first = got["obs"].view(torch.int32)[:, 0].cpu().numpy().astype(np.int64)     # and against the fill rule itself
    assert np.array_equal(first, ((flat % n) * d + ((flat // n) << 27)).astype(np.int32).astype(np.int64))
    del buf, got, want, cell
    torch.cuda.empty_cache()
