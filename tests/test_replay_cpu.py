"""SAC replay minibatches on the device (include/dronenav.h dn_replay_sample), the part that needs no GPU: the two entry points are
declared, exported and bound; the layouts of dn_replay_config and dn_replay_source, compiled from the header; the keyed draw through the
real library against the NumPy statement of tests/replay_support.py and its known answers, and as a stand-alone host program, plainly and
under the address and undefined-behaviour sanitizers; its uniformity; every refusal of dn_replay_sample, which validates before its first
device call, so the pointers here are never followed, and of dn_replay_indices; the Python surface's own refusals."""
import ctypes as C
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import abi_support as abi  # noqa: E402
import host_program_support  # noqa: E402
import replay_support as R  # noqa: E402

NAMES = ("dn_replay_indices", "dn_replay_sample")
INVALID = -1


@pytest.fixture(scope="module")
def pkg():
    import drl_dronenavigation_amd as p
    p.build.build_library()
    return p


# ---- names and layouts ----------------------------------------------------------------------------------------------------------------
def test_the_names_are_declared_exported_and_bound(pkg):
    code = abi.header_text()
    for define in ("DN_REPLAY_PLAIN 0", "DN_REPLAY_RING 1", "DN_REPLAY_MAX_OBS 64", "DN_REPLAY_MAX_ACT 8"):
        assert re.search(r"#define %s\b" % define, code), define
    assert re.search(r"typedef struct dn_replay_config \{\s*uint64_t seed;\s*uint64_t draw;\s*int64_t buffer_size;\s*int64_t n_envs;\s*int64_t valid;\s*"
                     r"int64_t skip;\s*int32_t obs_dim;\s*int32_t act_dim;\s*int32_t layout;\s*int32_t reserved;\s*\} dn_replay_config;", code)
    assert re.search(r"typedef struct dn_replay_source \{\s*const void \*obs;\s*const void \*next_obs;\s*const void \*actions;\s*const void \*rewards;\s*"
                     r"const void \*dones;\s*const void \*timeouts;\s*\} dn_replay_source;", code)
    abi.check_names(*NAMES)
    assert pkg.ReplaySampler is pkg.replay.ReplaySampler and "ReplaySampler" in pkg.__all__
    abi.check_version()
    build = pkg.build
    assert "dn_replay.hip" in build.SOURCES and "dn_replay_draw.h" in build.HEADERS


def test_struct_layouts_compiled_from_the_header(pkg):
    """dn_replay_config: 64 bytes, seed 0, draw 8, buffer_size 16, n_envs 24, valid 32, skip 40, obs_dim 48, act_dim 52, layout 56, reserved
    60; dn_replay_source: 48 bytes, six pointers -- by the C compiler from the header itself, and the ctypes mirrors agree."""
    K = pkg._capi
    abi.check_layout(K.DnReplayConfig, 64, seed=0, draw=8, buffer_size=16, n_envs=24, valid=32, skip=40, obs_dim=48, act_dim=52, layout=56, reserved=60)
    abi.check_layout(K.DnReplaySource, 48, obs=0, next_obs=8, actions=16, rewards=24, dones=32, timeouts=40)
    consts = abi.compiled().constants
    assert [consts["DN_REPLAY_" + k] for k in ("PLAIN", "RING", "MAX_OBS", "MAX_ACT")] == [0, 1, 64, 8]
    assert (K.REPLAY_PLAIN, K.REPLAY_RING, K.REPLAY_MAX_OBS, K.REPLAY_MAX_ACT) == (0, 1, 64, 8)
    assert (R.PLAIN, R.RING) == (0, 1)
    abi.check_version()


# ---- dn_replay_indices ------------------------------------------------------------------------------------------------------------------
def _lib_indices(lib, seed, draw, s, n, skip, start=0, count=8):
    out = np.full(count + 1, -7, np.int64)                      # one guard cell
    rc = lib.dn_replay_indices(seed, draw, s, n, skip, start, count, out.ctypes.data)
    assert rc == 0 and out[count] == -7, lib.dn_last_error()
    return out[:count]


def test_known_answers(pkg):
    lib = pkg._capi.load()
    for args, slots, envs in R.KNOWN:
        n, rows = args[3], len(slots)
        want = np.array(slots, np.int64) * n + np.array(envs, np.int64)
        got_slots, got_envs = R.draw(*args, count=rows)
        assert got_slots.tolist() == slots and got_envs.tolist() == envs, args
        assert np.array_equal(_lib_indices(lib, *args, count=rows), want), args


@pytest.mark.parametrize("s,n", R.UNIFORM_SHAPES + ((R.MAX, R.MAX), (R.MAX, 1), (1, R.MAX)))
def test_indices_are_the_numpy_statement(pkg, s, n):
    lib = pkg._capi.load()
    for seed in R.UNIFORM_SEEDS:
        for draw in R.UNIFORM_DRAWS:
            for skip in sorted({-1, 0, s // 2, s}):
                got = _lib_indices(lib, seed, draw, s, n, skip, 0, 4096)
                assert np.array_equal(got, R.flat(seed, draw, s, n, skip, 0, 4096)), (seed, draw, s, n, skip)
                assert got.min() >= 0 and got.max() < (s + (skip >= 0)) * n and not (got // n == skip).any()


def test_row_j_is_the_same_for_any_start_and_count(pkg):
    """The prefix property: a call for G B rows is G batches of B."""
    lib = pkg._capi.load()
    for s, n, skip in ((1000, 32768, -1), (7, 65, 3), (R.MAX, R.MAX, 5)):
        whole = _lib_indices(lib, 7, 3, s, n, skip, 0, 5000)
        for start, count in ((0, 1), (0, 256), (17, 100), (4999, 1), (5000, 0), (256, 256), (4096, 904)):
            assert np.array_equal(_lib_indices(lib, 7, 3, s, n, skip, start, count), whole[start:start + count]), (s, n, skip, start, count)
    last = _lib_indices(lib, 7, 3, 1000, 32768, -1, R.MAX - 4, 4)             # the last rows a call can have
    assert np.array_equal(last, R.flat(7, 3, 1000, 32768, -1, R.MAX - 4, 4))


def test_distinct_draws_give_distinct_batches(pkg):
    """Two independent batches of 256 from 64 x 32 768 transitions agree in 256 / 2^21 rows on average: fewer than 4."""
    lib = pkg._capi.load()
    base = _lib_indices(lib, 5, 11, 64, 32768, -1, 0, 256)
    for seed, draw in ((6, 11), (5, 12), (5 ^ 1 << 63, 11), (5, 11 + (1 << 40)), (5, 10)):
        same = int((_lib_indices(lib, seed, draw, 64, 32768, -1, 0, 256) == base).sum())
        assert same < 4, (seed, draw, same)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_draw_as_a_host_program(tmp_path, sanitize):
    """tests/tools/check_replay_draw.cpp includes csrc/dn_replay_draw.h alone: built with the host compiler, plainly and under the address
    and undefined-behaviour sanitizers, and run as its own process; it finds every row in range, off the skipped slot and independent of
    the rows around it, and every row it prints is the NumPy statement's -- the known answers among them."""
    exe = host_program_support.build("check_replay_draw", tmp_path, sanitize=sanitize, extra_flags=("-Wall", "-Werror"))
    result, lines = host_program_support.run_lines(exe, timeout=120)
    assert result == {"cases": 11, "bad": 0}
    seen = {}
    for line in lines[:-1]:
        key, values = line.split(":")
        args = tuple(int(v) for v in key.split())
        v = np.array(values.split(), np.int64)
        slots, envs = R.draw(*args, count=8)
        assert np.array_equal(v[0::2], slots) and np.array_equal(v[1::2], envs), args
        seen[args] = (v[0::2].tolist(), v[1::2].tolist())
    assert len(seen) == 11
    for args, slots, envs in R.KNOWN:
        assert seen[args][0][:len(slots)] == slots and seen[args][1][:len(envs)] == envs, args


# ---- uniformity -------------------------------------------------------------------------------------------------------------------------
BAR = 5.0


@pytest.mark.parametrize("s,n", R.UNIFORM_SHAPES)
def test_slots_drones_and_pairs_are_uniform(pkg, s, n):
    """2^20 rows per (seed, draw): (chi^2 - (k - 1)) / sqrt(2 (k - 1)) of the slot counts, the drone counts and the joint counts stays below
    5 (the NumPy statement's worst over the whole grid is 3.61).  The inputs are fixed, so the test is deterministic."""
    lib = pkg._capi.load()
    worst = 0.0
    for seed in R.UNIFORM_SEEDS:
        for draw in R.UNIFORM_DRAWS:
            flat = _lib_indices(lib, seed, draw, s, n, -1, 0, R.UNIFORM_ROWS)
            joint = np.bincount(flat, minlength=s * n).reshape(s, n)
            assert joint.size == s * n
            scores = [R.chi2_score(joint.sum(axis=1)), R.chi2_score(joint.sum(axis=0)), R.chi2_score(joint)]
            print(f"S={s} N={n} seed={seed:#x} draw={draw}: slots {scores[0]:.2f} drones {scores[1]:.2f} joint {scores[2]:.2f}")
            assert max(scores) < BAR, (s, n, seed, draw, scores)
            worst = max(worst, *scores)
    print(f"S={s} N={n}: worst {worst:.2f}")


@pytest.mark.parametrize("s,n,skip", [(7, 65, 0), (7, 65, 3), (7, 65, 7), (63, 64, 17), (1, 3, 0), (1, 3, 1)])
def test_the_skipped_slot_is_never_drawn_and_the_others_stay_uniform(pkg, s, n, skip):
    lib = pkg._capi.load()
    for seed in R.UNIFORM_SEEDS:
        for draw in R.UNIFORM_DRAWS:
            flat = _lib_indices(lib, seed, draw, s, n, skip, 0, R.UNIFORM_ROWS)
            joint = np.bincount(flat, minlength=(s + 1) * n).reshape(s + 1, n)
            assert joint.size == (s + 1) * n and joint[skip].sum() == 0, (s, n, skip, seed, draw)
            kept = np.delete(joint, skip, axis=0)                              # the S slots that can be drawn
            assert (kept.sum(axis=1) > 0).all()
            scores = [R.chi2_score(kept.sum(axis=1)), R.chi2_score(kept.sum(axis=0)), R.chi2_score(kept)]
            assert max(scores) < BAR, (s, n, skip, seed, draw, scores)


# ---- the refusals -----------------------------------------------------------------------------------------------------------------------
def test_dn_replay_indices_refuses(pkg):
    lib = pkg._capi.load()
    buf = np.zeros(8, np.int64).ctypes.data
    for args, text in (((0, 0, 0, 8, -1, 0, 1, buf), b"valid and n_envs must be in 1..2^31 - 1"),
                       ((0, 0, 1 << 31, 8, -1, 0, 1, buf), b"valid and n_envs must be in 1..2^31 - 1"),
                       ((0, 0, 8, 0, -1, 0, 1, buf), b"valid and n_envs must be in 1..2^31 - 1"),
                       ((0, 0, 8, 1 << 31, -1, 0, 1, buf), b"valid and n_envs must be in 1..2^31 - 1"),
                       ((0, 0, 8, 8, -2, 0, 1, buf), b"skip must be -1 or in 0..valid"), ((0, 0, 8, 8, 9, 0, 1, buf), b"skip must be -1 or in 0..valid"),
                       ((0, 0, 8, 8, -1, -1, 1, buf), b"start + count <= 2^31 - 1"), ((0, 0, 8, 8, -1, 0, -1, buf), b"start + count <= 2^31 - 1"),
                       ((0, 0, 8, 8, -1, R.MAX, 1, buf), b"start + count <= 2^31 - 1"), ((0, 0, 8, 8, -1, 1 << 62, 1 << 62, buf), b"start + count <= 2^31 - 1"),
                       ((0, 0, 8, 8, -1, 0, 8, None), b"out is required")):
        assert lib.dn_replay_indices(*args) == INVALID and text in lib.dn_last_error(), args
    assert lib.dn_replay_indices(0, 0, 8, 8, 8, R.MAX, 0, buf) == 0           # the edges pass


CFG = dict(seed=3, draw=0, buffer_size=8, n_envs=64, valid=7, skip=2, obs_dim=13, act_dim=4, layout=R.RING, reserved=0)
SRC = dict(obs=0x100000, next_obs=0x200000, actions=0x300000, rewards=0x400000, dones=0x500000, timeouts=0x600000)
OUT = dict(obs=0x1100000, next_obs=0x1200000, actions=0x1300000, rewards=0x1400000, dones=0x1500000)
PLAINLY = dict(layout=R.PLAIN, skip=-1)


def _call(lib, K, *, cfg=CFG, src=SRC, out=OUT, batch=100, indices=None, draw_offset=None, indices_out=0x1600000, **kw):
    c = s = None
    if cfg is not None:
        c = C.byref(K.DnReplayConfig(**dict(cfg, **{k: v for k, v in kw.items() if k in cfg})))
    if src is not None:
        s = C.byref(K.DnReplaySource(**dict(src, **{k[4:]: v for k, v in kw.items() if k.startswith("src_")})))
    o = dict(out, **{k[4:]: v for k, v in kw.items() if k.startswith("out_")})
    rc = lib.dn_replay_sample(c, s, batch, indices, draw_offset, o["obs"], o["next_obs"], o["actions"], o["rewards"], o["dones"], indices_out, 0, None)
    return rc, lib.dn_last_error().decode()


REFUSALS = [
    ("null_cfg", dict(cfg=None), "cfg and src are required"),
    ("null_src", dict(src=None), "cfg and src are required"),
    ("reserved_1", dict(reserved=1), "reserved must be 0 (got 1)"),
    ("layout_2", dict(layout=2), "layout must be 0 (DN_REPLAY_PLAIN) or 1 (DN_REPLAY_RING) (got 2)"),
    ("layout_negative", dict(layout=-1), "layout must be 0"),
    ("obs_dim_0", dict(obs_dim=0), "obs_dim must be in 1..64 (got 0)"),
    ("obs_dim_65", dict(obs_dim=65), "obs_dim must be in 1..64 (got 65)"),
    ("act_dim_0", dict(act_dim=0), "act_dim must be in 1..8 (got 0)"),
    ("act_dim_9", dict(act_dim=9), "act_dim must be in 1..8 (got 9)"),
    ("batch_0", dict(batch=0), "batch must be in 1..2^31 - 1 (got 0)"),
    ("batch_negative", dict(batch=-100), "batch must be in 1..2^31 - 1"),
    ("batch_2_to_31", dict(batch=1 << 31), "batch must be in 1..2^31 - 1"),
    ("buffer_size_0", dict(buffer_size=0), "buffer_size must be in 1..2^31 - 1 (got 0)"),
    ("buffer_size_2_to_31", dict(buffer_size=1 << 31), "buffer_size must be in 1..2^31 - 1"),
    ("n_envs_0", dict(n_envs=0), "valid and n_envs must be in 1..2^31 - 1"),
    ("n_envs_2_to_31", dict(n_envs=1 << 31), "valid and n_envs must be in 1..2^31 - 1"),
    ("valid_0", dict(valid=0, skip=-1), "valid and n_envs must be in 1..2^31 - 1"),
    ("valid_negative", dict(valid=-7), "valid and n_envs must be in 1..2^31 - 1"),
    ("skip_below", dict(skip=-2), "skip must be -1 or in 0..valid = 7 (got -2)"),
    ("skip_above", dict(skip=8), "skip must be -1 or in 0..valid = 7 (got 8)"),
    ("valid_beyond_the_buffer", dict(valid=9, skip=-1), "must be <= buffer_size = 8"),
    ("valid_and_skip_beyond_the_buffer", dict(valid=8, skip=0), "valid + 1 (the skipped slot) must be <= buffer_size = 8"),
    ("plain_with_skip", dict(layout=R.PLAIN), "skip must be -1 with DN_REPLAY_PLAIN"),
    ("indices_with_draw_offset", dict(indices=0x1700000, draw_offset=0x1800000), "draw_offset must be NULL with indices"),
    ("null_source_obs", dict(src_obs=None), "src.obs is required"),
    ("null_source_next_obs", dict(src_next_obs=None), "src.next_obs is required"),
    ("null_source_actions", dict(src_actions=None), "src.actions is required"),
    ("null_source_rewards", dict(src_rewards=None), "src.rewards is required"),
    ("null_source_dones", dict(src_dones=None), "src.dones is required"),
    ("null_source_timeouts", dict(src_timeouts=None), "src.timeouts is required"),
    ("null_obs", dict(out_obs=None), "obs is required"),
    ("null_next_obs", dict(out_next_obs=None), "next_obs is required"),
    ("null_actions", dict(out_actions=None), "actions is required"),
    ("null_rewards", dict(out_rewards=None), "rewards is required"),
    ("null_dones", dict(out_dones=None), "dones is required"),
    ("source_misaligned", dict(src_actions=0x300002), "src.actions must be 4-byte aligned"),
    ("plain_flags_misaligned", dict(PLAINLY, src_dones=0x500001), "src.dones must be 4-byte aligned"),
    ("output_misaligned", dict(out_rewards=0x1400002), "rewards must be 4-byte aligned"),
    ("indices_misaligned", dict(indices=0x1700004), "indices must be 8-byte aligned"),
    ("draw_offset_misaligned", dict(draw_offset=0x1800004), "draw_offset must be 8-byte aligned"),
    ("indices_out_misaligned", dict(indices_out=0x1600004), "indices_out must be 8-byte aligned"),
    ("output_is_a_source", dict(out_obs=SRC["obs"]), "obs overlaps src.obs: no output may be a source"),
    ("output_is_another_source", dict(out_next_obs=SRC["obs"]), "next_obs overlaps src.obs: no output may be a source"),
    ("output_in_the_spare_row", dict(out_dones=SRC["obs"] + 8 * 64 * 13 * 4), "dones overlaps src.obs"),
    ("output_in_the_flags", dict(out_rewards=SRC["timeouts"] + 8 * 64 - 4), "rewards overlaps src.timeouts"),
    ("indices_out_is_a_source", dict(indices_out=SRC["rewards"]), "indices_out overlaps src.rewards"),
]


@pytest.mark.parametrize("kw,message", [pytest.param(*r[1:], id=r[0]) for r in REFUSALS])
def test_dn_replay_sample_refuses(pkg, kw, message):
    """Every case returns DN_ERR_INVALID_ARGUMENT with its own text on dummy pointers: none gets as far as a device call."""
    K = pkg._capi
    rc, msg = _call(K.load(), K, **kw)
    assert rc == INVALID, msg
    assert message in msg, msg


def test_the_refusals_are_not_the_dummies_own(pkg):
    """The unchanged dummy call -- also plain, with indices, a draw offset, no indices_out, the edges of every range, a ring flag byte
    at an odd address, and an output just past the spare row -- passes every check but one chosen here, the last one validation makes:
    each refusal above is caused by what it changes."""
    K = pkg._capi
    lib = K.load()
    for kw in (dict(), PLAINLY, dict(indices=0x1700000), dict(draw_offset=0x1800000), dict(indices_out=None), dict(batch=1), dict(batch=R.MAX),
               dict(skip=-1), dict(skip=0), dict(skip=7), dict(valid=8, skip=-1), dict(valid=1, skip=1), dict(obs_dim=1, act_dim=1),
               dict(obs_dim=64, act_dim=8), dict(src_dones=0x500001), dict(seed=(1 << 64) - 1, draw=(1 << 64) - 1),
               dict(buffer_size=R.MAX, n_envs=1, valid=R.MAX - 1, skip=5), dict(buffer_size=1, n_envs=R.MAX, valid=1, skip=-1),
               dict(out_rewards=SRC["obs"] + 9 * 64 * 13 * 4), dict(PLAINLY, out_rewards=SRC["obs"] + 8 * 64 * 13 * 4)):
        rc, msg = _call(lib, K, **dict(kw, out_dones=SRC["actions"]))
        huge = kw.get("buffer_size", 0) == R.MAX or kw.get("n_envs", 0) == R.MAX       # sources of 2^31 - 1 cells reach the other dummies too
        assert rc == INVALID and ("overlaps src." if huge else "dones overlaps src.actions") in msg, (kw, msg)


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def test_python_surface_refuses(pkg):
    S = pkg.ReplaySampler
    ring = pkg.RingReplayBuffer(4, 6, 13, 4, "cpu")
    plain = pkg.ReplayBuffer(4, 6, 13, 4, "cpu")
    for buf in (ring, plain):
        with pytest.raises(RuntimeError, match="ReplaySampler needs a GPU device, got cpu"):      # everything else about the buffer was fine
            S(buf, 256)
    with pytest.raises(TypeError, match="ReplayBuffer or collector.RingReplayBuffer, got dict"):
        S({}, 256)
    for bad in (0, -1, 2.0, True, 1 << 31):
        with pytest.raises(ValueError, match="batch_size must be an integer in 1..2147483647"):
            S(ring, bad)
    for bad in (-1, 1 << 64, 1.5, True):
        with pytest.raises(ValueError, match="seed must be an integer in \\[0, 2\\^64\\)"):
            S(ring, 256, seed=bad)
    with pytest.raises(ValueError, match="rows of 65 observation and 4 action columns"):
        S(pkg.RingReplayBuffer(4, 6, 65, 4, "cpu"), 256)
    with pytest.raises(ValueError, match="rows of 13 observation and 9 action columns"):
        S(pkg.ReplayBuffer(4, 6, 13, 9, "cpu"), 256)
    ring.actions = torch.zeros(4, 6, 8)[:, :, :4]
    with pytest.raises(ValueError, match="'actions' must be dense"):
        S(ring, 256)
    ring.actions = torch.zeros(4, 6, 4)
    ring.done_flags = torch.zeros(4, 6)
    with pytest.raises(ValueError, match="'done_flags' must be torch.uint8 \\[4, 6\\] on cpu, got torch.float32"):
        S(ring, 256)
    plain.next_obs = torch.zeros(5, 6, 13)
    with pytest.raises(ValueError, match="'next_obs' must be torch.float32 \\[4, 6, 13\\]"):
        S(plain, 256)
    plain.next_obs = None
    with pytest.raises(ValueError, match="'next_obs' must be a tensor, got NoneType"):
        S(plain, 256)


def test_the_window_is_the_buffers_own_rule(pkg):
    """replay.window against replay_support.window and against the slots RingReplayBuffer.valid_slots() lists."""
    from drl_dronenavigation_amd.replay import window
    for t in (1, 2, 3, 5):
        ring, plain = pkg.RingReplayBuffer(t, 2, 13, 4, "cpu"), pkg.ReplayBuffer(t, 2, 13, 4, "cpu")
        for full in (False, True):
            for pos in range(t):
                for layout, buf in ((R.RING, ring), (R.PLAIN, plain)):
                    buf.pos, buf.full = pos, full
                    valid, skip = window(buf)
                    assert (valid, skip) == R.window(layout, t, pos, full), (t, full, pos, layout)
                    assert valid * 2 == len(buf)
                valid, skip = window(ring)
                slots = [s for s in range(valid + (skip >= 0)) if s != skip]
                assert slots == ring.valid_slots(), (t, full, pos)
