"""PPO minibatches on the device (include/dronenav.h dn_minibatch), the part that needs no GPU: the four entry points are declared,
exported and bound; the layouts of dn_minibatch_field and dn_minibatch_config, compiled from the header; the scratch-size rule; the keyed
permutation through the real library against the NumPy reference of tests/minibatch_support.py, and as a stand-alone host program,
plainly and under the address and undefined-behaviour sanitizers; every refusal of dn_minibatch, which validates before its first device
call, so the pointers here are never followed; the Python surface's own refusals; and the reference normalisation against itself."""
import ctypes as C
import math
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import abi_support as abi  # noqa: E402
import host_program_support  # noqa: E402
import minibatch_support as M  # noqa: E402

NAMES = ("dn_minibatch_scratch_bytes", "dn_minibatch_permutation", "dn_minibatch")
INVALID = -1


@pytest.fixture(scope="module")
def pkg():
    import drl_dronenavigation_amd as p
    p.build.build_library()
    return p


def test_the_names_are_declared_exported_and_bound(pkg):
    code = abi.header_text()
    assert re.search(r"#define DN_MINIBATCH_MAX_FIELDS 8\b", code)
    assert re.search(r"typedef struct dn_minibatch_field \{\s*const void \*src;\s*void \*dst;\s*int32_t width;\s*int32_t normalize;\s*\} "
                     r"dn_minibatch_field;", code)
    assert re.search(r"typedef struct dn_minibatch_config \{\s*uint64_t seed;\s*uint64_t epoch;\s*double epsilon;\s*int32_t num_fields;\s*"
                     r"int32_t reserved;\s*\} dn_minibatch_config;", code)
    abi.check_names(*NAMES)
    assert pkg.MinibatchSampler is pkg.minibatch.MinibatchSampler and "MinibatchSampler" in pkg.__all__
    abi.check_version()


def test_struct_layouts_compiled_from_the_header(pkg):
    """dn_minibatch_field: 24 bytes, src 0, dst 8, width 16, normalize 20; dn_minibatch_config: 32 bytes, seed 0, epoch 8, epsilon 16,
    num_fields 24, reserved 28 -- by the C compiler from the header itself, and the ctypes mirrors agree."""
    abi.check_layout(pkg._capi.DnMinibatchField, 24, src=0, dst=8, width=16, normalize=20)
    abi.check_layout(pkg._capi.DnMinibatchConfig, 32, seed=0, epoch=8, epsilon=16, num_fields=24, reserved=28)
    assert abi.compiled().constants["DN_MINIBATCH_MAX_FIELDS"] == pkg._capi.MINIBATCH_MAX_FIELDS == 8
    abi.check_version()


def test_scratch_sizes(pkg):
    """One (mean, m2) pair per block of 1024 output rows, plus the mean and the denominator."""
    lib = pkg._capi.load()
    for batch in (1, 2, 1024, 1025, 2048, 2049, 65536, (1 << 31) - 1):
        assert lib.dn_minibatch_scratch_bytes(batch) == 8 * 2 * (-(-batch // M.BLOCK_ROWS) + 1), batch
    for batch in (0, -1, 1 << 31, 1 << 62):
        assert lib.dn_minibatch_scratch_bytes(batch) == INVALID, batch
        assert b"batch must be in 1..2^31 - 1" in lib.dn_last_error()


# ---- the permutation ------------------------------------------------------------------------------------------------------------------
def _lib_permutation(lib, seed, epoch, m, start=0, count=None):
    count = m - start if count is None else count
    out = np.full(count + 1, -7, np.int64)                      # one guard cell
    rc = lib.dn_minibatch_permutation(seed, epoch, m, start, count, out.ctypes.data)
    assert rc == 0 and out[count] == -7, lib.dn_last_error()
    return out[:count]


@pytest.mark.parametrize("m", M.SIZES)
def test_permutation_is_the_reference_and_a_bijection(pkg, m):
    lib = pkg._capi.load()
    worst = 0
    for seed in M.SEEDS:
        for epoch in M.EPOCHS:
            want, walks = M.permutation(m, seed, epoch)
            got = _lib_permutation(lib, seed, epoch, m)
            assert np.array_equal(got, want), (m, seed, epoch)
            assert np.array_equal(np.sort(got), np.arange(m)), (m, seed, epoch)
            worst = max(worst, walks)
    print(f"M={m}: at most {worst} walk iterations")
    assert worst <= 64


def test_a_window_is_the_slice_of_the_whole(pkg):
    lib = pkg._capi.load()
    for m, start, count in ((1000, 0, 1000), (1000, 17, 100), (1000, 999, 1), (1000, 1000, 0), (65537, 65000, 537), (4097, 1, 4096)):
        whole = _lib_permutation(lib, 7, 3, m)
        assert np.array_equal(_lib_permutation(lib, 7, 3, m, start, count), whole[start:start + count]), (m, start, count)
        assert np.array_equal(M.permutation(m, 7, 3, start, count)[0], whole[start:start + count]), (m, start, count)


def test_two_seeds_or_two_epochs_share_few_slots(pkg):
    """Two independent permutations of 1000 agree in one slot on average: fewer than 1 % (10) of the slots."""
    lib = pkg._capi.load()
    base = _lib_permutation(lib, 5, 11, 1000)
    for seed, epoch in ((6, 11), (5, 12), (5 ^ 1 << 63, 11), (5, 11 + (1 << 40))):
        same = int((_lib_permutation(lib, seed, epoch, 1000) == base).sum())
        assert same < 10, (seed, epoch, same)


def test_dn_minibatch_permutation_refuses(pkg):
    lib = pkg._capi.load()
    buf = np.zeros(8, np.int64).ctypes.data
    for args, text in (((0, 0, 0, 0, 0, buf), b"m must be in 1..2^31 - 1"), ((0, 0, 1 << 31, 0, 1, buf), b"m must be in 1..2^31 - 1"),
                       ((0, 0, 8, -1, 1, buf), b"start + count <= m"), ((0, 0, 8, 0, 9, buf), b"start + count <= m"),
                       ((0, 0, 8, 5, 4, buf), b"start + count <= m"), ((0, 0, 8, 0, -1, buf), b"start + count <= m"),
                       ((0, 0, 8, 1 << 62, 1 << 62, buf), b"start + count <= m"), ((0, 0, 8, 0, 8, None), b"out is required")):
        assert lib.dn_minibatch_permutation(*args) == INVALID and text in lib.dn_last_error(), args


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_permutation_as_a_host_program(tmp_path, sanitize):
    """tests/tools/check_minibatch_permutation.cpp includes csrc/dn_permute.h alone: built with the host compiler, plainly and under the
    address and undefined-behaviour sanitizers, and run as its own process; its bitmap finds every pi a bijection, and every pi it prints
    is the NumPy reference's."""
    exe = host_program_support.build("check_minibatch_permutation", tmp_path, sanitize=sanitize, extra_flags=("-Wall", "-Werror"))
    result, lines = host_program_support.run_lines(exe, timeout=120)
    assert result == {"cases": len(M.SIZES) * len(M.SEEDS) * len(M.EPOCHS), "bad": 0}
    seen = set()
    for line in lines[:-1]:
        key, values = line.split(":")
        m, seed, epoch = (int(v) for v in key.split())
        assert np.array_equal(np.array(values.split(), np.int64), M.permutation(m, seed, epoch)[0]), (m, seed, epoch)
        seen.add((m, seed, epoch))
    assert seen == {(m, s, e) for m in M.SIZES for s in M.SEEDS for e in M.EPOCHS}


# ---- the refusals of dn_minibatch -------------------------------------------------------------------------------------------------------
CFG = dict(seed=3, epoch=0, epsilon=1e-8, num_fields=2, reserved=0)
FIELDS = [(0x20000, 0x40000, 13, 0), (0x60000, 0x70000, 1, 1)]         # src, dst, width, normalize
SAME = "same"


def _call(lib, K, *, cfg=CFG, fields=FIELDS, n_steps=4, n_envs=64, start=0, batch=100, indices=None, epoch_offset=None, indices_out=0x90000,
          scratch=0x80000, scratch_bytes=1 << 40, **cfg_kw):
    c = None
    if cfg is not None:
        d = dict(cfg, **cfg_kw)
        c = C.byref(K.DnMinibatchConfig(d["seed"], d["epoch"], d["epsilon"], d["num_fields"], d["reserved"]))
    f = None
    if fields is not None:
        f = (K.DnMinibatchField * max(len(fields), 1))(*[K.DnMinibatchField(*x) for x in fields])
    rc = lib.dn_minibatch(c, f, n_steps, n_envs, start, batch, indices, epoch_offset, indices_out, scratch, scratch_bytes, 0, None)
    return rc, lib.dn_last_error().decode()


def _fields(first=None, second=None, extra=()):
    return dict(fields=[first or FIELDS[0], second or FIELDS[1]] + list(extra))


NINE = dict(fields=[FIELDS[0]] * 9, num_fields=9)
REFUSALS = [
    ("null_cfg", dict(cfg=None), "cfg and fields are required"),
    ("null_fields", dict(fields=None), "cfg and fields are required"),
    ("null_src", _fields(first=(None, 0x40000, 13, 0)), "field 0: src and dst are required"),
    ("null_dst", _fields(second=(0x60000, None, 1, 1)), "field 1: src and dst are required"),
    ("null_scratch", dict(scratch=None), "scratch is required"),
    ("num_fields_0", dict(num_fields=0), "num_fields must be in 1..8 (got 0)"),
    ("num_fields_9", NINE, "num_fields must be in 1..8 (got 9)"),
    ("width_0", _fields(first=(0x20000, 0x40000, 0, 0)), "field 0: width must be in 1..64 (got 0)"),
    ("width_65", _fields(first=(0x20000, 0x40000, 65, 0)), "field 0: width must be in 1..64 (got 65)"),
    ("reserved_1", dict(reserved=1), "reserved must be 0 (got 1)"),
    ("epsilon_negative", dict(epsilon=-1e-8), "epsilon must be >= 0"),
    ("epsilon_nan", dict(epsilon=math.nan), "epsilon must be >= 0"),
    ("n_steps_0", dict(n_steps=0), "n_steps and n_envs must be >= 1"),
    ("n_envs_0", dict(n_envs=0), "n_steps and n_envs must be >= 1"),
    ("n_envs_negative", dict(n_envs=-64), "n_steps and n_envs must be >= 1"),
    ("m_2_to_31", dict(n_steps=1 << 10, n_envs=1 << 21), "more than the 2^31 - 1 of a buffer"),
    ("m_overflows_int64", dict(n_steps=1 << 40, n_envs=1 << 40), "more than the 2^31 - 1 of a buffer"),
    ("start_negative", dict(start=-1), "start must be >= 0 and batch >= 1 with start + batch <="),
    ("start_plus_batch_beyond_m", dict(start=157), "start must be >= 0 and batch >= 1 with start + batch <="),
    ("start_with_indices", dict(start=1, indices=0xA0000), "start must be 0 with indices"),
    ("batch_0", dict(batch=0), "start must be >= 0 and batch >= 1 with start + batch <="),
    ("batch_negative", dict(batch=-100), "start must be >= 0 and batch >= 1 with start + batch <="),
    # a grid beyond 2^31 - 1 workgroups would take a batch beyond 2^31 - 1 rows, which no buffer of M <= 2^31 - 1 samples holds
    ("batch_of_a_grid_beyond_2_to_31", dict(n_steps=1, n_envs=(1 << 31) - 1, batch=1 << 41), "start must be >= 0 and batch >= 1 with start + batch <="),
    ("two_normalize_fields", _fields(first=(0x20000, 0x40000, 1, 1)), "fields 0 and 1: at most one field is normalised"),
    ("normalize_of_width_13", _fields(first=(0x20000, 0x40000, 13, 1), second=(0x60000, 0x70000, 1, 0)), "the normalised field must be of width 1 (got 13)"),
    ("normalize_2", _fields(second=(0x60000, 0x70000, 1, 2)), "field 1: normalize must be 0 or 1 (got 2)"),
    ("dst_is_src", _fields(first=(0x20000, 0x20000, 13, 0)), "field 0: dst must not be src"),
    ("src_misaligned", _fields(first=(0x20002, 0x40000, 13, 0)), "field 0: src and dst must be 4-byte aligned"),
    ("scratch_one_byte_short", dict(scratch_bytes="short"), "scratch_bytes is too small"),
    ("scratch_0", dict(scratch_bytes=0), "scratch_bytes is too small"),
    ("scratch_misaligned", dict(scratch=0x80004), "must be 8-byte aligned"),
    ("indices_misaligned", dict(indices=0xA0004), "must be 8-byte aligned"),
    ("epoch_offset_misaligned", dict(epoch_offset=0xB0004), "must be 8-byte aligned"),
]


@pytest.mark.parametrize("kw,message", [pytest.param(*r[1:], id=r[0]) for r in REFUSALS])
def test_dn_minibatch_refuses(pkg, kw, message):
    """Every case returns DN_ERR_INVALID_ARGUMENT with its own text on dummy pointers: none gets as far as a device call."""
    K = pkg._capi
    lib = K.load()
    kw = dict(kw)
    if kw.get("scratch_bytes") == "short":
        kw["scratch_bytes"] = lib.dn_minibatch_scratch_bytes(100) - 1
    rc, msg = _call(lib, K, **kw)
    assert rc == INVALID, msg
    assert message in msg, msg


def test_the_refusals_are_not_the_dummies_own(pkg):
    """The unchanged dummy call -- also with indices, an epoch offset, epsilon 0, one field, eight fields, a batch of one and of the whole
    buffer, the last window of the epoch, the exact scratch size, and the largest buffer -- passes every check but one chosen here, the
    last one validation makes: each refusal above is caused by what it changes."""
    K = pkg._capi
    lib = K.load()
    for kw in (dict(), dict(indices=0xA0000), dict(epoch_offset=0xB0000), dict(epsilon=0.0), dict(fields=FIELDS[:1], num_fields=1),
               dict(fields=[FIELDS[0]] * 7 + [FIELDS[1]], num_fields=8), dict(batch=1), dict(batch=256), dict(start=156),
               dict(scratch_bytes=lib.dn_minibatch_scratch_bytes(100)), dict(n_steps=1, n_envs=(1 << 31) - 1, batch=(1 << 31) - 1),
               dict(seed=(1 << 64) - 1, epoch=(1 << 64) - 1)):
        rc, msg = _call(lib, K, indices_out=0x90004, **kw)
        assert rc == INVALID and "must be 8-byte aligned" in msg, (kw, msg)


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
SIX = {"obs": ((13,), torch.float32), "actions": ((4,), torch.float32), "values": ((), torch.float32), "log_probs": ((), torch.float32),
       "advantages": ((), torch.float32), "returns": ((), torch.float32)}


def test_python_surface_refuses_without_a_device(pkg):
    S = pkg.MinibatchSampler
    with pytest.raises(RuntimeError, match="no CPU path"):
        S(4, 64, 100, SIX, "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        S(4, 64, 100, SIX, torch.device("cpu"), seed=5, normalize=None)
    nine = dict(SIX, a=((), torch.int32), b=((), torch.int32), c=((), torch.int32))
    with pytest.raises(ValueError, match="1..8 fields, got 9"):
        S(4, 64, 100, nine, "cpu")
    with pytest.raises(ValueError, match="1..8 fields"):
        S(4, 64, 100, {}, "cpu")
    with pytest.raises(ValueError, match="'history' has 65 columns"):
        S(4, 64, 100, dict(SIX, history=((65,), torch.float32)), "cpu")
    with pytest.raises(ValueError, match="'history' has 65 columns"):
        S(4, 64, 100, dict(SIX, history=((5, 13), torch.float32)), "cpu")
    with pytest.raises(ValueError, match="'episode_starts' must be float32 or int32, got torch.uint8 .one byte a cell"):
        S(4, 64, 100, dict(SIX, episode_starts=((), torch.uint8)), "cpu")
    with pytest.raises(ValueError, match="'values' must be float32 or int32, got torch.float64"):
        S(4, 64, 100, dict(SIX, values=((), torch.float64)), "cpu")
    for kw, word in ((dict(normalize="advantage"), "not a field"), (dict(normalize="obs"), "one column"), (dict(epsilon=-1.0), "epsilon"),
                     (dict(epsilon=math.nan), "epsilon"), (dict(seed=-1), "seed"), (dict(seed=1 << 64), "seed"), (dict(seed=1.5), "seed")):
        with pytest.raises(ValueError, match=word):
            S(4, 64, 100, SIX, "cpu", **kw)
    for bad in (dict(n_steps=0), dict(num_envs=-1), dict(batch_size=0), dict(batch_size=2.0), dict(n_steps=True)):
        args = dict(dict(n_steps=4, num_envs=64, batch_size=100), **bad)
        with pytest.raises(ValueError, match=next(iter(bad))):
            S(args["n_steps"], args["num_envs"], args["batch_size"], SIX, "cpu")
    with pytest.raises(ValueError, match="more than the 2\\^31 - 1"):
        S(1 << 11, 1 << 20, 100, SIX, "cpu")


def test_for_rollout_reads_the_dict_and_refuses(pkg):
    S = pkg.MinibatchSampler
    T, N = 4, 6
    out = dict(obs=torch.zeros(T + 1, N, 13)[:T], actions=torch.zeros(T, N, 4), values=torch.zeros(T, N), log_probs=torch.zeros(T, N),
               advantages=torch.zeros(T, N), returns=torch.zeros(T, N), episode_starts=torch.zeros(T, N, dtype=torch.uint8))
    assert out["obs"].is_contiguous()                           # the fused collector's view of its n_steps + 1 slots
    with pytest.raises(RuntimeError, match="MinibatchSampler needs a GPU device, got cpu"):         # everything else about the dict was fine
        S.for_rollout(out, 10)
    with pytest.raises(ValueError, match="'episode_starts' must be float32 or int32, got torch.uint8 .one byte a cell"):
        S.for_rollout(out, 10, fields=("obs", "episode_starts"))
    with pytest.raises(ValueError, match="'actions' must be dense"):
        S.for_rollout(dict(out, actions=torch.zeros(T, N, 8)[:, :, :4]), 10)
    with pytest.raises(ValueError, match="'values' must be dense"):
        S.for_rollout(dict(out, values=torch.zeros(N, T).t()), 10)
    with pytest.raises(ValueError, match="'returns' must be torch.float32 \\[4, 6\\]"):
        S.for_rollout(dict(out, returns=torch.zeros(T, N + 1)), 10)
    with pytest.raises(ValueError, match="'rewards' must be a tensor"):
        S.for_rollout(out, 10, fields=("obs", "rewards"))
    with pytest.raises(ValueError, match="'history' has 65 columns"):
        S.for_rollout(dict(out, history=torch.zeros(T, N, 65)), 10, fields=("history",))


def test_permutation_works_without_a_device(pkg):
    got = pkg.minibatch.permutation(1025, 7, 1 << 40)
    assert got.dtype == torch.int64 and got.device.type == "cpu" and tuple(got.shape) == (1025,)
    assert np.array_equal(got.numpy(), M.permutation(1025, 7, 1 << 40)[0])
    with pytest.raises(ValueError, match="epoch"):
        pkg.minibatch.permutation(10, 0, -1)
    with pytest.raises(pkg.DroneNavError, match="m must be in"):
        pkg.minibatch.permutation(0, 0, 0)


# ---- the reference against itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", sorted(M.DATA))
def test_reference_agrees_with_itself_in_two_summation_orders(data):
    """The bar of the GPU test on the reference alone: the moments taken over the batch in both orders give outputs within
    M.tolerance() of each other, cell by cell, after the rounding to float32 -- a tolerance the reference itself keeps."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for batch in (2, 64, 1025, 2049):
        a = M.DATA[data](rng, batch)
        one, two = M.normalize(a), M.normalize(a, reverse=True)
        err = np.abs(one.astype(np.float32).astype(np.float64) - two)
        assert (err <= M.tolerance(two)).all(), (data, batch, float((err / M.tolerance(two)).max()))
        worst = max(worst, float((err / M.tolerance(two)).max()))
        mean, std = float(np.mean(a.astype(np.float64))), float(np.std(a.astype(np.float64), ddof=1))
        assert batch == 2 or abs(mean) * 2.0 ** -50 / std < 2.0 ** -40, (data, batch, mean, std)
    print(f"{data}: largest distance between the two orders {worst:.3f} of the tolerance")


def test_reference_is_exact_on_a_batch_without_spread():
    for value in (0.0, -0.0, 1.5, 4096.25, -3e-5):
        for batch in (2, 64, 1025):
            out = M.normalize(np.full(batch, value, np.float32))
            assert (out == 0.0).all(), (value, batch)
    assert M.normalize(np.array([2.5], np.float32))[0] == 2.5                  # a batch of one is returned as it is
    assert np.allclose(M.normalize(np.array([1.0, 3.0], np.float32)), [-1 / math.sqrt(2), 1 / math.sqrt(2)], rtol=1e-7)
