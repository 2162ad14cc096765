"""PPO minibatches on the device (include/dronenav.h dn_minibatch, csrc/dn_minibatch.hip, minibatch.py) on the HIP path.

 1. copies: every field equals the NumPy gather of tests/minibatch_support.py bit for bit, for the keyed permutation and for explicit
    indices -- an int32 field, a float32 field of NaN bit patterns and one of -0.0 and negative denormals included; `indices` are the
    reference's samples;
 2. an epoch covers the buffer: the concatenated indices are a permutation of [0, M), the last minibatch has M % batch_size rows;
 3. out-of-range indices are clamped;
 4. the advantages against the float64 reference within minibatch_support.tolerance(): both data sets, a batch of two, a batch of one (the
    raw copy), equal values (exact zeros), a NaN (all NaN);
 5. the same call twice gives the same bits; a call of 2049 rows equals calls of 1024, 1024 and 1 in its copied fields; the 16-byte path
    equals the 4-byte path (source and destination moved by one word);
 6. an epoch of minibatches and epoch_offset += 1 under graph replay; the capture guard of the scratch;
 7. with the two collectors.

Shapes: n_steps in {1, 3, 8} x n_envs in {1, 63, 65, 1000}; batch in {1, 2, 64, 1025, 2049} where it fits -- 1025 and 2049 cross one and
two boundaries of the 1024-row blocks, with a last block of one row; widths {1, 3, 4, 13, 52, 64}: 4, 52 and 64 take the 16-byte path.
Every source word is distinct (its own index plus a base per field), so a wrong row cannot pass."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import minibatch_support as M  # noqa: E402
from gpu_support import DEV  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402
from model_support import NOISE  # noqa: E402

STEPS, ENVS = (1, 3, 8), (1, 63, 65, 1000)
BATCHES = (1, 2, 64, 1025, 2049)
SEED, EPOCH = 11, 5
# name -> (trailing shape, dtype, the first word): seven copied fields and the advantages
F32, I32 = torch.float32, torch.int32
COPIED = {"w1": ((), F32, 0x01000000), "nan3": ((3,), F32, 0x7FC00000), "neg4": ((4,), F32, 0x80000000 - (1 << 32)),
          "w13": ((13,), F32, 0x02000000), "w52": ((52,), F32, 0x03000000), "w64": ((8, 8), F32, 0x04000000), "ids4": ((2, 2), I32, 0x05000000)}
SPEC = dict({k: v[:2] for k, v in COPIED.items()}, advantages=((), F32))
shapes = pytest.mark.parametrize("n_steps,n_envs", [(t, n) for t in STEPS for n in ENVS])


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _same(got, want, tag):
    """got: a device tensor; want: a NumPy array of the same words."""
    w = _dev(want)
    assert got.shape == w.shape and got.dtype == w.dtype and torch.equal(_bits(got), _bits(w)), tag


@functools.lru_cache(maxsize=None)
def _words(n_steps, n_envs):
    """The copied fields of one shape as NumPy arrays, made once: word i of a field is base + i, viewed as the field's dtype."""
    out = {}
    for name, (shape, dtype, base) in COPIED.items():
        w = (np.arange(n_steps * n_envs * int(np.prod(shape, dtype=np.int64)), dtype=np.int64) + base).astype(np.int32)
        out[name] = w.reshape((n_steps, n_envs) + shape).view(np.float32 if dtype == F32 else np.int32)
    assert np.isnan(out["nan3"]).all() and np.signbit(out["neg4"]).all() and out["neg4"].ravel()[0] == 0.0
    return out


@functools.lru_cache(maxsize=None)
def _rollout(n_steps, n_envs, data="noisy"):
    """(the NumPy arrays, the device dict) of one shape with the advantages of one data set."""
    host = dict(_words(n_steps, n_envs), advantages=M.DATA[data](np.random.default_rng(1000 * n_steps + n_envs), (n_steps, n_envs)))
    return host, {k: _dev(v) for k, v in host.items()}


def _fits(m):
    return [b for b in BATCHES if b <= m]


def _check_copies(got, host, samples, tag):
    for name in COPIED:
        _same(got[name], M.gather(host[name], samples), (tag, name))
    _same(got["indices"], np.asarray(samples, np.int64), (tag, "indices"))


# ---- 1. copies ----------------------------------------------------------------------------------------------------------------------------
@shapes
def test_copies_are_the_reference_gather(n_steps, n_envs):
    pkg = _pkg()
    m = n_steps * n_envs
    host, dev = _rollout(n_steps, n_envs)
    rng = np.random.default_rng(m)
    for batch in _fits(m):
        s = pkg.MinibatchSampler(n_steps, n_envs, batch, SPEC, DEV, seed=SEED, normalize=None)
        for start in sorted({0, (m - batch) // 2, m - batch}):
            want, _ = M.permutation(m, SEED, EPOCH, start, batch)
            got = s.gather(dev, EPOCH, start, batch)
            _check_copies(got, host, want, (n_steps, n_envs, batch, start))
            _same(got["advantages"], M.gather(host["advantages"], want), (n_steps, n_envs, batch, start, "advantages, not normalised"))
        picked = rng.integers(0, m, batch)                      # with repeats
        got = s.gather(dev, EPOCH, 0, indices=_dev(picked))
        _check_copies(got, host, picked, (n_steps, n_envs, batch, "indices"))
        assert np.array_equal(s.permutation(EPOCH).numpy(), M.permutation(m, SEED, EPOCH)[0])


# ---- 2. an epoch covers the buffer ------------------------------------------------------------------------------------------------------
@shapes
def test_an_epoch_covers_the_buffer(n_steps, n_envs):
    pkg = _pkg()
    m = n_steps * n_envs
    host, dev = _rollout(n_steps, n_envs)
    for batch_size in sorted({min(64, m), min(1025, m), 7}):
        s = pkg.MinibatchSampler(n_steps, n_envs, batch_size, SPEC, DEV, seed=SEED)
        taken, sizes = [], []
        for mb in s.epoch(dev, EPOCH + 1):
            taken.append(mb["indices"].clone())
            sizes.append(mb["w13"].shape[0])
        bs = s.batch_size
        assert sizes == [bs] * (m // bs) + ([m % bs] if m % bs else []), (n_steps, n_envs, batch_size, sizes)
        taken = torch.cat(taken).cpu().numpy()
        assert np.array_equal(taken, M.permutation(m, SEED, EPOCH + 1)[0]) and np.array_equal(np.sort(taken), np.arange(m))


# ---- 3. clamping ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps,n_envs", [(1, 63), (3, 65), (8, 1000)])
def test_out_of_range_indices_are_clamped(n_steps, n_envs):
    pkg = _pkg()
    m = n_steps * n_envs
    host, dev = _rollout(n_steps, n_envs)
    s = pkg.MinibatchSampler(n_steps, n_envs, 8, SPEC, DEV, normalize=None)
    asked = np.array([-5, m, 1 << 40, -(1 << 62), 0, m - 1], np.int64)
    got = s.gather(dev, 0, 0, indices=_dev(asked))
    _check_copies(got, host, [0, m - 1, m - 1, 0, 0, m - 1], (n_steps, n_envs))


# ---- 4. the advantages --------------------------------------------------------------------------------------------------------------------
def _check_advantages(got, a, tag):
    want = M.normalize(a)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    tol = M.tolerance(want)
    worst = float((err / tol).max())
    print(f"{tag}: largest distance from the float64 reference {worst:.3f} of the tolerance")
    assert (err <= tol).all(), (tag, worst)
    return worst


@pytest.mark.parametrize("data", sorted(M.DATA))
@shapes
def test_advantages_match_the_float64_reference(n_steps, n_envs, data):
    """(a - mean) / (std + 1e-8), unbiased std, moments and division in float64, one rounding: within one float32 ulp of the reference or
    2^-40.  A batch of two values d apart comes out as +-(d / 2) / (d / sqrt(2) + 1e-8), +-1/sqrt(2) but for the epsilon; a batch of one
    is the raw value.  The other fields of
    the same call are still the plain gather."""
    pkg = _pkg()
    m = n_steps * n_envs
    host, dev = _rollout(n_steps, n_envs, data)
    rng = np.random.default_rng(m + 1)
    for batch in _fits(m):
        s = pkg.MinibatchSampler(n_steps, n_envs, batch, SPEC, DEV, seed=SEED)
        for start in sorted({0, m - batch}):
            samples, _ = M.permutation(m, SEED, EPOCH, start, batch)
            got = s.gather(dev, EPOCH, start)
            a = M.gather(host["advantages"], samples)
            if batch == 1:
                _same(got["advantages"], a, (n_steps, n_envs, data, "a batch of one is the raw copy"))
            else:
                _check_advantages(got["advantages"], a, (n_steps, n_envs, data, batch, start))
            if batch == 2 and a[0] != a[1]:
                g, d = got["advantages"].cpu().numpy().astype(np.float64), abs(float(a[0]) - float(a[1]))
                assert np.allclose(np.abs(g), 0.5 * d / (d * 2.0 ** -0.5 + 1e-8), rtol=1e-6) and g[0] == -g[1], (g, "unbiased: +-1/sqrt(2)")
            _check_copies(got, host, samples, (n_steps, n_envs, data, batch, start))
        if batch > 1:
            picked = rng.integers(0, m, batch)
            got = s.gather(dev, EPOCH, 0, indices=_dev(picked))
            _check_advantages(got["advantages"], M.gather(host["advantages"], picked), (n_steps, n_envs, data, batch, "indices"))


@pytest.mark.parametrize("batch", [2, 64, 1025, 2049])
def test_equal_advantages_give_exact_zeros_and_a_nan_gives_all_nan(batch):
    pkg = _pkg()
    n_steps, n_envs = 3, 1000
    s = pkg.MinibatchSampler(n_steps, n_envs, batch, {"advantages": ((), F32)}, DEV, seed=SEED)
    for value in (4096.25, -3e-5, 0.0):
        flat = _dev(np.full((n_steps, n_envs), value, np.float32))
        got = s.gather({"advantages": flat}, EPOCH, 0)["advantages"]
        assert got.shape == (batch,) and bool((got == 0.0).all()), (batch, value)
    host = M.noisy_advantages(np.random.default_rng(batch), (n_steps, n_envs))
    samples, _ = M.permutation(n_steps * n_envs, SEED, EPOCH, 0, batch)
    for slot in (0, batch - 1):                                 # the block's shift, and the last row of the last block
        bad = host.copy()
        bad.reshape(-1)[M.source_rows(samples[slot], n_steps, n_envs)] = np.nan
        got = s.gather({"advantages": _dev(bad)}, EPOCH, 0)["advantages"]
        assert bool(torch.isnan(got).all()), (batch, slot)


# ---- 5. reproducible ----------------------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bits():
    pkg = _pkg()
    n_steps, n_envs, batch = 8, 1000, 2049
    _, dev = _rollout(n_steps, n_envs, "offset")
    s = pkg.MinibatchSampler(n_steps, n_envs, batch, SPEC, DEV, seed=SEED)
    first = {k: v.clone() for k, v in s.gather(dev, EPOCH, 17).items()}
    for v in s.out.values():
        v.view(torch.int32).fill_(0x7FC12345)
    again = s.gather(dev, EPOCH, 17)
    for k in first:
        assert torch.equal(_bits(first[k]), _bits(again[k])), k


def test_one_call_of_2049_rows_is_calls_of_1024_1024_and_1():
    pkg = _pkg()
    n_steps, n_envs = 3, 1000
    _, dev = _rollout(n_steps, n_envs)
    s = pkg.MinibatchSampler(n_steps, n_envs, 2049, SPEC, DEV, seed=SEED)
    whole = {k: v.clone() for k, v in s.gather(dev, EPOCH, 100, 2049).items()}
    parts = [{k: v.clone() for k, v in s.gather(dev, EPOCH, 100 + off, cnt).items()} for off, cnt in ((0, 1024), (1024, 1024), (2048, 1))]
    for k in list(COPIED) + ["indices"]:
        assert torch.equal(_bits(whole[k]), _bits(torch.cat([p[k] for p in parts]))), k


def test_the_16_byte_path_gives_the_bits_of_the_4_byte_path():
    """Widths 4, 52 and 64 on 16-byte-aligned tensors take 16-byte words; the same words behind a source and a destination moved by one
    4-byte word take the 4-byte path."""
    pkg = _pkg()
    n_steps, n_envs, batch = 3, 1000, 1025
    host, dev = _rollout(n_steps, n_envs)
    s = pkg.MinibatchSampler(n_steps, n_envs, batch, SPEC, DEV, seed=SEED)
    aligned = {k: v.clone() for k, v in s.gather(dev, EPOCH, 0).items()}
    moved = {}
    for name, x in dev.items():
        assert x.data_ptr() % 16 == 0 and s.out[name].data_ptr() % 16 == 0
        buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=DEV)
        moved[name] = buf[1:].view(x.shape).copy_(x)
        s.out[name] = torch.empty(s.out[name].numel() + 1, dtype=x.dtype, device=DEV)[1:].view(s.out[name].shape)
        assert moved[name].is_contiguous() and moved[name].data_ptr() % 16 == 4 and s.out[name].data_ptr() % 16 == 4
    other = s.gather(moved, EPOCH, 0)
    for k in aligned:
        assert torch.equal(_bits(aligned[k]), _bits(other[k])), k
    _check_copies(other, host, M.permutation(n_steps * n_envs, SEED, EPOCH, 0, batch)[0], "moved by one word")


# ---- 6. graph ---------------------------------------------------------------------------------------------------------------------------
def test_an_epoch_under_graph_replay_reshuffles_with_the_epoch_offset():
    """One epoch of minibatches and epoch_offset += 1, captured on one stream and replayed twice: the outputs are the references of
    epochs EPOCH and EPOCH + 1."""
    pkg = _pkg()
    n_steps, n_envs, batch_size = 3, 1000, 1025
    m = n_steps * n_envs
    host, dev = _rollout(n_steps, n_envs)
    s = pkg.MinibatchSampler(n_steps, n_envs, batch_size, SPEC, DEV, seed=SEED)
    offset = torch.zeros(1, dtype=torch.int64, device=DEV)
    kept = {k: torch.empty((m,) + tuple(v.shape[2:]), dtype=v.dtype, device=DEV) for k, v in dev.items()}
    kept["indices"] = torch.empty(m, dtype=torch.int64, device=DEV)

    def one_epoch():
        at = 0
        for mb in s.epoch(dev, EPOCH, epoch_offset=offset):
            n = mb["indices"].shape[0]
            for k, v in mb.items():
                kept[k][at:at + n].copy_(v)
            at += n
        offset.add_(1)

    one_epoch()                                                 # the scratch is made outside the capture
    offset.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one_epoch()
    for replay in range(2):
        graph.replay()
        torch.cuda.synchronize()
        samples, _ = M.permutation(m, SEED, EPOCH + replay)
        _check_copies(kept, host, samples, ("replay", replay))
        for start in range(0, m, batch_size):
            sl = slice(start, min(start + batch_size, m))
            _check_advantages(kept["advantages"][sl], M.gather(host["advantages"], samples[sl]), ("replay", replay, start))
    assert int(offset) == 2


def test_the_scratch_cannot_grow_inside_a_capture():
    pkg = _pkg()
    _, dev = _rollout(3, 65)
    s = pkg.MinibatchSampler(3, 65, 64, SPEC, DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="MinibatchSampler: the scratch would have to grow inside a graph capture"):
        with torch.cuda.graph(graph):
            s.gather(dev, 0, 0)
    torch.cuda.synchronize()
    got = s.gather(dev, 0, 0)                                   # and the sampler works afterwards
    assert got["indices"].shape == (64,)


# ---- 7. with the collectors ---------------------------------------------------------------------------------------------------------------
SIX = ("obs", "actions", "values", "log_probs", "advantages", "returns")


def _check_rollout(pkg, out, n_steps, n_envs):
    """for_rollout(out, 100) over one epoch against out[name].transpose(0, 1).reshape(M, ...)[perm] for the five copied fields (the
    normalised advantages are test 4's: nothing bounds |mean| / std of a rollout's advantages)."""
    m = n_steps * n_envs
    s = pkg.MinibatchSampler.for_rollout(out, 100, seed=SEED)
    assert (s.n_steps, s.num_envs, s.normalize, list(s.fields)) == (n_steps, n_envs, "advantages", list(SIX))
    perm = s.permutation(EPOCH).to(DEV)
    assert np.array_equal(perm.cpu().numpy(), M.permutation(m, SEED, EPOCH)[0])
    flat = {k: out[k].transpose(0, 1).reshape((m,) + tuple(out[k].shape[2:]))[perm] for k in SIX}
    rows = 0
    for mb in s.epoch(out, EPOCH):
        n = mb["indices"].shape[0]
        for k in SIX:
            if k != "advantages":
                assert torch.equal(_bits(mb[k]), _bits(flat[k][rows:rows + n])), (k, rows)
        assert torch.equal(mb["indices"], perm[rows:rows + n])
        assert bool(torch.isfinite(mb["advantages"]).all())
        rows += n
    assert rows == m and n == m % 100
    with pytest.raises(ValueError, match="'episode_starts' must be float32 or int32, got torch.uint8"):
        pkg.MinibatchSampler.for_rollout(out, 100, fields=SIX + ("episode_starts",))


def test_with_the_rollout_collector():
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    from drl_dronenavigation_amd.collector import RolloutCollector
    n, T = 64, 4
    env = pkg.DroneVecEnv(tracks.circle(1, 4, 1), n, max_steps=3, seed=17, device=DEV, normalize_obs=True, **NOISE)
    g = torch.Generator(device="cpu").manual_seed(3)
    Wa, Wv = (0.05 * torch.randn((13, 4), generator=g)).to(DEV), (0.1 * torch.randn((13,), generator=g)).to(DEV)

    def policy(rows):
        x = torch.nan_to_num(rows).clamp(-5, 5)
        return 0.0922 + 0.01 * torch.tanh(x @ Wa), x @ Wv, -(x * x).sum(dim=1)
    out = RolloutCollector(env, policy, T).collect()
    torch.cuda.synchronize()
    _check_rollout(pkg, out, T, n)
    env.close()


def test_with_the_fused_rollout_collector():
    """Its `obs` is the view [:n_steps] of n_steps + 1 slots: dense, and read in place."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    from drl_dronenavigation_amd.collector import FusedRolloutCollector
    n, T = 64, 4
    env = pkg.DroneVecEnv(tracks.circle(1, 4, 1), n, max_steps=3, seed=17, device=DEV, normalize_obs=True)
    torch.manual_seed(4)
    pol = pkg.FusedMlpPolicy(pkg.MlpActorCritic(log_std_init=-5.0).to(DEV), n, DEV)
    out = FusedRolloutCollector(env, pol, T, use_graph=False, seed=1).collect()
    torch.cuda.synchronize()
    assert out["obs"].shape == (T, n, 13) and out["obs"].is_contiguous()
    _check_rollout(pkg, out, T, n)
    env.close()
