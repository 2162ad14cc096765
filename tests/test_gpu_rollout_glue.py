"""The small kernels between the policy and the step -- dn_gae, dn_add_bootstrap, dn_policy_sample, dn_squashed_sample, dn_pack_done /
dn_compact_done, dn_preprocess_action -- each against the plain statement of its operation (tests/rollout_glue_support.py) at every
fleet edge, on a real MI355X.  These produce the numbers PPO trains on; an error in them crashes nothing, it biases learning.

Bit for bit (the float32 references round every operation as the kernels do; tests/test_rollout_glue_cpu.py holds gae32 to the oracle's
loop and to the reference's torch lines): advantages and returns, the bootstrapped rewards and every reward that is not bootstrapped,
the Gaussian log-probability, the clipped action, the deterministic action, the packed episode records and index lists, and each
optional output of the action chain.  Within a derived allowance: the sampled action against the float64 form (one ulp of expf -- the
device library's documented accuracy --, half an ulp each for the product and the sum).  Within the project's existing bars: the
N(0,1) draws against the oracle's generator (4.8e-7, and 99.99 % bit-equal at 16 421 drones), the squashed action (2e-6) and its
log-probability (1e-5 relative).  Every output that has a size sits between guard cells of a sentinel bit pattern.
Measured maxima: profiles/rollout_glue_errors.txt."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import rollout_glue_support as R  # noqa: E402
from gpu_support import DEV  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402
from model_support import _noise  # noqa: E402

pytestmark = pytest.mark.gpu

G = 64                                  # guard words on each side: 256 bytes, so an output keeps the alignment of the allocation
SEED = 20240917
BIG_OFFSET = (1 << 33) + 12345          # global drone ids in the Philox counter's high word


def _lib():
    pkg = _pkg()
    return pkg, pkg._capi, pkg._capi.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def guarded(shape, dtype=torch.float32):
    """(buf, out): `out` of `shape` (a 4-byte dtype) inside a sentinel-filled int32 buffer with G guard words in front and G behind."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * G,), R.PATTERN, dtype=torch.int32, device=DEV)
    return buf, buf[G:G + numel].view(dtype).view(*shape)


def check_guards(buf, tag, written=True):
    assert bool((buf[:G] == R.PATTERN).all()) and bool((buf[-G:] == R.PATTERN).all()), f"{tag}: a store left the output"
    if written:
        assert not bool((buf[G:-G] == R.PATTERN).any()), f"{tag}: an output word was never written"


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)         # a writable, contiguous copy: the shared inputs are read-only


def host(t):
    return t.detach().cpu().numpy()


def _env(n, offset=12345, **kw):
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    env = pkg.DroneVecEnv(tracks.reaching(), n, device=torch.device(DEV), env_id_offset=offset, **kw)
    env.reset_tensor()
    return env


def policy_sample(env, mean, log_std, deterministic=0, seed=SEED):
    """dn_policy_sample into guarded outputs: (actions [n, 4], clipped [n, 4], log_prob [n]) as numpy, guards checked."""
    _, capi, lib = _lib()
    n = env.num_envs
    (ba, a), (bc, c), (bl, lp) = guarded((n, 4)), guarded((n, 4)), guarded((n,))
    capi.check(lib.dn_policy_sample(env._handle, mean.data_ptr(), (C.c_float * 4)(*[float(x) for x in log_std]), seed, deterministic,
                                    a.data_ptr(), c.data_ptr(), lp.data_ptr(), _stream()))
    torch.cuda.synchronize()
    for b, name in ((ba, "actions"), (bc, "clipped"), (bl, "log_prob")):
        check_guards(b, f"dn_policy_sample n={n} {name}")
    return host(a), host(c), host(lp)


def draws(env, seed=SEED):
    """The N(0,1) draws of the fleet at the environment's counter: mean 0 and log_std 0 make the action the draw itself (0 + 1 z)."""
    z, _, _ = policy_sample(env, torch.zeros((env.num_envs, 4), device=DEV), (0.0, 0.0, 0.0, 0.0), seed=seed)
    return z


def squashed_sample(env, rows, deterministic=0, want_lp=True, seed=SEED):
    _, capi, lib = _lib()
    n = env.num_envs
    (ba, a), (bl, lp) = guarded((n, 4)), guarded((n,))
    capi.check(lib.dn_squashed_sample(env._handle, rows.data_ptr(), seed, deterministic, a.data_ptr(), lp.data_ptr() if want_lp else None,
                                      _stream()))
    torch.cuda.synchronize()
    check_guards(ba, f"dn_squashed_sample n={n} actions")
    check_guards(bl, f"dn_squashed_sample n={n} log_prob", written=want_lp)
    return host(a), host(lp) if want_lp else None


# ---- GAE ----------------------------------------------------------------------------------------------------------------------------
def _gae_abi(r, v, d, lv, ld, gamma, lam, tag):
    _, capi, lib = _lib()
    T, N = r.shape
    (ba, adv), (br, ret) = guarded((T, N)), guarded((T, N))
    tr, tv, td, tlv, tld = dev(r), dev(v), dev(d), dev(lv), dev(ld)
    capi.check(lib.dn_gae(tr.data_ptr(), tv.data_ptr(), td.data_ptr(), tlv.data_ptr(), tld.data_ptr(), T, N, gamma, lam, adv.data_ptr(),
                          ret.data_ptr(), 0, _stream()))
    torch.cuda.synchronize()
    check_guards(ba, f"dn_gae {tag} advantages")
    check_guards(br, f"dn_gae {tag} returns")
    return host(adv), host(ret)


@pytest.mark.parametrize("shape", R.GAE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gae_is_the_float32_loop_bit_for_bit(shape):
    """One step, one drone, the 256-lane workgroup and one lane either side of it, at every discount pair (gamma or lambda of 0 and 1
    included) with no, some and only episode starts: advantages and returns are the bits of gae32, which are the oracle's."""
    for density, last_all, gamma, lam in R.gae_cases():
        args = R.gae_inputs(*shape, density, last_all)
        tag = (shape, density, last_all, gamma, lam)
        adv, ret = _gae_abi(*args, gamma, lam, tag)
        want_adv, want_ret = R.gae32(*args, gamma, lam)
        assert R.same_bits(adv, want_adv), (tag, float(np.abs(adv - want_adv).max()))
        assert R.same_bits(ret, want_ret), (tag, float(np.abs(ret - want_ret).max()))


def test_gae_wrapper_takes_views_and_bool_flags():
    """pkg.gae on a transposed (non-contiguous) reward view and bool flags: the same bits."""
    pkg = _pkg()
    r, v, d, lv, ld = R.gae_inputs(7, 256, 0.05)
    rt = dev(r.T)                                           # [N, T] contiguous: its transpose is the [T, N] rewards, strided
    assert not rt.t().is_contiguous()
    adv, ret = pkg.gae(rt.t(), dev(v), dev(d).bool(), dev(lv), dev(ld).bool(), 0.99, 0.95)
    torch.cuda.synchronize()
    want_adv, want_ret = R.gae32(r, v, d, lv, ld, 0.99, 0.95)
    assert R.same_bits(host(adv), want_adv) and R.same_bits(host(ret), want_ret)


def test_a_non_finite_gae_cell_stays_in_its_column():
    """A NaN reward and a +inf value at mid-T in two columns: every other drone's bits are those of the run without them, and the two
    columns are gae32's -- NaN where it has NaN, the same bits elsewhere."""
    T, N = 7, 256
    r, v, d, lv, ld = R.gae_inputs(T, N, 0.05)
    clean = _gae_abi(r, v, d, lv, ld, 0.99, 0.95, "clean")
    rb, vb = r.copy(), v.copy()
    rb[T // 2, 5], vb[T // 2, 200] = np.nan, np.inf
    bad = _gae_abi(rb, vb, d, lv, ld, 0.99, 0.95, "non-finite")
    want = R.gae32(rb, vb, d, lv, ld, 0.99, 0.95)
    others = np.ones(N, bool)
    others[[5, 200]] = False
    for got, ref, base, name in zip(bad, want, clean, ("advantages", "returns")):
        assert R.same_bits(got[:, others], base[:, others]), name
        assert np.isnan(ref[:, [5, 200]]).any() and not np.isnan(ref[:, others]).any()
        for col in (5, 200):
            nan = np.isnan(ref[:, col])
            assert np.array_equal(np.isnan(got[:, col]), nan), (name, col)
            assert R.same_bits(got[~nan, col], ref[~nan, col]), (name, col)


# ---- bootstrap ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.FLEETS + (65537,))
def test_bootstrap_touches_truncated_cells_only(n):
    """reward += gamma V(terminal_observation) where truncated: bit-equal to bootstrap32 there, and the exact input bits everywhere
    else while terminal_value holds NaN, inf and 1e30 there (the masked critic forward leaves such cells unwritten).  Without a
    truncation the call changes nothing."""
    _, capi, lib = _lib()
    rng = np.random.default_rng(n)
    reward = rng.standard_normal(n).astype(np.float32)
    reward[rng.random(n) < 0.1] = np.float32(-10.0)
    tv = (3.0 * rng.standard_normal(n)).astype(np.float32)
    trunc = rng.choice(np.array([0, 0, 1, 255], np.uint8), n)
    trunc[n // 2] = 0
    if n > 1:
        reward.view(np.uint32)[n // 2] = 0x7FC00001         # a reward that is itself a NaN keeps its payload where it is not bootstrapped
    if n > 2:
        trunc[0], trunc[n - 1] = 1, 255
    tv[trunc == 0] = np.resize(np.array([np.nan, np.inf, 1e30, -np.inf], np.float32), int((trunc == 0).sum()))
    for tr in (trunc, np.zeros(n, np.uint8)):
        garbage = tv if tr is trunc else np.full(n, np.nan, np.float32)
        buf, out = guarded((n,))
        out.copy_(dev(reward))
        t_tv, t_tr = dev(garbage), dev(tr)
        capi.check(lib.dn_add_bootstrap(out.data_ptr(), t_tv.data_ptr(), t_tr.data_ptr(), 0.99, n, 0, _stream()))
        torch.cuda.synchronize()
        check_guards(buf, f"dn_add_bootstrap n={n}", written=False)
        got, want = host(out), R.bootstrap32(reward, garbage, tr, 0.99)
        keep = tr == 0
        assert np.array_equal(R.u32(got)[keep], R.u32(reward)[keep]), "a reward that was not truncated changed"
        assert R.same_bits(got, want), float(np.nanmax(np.abs(got - want)))
        assert np.isfinite(got[~keep]).all()
        if tr is not trunc:
            assert R.same_bits(got, reward)


# ---- policy sample ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _sampled(n):
    """One environment per fleet size, its draws, and the sampled outputs per log_std row (computed once, shared, left unchanged)."""
    env = _env(n)
    z = draws(env)
    mean = dev(R.means(n))
    out = {ls: policy_sample(env, mean, ls) for ls in R.LOG_STD_ROWS}
    det = {ls: policy_sample(env, mean, ls, deterministic=1) for ls in R.LOG_STD_ROWS}
    env.close()
    return z, out, det


@pytest.mark.parametrize("n", R.FLEETS)
def test_policy_sample_log_prob_and_clip_are_bit_exact(n):
    z, out, _ = _sampled(n)
    assert np.isfinite(z).all() and (n < 64 or np.abs(z).max() > 2.0)
    for ls in R.LOG_STD_ROWS:
        a, c, lp = out[ls]
        assert R.same_bits(lp, R.logprob32(z, ls)), (n, ls, float(np.abs(lp - R.logprob32(z, ls)).max()))
        assert R.same_bits(c, np.clip(a, np.float32(-1.0), np.float32(1.0))), (n, ls)


@pytest.mark.parametrize("n", R.FLEETS)
def test_policy_sample_action_is_within_the_float32_allowance(n):
    """actions against mean + exp(log_std) z in float64, z being the device's own draw: one ulp of expf and half an ulp of the product
    (1.5 x 2^-23 of the product) plus half an ulp of the sum.  The bar is derived, not measured: numpy's float32 evaluation meets it
    (tests/test_rollout_glue_cpu.py)."""
    z, out, _ = _sampled(n)
    for ls in R.LOG_STD_ROWS:
        a = out[ls][0]
        ls32 = np.asarray(ls, np.float32)
        ratio = np.abs(a.astype(np.float64) - R.sample64(R.means(n), ls32, z)) / R.sample_allowance(ls32, z, a)
        print(f"dn_policy_sample n={n} log_std {ls}: largest |action - sample64| / allowance {float(ratio.max()):.3f}")
        assert float(ratio.max()) <= 1.0, (n, ls, float(ratio.max()))


@pytest.mark.parametrize("n", R.FLEETS)
def test_policy_sample_deterministic_is_the_mean(n):
    _, _, det = _sampled(n)
    for ls in R.LOG_STD_ROWS:
        a, c, lp = det[ls]
        assert torch.equal(torch.from_numpy(a), torch.from_numpy(R.means(n).copy())), (n, ls)
        assert R.same_bits(lp, R.logprob32(np.zeros((n, 4), np.float32), ls)), (n, ls)
        assert R.same_bits(c, np.clip(a, np.float32(-1.0), np.float32(1.0))), (n, ls)


# ---- counter keying -----------------------------------------------------------------------------------------------------------------
def _advance(env, n):
    """reset (done), three dn_step and -- where the fleet allows the fused launch -- one dn_step_many of five: the counter after it."""
    hover = torch.full((n, 4), 0.0922, device=DEV)
    for _ in range(3):
        env.step_tensor(hover)
    if n % 4 == 0:
        env.rollout_tensor(hover.expand(5, n, 4).contiguous())
        return 8
    return 3


def _check_keying(env, n, count, share=False):
    """Every drone's draw -- the ragged last tile's included -- is the oracle's at (seed, global id, `count`, stream 9), and
    dn_squashed_sample draws the same normals (mu 0, log_std 0: the action is tanh z)."""
    assert env.step_count == count
    z = draws(env)
    ref = _noise(SEED, BIG_OFFSET, n, count, 9)
    err = np.abs(z - ref)
    assert float(err.max()) <= 4.8e-7, (n, count, int(err.max(1).argmax()), float(err.max()))
    if share:
        eq = float((R.u32(z) == R.u32(ref)).mean())
        print(f"draws n={n} counter {count}: {eq:.6f} bit-equal to the oracle's, max |diff| {float(err.max()):.3e}")
        assert eq >= 0.9999
    a, _ = squashed_sample(env, torch.zeros((n, 8), device=DEV), want_lp=False)
    assert float(np.abs(a - np.tanh(z.astype(np.float64))).max()) <= 2e-6, (n, count)


@pytest.mark.parametrize("n", [65, 1000])
def test_draws_are_keyed_by_each_tiles_own_counter(n):
    """The samplers read the Philox counter from their drone's tile.  After single steps and a fused launch, and again with a counter
    whose high word is set, every tile's counter -- a last tile of one drone (65) or of 40 (1000) included -- is the environment's."""
    env = _env(n, BIG_OFFSET)
    _check_keying(env, n, _advance(env, n))
    env.step_count = (1 << 40) + 5
    _check_keying(env, n, (1 << 40) + 5)
    env.step_tensor(torch.full((n, 4), 0.0922, device=DEV))
    _check_keying(env, n, (1 << 40) + 6)
    env.close()


def test_draws_at_a_large_ragged_fleet_are_bit_equal_to_the_oracles():
    """16 384 + 37 drones: at least 99.99 % of the draws bit-equal (a smaller fleet would fail that on one legitimate 1-ulp draw)."""
    n = 16384 + 37
    env = _env(n, BIG_OFFSET)
    _check_keying(env, n, _advance(env, n), share=True)
    env.step_count = (1 << 40) + 5
    _check_keying(env, n, (1 << 40) + 5, share=True)
    env.close()


# ---- squashed sample ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.FLEETS)
def test_squashed_sample_at_every_fleet(n):
    """tanh(mu + exp(clamp(log_std)) z) within 2e-6 of float64 and the log-probability within 1e-5 (relative) of its float32 form, the
    bars of test_squashed_sample_draws_the_policy_sample_normals, with rows at the clamp edges, saturated rows (mu = +-12, log_std =
    -20: |a| never above 1, a finite log-probability) and means of +-1e-30."""
    rows, saturated, tiny = R.squashed_rows(n)
    env = _env(n)
    z = draws(env)
    a, lp = squashed_sample(env, dev(rows))
    det, _ = squashed_sample(env, dev(rows), deterministic=1, want_lp=False)
    a_only, _ = squashed_sample(env, dev(rows), want_lp=False)
    env.close()
    err = np.abs(a - R.squashed64(rows[:, :4], rows[:, 4:], z))
    want_lp = R.squashed_logprob32(z, rows[:, 4:], a)
    lp_err = np.abs(lp.astype(np.float64) - want_lp) / (1.0 + np.abs(want_lp))
    print(f"dn_squashed_sample n={n}: max |action - float64| {float(err.max()):.3e} (bar 2e-6), log_prob relative {float(lp_err.max()):.3e} (bar 1e-5)")
    assert float(err.max()) <= 2e-6
    assert float(np.abs(a).max()) <= 1.0 and np.isfinite(lp).all()
    assert float(lp_err.max()) <= 1e-5
    assert R.same_bits(a_only, a), "the action depends on whether the log-probability was asked for"
    assert float(np.abs(det - np.tanh(rows[:, :4].astype(np.float64))).max()) <= 2e-6
    if n >= 16:
        assert saturated.any() and tiny.any()
    assert (np.sign(a[saturated]) == np.sign(rows[saturated, :4])).all() and float(np.abs(a[saturated]).min(initial=1.0)) >= 1.0 - 2e-6
    assert np.isfinite(a[tiny]).all() and np.isfinite(lp[tiny]).all()


# ---- pack_done and compact_done -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.PACK_SIZES)
def test_pack_done_rows_and_indices_are_bit_exact(n):
    """Synthetic records, no environment: at the 64-drone word and the 65 536-drone workgroup boundaries, with all, half, a few and no
    drones finished, indices[:count] and packed[:count] are pack_reference's bits -- episode lengths whose float reinterpretation is a
    signalling or a quiet NaN included: the int words travel as float bit patterns --, nothing past count is written, and
    dn_compact_done returns the same list."""
    _, capi, lib = _lib()
    tobs, ep_ret, ep_len, trunc, found = R.pack_inputs(n)
    t_tobs, t_ret, t_len, t_trunc, t_found = dev(tobs), dev(ep_ret), dev(ep_len), dev(trunc), dev(found)
    for density in R.PACK_DENSITIES:
        bits = R.done_bits(n, density)
        want_idx, want_rows = R.pack_reference(bits, tobs, ep_ret, ep_len, trunc, found)
        k = want_idx.size
        mask = dev(R.mask_words(bits, n))
        (bi, idx), (bc, cnt), (bp, packed) = guarded((n,), torch.int32), guarded((1,), torch.int32), guarded((n, 16))
        capi.check(lib.dn_pack_done(mask.data_ptr(), n, t_tobs.data_ptr(), t_ret.data_ptr(), t_len.data_ptr(), t_trunc.data_ptr(),
                                    t_found.data_ptr(), idx.data_ptr(), cnt.data_ptr(), packed.data_ptr(), 0, _stream()))
        (bi2, idx2), (bc2, cnt2) = guarded((n,), torch.int32), guarded((1,), torch.int32)
        capi.check(lib.dn_compact_done(mask.data_ptr(), n, idx2.data_ptr(), cnt2.data_ptr(), 0, _stream()))
        torch.cuda.synchronize()
        tag = f"n={n} density={density}"
        for b in (bi, bp, bi2):
            check_guards(b, tag, written=False)
        for b in (bc, bc2):
            check_guards(b, tag)
        assert int(cnt.item()) == k == int(cnt2.item()), (tag, int(cnt.item()), int(cnt2.item()), k)
        assert np.array_equal(host(idx[:k]), want_idx), tag
        assert np.array_equal(host(idx2[:k]), want_idx), tag
        assert np.array_equal(host(packed[:k].view(torch.int32)), want_rows.view(np.int32)), tag
        assert bool((idx[k:] == R.PATTERN).all()) and bool((idx2[k:] == R.PATTERN).all()), f"{tag}: an index past count was written"
        assert bool((packed[k:].view(torch.int32) == R.PATTERN).all()), f"{tag}: a row past count was written"
        if density == 1.0 and n >= 8:
            assert {R.SNAN_INT, R.QNAN_INT} <= set(want_rows[:, 14].tolist()), "the case lost its NaN patterns"


# ---- preprocess_action ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257])
def test_preprocess_action_with_any_subset_of_outputs(n):
    """rpm, forces and z_torque are optional: each of the seven non-empty subsets gives, bit for bit, the outputs of the call with all
    three, and writes nothing else."""
    _, capi, lib = _lib()
    acts = dev(np.random.default_rng(n).uniform(-1.2, 1.2, (n, 4)).astype(np.float32))
    shapes = dict(rpm=(n, 4), forces=(n, 4), z_torque=(n,))

    def run(names, normalize):
        bufs = {k: guarded(shapes[k]) for k in names}
        ptr = [bufs[k][1].data_ptr() if k in bufs else None for k in ("rpm", "forces", "z_torque")]
        capi.check(lib.dn_preprocess_action(acts.data_ptr(), n, normalize, *ptr, 0, _stream()))
        torch.cuda.synchronize()
        for k, (b, _) in bufs.items():
            check_guards(b, f"dn_preprocess_action n={n} {names} {k}")
        return {k: host(o) for k, (_, o) in bufs.items()}

    for normalize in (1, 0):
        full = run(("rpm", "forces", "z_torque"), normalize)
        assert all(np.isfinite(x).all() for x in full.values()) and float(full["rpm"].max()) > 0.0
        for m in range(1, 8):
            names = tuple(k for j, k in enumerate(("rpm", "forces", "z_torque")) if m >> j & 1)
            got = run(names, normalize)
            for k in names:
                assert R.same_bits(got[k], full[k]), (n, normalize, names, k)
