"""dn_mlp_forward over the whole range its ABI promises on rows of up to 16 columns -- obs_dim 1 .. 16, out_dim 1 .. 32, fleets at every
workgroup edge -- for each of the kernels that serve it (csrc/dn_mlp.hip), and the three wide kernels (csrc/dn_mlp_wide.hip) at 40
columns for everything that is not about the input width, on a real MI355X.

 1. every input width x every head size against the reference, `out` between guard rows; two PPO networks of different head sizes in one
    launch equal their single launches;
 2. every input column lands where its weights are (bit for bit against the same kernel at obs_dim = 1);
 3. every head row is its own (a 32-row head against 32 single-row heads, bit for bit);
 4. fleets of 1 / 33 / 65 / 128 / 129 / 300 drones: guards, reference, and a drone's bits do not depend on the fleet;
 5. the masked forward at other head sizes;
 6. a non-finite input row stays in its MFMA column;
 7. input rows that are 4-byte aligned only;
 8. dn_mlp_step_sampled at 8 and 16 columns against dn_mlp_forward + dn_step_sampled.

Networks: layers 2 and 3 are packed once per architecture, grade and seed; layer 1 is repacked per obs_dim and the head per out_dim.
References and bars are the project's: the bf16 emulation (max < 1e-2, mean < 3e-4) for the PPO bf16 grade, the float64 evaluation of the
float32 network for everything else (PPO fp32 1e-4, fp16 5e-3: the value-head bar, random_layers' heads are at value_net scale; SAC fp32
1e-4, fp16 5e-3, bf16 5e-2).  Measured maxima: profiles/mlp_shapes_errors.txt."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mlp_support as S  # noqa: E402
from gpu_support import DEV  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402

pytestmark = pytest.mark.gpu

OBS_DIMS = (1, 7, 8, 9, 15, 16)
OUT_DIMS = (1, 2, 5, 17, 32)
SAC_OUT_DIMS = (2, 6, 8, 18, 32)                # 2 act_dim for act_dim in (1, 3, 4, 9, 16)
FLEETS = S.FLEETS + (65, 128)                   # and the first drone past the float32-grade kernel's workgroup, the last one inside the others'
WIDE = 40


class Variant:
    """One kernel of dn_mlp.hip / dn_mlp_wide.hip: the networks that reach it and the environment variable that picks it."""

    def __init__(self, arch, grade, shape, wide=False):
        self.arch, self.grade, self.shape, self.wide = arch, grade, shape, wide
        self.obs_dims = (WIDE,) if wide else OBS_DIMS
        self.out_dims = OUT_DIMS if arch == "ppo" else SAC_OUT_DIMS
        self.id = f"{arch}-{'wide-' if wide else ''}{shape}-{grade}"

    def pick(self, monkeypatch):
        monkeypatch.setenv("DN_MLP_SHAPE" if self.arch == "ppo" else "DN_MLP_SAC_SHAPE", self.shape.split()[0])     # read per call: 1 | 4 | 8

    def dims(self, pairs):
        """(obs_dim, out_dim) pairs of a test, stated for the narrow PPO kernels, as this variant runs them."""
        return [(WIDE if self.wide else d, o if self.arch == "ppo" else SAC_OUT_DIMS[OUT_DIMS.index(o)]) for d, o in pairs]


NARROW = [Variant("ppo", "bf16", "1 wave"), Variant("ppo", "bf16", "4 waves"), Variant("ppo", "fp16", "4 waves"),
          Variant("ppo", "bf16", "8 waves"), Variant("ppo", "fp16", "8 waves"), Variant("ppo", "fp32", "4 waves x3"),
          Variant("sac", "bf16", "1 wave"), Variant("sac", "fp32", "1 wave"),
          Variant("sac", "bf16", "4 waves"), Variant("sac", "fp32", "4 waves"), Variant("sac", "fp16", "4 waves")]
VARIANTS = NARROW + [Variant("ppo", "bf16", "4 waves", wide=True), Variant("ppo", "fp16", "4 waves", wide=True),
                     Variant("ppo", "fp32", "4 waves x3", wide=True)]
every_variant = pytest.mark.parametrize("v", [pytest.param(v, id=v.id) for v in VARIANTS])
narrow_variants = pytest.mark.parametrize("v", [pytest.param(v, id=v.id) for v in NARROW])

BARS = {("ppo", "bf16"): (1e-2, 3e-4), ("ppo", "fp32"): (1e-4, None), ("ppo", "fp16"): (5e-3, None),
        ("sac", "bf16"): (5e-2, None), ("sac", "fp32"): (1e-4, None), ("sac", "fp16"): (5e-3, None)}       # (max, mean or None)


def _pm():
    _pkg()
    from drl_dronenavigation_amd import policy_mfma as pm
    return pm


class Family:
    """The networks of one (architecture, grade, seed): layers 2 (and 3) fixed and packed once, layer 1 drawn per obs_dim, the head per
    out_dim, both by mlp_support.random_layers / random_sac_layers."""

    def __init__(self, arch, grade, seed):
        pm = _pm()
        self.pm, self.arch, self.grade, self.seed = pm, arch, grade, seed
        self.ppo = arch == "ppo"
        self.base_layers = S.random_layers(16, 32, seed) if self.ppo else S.random_sac_layers(16, 16, seed)
        self.base = pm.pack_mlp(self.base_layers, DEV, grade) if self.ppo else pm.pack_sac_actor(self.base_layers, DEV, grade)
        self.first = functools.lru_cache(None)(self._first)
        self.head = functools.lru_cache(None)(self._head)
        self._packed_first, self._packed_head = {}, {}

    def _first(self, d):
        return (S.random_layers if self.ppo else S.random_sac_layers)(d, 1, 1000 * self.seed + d)[0]

    def _head(self, o):
        """(W [o, 256], b [o]); the SAC actor's two heads stacked as pack_sac_actor stacks them."""
        if self.ppo:
            return S.random_layers(16, o, 2000 * self.seed + o)[3]
        (wm, bm), (ws, bs) = S.random_sac_layers(16, o // 2, 2000 * self.seed + o)[2:]
        return torch.cat((wm, ws), 0), torch.cat((bm, bs), 0)

    def layers(self, d, o):
        """The float32 network of pack(d, o), in the form the references take."""
        if self.ppo:
            return [self.first(d)] + self.base_layers[1:3] + [self.head(o)]
        wh, bh = self.head(o)
        return [self.first(d), self.base_layers[1], (wh[: o // 2], bh[: o // 2]), (wh[o // 2:], bh[o // 2:])]

    def pack_first(self, w, b):
        pw, pb = self.pm.pack_layer(w, b, True, scale=self.pm.TANH_PRESCALE if self.ppo else 1.0, grade=self.grade)
        return pw.to(DEV), pb.to(DEV), int(w.shape[1])

    def pack_head(self, w, b):
        pw, pb = self.pm.pack_layer(w, b, False, scale=1.0, grade=self.grade)
        return pw.to(DEV), pb.to(DEV), int(w.shape[0])

    def with_(self, first, head):
        """The base pack with another layer 1 and another head (the results of pack_first / pack_head)."""
        p = dict(self.base)
        (p["w1"], p["b1"], p["obs_dim"]), (p["wh"], p["bh"], p["out_dim"]) = first, head
        return p

    def pack(self, d, o):
        if d not in self._packed_first:
            self._packed_first[d] = self.pack_first(*self.first(d))
        if o not in self._packed_head:
            self._packed_head[o] = self.pack_head(*self.head(o))
        return self.with_(self._packed_first[d], self._packed_head[o])


@functools.lru_cache(None)
def family(arch, grade, seed=1):
    return Family(arch, grade, seed)


@functools.lru_cache(None)
def inputs(n, d, seed=0):
    """[n, d] float32 in (-1, 1), on the CPU and on the device."""
    x = torch.rand((n, d), generator=torch.Generator().manual_seed(10000 * seed + 100 * n + d)) * 2 - 1
    return x, x.to(DEV)


@functools.lru_cache(None)
def reference(arch, grade, seed, d, o, n, xseed=0):
    """The reference of family(arch, grade, seed).pack(d, o) on inputs(n, d, xseed): computed once, shared, left unchanged."""
    layers, x = family(arch, grade, seed).layers(d, o), inputs(n, d, xseed)[0]
    if arch == "sac":
        return S.sac_f64(layers, x)
    return S.mlp_reference(layers, x).double() if grade == "bf16" else S.f64(layers, x)


class Worst:
    """The largest errors of a test's cases and where they were met; failures against the variant's bars."""

    def __init__(self, v):
        self.v, self.bars = v, BARS[(v.arch, v.grade)]
        self.max = self.mean = 0.0
        self.at = None
        self.fails = []

    def add(self, got, ref, where):
        err = (got.double().cpu() - ref).abs()
        mx, mean = float(err.max()), float(err.mean())
        if not bool(torch.isfinite(err).all()):
            self.fails.append((where, "not finite"))
        if mx > self.max:
            self.max, self.at = mx, where
        self.mean = max(self.mean, mean)
        if self.bars[1] is not None:                         # the bf16 emulation's bars are strict
            if not (mx < self.bars[0] and mean < self.bars[1]):
                self.fails.append((where, mx, mean))
        elif not mx <= self.bars[0]:
            self.fails.append((where, mx))

    def report(self, test):
        ref = "the bf16 emulation" if self.bars[1] is not None else "float64"
        mean = f" mean {self.mean:.3e} (bar {self.bars[1]:.0e})" if self.bars[1] is not None else ""
        print(f"{test} {self.v.id}: max |err| vs {ref} {self.max:.3e} at {self.at} (bar {self.bars[0]:.0e}){mean}")
        assert not self.fails, self.fails


def _run_guarded(pm, packs, x, n, tag):
    """One launch with every `out` between guard rows; returns the outputs after checking the guards."""
    bufs = [S.guarded_out(n, p["out_dim"], DEV) for p in packs]
    pm.mlp_forward(packs, x, [o for _, o in bufs])
    for (buf, _), p in zip(bufs, packs):
        S.check_guards(buf, n, p["out_dim"], tag)
    return [o for _, o in bufs]


@every_variant
def test_every_input_width_and_head_size(v, monkeypatch):
    """N = 129: a ragged tile, and a second workgroup for every kernel.  A store at j >= out_dim lands in the next drone's row or in the
    guard row behind the last one; a row of the head that comes from the wrong accumulator register misses the reference."""
    pm, fam, n = _pm(), family(v.arch, v.grade), 129
    v.pick(monkeypatch)
    worst = Worst(v)
    for d in v.obs_dims:
        x = inputs(n, d)[1]
        for o in v.out_dims:
            (out,) = _run_guarded(pm, [fam.pack(d, o)], x, n, (d, o))
            worst.add(out, reference(v.arch, v.grade, 1, d, o, n), (d, o))
    worst.report("width x head, N=129")
    if v.arch != "ppo":
        return
    other = family(v.arch, v.grade, 2)                      # two networks in one launch: other weights in every layer, another head size
    for d in v.obs_dims:
        x = inputs(n, d)[1]
        for oa, ob in ((32, 1), (5, 17), (1, 32)):
            pa, pb = fam.pack(d, oa), other.pack(d, ob)
            both = _run_guarded(pm, [pa, pb], x, n, (d, oa, ob))
            (alone_a,), (alone_b,) = _run_guarded(pm, [pa], x, n, (d, oa)), _run_guarded(pm, [pb], x, n, (d, ob))
            assert torch.equal(both[0], alone_a) and torch.equal(both[1], alone_b), (d, oa, ob)
            assert not torch.equal(alone_a[:, :1], alone_b[:, :1])


@narrow_variants
def test_every_column_lands_where_its_weights_are(v, monkeypatch):
    """A W1 whose only non-zero column is j (zero b1) at obs_dim = D against the same kernel at obs_dim = 1, fed column j with that column
    of W1: each layer-1 pre-activation is one product plus exact zeros, so the outputs are the same bits -- unless the load predicates
    drop the column, read it from another drone's row, or put it in another slot than the packer."""
    pm, fam, n, o = _pm(), family(v.arch, v.grade), 33, v.out_dims[2]
    v.pick(monkeypatch)
    head = fam.pack_head(*fam.head(o))
    zero_b1 = torch.zeros(fam.first(1)[0].shape[0])
    for d in OBS_DIMS:
        w1, x = fam.first(d)[0], inputs(n, d)[1]
        seen = set()
        for j in range(d):
            wj = torch.zeros_like(w1)
            wj[:, j] = w1[:, j]
            (got,) = pm.mlp_forward([fam.with_(fam.pack_first(wj, zero_b1), head)], x)
            (want,) = pm.mlp_forward([fam.with_(fam.pack_first(w1[:, j:j + 1].contiguous(), zero_b1), head)], x[:, j:j + 1].contiguous())
            assert torch.equal(got, want), (d, j, float((got - want).abs().max()))
            seen.add(got.cpu().numpy().tobytes())
        assert len(seen) == d, f"obs_dim {d}: the outputs do not depend on the column: the check is vacuous"


@every_variant
def test_every_head_row_is_its_own(v, monkeypatch):
    """A row of an MFMA tile does not depend on the other rows, and neither may the split-K hand-over of the head through LDS: column j of
    a 32-row head is, bit for bit, the output of the one-row head made of its row j and bias j."""
    pm, fam, n, d = _pm(), family(v.arch, v.grade), 33, v.obs_dims[3 if not v.wide else 0]
    v.pick(monkeypatch)
    first, x = fam.pack_first(*fam.first(d)), inputs(n, d)[1]
    wh, bh = fam.head(32)
    (full,) = _run_guarded(pm, [fam.with_(first, fam.pack_head(wh, bh))], x, n, "32 rows")
    assert len({full[:, j].cpu().numpy().tobytes() for j in range(32)}) == 32
    for j in range(32):
        (one,) = _run_guarded(pm, [fam.with_(first, fam.pack_head(wh[j:j + 1].contiguous(), bh[j:j + 1].contiguous()))], x, n, j)
        assert torch.equal(one[:, 0], full[:, j]), (j, float((one[:, 0] - full[:, j]).abs().max()))


@every_variant
def test_fleet_edges(v, monkeypatch):
    """Fleets that end inside the first tile, one drone into the second, at and one past the 64-drone workgroup of the float32-grade kernel
    and the 128-drone workgroup of the others: whole waves without a drone keep the barriers and their share of the weight stream.  Rows
    [0, n) of an n-drone launch are the bits of the 300-drone launch on the same rows."""
    pm, fam = _pm(), family(v.arch, v.grade)
    v.pick(monkeypatch)
    worst = Worst(v)
    for d, o in v.dims([(16, 32), (1, 1), (9, 5)]):
        pk, (_, x) = fam.pack(d, o), inputs(300, d)
        ref = reference(v.arch, v.grade, 1, d, o, 300)
        (big,) = _run_guarded(pm, [pk], x, 300, (d, o, 300))
        for n in FLEETS:
            (out,) = _run_guarded(pm, [pk], x[:n].contiguous(), n, (d, o, n))
            worst.add(out, ref[:n], (d, o, n))
            assert torch.equal(out, big[:n]), (d, o, n, float((out - big[:n]).abs().max()))
    worst.report("fleet edges")


@every_variant
def test_masked_forward_at_other_head_sizes(v, monkeypatch):
    pm, fam, n = _pm(), family(v.arch, v.grade), 300
    v.pick(monkeypatch)
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    mask[::97] = 1
    has = S.tiles_with_a_flag(mask)
    assert bool(has.any()) and bool((~has).any())
    for d, o in v.dims([(9, 32), (16, 5)]):
        pk, x = fam.pack(d, o), inputs(n, d)[1]
        (full,) = pm.mlp_forward([pk], x)
        assert float(full.abs().min()) > 0
        for m, flagged in ((mask, has), (torch.zeros_like(mask), torch.zeros_like(has)), (torch.ones_like(mask), torch.ones_like(has))):
            buf = torch.full((n + 2, o), 7.0, device=DEV)    # guard rows here too: the zeroing loop writes out_dim floats per drone
            pm.mlp_forward([pk], x, [buf[1:-1]], row_mask=m)
            out = buf[1:-1]
            assert torch.equal(out[flagged], full[flagged]) and float(out[~flagged].abs().sum()) == 0.0, (d, o, int(m.sum()))
            assert bool((buf[0] == 7.0).all()) and bool((buf[-1] == 7.0).all()), (d, o, int(m.sum()))


@every_variant
def test_a_non_finite_row_stays_in_its_column(v, monkeypatch):
    """A drone is an MFMA column: NaN or +-Inf in drone i's inputs changes no bit of any other drone's outputs (first and last lane of a
    tile, first lane of the next, the single live lane of the last tile), also across the split-K hand-over through LDS.  A NaN row gives
    NaN outputs, as the float64 reference does (the SAC kernels' ReLU was fmaxf, which turns a NaN into 0: they answered such a row
    with finite numbers); nothing is claimed about drone i under +-Inf.  This is also where a load past the end of a row shows: the packed
    W1 is zero there, and only 0 x NaN is not 0.  Ordinary float values through ordinary arithmetic."""
    pm, fam, n = _pm(), family(v.arch, v.grade), 129
    v.pick(monkeypatch)
    for d, o in v.dims([(9, 32), (16, 5)]):
        pk, (x_cpu, x) = fam.pack(d, o), inputs(n, d)
        (clean,) = pm.mlp_forward([pk], x)
        clean = clean.clone()
        assert bool(torch.isfinite(clean).all())
        for i in (0, 31, 32, 128):
            others = torch.arange(n, device=DEV) != i
            for value in (float("nan"), float("inf"), float("-inf")):
                bad = x.clone()
                bad[i] = value
                (out,) = _run_guarded(pm, [pk], bad, n, (d, o, i, value))
                assert torch.equal(out[others], clean[others]), (d, o, i, value)
                if value != value:
                    bad_cpu = x_cpu.clone()
                    bad_cpu[i] = value
                    ref = S.sac_f64(fam.layers(d, o), bad_cpu[i:i + 1]) if v.arch == "sac" else S.f64(fam.layers(d, o), bad_cpu[i:i + 1])
                    assert bool(torch.isnan(ref).all())
                    assert bool(torch.isnan(out[i]).all()), (d, o, i, out[i].tolist())


@every_variant
def test_rows_that_are_four_byte_aligned_only(v, monkeypatch):
    """The same [n, obs_dim] data read from a flat buffer one float past a 16-byte boundary: the same bits."""
    pm, fam, n, o = _pm(), family(v.arch, v.grade), 129, v.out_dims[2]
    v.pick(monkeypatch)
    for d in ((WIDE,) if v.wide else (1, 9, 16)):
        pk, x = fam.pack(d, o), inputs(n, d)[1]
        flat = torch.zeros(n * d + 8, device=DEV)
        assert flat.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
        shifted = flat[1:1 + n * d].view(n, d)
        shifted.copy_(x)
        assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
        (want,) = pm.mlp_forward([pk], x)
        (got,) = _run_guarded(pm, [pk], shifted, n, d)
        assert torch.equal(got, want), (d, float((got - want).abs().max()))


@pytest.mark.parametrize("obs_dim", [8, 16])
@pytest.mark.parametrize("grade,n", [("bf16", 256), ("fp16", 256), ("fp32", 320)])
def test_fused_policy_step_at_other_widths(grade, n, obs_dim, monkeypatch):
    """dn_mlp_step_sampled shares mlp_pair_body / mlp_x3_body with dn_mlp_forward and takes the same obs_dim 1 .. 16: at 8 columns (the
    row ends at the lane-group boundary) and 16 (a full row) it gives the bits of dn_mlp_forward + dn_step_sampled on a twin environment
    -- means, values, actions, log-probabilities, every step output and the final state -- over episodes that end and restart
    (tests/test_gpu_round3.py holds the 13-column case and the collector)."""
    monkeypatch.setenv("DN_MLP_SHAPE", "8")
    pkg = _pkg()
    from drl_dronenavigation_amd import _capi, tracks
    from drl_dronenavigation_amd.policy_mfma import _net_struct, mlp_forward
    lib = _capi.load()
    dev = torch.device(DEV)
    kw = dict(normalize_obs=grade != "fp16", max_steps=9, env_id_offset=777)
    a, b = pkg.DroneVecEnv(tracks.reaching(), n, device=dev, **kw), pkg.DroneVecEnv(tracks.reaching(), n, device=dev, **kw)
    assert a.kernel_waves(fused=False) == 3
    torch.manual_seed(6 + obs_dim)
    net = pkg.MlpActorCritic(obs_dim=obs_dim, log_std_init=-4.0).to(dev)
    with torch.no_grad():
        net.action_net.bias.fill_(0.0922)
    pol = pkg.FusedMlpPolicy(net, n, dev, grade=grade)
    extra = torch.tensor([0.25, -0.5, 0.75], device=dev).expand(n, 3)

    def policy_obs(obs):
        return obs[:, :8].contiguous() if obs_dim == 8 else torch.cat((obs, extra), dim=1)

    mk = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)        # noqa: E731
    A, B = [dict(mean=mk(n, 4), val=mk(n, 1), obs=mk(n, 13), rew=mk(n), done=mk(n, dt=torch.uint8), trunc=mk(n, dt=torch.uint8),
                 found=mk(n, dt=torch.int32), act=mk(n, 4), logp=mk(n), term=mk(n, 13)) for _ in range(2)]
    log_std = (C.c_float * 4)(*[float(x) for x in pol.log_std_host])
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    oa, ob = a.reset_tensor().clone(), b.reset_tensor().clone()
    assert torch.equal(oa, ob)
    n_done = 0
    for t in range(10):
        pa, pb = policy_obs(oa), policy_obs(ob)
        mlp_forward([pol.pi, pol.vf], pa, [A["mean"], A["val"]])
        _capi.check(lib.dn_step_sampled(a._handle, A["mean"].data_ptr(), log_std, 5, 0, A["act"].data_ptr(), A["logp"].data_ptr(), A["obs"].data_ptr(),
                                        A["rew"].data_ptr(), A["done"].data_ptr(), A["trunc"].data_ptr(), A["found"].data_ptr(), A["term"].data_ptr(),
                                        None, None, None, stream))
        nets = (_capi.DnMlpNet * 2)(_net_struct(pol.pi, B["mean"]), _net_struct(pol.vf, B["val"]))
        _capi.check(lib.dn_mlp_step_sampled(b._handle, C.cast(nets, C.c_void_p), 2, pb.data_ptr(), obs_dim, log_std, 5, 0, B["act"].data_ptr(),
                                            B["logp"].data_ptr(), B["obs"].data_ptr(), B["rew"].data_ptr(), B["done"].data_ptr(),
                                            B["trunc"].data_ptr(), B["found"].data_ptr(), B["term"].data_ptr(), None, None, None, stream))
        torch.cuda.synchronize()
        for k in A:
            assert torch.equal(A[k], B[k]), (t, k)
        n_done += int(A["done"].sum())
        oa.copy_(A["obs"]); ob.copy_(B["obs"])
    assert n_done > 0
    sa, sb = a.get_state(), b.get_state()
    for k in sa.dtype.names:
        assert np.ascontiguousarray(sa[k]).tobytes() == np.ascontiguousarray(sb[k]).tobytes(), k
    assert a.stats() == b.stats() and a.step_count == b.step_count == 10
    a.close(); b.close()
