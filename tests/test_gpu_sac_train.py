"""The training pass of the SAC networks and the Polyak update (include/dronenav.h dn_sac_train_forward / dn_sac_train_backward,
dn_polyak_update, csrc/dn_sac_train.hip, sac_train.py) on the HIP path, against the same float32 parameters and inputs evaluated in
float64 through torch autograd on the CPU, through the C ABI with guard rows unless said.

 1. accuracy: max |out - out64| <= 1e-4, and per gradient tensor, d_x0 and d_x1 included, max |g - g64| <= 1e-4 max |g64|, for every
    group and batch of sac_train_support.CASES (the rows selected as that module says);
 2. guards: every output word is written and nothing beside it; with d_x0 = NULL, d_x1 and every gradient keep the bits of the full run,
    and the other way round;
 3. ReLU's exact zeros: d_out = 0 gives gradients and d_x that are exactly zero over sentinel-filled tensors; a hidden unit whose bias is
    -1e3 is dead on every row: its d_weight row, its d_bias and the next layer's d_weight column are exactly 0.0, and d_x is that of the
    run with the unit's outgoing weights zeroed;
 4. flags: ACCUMULATE over a random pre-fill p is bit-equal to p + g; with NO_PARAM_GRADS the gradient tensors keep their sentinel bits
    and d_x1 keeps the bits of the full run;
 5. the three generalisations are addressing only (torch.equal): a network of a group against that network alone; (x0, x1) against
    cat(x0, x1); head parts against one part of the concatenated rows; Tanh, one network, one input, one part against dn_mlp_train_*;
 6. the same call twice gives equal bits; rows 0..32 at batch 33 are those rows at batch 2 R + 5; a captured forward + backward replays the
    eager bits, and again after the inputs are overwritten in place;
 7. the Polyak update bit for bit against the numpy float64 statement, with guards and a captured replay;
 8. one SAC gradient step of 257 rows through SacTrainer x 3, the loss heads, ClippedAdam x 3 and PolyakUpdate.

The device results of a case are computed once and shared, the references once per case (sac_train_support)."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import mlp_support as ms  # noqa: E402
import mlp_train_support as T  # noqa: E402
import sac_train_support as S  # noqa: E402
from gpu_support import DEV  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402

R = S.R
A, B, C4, F, H, J = (S.BY_NAME[k] for k in "ABCFHJ")


def _ints(t):
    return t.view(torch.int32)


class _Call:
    """One group on the device with every output between guard rows: forward(), backward(); the tensors are views of the guarded
    buffers.  want: (d_x0, d_x1) are asked for; layers: [network][entry] = (W, b) instead of the group's own."""

    def __init__(self, g, act, batch, *, flags=0, want=(True, True), layers=None):
        self.pkg = _pkg()
        self.K, self.lib = self.pkg._capi, self.pkg._capi.load()
        self.g, self.act, self.batch = g, act, batch
        self.want = (want[0], want[1] and g.in1 > 0)
        self.layers = [[(w.to(DEV), b.to(DEV)) for w, b in net] for net in (layers or S.layers_of(g))]
        self.guarded = []                              # (buf, rows, width, name) of every output, for the guard checks
        self.outs = [self._guard(batch, o, f"out[{c * len(g.parts) + p}]") for c in range(g.n_nets) for p, o in enumerate(g.parts)]
        self.d_x0 = self._guard(batch, g.in0, "d_x0")
        self.d_x1 = self._guard(batch, g.in1, "d_x1") if g.in1 else None
        self.grads = []
        for c, net in enumerate(self.layers):
            for l, (w, b) in enumerate(net):
                self.grads += [self._guard(w.shape[0], w.shape[1], f"layers[{c}][{l}].d_weight"), self._guard(1, b.shape[0], f"layers[{c}][{l}].d_bias")]
        n = len(self.layers[0])
        ptrs = [[(w.data_ptr(), b.data_ptr(), self.grads[2 * (c * n + l)].data_ptr(), self.grads[2 * (c * n + l) + 1].data_ptr())
                 for l, (w, b) in enumerate(net)] for c, net in enumerate(self.layers)]
        self.cfg, self.table = S.tables(self.K, g, act, ptrs, flags)
        need = self.lib.dn_sac_train_scratch_bytes(C.byref(self.cfg), self.table, batch)
        assert need == S.scratch_bytes(g, batch)
        self.scratch = torch.empty(need // 8, dtype=torch.float64, device=DEV)
        self.out_table = S.pointer_table([t.data_ptr() for t in self.outs])

    def _guard(self, rows, width, name):
        buf, view = ms.guarded_out(rows, width, DEV)
        self.guarded.append((buf, rows, width, name))
        return view

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def forward(self, x0, x1):
        self.K.check(self.lib.dn_sac_train_forward(C.byref(self.cfg), self.table, x0.data_ptr(), x1.data_ptr() if x1 is not None else None,
                                                   self.batch, self.out_table, self.scratch.data_ptr(), self.scratch.numel() * 8, 0, self.stream()))

    def backward(self, x0, x1, d_out):
        table = S.pointer_table([d.data_ptr() for d in d_out])
        self.K.check(self.lib.dn_sac_train_backward(C.byref(self.cfg), self.table, x0.data_ptr(), x1.data_ptr() if x1 is not None else None, table,
                                                    self.batch, self.d_x0.data_ptr() if self.want[0] else None,
                                                    self.d_x1.data_ptr() if self.want[1] else None, self.scratch.data_ptr(),
                                                    self.scratch.numel() * 8, 0, self.stream()))

    def run(self, x0, x1, d_out):
        self.forward(x0, x1)
        self.backward(x0, x1, d_out)
        torch.cuda.synchronize()
        return self

    def check_guards(self, tag, skip=()):
        """Every output is written and nothing beside it; those whose name begins with one of `skip` keep every sentinel word."""
        for buf, rows, width, name in self.guarded:
            if name.startswith(tuple(skip)) if skip else False:
                assert bool((buf == ms.PATTERN).all()), f"{tag}: {name} was touched"
            else:
                ms.check_guards(buf, rows, width, f"{tag}: {name}")

    def bits(self):
        return [_ints(t).clone() for t in self.outs + [self.d_x0] + ([self.d_x1] if self.d_x1 is not None else []) + self.grads]


def _dev(x0, x1, d_out):
    return x0.to(DEV), (x1.to(DEV) if x1 is not None else None), [d.to(DEV) for d in d_out]


@functools.lru_cache(maxsize=None)
def _result(g, act, batch):
    """The plain call of a case, run once."""
    return _Call(g, act, batch).run(*_dev(*S.inputs(g, batch)))


def _skipped(call):
    return (() if call.want[0] else ("d_x0",)) + (() if call.want[1] or call.d_x1 is None else ("d_x1",))


# ---- 1. accuracy, 2. guards -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_forward_and_every_gradient_are_float32_grade(case):
    g, act, batch = case
    call, ref = _result(*case), S.reference(*case)
    fwd = max(float((o.cpu().double() - r).abs().max()) for o, r in zip(call.outs, ref.outs))
    worst, where = 0.0, None
    pairs = list(zip(call.grads, ref.grads)) + [(call.d_x0, ref.d_x0)] + ([(call.d_x1, ref.d_x1)] if g.in1 else [])
    for j, (got, want) in enumerate(pairs):
        scale = float(want.abs().max())
        assert scale > 0.0, j
        err = float((got.cpu().double().reshape(want.shape) - want).abs().max()) / scale
        if err > worst:
            worst, where = err, j
    print(f"sac_train {S.case_id(case)}: forward error {fwd:.3e}, largest normalised gradient error {worst:.3e} (tensor {where})")
    assert fwd <= S.BOUND, fwd
    assert worst <= S.BOUND, (worst, where)


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_every_output_word_is_written_and_nothing_beside(case):
    _result(*case).check_guards(S.case_id(case))


@pytest.mark.parametrize("g", [g for g in S.GROUPS if g.in1], ids=lambda g: g.name)
@pytest.mark.parametrize("keep", (0, 1), ids=("d_x0-only", "d_x1-only"))
def test_without_one_input_gradient_nothing_else_changes(g, keep):
    batch = 33
    full = _result(g, S.RELU, batch)
    call = _Call(g, S.RELU, batch, want=(keep == 0, keep == 1)).run(*_dev(*S.inputs(g, batch)))
    call.check_guards("one input gradient", skip=_skipped(call))
    kept = (call.d_x0, full.d_x0) if keep == 0 else (call.d_x1, full.d_x1)
    assert torch.equal(_ints(kept[0]), _ints(kept[1]))
    for j, (a, b) in enumerate(zip(call.outs + call.grads, full.outs + full.grads)):
        assert torch.equal(_ints(a), _ints(b)), j


# ---- 3. ReLU's exact zeros --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(g, S.RELU, 33) for g in S.GROUPS] + [(A, S.RELU, 2 * R + 5), (F, S.RELU, R + 1)], ids=S.case_id)
def test_zero_head_gradient_gives_exact_zeros(case):
    g, act, batch = case
    x0, x1, d_out = _dev(*S.inputs(g, batch))
    call = _Call(g, act, batch).run(x0, x1, [torch.zeros_like(d) for d in d_out])
    call.check_guards(S.case_id(case))
    for j, t in enumerate(call.bits()[len(call.outs):]):
        assert not bool(t.bitwise_and(0x7FFFFFFF).any()), j       # +0 or -0, nothing else


@pytest.mark.parametrize("case", [(A, 1, 1, 7), (A, 0, 0, 255), (B, 0, 1, 100), (J, 1, 0, 159), (H, 0, 2, 31)], ids=lambda c: f"{c[0].name}-{c[1]}-{c[2]}-{c[3]}")
def test_a_dead_unit_has_exactly_zero_gradients(case):
    """Unit u of hidden layer l of network c, bias -1e3: h = +0 on every row, so the mask of the saved activation stops its gradient."""
    g, c, l, u = case
    batch = 33
    x0, x1, d_out = _dev(*S.inputs(g, batch))
    dead = [[(w.clone(), b.clone()) for w, b in net] for net in S.layers_of(g)]
    dead[c][l][1][u] = -1e3
    call = _Call(g, S.RELU, batch, layers=dead).run(x0, x1, d_out)
    n = len(dead[0])
    d_w, d_b = call.grads[2 * (c * n + l)], call.grads[2 * (c * n + l) + 1]
    assert bool((d_w[u] == 0.0).all()) and float(d_b[0, u]) == 0.0
    followers = range(l + 1, n) if l == len(g.hidden) - 1 else (l + 1,)          # the layers that read hidden layer l: every head part after the last
    for k in followers:
        assert bool((call.grads[2 * (c * n + k)][:, u] == 0.0).all()), k
    assert bool((d_w != 0.0).any())                    # ... and the other units live
    cut = [[(w.clone(), b.clone()) for w, b in net] for net in dead]
    for k in followers:
        cut[c][k][0][:, u] = 0.0
    other = _Call(g, S.RELU, batch, layers=cut).run(x0, x1, d_out)
    assert torch.equal(call.d_x0, other.d_x0) and (g.in1 == 0 or torch.equal(call.d_x1, other.d_x1))


# ---- 4. flags ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(A, S.RELU, R + 1), (F, S.RELU, 2 * R + 5), (B, S.RELU, 33), (C4, S.RELU, 33)], ids=S.case_id)
def test_flags(case):
    g, act, batch = case
    K = _pkg()._capi
    x0, x1, d_out = _dev(*S.inputs(g, batch))
    full = _result(*case)
    acc = _Call(g, act, batch, flags=K.TRAIN_ACCUMULATE)
    gen = torch.Generator().manual_seed(5)
    pre = [torch.randn(t.shape, generator=gen).to(DEV) for t in acc.grads]
    for t, p in zip(acc.grads, pre):
        t.copy_(p)
    acc.run(x0, x1, d_out)
    acc.check_guards("accumulate")
    for j, (t, p, plain) in enumerate(zip(acc.grads, pre, full.grads)):
        assert torch.equal(_ints(t), _ints(p + plain)), j
    assert torch.equal(_ints(acc.d_x0), _ints(full.d_x0))                       # d_x is overwritten either way
    only = _Call(g, act, batch, flags=K.TRAIN_NO_PARAM_GRADS).run(x0, x1, d_out)
    only.check_guards("no parameter gradients", skip=("layers",))
    assert torch.equal(_ints(only.d_x0), _ints(full.d_x0))
    if g.in1:
        assert torch.equal(_ints(only.d_x1), _ints(full.d_x1))
        just = _Call(g, act, batch, flags=K.TRAIN_NO_PARAM_GRADS, want=(False, True)).run(x0, x1, d_out)
        just.check_guards("no parameter gradients, d_x1 only", skip=("layers", "d_x0"))
        assert torch.equal(_ints(just.d_x1), _ints(full.d_x1))


# ---- 5. the generalisations are addressing only -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(A, S.RELU, R + 1), (C4, S.RELU, 33), (F, S.RELU, 2 * R + 5), (H, S.RELU, 33), (A, S.TANH, R + 1)], ids=S.case_id)
def test_a_network_of_a_group_has_the_bits_it_gets_alone(case):
    g, act, batch = case
    x0, x1, d_out = _dev(*S.inputs(g, batch))
    group = _result(*case)
    one, P, n = g._replace(n_nets=1), len(g.parts), len(S.entry_dims(g))
    for c in range(g.n_nets):
        mine = d_out[c * P:(c + 1) * P]
        alone = _Call(one, act, batch, layers=[S.layers_of(g)[c]]).run(x0, x1, mine)
        for j, (a, b) in enumerate(zip(alone.outs + alone.grads, group.outs[c * P:(c + 1) * P] + group.grads[2 * c * n:2 * (c + 1) * n])):
            assert torch.equal(a, b), (c, j)
        masked = [d if c * P <= i < (c + 1) * P else torch.zeros_like(d) for i, d in enumerate(d_out)]
        whole = _Call(g, act, batch).run(x0, x1, masked)
        assert torch.equal(whole.d_x0, alone.d_x0) and (g.in1 == 0 or torch.equal(whole.d_x1, alone.d_x1)), c


@pytest.mark.parametrize("case", [(g, S.RELU, 33) for g in S.GROUPS if g.in1] + [(A, S.RELU, R + 1), (F, S.RELU, R + 1)], ids=S.case_id)
def test_two_inputs_have_the_bits_of_their_concatenation(case):
    g, act, batch = case
    x0, x1, d_out = _dev(*S.inputs(g, batch))
    two = _result(*case)
    cat = _Call(g._replace(in0=g.in0 + g.in1, in1=0), act, batch, layers=S.layers_of(g)).run(torch.cat((x0, x1), dim=1).contiguous(), None, d_out)
    for j, (a, b) in enumerate(zip(two.outs + two.grads, cat.outs + cat.grads)):
        assert torch.equal(a, b), j
    assert torch.equal(torch.cat((two.d_x0, two.d_x1), dim=1), cat.d_x0)


@pytest.mark.parametrize("case", [(g, S.RELU, 33) for g in S.GROUPS if len(g.parts) == 2] + [(B, S.RELU, R + 1), (F, S.RELU, R + 1)], ids=S.case_id)
def test_head_parts_have_the_bits_of_one_head(case):
    g, act, batch = case
    x0, x1, d_out = _dev(*S.inputs(g, batch))
    parts = _result(*case)
    joined = [net[:-2] + [(torch.cat((net[-2][0], net[-1][0])), torch.cat((net[-2][1], net[-1][1])))] for net in S.layers_of(g)]
    d_joined = [torch.cat((d_out[2 * c], d_out[2 * c + 1]), dim=1).contiguous() for c in range(g.n_nets)]
    one = _Call(g._replace(parts=(sum(g.parts),)), act, batch, layers=joined).run(x0, x1, d_joined)
    n, o0 = len(S.entry_dims(g)), g.parts[0]
    for c in range(g.n_nets):
        assert torch.equal(torch.cat((parts.outs[2 * c], parts.outs[2 * c + 1]), dim=1), one.outs[c]), c
        mine, theirs = parts.grads[2 * c * n:2 * (c + 1) * n], one.grads[2 * c * (n - 1):2 * (c + 1) * (n - 1)]
        for j, (a, b) in enumerate(zip(mine[:-4], theirs[:-2])):
            assert torch.equal(a, b), (c, j)
        assert torch.equal(torch.cat((mine[-4], mine[-2])), theirs[-2]) and torch.equal(torch.cat((mine[-3], mine[-1]), dim=1), theirs[-1]), c
        assert mine[-4].shape[0] == o0
    assert torch.equal(parts.d_x0, one.d_x0) and (g.in1 == 0 or torch.equal(parts.d_x1, one.d_x1))


@pytest.mark.parametrize("sizes", (T.NETS[0], T.NETS[7]), ids=lambda s: "-".join(map(str, s)))
def test_tanh_has_the_bits_of_the_tanh_family(sizes):
    """dn_sac_train_* with Tanh, one network, one input tensor and a head of one part against dn_mlp_train_* on the same network."""
    pkg = _pkg()
    K, lib = pkg._capi, pkg._capi.load()
    batch = R + 1
    x, d = (t.to(DEV) for t in T.inputs(sizes, batch))
    g = S.Group("T", 1, sizes[0], 0, tuple(sizes[1:-1]), (sizes[-1],))
    layers = T.layers_of(sizes)
    mine = _Call(g, S.TANH, batch, layers=[layers]).run(x, None, [d])
    mine.check_guards("tanh")
    dev = [(w.to(DEV), b.to(DEV)) for w, b in layers]
    grads = [torch.zeros_like(t) for pair in dev for t in pair]
    out, d_x = torch.zeros((batch, sizes[-1]), device=DEV), torch.zeros((batch, sizes[0]), device=DEV)
    cfg, table = T.tables(K, sizes, [(w.data_ptr(), b.data_ptr(), grads[2 * i].data_ptr(), grads[2 * i + 1].data_ptr()) for i, (w, b) in enumerate(dev)])
    need = lib.dn_mlp_train_scratch_bytes(C.byref(cfg), table, batch)
    scratch = torch.empty(need // 8, dtype=torch.float64, device=DEV)
    K.check(lib.dn_mlp_train_forward(C.byref(cfg), table, x.data_ptr(), batch, out.data_ptr(), scratch.data_ptr(), need, 0, mine.stream()))
    K.check(lib.dn_mlp_train_backward(C.byref(cfg), table, x.data_ptr(), d.data_ptr(), batch, d_x.data_ptr(), scratch.data_ptr(), need, 0, mine.stream()))
    torch.cuda.synchronize()
    assert torch.equal(mine.outs[0], out) and torch.equal(mine.d_x0, d_x)
    for j, (a, b) in enumerate(zip(mine.grads, grads)):
        assert torch.equal(a.reshape(b.shape), b), j


# ---- 6. repeatability -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(A, S.RELU, 2 * R + 5), (F, S.RELU, R + 1), (B, S.RELU, 33)], ids=S.case_id)
def test_the_same_call_twice_gives_the_same_bits(case):
    g, act, batch = case
    again = _Call(g, act, batch).run(*_dev(*S.inputs(g, batch)))
    for j, (a, b) in enumerate(zip(again.bits(), _result(*case).bits())):
        assert torch.equal(a, b), j


@pytest.mark.parametrize("g", (A, F), ids=lambda g: g.name)
def test_a_row_does_not_depend_on_the_batch(g):
    """Rows 0..32 of the inputs of batch 2 R + 5, run as a batch of 33: out, and d_x for the same head gradients, are those rows of the large run."""
    x0, x1, d_out = _dev(*S.inputs(g, 2 * R + 5))
    large = _result(g, S.RELU, 2 * R + 5)
    small = _Call(g, S.RELU, 33).run(x0[:33].contiguous(), x1[:33].contiguous(), [d[:33].contiguous() for d in d_out])
    for j, (a, b) in enumerate(zip(small.outs + [small.d_x0, small.d_x1], large.outs + [large.d_x0, large.d_x1])):
        assert torch.equal(_ints(a), _ints(b[:33])), j


@pytest.mark.parametrize("case", [(A, S.RELU, R + 1), (F, S.RELU, 33)], ids=S.case_id)
def test_a_captured_pass_replays_the_eager_bits(case):
    g, act, batch = case
    x0, x1, d_out = _dev(*S.inputs(g, batch))
    x0, x1, d_out = x0.clone(), x1.clone(), [d.clone() for d in d_out]
    eager = _result(*case).bits()
    call = _Call(g, act, batch)
    call.run(x0, x1, d_out)                            # warm: nothing is made inside the capture
    for buf, _, _, _ in call.guarded:
        buf.fill_(ms.PATTERN)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call.forward(x0, x1)
        call.backward(x0, x1, d_out)
    graph.replay()
    torch.cuda.synchronize()
    call.check_guards("replay")
    for j, (a, b) in enumerate(zip(call.bits(), eager)):
        assert torch.equal(a, b), j
    other = 33 if batch != 33 else 256                 # other selected rows of the group, cut or repeated to this batch
    y0, y1, e_out = _dev(*S.inputs(g, other))
    pick = torch.arange(batch, device=DEV) % other
    y0, y1, e_out = y0[pick].contiguous(), y1[pick].contiguous(), [e[pick].contiguous() for e in e_out]
    fresh = _Call(g, act, batch).run(y0, y1, e_out).bits()
    x0.copy_(y0)
    x1.copy_(y1)
    for d, e in zip(d_out, e_out):
        d.copy_(e)
    graph.replay()
    torch.cuda.synchronize()
    for j, (a, b) in enumerate(zip(call.bits(), fresh)):
        assert torch.equal(a, b), j


# ---- 7. the Polyak update ---------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 1025)


def _polyak_data(n):
    gen = torch.Generator().manual_seed(40 + n)
    counts = [COUNTS[i % len(COUNTS)] for i in range(n)]
    return counts, [torch.randn(c, generator=gen) for c in counts], [torch.randn(c, generator=gen) for c in counts]


def _polyak_reference(t, s, tau):
    omt = 1.0 - tau
    return (omt * t.numpy().astype(np.float64) + tau * s.numpy().astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("tau", (0.0, 0.005, 0.5, 1.0))
@pytest.mark.parametrize("n", (1, 16, 32))
def test_polyak_is_the_float64_statement_bit_for_bit(n, tau):
    pkg = _pkg()
    lib = pkg._capi.load()
    counts, source, target = _polyak_data(n)
    src = [s.to(DEV) for s in source]
    bufs, dst = zip(*[ms.guarded_out(1, c, DEV) for c in counts])
    for d, t in zip(dst, target):
        d.copy_(t.view(1, -1))
    pkg._capi.check(lib.dn_polyak_update(n, S.pointer_table([s.data_ptr() for s in src]), S.pointer_table([d.data_ptr() for d in dst]),
                                         (C.c_int64 * n)(*counts), tau, 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for i, (buf, d, s, t, c) in enumerate(zip(bufs, dst, source, target, counts)):
        ms.check_guards(buf, 1, c, f"polyak tensor {i}")
        assert np.array_equal(d.cpu().numpy().view(np.int32).ravel(), _polyak_reference(t, s, tau).view(np.int32)), i
        assert torch.equal(src[i].cpu(), s)
        if tau in (0.0, 1.0):
            assert torch.equal(_ints(d.cpu().view(-1)), _ints(t if tau == 0.0 else s)), i


def test_polyak_update_steps_and_replays():
    pkg = _pkg()
    counts, source, target = _polyak_data(16)
    src, dst = [s.to(DEV) for s in source], [t.to(DEV) for t in target]
    up = pkg.PolyakUpdate(src, dst, tau=0.005)
    up.step()                                          # eager once, then twice from a graph
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        up.step()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for i, (d, s, t) in enumerate(zip(dst, source, target)):
        want = t
        for _ in range(3):
            want = torch.from_numpy(_polyak_reference(want, s, 0.005))
        assert torch.equal(_ints(d.cpu()), _ints(want)), i
    with pytest.raises(ValueError, match="is target_params"):
        pkg.PolyakUpdate(src, src)


# ---- 8. one SAC gradient step -----------------------------------------------------------------------------------------------------------------
def _step_data(actor, critic, n):
    """n rows of a replay batch, selected as sac_train_support selects rows: the first n candidates in which every hidden pre-activation
    of the actor at obs and of every critic at (obs, actions) and at (obs, a_pi), evaluated in float64, keeps |z| >= 2 BOUND max |z|.
    Five passes over 256-wide layers have to hold at once (about one candidate in eighteen does, measured on the CPU), so 32 n
    candidates are drawn; the next-observation passes carry no gradient and ReLU is continuous, so they need no condition."""
    gen = torch.Generator().manual_seed(21)
    m = 32 * n
    d = dict(obs=torch.randn((m, 13), generator=gen), next_obs=torch.randn((m, 13), generator=gen), actions=torch.rand((m, 4), generator=gen) * 2 - 1,
             rewards=torch.randn(m, generator=gen), dones=(torch.rand(m, generator=gen) < 0.1).float(), eps=torch.randn((m, 4), generator=gen),
             eps_n=torch.randn((m, 4), generator=gen))
    a64, c64 = copy.deepcopy(actor).double().cpu(), copy.deepcopy(critic).double().cpu()
    ok = torch.ones(m, dtype=torch.bool)

    def walk(seq, x):
        nonlocal ok
        for mod in seq:
            x = mod(x)
            if isinstance(mod, torch.nn.Linear):
                ok &= (x.abs() >= 2 * S.BOUND * float(x.abs().max())).all(dim=1)
        return x

    with torch.no_grad():
        z = walk(a64.latent_pi, d["obs"].double())
        a_pi = torch.tanh(a64.mu(z) + torch.exp(torch.clamp(a64.log_std(z), -20.0, 2.0)) * d["eps"].double())
        for q in c64.q_networks:
            walk(list(q)[:-1], torch.cat((d["obs"].double(), d["actions"].double()), dim=1))
            walk(list(q)[:-1], torch.cat((d["obs"].double(), a_pi), dim=1))
    rows = torch.nonzero(ok).flatten()
    assert len(rows) >= n, len(rows)
    return {k: v[rows[:n]].contiguous() for k, v in d.items()}


def test_one_sac_gradient_step():
    """257 rows through SacTrainer.for_actor, for_critics (training and target), the loss heads, ClippedAdam x 3 and PolyakUpdate in the
    order of INTEGRATION.md 3b.  Every parameter's .grad before its Adam step against the float64 autograd of the same step on the CPU
    (the reference composition of sac_loss_support), the critics' .grad untouched by the actor-loss pass, and the targets after the
    step equal to the float64 Polyak of the stepped critics."""
    import sac_loss_support as L
    pkg = _pkg()
    n, gamma, target_entropy, tau = 257, 0.99, -4.0, 0.005
    torch.manual_seed(3)
    actor, critic = pkg.SacActor().to(DEV), pkg.SacCritic().to(DEV)
    target = copy.deepcopy(critic).requires_grad_(False)
    with torch.no_grad():
        for p in target.parameters():
            p.mul_(0.9)
    lec = torch.log(torch.full((1,), 0.3, device=DEV)).requires_grad_()
    host = _step_data(actor, critic, n)
    mb = {k: v.to(DEV) for k, v in host.items()}
    actor64, critic64, target64 = (copy.deepcopy(m).double().cpu().requires_grad_(True) for m in (actor, critic, target))
    lec64 = lec.detach().double().cpu().requires_grad_()

    actor_t, critic_t = pkg.SacTrainer.for_actor(actor, n), pkg.SacTrainer.for_critics(critic, n)
    target_t = pkg.SacTrainer.for_critics(target, n, grads=False)
    head, head_next = pkg.SacPolicyHead(n, 4, DEV), pkg.SacPolicyHead(n, 4, DEV)
    crit = pkg.SacCriticLoss(n, DEV, n_critics=2, gamma=gamma)
    act = pkg.SacActorLoss(n, DEV, n_critics=2, target_entropy=target_entropy)
    adam = dict(lr=3e-4, eps=1e-8, max_grad_norm=None, zero_grads=False)
    opt_actor, opt_critic, opt_coef = pkg.ClippedAdam(actor_t.params, **adam), pkg.ClippedAdam(critic_t.params, **adam), pkg.ClippedAdam([lec], **adam)
    polyak = pkg.PolyakUpdate(critic_t.params, list(target.parameters()), tau)
    assert all(p.grad is None for p in target.parameters()) and all(p.grad is g for p, g in zip(critic_t.params, critic_t.grads))

    with torch.no_grad():
        a_next, next_log_prob = head_next(*actor_t(mb["next_obs"]), mb["eps_n"])
        next_q = [q.clone() for q in target_t(mb["next_obs"], a_next)]
    assert all(not q.requires_grad for q in next_q) and all(p.grad is None for p in target.parameters())
    a_pi, log_prob = head(*actor_t(mb["obs"]), mb["eps"])
    critic_loss = crit(list(critic_t(mb["obs"], mb["actions"])), next_q, next_log_prob, mb, lec)
    critic_loss.backward()
    torch.cuda.synchronize()
    got_critic = [g.clone() for g in critic_t.grads]
    opt_critic.step()
    stepped = [p.detach().clone() for p in critic_t.params]
    actor_loss, ent_coef_loss = act(log_prob, list(critic_t(mb["obs"], a_pi, param_grads=False)), lec)
    (actor_loss + ent_coef_loss).backward()
    torch.cuda.synchronize()
    for j, (g, before) in enumerate(zip(critic_t.grads, got_critic)):
        assert torch.equal(_ints(g), _ints(before)), j                         # the actor-loss pass left the critics' .grad alone
    got_actor = [g.clone() for g in actor_t.grads]
    opt_actor.step()
    opt_coef.step()
    before_polyak = [p.detach().clone() for p in target.parameters()]
    polyak.step()
    torch.cuda.synchronize()

    # the same step in float64 on the CPU, the critic step taken from the device so that the actor loss sees the stepped critics
    b64 = {k: v.double() for k, v in host.items()}
    z = actor64.latent_pi(b64["obs"])
    a64, lp64, _ = L.squash_composition(actor64.mu(z), actor64.log_std(z), b64["eps"])
    with torch.no_grad():
        zn = actor64.latent_pi(b64["next_obs"])
        an64, lpn64, _ = L.squash_composition(actor64.mu(zn), actor64.log_std(zn), b64["eps_n"])
        nq = torch.min(torch.stack(target64(b64["next_obs"], an64)), dim=0).values
        y = b64["rewards"] + (1.0 - b64["dones"]) * gamma * (nq - torch.exp(lec64.detach()) * lpn64)
    loss_c = 0.5 * sum(((q - y) ** 2).mean() for q in critic64(b64["obs"], b64["actions"]))
    want_critic = torch.autograd.grad(loss_c, list(critic64.parameters()))
    with torch.no_grad():
        for p, s in zip(critic64.parameters(), stepped):
            p.copy_(s.double().cpu())
    loss_a = (torch.exp(lec64.detach()) * lp64 - torch.min(torch.stack(critic64(b64["obs"], a64)), dim=0).values).mean()
    want_actor = torch.autograd.grad(loss_a, list(actor_t_order(actor64)))
    for name, got, want in (("critic", got_critic, want_critic), ("actor", got_actor, want_actor)):
        for j, (g, w) in enumerate(zip(got, want)):
            err = float((g.double().cpu() - w).abs().max()) / float(w.abs().max())
            print(f"sac_train SAC step {name}[{j}]: {err:.3e}")
            assert err <= S.BOUND, (name, j, err)
    for j, (t, old, s) in enumerate(zip(target.parameters(), before_polyak, stepped)):
        want = _polyak_reference(old.cpu().reshape(-1), s.cpu().reshape(-1), tau)
        assert np.array_equal(t.detach().cpu().numpy().view(np.int32).ravel(), want.view(np.int32)), j


def actor_t_order(actor):
    """The actor's parameters in SacTrainer.for_actor's order: latent_pi, mu, log_std."""
    return [p for m in [x for x in actor.latent_pi if isinstance(x, torch.nn.Linear)] + [actor.mu, actor.log_std] for p in (m.weight, m.bias)]
