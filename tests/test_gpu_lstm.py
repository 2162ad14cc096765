"""The LSTM layer (include/dronenav.h dn_lstm_forward / dn_lstm_backward, csrc/dn_lstm.hip, lstm_train.py) on the HIP path, against the
same float32 parameters and inputs evaluated in float64 through torch.nn.LSTM(...).double() and autograd on the CPU.

 1. forward accuracy: teacher-forced (the float64 cell fed the kernel's own h_seq[t - 1], c_seq[t - 1]) and free-running against the
    float64 sequence, max |h_t - ref| and max |c_t - ref| <= 1e-4, the project's float32-grade bar;
 2. gradient accuracy: every gradient tensor and d_x against float64 autograd over the whole sequence, max |g - g64| <= 1e-4 max |g64|
    with max |g64| > 0; where T = 1 and every row's episode starts, d_w_hh's reference is identically zero and the device tensor must
    be exact zeros;
 3. one call of T steps gives h_seq, c_seq, h_T, c_T bit-equal to T calls of one step that chain the state in place;
 4. rows 0..32 of every per-row output at B = 33 are those rows at B = 129;
 5. resets: a row whose episode starts at t has, from t on, the bits of a fresh sequence that starts at t with zero state, and no
    gradient reaches its x before t;
 6. guards: every output has every word written and nothing written outside it; with d_x = NULL nothing else changes;
 7. d_hseq = 0 gives gradients and d_x that are exactly zero, over sentinel-filled tensors;
 8. flags: ACCUMULATE over a random pre-fill p is bit-equal to p + g; with NO_PARAM_GRADS the gradient tensors keep their sentinel bits
    and d_x keeps the bits of the full run;
 9. d_b_ih and d_b_hh are bit-equal;
10. the same call twice gives equal bits; a captured forward + backward replays the eager bits, and again after the inputs are
    overwritten in place; a captured LstmStepper.step replays the eager bits;
11. LstmTrainer -> MlpTrainer -> a weighted sum -> backward(): the gradients of both networks against the float64 composition, then one
    ClippedAdam.step().

The device results of a case are computed once and shared, the references once per case (lstm_support).  Largest errors seen on an
MI355X are in profiles/time_lstm.txt and DESIGN.md 4.2.4."""
import ctypes as C
import functools

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import lstm_support as L  # noqa: E402
import mlp_support as ms  # noqa: E402
from gpu_support import DEV  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402

GRAD_NAMES = ("d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class _Call:
    """One layer on the device with every output between guard rows: forward(), backward(); the tensors are views of the guarded
    buffers.  state: (h, c) device tensors that are h0, c0 AND h_T, c_T -- the in-place step."""

    def __init__(self, layer, shape, *, flags=0, want_dx=True, params=None, state=None):
        self.pkg = _pkg()
        self.K, self.lib = self.pkg._capi, self.pkg._capi.load()
        (self.I, self.H), (self.T, self.B) = layer, shape
        self.layer, self.shape, self.want_dx, self.state = layer, shape, want_dx, state
        self.params = [p.to(DEV) for p in (params or L.params_of(layer))]
        rows, I, H = self.T * self.B, self.I, self.H
        self.bufs = {}
        for name, n, width in (("h_seq", rows, H), ("c_seq", rows, H), ("h_T", self.B, H), ("c_T", self.B, H), ("d_x", rows, I),
                               ("d_w_ih", 4 * H, I), ("d_w_hh", 4 * H, H), ("d_b_ih", 1, 4 * H), ("d_b_hh", 1, 4 * H)):
            buf, view = ms.guarded_out(n, width, DEV)
            self.bufs[name] = (buf, n, width)
            setattr(self, name, view)
        self.grads = [getattr(self, n) for n in GRAD_NAMES]
        self.cfg, self.table = L.tables(self.K, layer, [p.data_ptr() for p in self.params] + [g.data_ptr() for g in self.grads], flags)
        need = self.lib.dn_lstm_scratch_bytes(C.byref(self.cfg), self.T, self.B)
        assert need == L.scratch_bytes(layer, shape)
        self.scratch = torch.empty(need // 8, dtype=torch.float64, device=DEV)

    def seq(self, t, width):
        return t.view(self.T, self.B, width)

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def forward(self, x, starts, h0, c0, scratch_bytes=None):
        h_T, c_T = (self.state[0], self.state[1]) if self.state else (self.h_T, self.c_T)
        self.K.check(self.lib.dn_lstm_forward(C.byref(self.cfg), C.byref(self.table), x.data_ptr(), starts.data_ptr() if starts is not None else None,
                                              h0.data_ptr(), c0.data_ptr(), self.T, self.B, self.h_seq.data_ptr(), self.c_seq.data_ptr(),
                                              h_T.data_ptr(), c_T.data_ptr(), self.scratch.data_ptr(),
                                              self.scratch.numel() * 8 if scratch_bytes is None else scratch_bytes, 0, self.stream()))

    def backward(self, x, starts, h0, c0, d_hseq):
        self.K.check(self.lib.dn_lstm_backward(C.byref(self.cfg), C.byref(self.table), x.data_ptr(), starts.data_ptr() if starts is not None else None,
                                               h0.data_ptr(), self.h_seq.data_ptr(), self.c_seq.data_ptr(), c0.data_ptr(), d_hseq.data_ptr(),
                                               self.T, self.B, self.d_x.data_ptr() if self.want_dx else None, self.scratch.data_ptr(),
                                               self.scratch.numel() * 8, 0, self.stream()))

    def run(self, x, starts, h0, c0, d_hseq):
        self.forward(x, starts, h0, c0)
        self.backward(x, starts, h0, c0, d_hseq)
        torch.cuda.synchronize()
        return self

    def check_guards(self, tag, names=None):
        for name in names or self.bufs:
            buf, n, width = self.bufs[name]
            ms.check_guards(buf, n, width, f"{tag}: {name}")

    def untouched(self, name):
        return bool((self.bufs[name][0] == ms.PATTERN).all())

    def outputs(self):
        return [self.h_seq, self.c_seq, self.h_T, self.c_T, self.d_x] + self.grads


FORWARD = ("h_seq", "c_seq", "h_T", "c_T")


def _device_inputs(layer, shape, pattern):
    """x, starts, h0, c0, d_hseq on the device."""
    x, d, h0, c0 = L.inputs(layer, shape)
    s = L.starts_of(shape, pattern)
    return x.to(DEV), (s.to(DEV) if s is not None else None), h0.to(DEV), c0.to(DEV), d.to(DEV)


@functools.lru_cache(maxsize=None)
def _result(case):
    """The plain call of a case, run once."""
    layer, shape, pattern = case
    return _Call(layer, shape).run(*_device_inputs(layer, shape, pattern))


WORST = {"teacher": 0.0, "free": 0.0, "grad": 0.0}


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_the_forward_is_float32_grade(case):
    layer, shape, pattern = case
    call = _result(case)
    x, _, h0, c0 = L.inputs(layer, shape)
    h_dev, c_dev = call.seq(call.h_seq, call.H).cpu(), call.seq(call.c_seq, call.H).cpu()
    h_tf, c_tf = L.teacher_forced(L.params_of(layer), x, L.starts_of(shape, pattern), h0, c0, h_dev, c_dev)
    h64, c64, _, _ = L.reference(case)
    teacher = max(float((h_dev.double() - h_tf).abs().max()), float((c_dev.double() - c_tf).abs().max()))
    free = max(float((h_dev.double() - h64).abs().max()), float((c_dev.double() - c64).abs().max()))
    WORST["teacher"], WORST["free"] = max(WORST["teacher"], teacher), max(WORST["free"], free)
    print(f"lstm {L.case_id(case)}: teacher-forced error {teacher:.3e}, free-running error {free:.3e}; largest so far {WORST['teacher']:.3e}, "
          f"{WORST['free']:.3e}")
    assert teacher <= L.BOUND, teacher
    assert free <= L.BOUND, free
    assert _same(call.h_T, h_dev[-1].to(DEV)) and _same(call.c_T, c_dev[-1].to(DEV))           # the last step's state


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_every_gradient_is_float32_grade(case):
    call = _result(case)
    _, _, g64, dx64 = L.reference(case)
    worst, where = 0.0, None
    for name, g, ref in zip(GRAD_NAMES + ("d_x",), call.grads + [call.d_x], g64 + [dx64]):
        scale = float(ref.abs().max())
        if name == "d_w_hh" and L.all_start(case[1], case[2]):         # no row of hprev survives: the reference is identically zero ...
            assert scale == 0.0
            assert not bool(g.view(torch.int32).bitwise_and(0x7FFFFFFF).any()), name           # ... and the device writes +0 or -0
            continue
        assert scale > 0.0, name
        err = float((g.cpu().double().reshape(ref.shape) - ref).abs().max()) / scale
        if err > worst:
            worst, where = err, name
    WORST["grad"] = max(WORST["grad"], worst)
    print(f"lstm {L.case_id(case)}: largest normalised gradient error {worst:.3e} ({where}); largest so far {WORST['grad']:.3e}")
    assert worst <= L.BOUND, (worst, where)


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_every_output_word_is_written_and_nothing_beside_and_the_bias_gradients_agree(case):
    call = _result(case)
    call.check_guards(L.case_id(case))
    assert _same(call.d_b_ih, call.d_b_hh)


@pytest.mark.parametrize("pair", [p for p in L.PAIRS if p[1][0] > 1], ids=lambda p: L.case_id(p + ("random",)))
def test_a_sequence_is_its_steps_chained_in_place(pair):
    layer, shape = pair
    whole = _result((layer, shape, "random"))
    x, starts, h0, c0, _ = _device_inputs(layer, shape, "random")
    h, c = h0.clone(), c0.clone()                      # the resident state: h0 and h_T, c0 and c_T of every step
    step = _Call(layer, (1, shape[1]), state=(h, c))
    gates = L.gates_bytes(layer, (1, shape[1]))        # the rollout step asks for the gates alone
    for t in range(shape[0]):
        for name in ("h_seq", "c_seq"):
            step.bufs[name][0].fill_(ms.PATTERN)
        step.forward(x[t], starts[t], h, c, scratch_bytes=gates)
        torch.cuda.synchronize()
        step.check_guards(f"step {t}", ("h_seq", "c_seq"))
        assert _same(step.h_seq, whole.seq(whole.h_seq, whole.H)[t]) and _same(step.c_seq, whole.seq(whole.c_seq, whole.H)[t]), t
        assert _same(h, step.h_seq) and _same(c, step.c_seq), t
    assert _same(h, whole.h_T) and _same(c, whole.c_T)
    assert step.untouched("h_T") and step.untouched("c_T")


@pytest.mark.parametrize("layer", L.LAYERS[:2], ids=lambda l: f"{l[0]}-{l[1]}")
@pytest.mark.parametrize("pattern", ("none", "random"))
def test_a_row_does_not_depend_on_the_other_rows(layer, pattern):
    shape = (5, 129)
    large = _result((layer, shape, pattern))
    x, starts, h0, c0, d = _device_inputs(layer, shape, pattern)
    cut = lambda t: t[:, :33].contiguous() if t is not None else None      # noqa: E731
    small = _Call(layer, (5, 33)).run(cut(x), cut(starts), h0[:33].contiguous(), c0[:33].contiguous(), cut(d))
    small.check_guards("B = 33")
    for name, width in (("h_seq", large.H), ("c_seq", large.H), ("d_x", large.I)):
        assert _same(small.seq(getattr(small, name), width), large.seq(getattr(large, name), width)[:, :33]), name
    assert _same(small.h_T, large.h_T[:33]) and _same(small.c_T, large.c_T[:33])


@pytest.mark.parametrize("layer", L.LAYERS[:3], ids=lambda l: f"{l[0]}-{l[1]}")
def test_an_episode_start_cuts_the_sequence(layer):
    shape, t0 = (5, 129), 2
    x, _, h0, c0, d = _device_inputs(layer, shape, "none")
    starts = torch.zeros(shape, dtype=torch.uint8)
    starts[t0, 0::2] = 1                               # the even rows start an episode at t0
    even, odd = torch.arange(0, shape[1], 2, device=DEV), torch.arange(1, shape[1], 2, device=DEV)
    d = d.clone()
    d[:t0, 0::2] = 0.0                                 # ... and receive a gradient from t0 on only
    cut = _Call(layer, shape).run(x, starts.to(DEV), h0, c0, d)
    cut.check_guards("with starts")
    zeros = torch.zeros_like(h0)
    fresh = _Call(layer, (shape[0] - t0, shape[1]))
    fresh.forward(x[t0:].contiguous(), None, zeros, zeros)
    torch.cuda.synchronize()
    for name in ("h_seq", "c_seq"):
        a, b = cut.seq(getattr(cut, name), cut.H)[t0:], fresh.seq(getattr(fresh, name), fresh.H)
        assert _same(a[:, even], b[:, even]), name
        assert not _same(a[:, odd], b[:, odd]), name                 # the odd rows carry their state across t0
    assert _same(cut.h_T[even], fresh.h_T[even]) and _same(cut.c_T[even], fresh.c_T[even])
    d_x = cut.seq(cut.d_x, cut.I)
    assert not bool(d_x[:t0, even].view(torch.int32).bitwise_and(0x7FFFFFFF).any())        # +0 or -0, nothing else
    assert bool((d_x[:t0, odd] != 0).any()) and bool((d_x[t0:, even] != 0).any())


@pytest.mark.parametrize("pair", [(l, (5, 129)) for l in L.LAYERS], ids=lambda p: L.case_id(p + ("random",)))
def test_without_d_x_nothing_else_changes(pair):
    layer, shape = pair
    full = _result((layer, shape, "random"))
    call = _Call(layer, shape, want_dx=False).run(*_device_inputs(layer, shape, "random"))
    call.check_guards("d_x = NULL", [n for n in call.bufs if n != "d_x"])
    assert call.untouched("d_x")
    for j, (a, b) in enumerate(zip(call.outputs(), full.outputs())):
        assert j == 4 or _same(a, b), j


@pytest.mark.parametrize("pair", [(l, (5, 205)) for l in L.LAYERS] + [(L.LAYERS[1], (1, 1)), (L.LAYERS[0], (3, 683))],
                         ids=lambda p: L.case_id(p + ("random",)))
def test_zero_gradient_in_gives_exact_zeros(pair):
    layer, shape = pair
    x, starts, h0, c0, d = _device_inputs(layer, shape, "random")
    call = _Call(layer, shape).run(x, starts, h0, c0, torch.zeros_like(d))
    call.check_guards(L.case_id(pair + ("random",)))
    for name, g in zip(GRAD_NAMES + ("d_x",), call.grads + [call.d_x]):
        assert not bool(g.view(torch.int32).bitwise_and(0x7FFFFFFF).any()), name        # +0 or -0, nothing else


@pytest.mark.parametrize("case", [(L.LAYERS[0], (5, 205), "random"), (L.LAYERS[1], (3, 683), "step"), (L.LAYERS[3], (5, 129), "none"),
                                  (L.LAYERS[1], (1, 1), "none")], ids=L.case_id)
def test_flags(case):
    layer, shape, pattern = case
    K = _pkg()._capi
    args = _device_inputs(layer, shape, pattern)
    full = _result(case)
    acc = _Call(layer, shape, flags=K.TRAIN_ACCUMULATE)
    gen = torch.Generator().manual_seed(5)
    pre = [torch.randn(g.shape, generator=gen).to(DEV) for g in acc.grads]
    for g, p in zip(acc.grads, pre):
        g.copy_(p)
    acc.run(*args)
    acc.check_guards("accumulate")
    for name, g, p, plain in zip(GRAD_NAMES, acc.grads, pre, full.grads):
        assert _same(g, p + plain), name
    assert _same(acc.d_x, full.d_x)                    # d_x is overwritten either way
    only = _Call(layer, shape, flags=K.TRAIN_NO_PARAM_GRADS).run(*args)
    only.check_guards("no parameter gradients", FORWARD + ("d_x",))
    assert all(only.untouched(n) for n in GRAD_NAMES)
    assert _same(only.d_x, full.d_x)


@pytest.mark.parametrize("case", [(L.LAYERS[0], (3, 683), "random"), (L.LAYERS[4], (5, 205), "step"), (L.LAYERS[1], (2, 31), "first")], ids=L.case_id)
def test_the_same_call_twice_gives_the_same_bits(case):
    layer, shape, pattern = case
    again = _Call(layer, shape).run(*_device_inputs(layer, shape, pattern))
    for j, (a, b) in enumerate(zip(again.outputs(), _result(case).outputs())):
        assert _same(a, b), j


@pytest.mark.parametrize("case", [(L.LAYERS[0], (5, 205), "random"), (L.LAYERS[2], (5, 129), "step")], ids=L.case_id)
def test_a_captured_pass_replays_the_eager_bits(case):
    layer, shape, pattern = case
    x, starts, h0, c0, d = (t.clone() for t in _device_inputs(layer, shape, pattern))
    eager = [_bits(t).clone() for t in _result(case).outputs()]
    call = _Call(layer, shape)
    call.run(x, starts, h0, c0, d)                     # warm: nothing is made inside the capture
    for buf, _, _ in call.bufs.values():
        buf.fill_(ms.PATTERN)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call.forward(x, starts, h0, c0)
        call.backward(x, starts, h0, c0, d)
    graph.replay()
    torch.cuda.synchronize()
    call.check_guards("replay")
    for j, (a, b) in enumerate(zip(call.outputs(), eager)):
        assert torch.equal(_bits(a), b), j
    gen = torch.Generator().manual_seed(9)
    new = [torch.randn(x.shape, generator=gen), (torch.rand(starts.shape, generator=gen) < 0.3).to(torch.uint8), 0.5 * torch.randn(h0.shape, generator=gen),
           0.5 * torch.randn(c0.shape, generator=gen), torch.randn(d.shape, generator=gen) / (shape[0] * shape[1])]
    new = [t.to(DEV) for t in new]
    fresh = [_bits(t).clone() for t in _Call(layer, shape).run(*new).outputs()]
    for old, t in zip((x, starts, h0, c0, d), new):
        old.copy_(t)
    graph.replay()
    torch.cuda.synchronize()
    for j, (a, b) in enumerate(zip(call.outputs(), fresh)):
        assert torch.equal(_bits(a), b), j


def _module(layer):
    lstm = torch.nn.LSTM(*layer)
    with torch.no_grad():
        for n, p in zip(("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"), L.params_of(layer)):
            getattr(lstm, n).copy_(p)
    return lstm.to(DEV)


def test_a_captured_stepper_replays_the_eager_bits():
    pkg = _pkg()
    layer, n, steps = L.LAYERS[0], 129, 4
    lstm = _module(layer)
    gen = torch.Generator().manual_seed(21)
    xs = torch.randn((steps, n, layer[0]), generator=gen).to(DEV)
    starts = (torch.rand((steps, n), generator=gen) < 0.2).to(torch.uint8).to(DEV)
    h0, c0 = (0.5 * torch.randn((n, layer[1]), generator=gen)).to(DEV), (0.5 * torch.randn((n, layer[1]), generator=gen)).to(DEV)
    # the steps are the sequence: the stepper against one dn_lstm_forward over the four steps
    whole = _Call(layer, (steps, n))
    whole.forward(xs, starts, h0, c0)
    torch.cuda.synchronize()
    eager = pkg.LstmStepper(lstm, n, DEV)
    assert not bool(eager.h.any()) and not bool(eager.c.any())
    eager.set_state(h0, c0)
    for t in range(steps):
        h = eager.step(xs[t], starts[t])
        assert h is eager.h
        torch.cuda.synchronize()
        assert _same(h, whole.seq(whole.h_seq, whole.H)[t]), t
    assert _same(eager.c, whole.c_T) and all(_same(a, b) for a, b in zip(eager.state(), (eager.h, eager.c)))
    captured = pkg.LstmStepper(lstm, n, DEV)
    captured.set_state(h0, c0)
    x, s = xs[0].clone(), starts[0].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.step(x, s)
    for t in range(steps):
        x.copy_(xs[t])
        s.copy_(starts[t])
        graph.replay()
    torch.cuda.synchronize()
    assert _same(captured.h, eager.h) and _same(captured.c, eager.c)
    with pytest.raises(ValueError, match="x must be a dense torch.float32"):
        eager.step(xs[0][:5])


def test_the_trainer_feeds_an_mlp_trainer_and_an_optimiser_step():
    """LstmTrainer (13 -> 64, T = 4, B = 65) -> MlpTrainer (64-32-4) -> a weighted sum -> backward(): the MlpTrainer's d_x flows into the
    one dn_lstm_backward call.  All gradients of both networks against the float64 torch composition, then one ClippedAdam.step()."""
    pkg = _pkg()
    layer, T, B = (13, 64), 4, 65
    nn = torch.nn
    lstm = _module(layer)
    torch.manual_seed(4)
    linears = [nn.Linear(64, 32).to(DEV), nn.Linear(32, 4).to(DEV)]
    rnn, mlp = pkg.LstmTrainer(lstm, T, B), pkg.MlpTrainer(linears, T * B)
    statics = [(p, g) for t in (rnn, mlp) for p, g in zip(t.params, t.grads)]
    assert all(p.grad is g for p, g in statics)
    gen = torch.Generator().manual_seed(12)
    x = torch.randn((T, B, 13), generator=gen).to(DEV)
    starts = (torch.rand((T, B), generator=gen) < 0.2).to(torch.uint8).to(DEV)
    h0, c0 = (0.5 * torch.randn((B, 64), generator=gen)).to(DEV), (0.5 * torch.randn((B, 64), generator=gen)).to(DEV)
    weight = (torch.randn((T * B, 4), generator=gen) / (T * B)).to(DEV)

    stale = rnn(x, starts, h0, c0)
    twice = rnn(x, starts, h0, c0)
    with pytest.raises(RuntimeError, match="backward of call"):
        stale.sum().backward()
    twice.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="a second backward of call"):
        twice.sum().backward()
    # the trainer's own last state as the next h0 / c0: the forward would overwrite what the backward reads again
    for bad in (dict(h0=rnn.h_T[:B]), dict(c0=rnn.c_T[:B]), dict(h0=rnn.c_T[:B]), dict(c0=rnn.h_seq[-1])):
        (name,) = bad
        with pytest.raises(ValueError, match=f"{name} overlaps this trainer's static"):
            rnn(x, starts, **dict(dict(h0=h0, c0=c0), **bad))
    chained = rnn(x, starts, rnn.h_T[:B].clone(), rnn.c_T[:B].clone())             # copies are taken
    assert tuple(chained.shape) == (T, B, 64)
    h_seq = rnn(x, starts, h0, c0)
    assert tuple(h_seq.shape) == (T, B, 64) and h_seq.is_contiguous() and h_seq.data_ptr() == rnn.h_seq.data_ptr()
    out = mlp(h_seq.reshape(T * B, 64))
    (out * weight).sum().backward()
    torch.cuda.synchronize()
    assert all(p.grad is g for p, g in statics)

    ref = L.lstm64([p.detach().cpu() for p in rnn.params])
    hs, _ = L.sequence64(ref, x.cpu().double(), starts.cpu(), h0.cpu().double(), c0.cpu().double())
    lin64 = [(m.weight.detach().cpu().double().requires_grad_(), m.bias.detach().cpu().double().requires_grad_()) for m in linears]
    (ms.f64(lin64, hs.reshape(T * B, 64)) * weight.cpu().double()).sum().backward()
    g64 = [getattr(ref, n).grad for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")] + [t.grad for pair in lin64 for t in pair]
    assert float((h_seq.detach().cpu().double() - hs.detach()).abs().max()) <= L.BOUND
    for j, ((p, g), want) in enumerate(zip(statics, g64)):
        scale = float(want.abs().max())
        assert scale > 0.0, j
        err = float((g.cpu().double() - want).abs().max()) / scale
        print(f"lstm composition gradient {j}: {err:.3e}")
        assert err <= L.BOUND, (j, err)

    before = [p.detach().clone() for p, _ in statics]
    opt = pkg.ClippedAdam([p for p, _ in statics], zero_grads=False)
    opt.step()
    torch.cuda.synchronize()
    assert all(p.grad is g for p, g in statics)
    for j, ((p, _), old) in enumerate(zip(statics, before)):
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), old), j
