"""The training pass of the Tanh networks (include/dronenav.h dn_mlp_train_forward / dn_mlp_train_backward, csrc/dn_mlp_train.hip,
mlp_train.py) on the HIP path, against the same float32 parameters and inputs evaluated in float64 through torch autograd on the CPU.

 1. accuracy: max |out - out64| <= 1e-4, and per gradient tensor, d_x included, max |g - g64| <= 1e-4 max |g64| -- the project's
    float32-grade bar (dn_mlp_forward grade 1), for every network and batch of mlp_train_support.CASES;
 2. guards: out, d_x and every gradient tensor have every word written and nothing written outside them; with d_x = NULL nothing else
    changes;
 3. d_out = 0 gives gradients and d_x that are exactly zero, over sentinel-filled tensors;
 4. flags: ACCUMULATE over a random pre-fill p is bit-equal to p + g; with NO_PARAM_GRADS the gradient tensors keep their sentinel bits
    and d_x keeps the bits of the full run;
 5. the same call twice gives equal bits; rows 0..32 of out at batch 33 are those rows at batch 2 R + 5; a captured forward + backward
    replays the eager bits, and again after the inputs are overwritten in place;
 6. one learner step of 257 rows through MlpTrainer + PpoLoss + loss.backward() + ClippedAdam.step().

The device results of a case are computed once and shared by tests 1 and 2, the references once per case (mlp_train_support).
Largest errors seen on an MI355X are in profiles/time_mlp_train.txt and DESIGN.md 4.2.2."""
import ctypes as C
import functools

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import mlp_support as ms  # noqa: E402
import mlp_train_support as T  # noqa: E402
from gpu_support import DEV  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402

R = T.R


class _Call:
    """One network on the device with every output between guard rows: forward(), backward(); the tensors are views of the guarded
    buffers.  prefill: what the gradient tensors hold before the call (default: the sentinel)."""

    def __init__(self, sizes, batch, *, flags=0, want_dx=True, layers=None):
        self.pkg = _pkg()
        self.K, self.lib = self.pkg._capi, self.pkg._capi.load()
        self.sizes, self.batch, self.want_dx = sizes, batch, want_dx
        self.layers = [(w.to(DEV), b.to(DEV)) for w, b in (layers or T.layers_of(sizes))]
        self.out_buf, self.out = ms.guarded_out(batch, sizes[-1], DEV)
        self.dx_buf, self.d_x = ms.guarded_out(batch, sizes[0], DEV)
        self.grad_bufs, self.grads = [], []
        for w, b in self.layers:
            for n, width in ((w.shape[0], w.shape[1]), (1, b.shape[0])):
                buf, view = ms.guarded_out(n, width, DEV)
                self.grad_bufs.append((buf, n, width))
                self.grads.append(view)
        ptrs = [(w.data_ptr(), b.data_ptr(), self.grads[2 * i].data_ptr(), self.grads[2 * i + 1].data_ptr()) for i, (w, b) in enumerate(self.layers)]
        self.cfg, self.table = T.tables(self.K, sizes, ptrs, flags)
        need = self.lib.dn_mlp_train_scratch_bytes(C.byref(self.cfg), self.table, batch)
        assert need == T.scratch_bytes(sizes, batch)
        self.scratch = torch.empty(need // 8, dtype=torch.float64, device=DEV)

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def forward(self, x):
        self.K.check(self.lib.dn_mlp_train_forward(C.byref(self.cfg), self.table, x.data_ptr(), self.batch, self.out.data_ptr(),
                                                   self.scratch.data_ptr(), self.scratch.numel() * 8, 0, self.stream()))

    def backward(self, x, d_out):
        self.K.check(self.lib.dn_mlp_train_backward(C.byref(self.cfg), self.table, x.data_ptr(), d_out.data_ptr(), self.batch,
                                                    self.d_x.data_ptr() if self.want_dx else None, self.scratch.data_ptr(),
                                                    self.scratch.numel() * 8, 0, self.stream()))

    def run(self, x, d_out):
        self.forward(x)
        self.backward(x, d_out)
        torch.cuda.synchronize()
        return self

    def check_guards(self, tag, grads=True, d_x=True):
        ms.check_guards(self.out_buf, self.batch, self.sizes[-1], f"{tag}: out")
        if d_x:
            ms.check_guards(self.dx_buf, self.batch, self.sizes[0], f"{tag}: d_x")
        if grads:
            for j, (buf, n, width) in enumerate(self.grad_bufs):
                ms.check_guards(buf, n, width, f"{tag}: gradient tensor {j}")

    def untouched(self, buf):
        return bool((buf == ms.PATTERN).all())


def _device_inputs(sizes, batch):
    x, d = T.inputs(sizes, batch)
    return x.to(DEV), d.to(DEV)


@functools.lru_cache(maxsize=None)
def _result(sizes, batch):
    """The plain call of a case, run once."""
    return _Call(sizes, batch).run(*_device_inputs(sizes, batch))


def _errors(call, sizes, batch):
    """(forward error, the largest normalised gradient error, its tensor) against the float64 reference."""
    out64, g64, dx64 = T.reference(sizes, batch)
    fwd = float((call.out.cpu().double() - out64).abs().max())
    worst, where = 0.0, None
    for j, (g, ref) in enumerate(zip(call.grads + [call.d_x], g64 + [dx64])):
        scale = float(ref.abs().max())
        assert scale > 0.0, j
        err = float((g.cpu().double() - ref).abs().max()) / scale
        if err > worst:
            worst, where = err, j
    return fwd, worst, where


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_forward_and_every_gradient_are_float32_grade(case):
    sizes, batch = case
    fwd, grad, where = _errors(_result(sizes, batch), sizes, batch)
    print(f"mlp_train {T.case_id(case)}: forward error {fwd:.3e}, largest normalised gradient error {grad:.3e} (tensor {where})")
    assert fwd <= T.BOUND, fwd
    assert grad <= T.BOUND, (grad, where)


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_every_output_word_is_written_and_nothing_beside(case):
    _result(*case).check_guards(T.case_id(case))


@pytest.mark.parametrize("sizes", T.NETS, ids=lambda s: "-".join(map(str, s)))
def test_without_d_x_nothing_else_changes(sizes):
    batch = 33
    full = _result(sizes, batch)
    call = _Call(sizes, batch, want_dx=False).run(*_device_inputs(sizes, batch))
    call.check_guards("d_x = NULL", d_x=False)
    assert call.untouched(call.dx_buf)
    assert torch.equal(call.out, full.out)
    for j, (a, b) in enumerate(zip(call.grads, full.grads)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), j


@pytest.mark.parametrize("case", [(n, 33) for n in T.NETS] + [(T.NETS[0], 2 * R + 5), (T.NETS[7], R + 1)], ids=T.case_id)
def test_zero_head_gradient_gives_exact_zeros(case):
    sizes, batch = case
    x, d = _device_inputs(sizes, batch)
    call = _Call(sizes, batch).run(x, torch.zeros_like(d))
    call.check_guards(T.case_id(case))
    for j, g in enumerate(call.grads + [call.d_x]):
        assert not bool(g.view(torch.int32).bitwise_and(0x7FFFFFFF).any()), j       # +0 or -0, nothing else


@pytest.mark.parametrize("case", [(T.NETS[0], R + 1), (T.NETS[7], 2 * R + 5), (T.NETS[5], 33), (T.NETS[4], 65)], ids=T.case_id)
def test_flags(case):
    sizes, batch = case
    K = _pkg()._capi
    x, d = _device_inputs(sizes, batch)
    full = _result(sizes, batch)
    acc = _Call(sizes, batch, flags=K.TRAIN_ACCUMULATE)
    gen = torch.Generator().manual_seed(5)
    pre = [torch.randn(g.shape, generator=gen).to(DEV) for g in acc.grads]
    for g, p in zip(acc.grads, pre):
        g.copy_(p)
    acc.run(x, d)
    acc.check_guards("accumulate")
    for j, (g, p, plain) in enumerate(zip(acc.grads, pre, full.grads)):
        assert torch.equal(g.view(torch.int32), (p + plain).view(torch.int32)), j
    assert torch.equal(acc.d_x.view(torch.int32), full.d_x.view(torch.int32))        # d_x is overwritten either way
    only = _Call(sizes, batch, flags=K.TRAIN_NO_PARAM_GRADS).run(x, d)
    only.check_guards("no parameter gradients", grads=False)
    assert all(only.untouched(buf) for buf, _, _ in only.grad_bufs)
    assert torch.equal(only.d_x.view(torch.int32), full.d_x.view(torch.int32))


def _bits(call):
    return [t.view(torch.int32).clone() for t in [call.out, call.d_x] + call.grads]


@pytest.mark.parametrize("case", [(T.NETS[0], 2 * R + 5), (T.NETS[7], R + 1), (T.NETS[2], 33)], ids=T.case_id)
def test_the_same_call_twice_gives_the_same_bits(case):
    sizes, batch = case
    again = _Call(sizes, batch).run(*_device_inputs(sizes, batch))
    for j, (a, b) in enumerate(zip(_bits(again), _bits(_result(sizes, batch)))):
        assert torch.equal(a, b), j


@pytest.mark.parametrize("sizes", T.NETS, ids=lambda s: "-".join(map(str, s)))
def test_a_row_of_out_does_not_depend_on_the_batch(sizes):
    small, large = _result(sizes, 33), _result(sizes, 2 * R + 5)
    assert torch.equal(small.out.view(torch.int32), large.out[:33].view(torch.int32))


@pytest.mark.parametrize("case", [(T.NETS[0], R + 1), (T.NETS[7], 65)], ids=T.case_id)
def test_a_captured_pass_replays_the_eager_bits(case):
    sizes, batch = case
    x, d = (t.clone() for t in _device_inputs(sizes, batch))
    eager = _bits(_result(sizes, batch))
    call = _Call(sizes, batch)
    call.run(x, d)                                     # warm: nothing is made inside the capture
    for buf in [call.out_buf, call.dx_buf] + [b for b, _, _ in call.grad_bufs]:
        buf.fill_(ms.PATTERN)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call.forward(x)
        call.backward(x, d)
    graph.replay()
    torch.cuda.synchronize()
    call.check_guards("replay")
    for j, (a, b) in enumerate(zip(_bits(call), eager)):
        assert torch.equal(a, b), j
    gen = torch.Generator().manual_seed(9)
    x2, d2 = torch.randn(x.shape, generator=gen).to(DEV), (torch.randn(d.shape, generator=gen) / batch).to(DEV)
    fresh = _bits(_Call(sizes, batch).run(x2, d2))
    x.copy_(x2)
    d.copy_(d2)
    graph.replay()
    torch.cuda.synchronize()
    for j, (a, b) in enumerate(zip(_bits(call), fresh)):
        assert torch.equal(a, b), j


def test_one_learner_step_through_the_trainer():
    """257 rows through MlpTrainer.for_actor / for_critic + PpoLoss + loss.backward(), then ClippedAdam.step().  The gradients of the
    head outputs that PpoLoss stored are handed to the float64 composition and to torch's float32 autograd of the same module: the
    trainer's gradients and torch's are both within the bound of test 1 of the float64 ones."""
    pkg = _pkg()
    n = 257
    net = ms.perturbed_net(pkg, 13, 3, DEV)
    actor, critic = pkg.MlpTrainer.for_actor(net, n), pkg.MlpTrainer.for_critic(net, n)
    ppo = pkg.PpoLoss(n, 4, DEV)
    statics = [(p, g) for t in (actor, critic) for p, g in zip(t.params, t.grads)]
    assert all(p.grad is g for p, g in statics)
    gen = torch.Generator().manual_seed(11)
    obs = torch.randn((n, 13), generator=gen).to(DEV)
    mb = dict(actions=torch.randn((n, 4), generator=gen).to(DEV), log_probs=(-4.0 + 0.3 * torch.randn(n, generator=gen)).to(DEV),
              advantages=torch.randn(n, generator=gen).to(DEV), returns=torch.randn(n, generator=gen).to(DEV))

    stale = actor(obs)
    mean = actor(obs)
    with pytest.raises(RuntimeError, match="backward of call"):
        stale.sum().backward()
    values = critic(obs).squeeze(-1)
    loss = ppo(mean, net.log_std, values, mb)
    loss.backward()
    torch.cuda.synchronize()
    assert all(p.grad is g for p, g in statics)
    d_mean, d_value = ppo.d_mean[:n].clone(), ppo.d_value[:n].clone()
    got = {"pi": [g.clone() for g in actor.grads], "vf": [g.clone() for g in critic.grads]}

    pi, vf = ms.layers_of(net)
    worst = 0.0
    for name, layers, d_out, seq, head in (("pi", pi, d_mean, net.pi, net.action_net), ("vf", vf, d_value.unsqueeze(1), net.vf, net.value_net)):
        _, g64, _ = T.reference_of([(w.cpu(), b.cpu()) for w, b in layers], obs.cpu(), d_out.cpu())
        params = [p for m in list(seq)[0::2] + [head] for p in (m.weight, m.bias)]
        g32 = torch.autograd.grad(head(seq(obs)), params, d_out)
        for j, (ref, mine, theirs) in enumerate(zip(g64, got[name], g32)):
            scale = float(ref.abs().max())
            e_mine, e_torch = (float((t.cpu().double() - ref).abs().max()) / scale for t in (mine, theirs))
            print(f"mlp_train learner step {name}[{j}]: trainer {e_mine:.3e}, torch float32 {e_torch:.3e}")
            assert e_mine <= T.BOUND and e_torch <= T.BOUND, (name, j, e_mine, e_torch)
            worst = max(worst, e_mine)
        if name == "pi":
            norm_sq = sum(float((g * g).sum()) for g in g64)
        else:
            norm_sq += sum(float((g * g).sum()) for g in g64)

    opt = pkg.ClippedAdam(actor.params + critic.params, zero_grads=False)
    opt.step()
    torch.cuda.synchronize()
    assert all(p.grad is g for p, g in statics)
    assert opt.stats_dict()["grad_norm"] == pytest.approx(norm_sq ** 0.5, rel=1e-4)
