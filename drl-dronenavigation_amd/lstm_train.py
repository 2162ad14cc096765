"""One LSTM layer on the device (include/dronenav.h dn_lstm_forward / dn_lstm_backward): the recurrent policy's training pass and its
rollout step.

LstmTrainer is what a recurrent learner step does between the sequence minibatch and the networks behind the LSTM: the forward of a
torch.nn.LSTM over a time-major sequence with episode starts inside it, with what the backward needs saved, and the backward from the
gradient of h_seq to the four parameter gradients and, where asked, to the input -- float32 grade on the bf16 matrix cores,
bit-reproducible, plain launches.  LstmStepper is the rollout side: a resident (h, c) per drone, advanced in place one step a call.  The
nn.LSTM parameters are read in place; the gradients land in static tensors that are the parameters' .grad, which is what
optim.ClippedAdam reads.

What sits behind the LSTM is the caller's: an LSTM of hidden <= 64 feeds mlp_train.MlpTrainer / dn_mlp_forward directly (their layer 0
reads at most 64 columns), a wider one feeds torch layers.  Sequence minibatches out of collector.RolloutCollector and
minibatch.MinibatchSampler are the caller's too.
"""
import ctypes as C

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi
from ._fleetnorm import DeviceScratch, LossHead

_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def _lstm_dims(who, lstm):
    """(in_dim, hidden) of a torch.nn.LSTM the kernels take; anything else is refused by name.  Needs no device."""
    if not isinstance(lstm, nn.LSTM):
        raise ValueError(f"{who}: lstm must be a torch.nn.LSTM, got {type(lstm).__name__}")
    if lstm.num_layers != 1:
        raise ValueError(f"{who}: lstm.num_layers must be 1, got {lstm.num_layers}")
    if lstm.bidirectional:
        raise ValueError(f"{who}: lstm.bidirectional must be False; the kernels run one direction")
    if lstm.proj_size != 0:
        raise ValueError(f"{who}: lstm.proj_size must be 0, got {lstm.proj_size}")
    if not lstm.bias:
        raise ValueError(f"{who}: lstm.bias must be True; the kernels add both biases")
    if lstm.batch_first:
        raise ValueError(f"{who}: lstm.batch_first must be False; the kernels are time-major")
    for name in _NAMES:
        p = getattr(lstm, name)
        if p.dtype != torch.float32:
            raise ValueError(f"{who}: lstm.{name} must be torch.float32, got {p.dtype}")
        if not p.is_contiguous():
            raise ValueError(f"{who}: lstm.{name} must be dense (strides {p.stride()}); the kernels read it in place")
    if not 1 <= lstm.input_size <= _capi.RNN_MAX_IN:
        raise ValueError(f"{who}: lstm.input_size must be in 1..{_capi.RNN_MAX_IN}, got {lstm.input_size}")
    if not 32 <= lstm.hidden_size <= _capi.RNN_MAX_HIDDEN or lstm.hidden_size % 32:
        raise ValueError(f"{who}: lstm.hidden_size must be a multiple of 32 in 32..{_capi.RNN_MAX_HIDDEN}, got {lstm.hidden_size}")
    return lstm.input_size, lstm.hidden_size


def _lstm_device(who, lstm, device):
    params = [getattr(lstm, n) for n in _NAMES]
    for name, p in zip(_NAMES, params):
        if p.device.type != "cuda":
            raise ValueError(f"{who}: lstm.{name} is on {p.device}; the parameters must be on a GPU, there is no CPU path")
        if p.device != params[0].device:
            raise ValueError(f"{who}: lstm.{name} is on {p.device}, lstm.{_NAMES[0]} on {params[0].device}; one device")
    if device is not None and torch.device(device).type == "cuda" and torch.device(device).index not in (None, params[0].device.index):
        raise ValueError(f"{who}: device {device} is not the parameters' {params[0].device}")
    return params, (params[0].device if device is None else device)


def _overlap(a, b):
    """Do the bytes of two dense tensors on one device overlap?"""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def step_scratch_bytes(num_envs, hidden):
    """What a T = 1 dn_lstm_forward over num_envs rows asks of its scratch: the gates [num_envs][4 hidden] float32, the first region of
    include/dronenav.h's layout (csrc/dn_internal.h dn_lstm_layout: the offset carry_h), rounded up to 256 bytes.  The library has no
    entry point that answers it; tests/test_lstm_cpu.py holds this figure to the forward's refusal of one byte less."""
    return (16 * num_envs * hidden + 255) // 256 * 256


class _LstmTrainFunction(torch.autograd.Function):
    """forward: dn_lstm_forward; backward: the one dn_lstm_backward call, which writes the parameter gradients itself.  The parameters are
    inputs only so that the output requires grad; their gradients are returned as None.  h0 and c0 receive no gradient."""

    @staticmethod
    def forward(ctx, x, owner, starts, h0, c0, param_grads, *params):
        steps, count = owner._forward(x, starts, h0, c0)
        ctx.owner, ctx.call, ctx.param_grads, ctx.n_params = owner, owner._calls, param_grads, len(params)
        ctx.starts, ctx.h0, ctx.c0 = starts, h0, c0
        ctx.save_for_backward(x)
        return owner._seq(owner.h_seq, steps, count, owner.hidden)

    @staticmethod
    @once_differentiable                               # the saved gates are a plain buffer that the backward consumes: no double backward
    def backward(ctx, d_hseq):
        owner = ctx.owner
        owner._stale(ctx)
        if ctx.call == owner._spent:
            raise RuntimeError(f"LstmTrainer: a second backward of call {ctx.call}: the first has written dZ over the saved gates")
        (x,) = ctx.saved_tensors
        d_x = owner._backward(x, ctx.starts, ctx.h0, ctx.c0, d_hseq, ctx.needs_input_grad[0], ctx.param_grads)
        return (d_x, None, None, None, None, None) + (None,) * ctx.n_params


class LstmTrainer(LossHead):
    """lstm: a torch.nn.LSTM with num_layers=1, one direction, proj_size=0, bias=True, batch_first=False, float32, dense, on one GPU;
    input_size 1..64, hidden_size a multiple of 32 in 32..512.  n_steps: the most steps of a call, 1..1024; batch_size: the most
    sequences of a call; n_steps x batch_size <= 2^24.  accumulate: add each gradient to its tensor instead of overwriting it.

    Static tensors: grads, the four parameters' in the order weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0, installed as .grad here
    and again at every call that finds another tensor there; h_seq, c_seq [n_steps, batch_size, hidden]; h_T, c_T [batch_size, hidden];
    d_x [n_steps, batch_size, input_size].
    h_seq = trainer(x, episode_starts, h0, c0, param_grads=True): x [T, count, input_size] float32, dense, on the device, T <= n_steps,
    count <= batch_size; episode_starts uint8 [T, count] or None; h0, c0 [count, hidden] float32 or None (zeros).  A row whose
    episode_starts[t] is set enters step t with zero state.  Returns h_seq [T, count, hidden], a dense view at the front of the static
    tensor that the next call overwrites, connected to autograd: what follows the LSTM (an MlpTrainer's d_x, torch layers) hands its
    gradient to the one dn_lstm_backward call.  trainer.h_T[:count] and trainer.c_T[:count] hold the last step's state, trainer.c_seq the
    cells; to chain sequences pass copies of them as the next h0, c0 -- the backward reads h0 and c0 again, so tensors that overlap
    the trainer's own static outputs are refused (ValueError).  x receives a gradient only if it requires one; h0 and c0 never do.
    param_grads=False: only x's gradient is formed.
    Backward must come before the next call and at most once (RuntimeError otherwise); there is no double backward.
    Capturable after one eager call: the scratch is made here, for n_steps x batch_size rows, and never grows."""
    _NAME, _NOUN = "LstmTrainer", "sequences"

    def __init__(self, lstm, n_steps, batch_size, device=None, *, accumulate=False):
        self.in_dim, self.hidden = _lstm_dims(self._NAME, lstm)
        self._count("n_steps", n_steps, _capi.RNN_MAX_STEPS)
        self._count("batch_size", batch_size, _capi.RNN_MAX_ROWS)
        if n_steps * batch_size > _capi.RNN_MAX_ROWS:
            raise ValueError(f"{self._NAME}: n_steps x batch_size must be <= 2^24 rows, got {n_steps} x {batch_size}")
        params, device = _lstm_device(self._NAME, lstm, device)
        super().__init__(device)
        self.lstm, self.params, self.n_steps, self.batch_size, self.accumulate = lstm, params, n_steps, batch_size, bool(accumulate)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.grads = [torch.zeros_like(p) for p in params]
        self.h_seq = torch.zeros((n_steps, batch_size, self.hidden), **f32)
        self.c_seq = torch.zeros((n_steps, batch_size, self.hidden), **f32)
        self.h_T = torch.zeros((batch_size, self.hidden), **f32)
        self.c_T = torch.zeros((batch_size, self.hidden), **f32)
        self.d_x = torch.zeros((n_steps, batch_size, self.in_dim), **f32)
        self._zeros = torch.zeros((batch_size, self.hidden), **f32)
        self._install()
        self._spent = 0
        self._need = int(self._lib.dn_lstm_scratch_bytes(C.byref(self._cfg(True)), n_steps, batch_size))
        self._scratch_for(self._need)                  # of the largest call, made here: a capture never sees it grow

    def _cfg(self, param_grads):
        flags = (_capi.TRAIN_ACCUMULATE if self.accumulate else 0) | (0 if param_grads else _capi.TRAIN_NO_PARAM_GRADS)
        return _capi.DnLstmConfig(self.in_dim, self.hidden, flags, 0)

    def _table(self):
        """The parameters are read where they are now: load_state_dict keeps them, .to() does not."""
        return _capi.DnLstmParams(*[getattr(self.lstm, n).data_ptr() for n in _NAMES], *[g.data_ptr() for g in self.grads])

    def _install(self):
        for p, g in zip(self.params, self.grads):
            if p.grad is not g:
                p.grad = g

    @staticmethod
    def _seq(static, steps, count, width):
        """[steps, count, width] dense at the front of a static [n_steps, batch_size, width] tensor."""
        return static.view(-1)[:steps * count * width].view(steps, count, width)

    def __call__(self, x, episode_starts=None, h0=None, c0=None, param_grads=True):
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise ValueError(f"{self._NAME}: x must be a tensor [T, count, {self.in_dim}]")
        steps, count = int(x.shape[0]), int(x.shape[1])
        if not 1 <= steps <= self.n_steps:
            raise ValueError(f"{self._NAME}: x has {steps} steps; a call takes 1..{self.n_steps} (n_steps)")
        if not 1 <= count <= self.batch_size:
            raise ValueError(f"{self._NAME}: x has {count} sequences; a call takes 1..{self.batch_size} (batch_size)")
        self._check("x", x, (steps, count, self.in_dim))
        if episode_starts is not None:
            if (not isinstance(episode_starts, torch.Tensor) or tuple(episode_starts.shape) != (steps, count) or episode_starts.dtype != torch.uint8
                    or episode_starts.device != self.device or not episode_starts.is_contiguous()):
                raise ValueError(f"{self._NAME}: episode_starts must be a dense torch.uint8 [{steps}, {count}] on {self.device} or None")
        for name, t in (("h0", h0), ("c0", c0)):
            if t is not None:
                self._check(name, t, (count, self.hidden))
                for mine in ("h_T", "c_T", "h_seq", "c_seq"):
                    if _overlap(t, getattr(self, mine)):
                        raise ValueError(f"{self._NAME}: {name} overlaps this trainer's static {mine}, which the forward overwrites before the "
                                         f"backward reads {name} again; pass a copy (trainer.{mine}[:count].clone())")
        param_grads = bool(param_grads)
        if param_grads:
            self._install()
        return _LstmTrainFunction.apply(x, self, episode_starts, h0, c0, param_grads, *(self.params if param_grads else ()))

    def _pointers(self, starts, h0, c0):
        return (starts.data_ptr() if starts is not None else None, (self._zeros if h0 is None else h0).data_ptr(),
                (self._zeros if c0 is None else c0).data_ptr())

    def _forward(self, x, starts, h0, c0):
        steps, count = int(x.shape[0]), int(x.shape[1])
        scratch = self._scratch_for(self._need)
        sp, hp, cp = self._pointers(starts, h0, c0)
        table = self._table()
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_lstm_forward(C.byref(self._cfg(True)), C.byref(table), x.data_ptr(), sp, hp, cp, steps, count,
                                                  self.h_seq.data_ptr(), self.c_seq.data_ptr(), self.h_T.data_ptr(), self.c_T.data_ptr(),
                                                  scratch.data_ptr(), scratch.numel() * 8, self.device.index, self._stream()))
        self._calls += 1
        return steps, count

    def _backward(self, x, starts, h0, c0, d_hseq, want_dx, param_grads):
        if not want_dx and not param_grads:
            return None
        steps, count = int(x.shape[0]), int(x.shape[1])
        d_hseq = d_hseq.contiguous()                   # an expanded gradient (h_seq.sum().backward()) is staged
        self._check("the gradient of h_seq", d_hseq, (steps, count, self.hidden))
        scratch = self._scratch_for(self._need)
        sp, hp, cp = self._pointers(starts, h0, c0)
        table = self._table()
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_lstm_backward(C.byref(self._cfg(param_grads)), C.byref(table), x.data_ptr(), sp, hp, self.h_seq.data_ptr(),
                                                   self.c_seq.data_ptr(), cp, d_hseq.data_ptr(), steps, count,
                                                   self.d_x.data_ptr() if want_dx else None, scratch.data_ptr(), scratch.numel() * 8,
                                                   self.device.index, self._stream()))
        self._spent = self._calls
        return self._seq(self.d_x, steps, count, self.in_dim) if want_dx else None

    def __repr__(self):
        return (f"LstmTrainer({self.in_dim}->{self.hidden}, n_steps={self.n_steps}, batch_size={self.batch_size}, device={str(self.device)!r}, "
                f"accumulate={self.accumulate})")


class LstmStepper(DeviceScratch):
    """The rollout side of the same layer: a resident state h, c [num_envs, hidden], zeros at first.
    h = stepper.step(x, episode_starts): x [num_envs, input_size] float32, episode_starts uint8 [num_envs] or None -- one dn_lstm_forward
    with T = 1 whose h_T, c_T are h0, c0: the state advances in place, and the static h is returned (the next step overwrites it).  A drone
    whose episode_starts is set enters the step with zero state.  state() returns copies of (h, c); set_state(h, c) overwrites them (the
    initial state of a rollout, which the learner hands to LstmTrainer as h0, c0).  No autograd, and no gradient scratch: the scratch is
    the step's gates alone.  Capturable: everything is made here."""
    _NAME, _NOUN = "LstmStepper", "drones"

    def __init__(self, lstm, num_envs, device=None):
        self.in_dim, self.hidden = _lstm_dims(self._NAME, lstm)
        if isinstance(num_envs, bool) or not isinstance(num_envs, int) or not 1 <= num_envs <= _capi.RNN_MAX_ROWS:
            raise ValueError(f"{self._NAME}.num_envs must be an integer in 1..{_capi.RNN_MAX_ROWS}, got {num_envs!r}")
        _, device = _lstm_device(self._NAME, lstm, device)
        super().__init__(device)
        self.lstm, self.num_envs = lstm, num_envs
        f32 = dict(dtype=torch.float32, device=self.device)
        self.h, self.c = torch.zeros((num_envs, self.hidden), **f32), torch.zeros((num_envs, self.hidden), **f32)
        self._h_seq, self._c_seq = torch.zeros((1, num_envs, self.hidden), **f32), torch.zeros((1, num_envs, self.hidden), **f32)
        self._cfg = _capi.DnLstmConfig(self.in_dim, self.hidden, 0, 0)
        self._need = step_scratch_bytes(num_envs, self.hidden)
        self._scratch_for(self._need)

    def step(self, x, episode_starts=None):
        n = self.num_envs
        if (not isinstance(x, torch.Tensor) or tuple(x.shape) != (n, self.in_dim) or x.dtype != torch.float32 or x.device != self.device
                or not x.is_contiguous()):
            raise ValueError(f"{self._NAME}: x must be a dense torch.float32 [{n}, {self.in_dim}] on {self.device}")
        if episode_starts is not None:
            if (not isinstance(episode_starts, torch.Tensor) or tuple(episode_starts.shape) != (n,) or episode_starts.dtype != torch.uint8
                    or episode_starts.device != self.device or not episode_starts.is_contiguous()):
                raise ValueError(f"{self._NAME}: episode_starts must be a dense torch.uint8 [{n}] on {self.device} or None")
        table = _capi.DnLstmParams(*[getattr(self.lstm, k).data_ptr() for k in _NAMES], None, None, None, None)
        scratch = self._scratch_for(self._need)
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_lstm_forward(C.byref(self._cfg), C.byref(table), x.data_ptr(),
                                                  episode_starts.data_ptr() if episode_starts is not None else None, self.h.data_ptr(),
                                                  self.c.data_ptr(), 1, n, self._h_seq.data_ptr(), self._c_seq.data_ptr(), self.h.data_ptr(),
                                                  self.c.data_ptr(), scratch.data_ptr(), scratch.numel() * 8, self.device.index, self._stream()))
        return self.h

    def state(self):
        return self.h.clone(), self.c.clone()

    def set_state(self, h, c):
        for name, t in (("h", h), ("c", c)):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (self.num_envs, self.hidden):
                raise ValueError(f"{self._NAME}: {name} must be a tensor [{self.num_envs}, {self.hidden}]")
        self.h.copy_(h)
        self.c.copy_(c)

    def __repr__(self):
        return f"LstmStepper({self.in_dim}->{self.hidden}, num_envs={self.num_envs}, device={str(self.device)!r})"
