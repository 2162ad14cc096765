"""The training pass of the Tanh networks on the device (include/dronenav.h dn_mlp_train_forward / dn_mlp_train_backward).

What a PPO learner step does between the minibatch and the loss head, and between the loss head and the optimiser: the forward of one
network of MlpActorCritic (or MlpValue) with its hidden activations saved, and the backward from the gradient of the head output to every
weight and bias gradient and, where asked, to the input -- float32 grade on the bf16 matrix cores, bit-reproducible, plain launches.  The
nn.Linear parameters are read in place; the gradients land in static tensors that are the parameters' .grad, which is what
optim.ClippedAdam reads.  The loss head, the optimiser and the learner loop are ppo.PpoLoss, optim.ClippedAdam and the caller's.
"""
import ctypes as C

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi
from ._fleetnorm import LossHead

MAX_BATCH = 1 << 24


class _MlpTrainFunction(torch.autograd.Function):
    """forward: dn_mlp_train_forward; backward: the one dn_mlp_train_backward call, which writes the parameter gradients itself.  The
    parameters are inputs only so that the output requires grad; their gradients are returned as None."""

    @staticmethod
    def forward(ctx, x, owner, count, param_grads, *params):
        owner._forward(x, count)
        ctx.owner, ctx.count, ctx.call, ctx.param_grads, ctx.n_params = owner, count, owner._calls, param_grads, len(params)
        ctx.save_for_backward(x)
        return owner.out[:count]

    @staticmethod
    @once_differentiable                               # the saved activations are plain buffers: there is no double backward
    def backward(ctx, d_out):
        owner = ctx.owner
        owner._stale(ctx)
        (x,) = ctx.saved_tensors
        d_x = owner._backward(x, d_out, ctx.count, ctx.needs_input_grad[0], ctx.param_grads)
        return (d_x, None, None, None) + (None,) * ctx.n_params


def _linears_of(name, seq):
    """The nn.Linear modules of a trunk built as Linear, Tanh, Linear, Tanh, ...; anything else is refused under `name`."""
    mods = list(seq)
    if not mods or len(mods) % 2:
        raise ValueError(f"MlpTrainer: {name} must be Linear, Tanh pairs, got {[type(m).__name__ for m in mods]}")
    for lin, act in zip(mods[0::2], mods[1::2]):
        if not isinstance(lin, nn.Linear) or not isinstance(act, nn.Tanh):
            raise ValueError(f"MlpTrainer: {name} must be Linear, Tanh pairs (the kernels know Tanh only), got "
                             f"{[type(m).__name__ for m in mods]}")
    return mods[0::2]


class MlpTrainer(LossHead):
    """linears: the nn.Linear modules of one network in order, the head last -- 2..4 of them, float32, dense, on one GPU; layer 0 reads
    1..64 columns, every hidden width is a multiple of 32 in 32..512, the head has 1..32 outputs; Tanh follows every layer but the head.
    batch_size: the most rows of a call, 1..2^24; accumulate: add each gradient to its tensor instead of overwriting it.
    for_actor(net) / for_critic(net): the two networks of an MlpActorCritic (pi + action_net, vf + value_net); for_value(v): an MlpValue.

    Static tensors: grads, one per parameter in the order (weight, bias) per layer, installed as that parameter's .grad here and again at
    every call that finds another tensor there -- the same tensors at every replay of a captured step, which is what ClippedAdam needs;
    out [batch_size, out_dim]; d_x [batch_size, in_dim].
    out = trainer(x, param_grads=True): x [count, in_dim] float32, dense, on the device, 1 <= count <= batch_size.  Returns
    out[:count], a view of the static tensor that the next call overwrites, connected to autograd: backward makes the one
    dn_mlp_train_backward call with the incoming gradient.  The kernel overwrites the parameter gradients (adds, with accumulate=True)
    -- with overwrite semantics nothing needs zeroing between minibatches -- and x receives a gradient only if it requires one.
    param_grads=False: a pass whose parameter gradients would be discarded (only x's gradient is formed).  Backward must come before the
    next call (RuntimeError otherwise); there is no double backward.
    Capturable after one eager call: the scratch is made here, for batch_size rows, and never grows."""
    _NAME, _NOUN = "MlpTrainer", "rows"

    def __init__(self, linears, batch_size, device=None, *, accumulate=False):
        linears = list(linears)
        top = _capi.TRAIN_MAX_LAYERS
        if not 2 <= len(linears) <= top:
            raise ValueError(f"MlpTrainer: linears must hold 2..{top} nn.Linear modules, the head last, got {len(linears)}")
        for i, m in enumerate(linears):
            if not isinstance(m, nn.Linear):
                raise ValueError(f"MlpTrainer: linears[{i}] must be an nn.Linear, got {type(m).__name__}")
            if m.bias is None:
                raise ValueError(f"MlpTrainer: linears[{i}] has no bias; the kernels add one")
            for what, p in (("weight", m.weight), ("bias", m.bias)):
                if p.dtype != torch.float32:
                    raise ValueError(f"MlpTrainer: linears[{i}].{what} must be torch.float32, got {p.dtype}")
                if not p.is_contiguous():
                    raise ValueError(f"MlpTrainer: linears[{i}].{what} must be dense (strides {p.stride()}); the kernels read it in place")
        self._count("batch_size", batch_size, MAX_BATCH)
        dims = [(m.in_features, m.out_features) for m in linears]
        if not 1 <= dims[0][0] <= 64:
            raise ValueError(f"MlpTrainer: linears[0].in_features must be in 1..64, got {dims[0][0]}")
        for i, (_, o) in enumerate(dims[:-1]):
            if not 32 <= o <= 512 or o % 32:
                raise ValueError(f"MlpTrainer: linears[{i}].out_features, a hidden width, must be a multiple of 32 in 32..512, got {o}")
        if not 1 <= dims[-1][1] <= 32:
            raise ValueError(f"MlpTrainer: linears[{len(dims) - 1}].out_features, the head's, must be in 1..32, got {dims[-1][1]}")
        for i in range(1, len(dims)):
            if dims[i][0] != dims[i - 1][1]:
                raise ValueError(f"MlpTrainer: linears[{i}].in_features must be linears[{i - 1}].out_features = {dims[i - 1][1]}, got {dims[i][0]}")
        params = [p for m in linears for p in (m.weight, m.bias)]
        for i, m in enumerate(linears):
            for what, p in (("weight", m.weight), ("bias", m.bias)):
                if p.device.type != "cuda":
                    raise ValueError(f"MlpTrainer: linears[{i}].{what} is on {p.device}; the parameters must be on a GPU, there is no CPU path")
                if p.device != params[0].device:
                    raise ValueError(f"MlpTrainer: linears[{i}].{what} is on {p.device}, linears[0].weight on {params[0].device}; one device")
        if device is not None and torch.device(device).type == "cuda" and torch.device(device).index not in (None, params[0].device.index):
            raise ValueError(f"MlpTrainer: device {device} is not the parameters' {params[0].device}")
        super().__init__(params[0].device if device is None else device)
        self.linears, self.params, self.batch_size, self.accumulate = linears, params, batch_size, bool(accumulate)
        self.in_dim, self.out_dim = dims[0][0], dims[-1][1]
        f32 = dict(dtype=torch.float32, device=self.device)
        self.grads = [torch.zeros_like(p) for p in params]
        self.out = torch.zeros((batch_size, self.out_dim), **f32)
        self.d_x = torch.zeros((batch_size, self.in_dim), **f32)
        self._install()
        n = len(linears)
        self._table = (_capi.DnMlpTrainLayer * n)(*[_capi.DnMlpTrainLayer(m.weight.data_ptr(), m.bias.data_ptr(), self.grads[2 * i].data_ptr(),
                                                                         self.grads[2 * i + 1].data_ptr(), m.in_features, m.out_features)
                                                    for i, m in enumerate(linears)])
        self._need = int(self._lib.dn_mlp_train_scratch_bytes(C.byref(self._cfg(True)), self._table, batch_size))
        self._scratch_for(self._need)                  # of a full minibatch, made here: a capture never sees it grow

    @classmethod
    def for_actor(cls, net, batch_size, device=None, **kw):
        """pi + action_net of an MlpActorCritic."""
        cls._plain_trunk(net)
        return cls(_linears_of("net.pi", net.pi) + [net.action_net], batch_size, device, **kw)

    @classmethod
    def for_critic(cls, net, batch_size, device=None, **kw):
        """vf + value_net of an MlpActorCritic."""
        cls._plain_trunk(net)
        return cls(_linears_of("net.vf", net.vf) + [net.value_net], batch_size, device, **kw)

    @classmethod
    def for_value(cls, value, batch_size, device=None, **kw):
        """vf + value_net of an MlpValue."""
        return cls(_linears_of("value.vf", value.vf) + [value.value_net], batch_size, device, **kw)

    @staticmethod
    def _plain_trunk(net):
        if getattr(net, "trunk_dtype", None) is not None:
            raise ValueError(f"MlpTrainer: net.trunk_dtype must be None (float32 throughout), got {net.trunk_dtype}; the pass is float32 grade")

    def _cfg(self, param_grads):
        flags = (_capi.TRAIN_ACCUMULATE if self.accumulate else 0) | (0 if param_grads else _capi.TRAIN_NO_PARAM_GRADS)
        return _capi.DnMlpTrainConfig(len(self.linears), _capi.TRAIN_ACT_TANH, flags, 0)

    def _install(self):
        for p, g in zip(self.params, self.grads):
            if p.grad is not g:
                p.grad = g

    def __call__(self, x, param_grads=True):
        count = self._rows("x", x, self.in_dim)
        param_grads = bool(param_grads)
        if param_grads:
            self._install()
        return _MlpTrainFunction.apply(x, self, count, param_grads, *(self.params if param_grads else ()))

    def _refresh(self):
        for i, m in enumerate(self.linears):           # the parameters are read where they are now: load_state_dict keeps them, .to() does not
            self._table[i].weight, self._table[i].bias = m.weight.data_ptr(), m.bias.data_ptr()

    def _forward(self, x, count):
        self._refresh()
        scratch = self._scratch_for(self._need)
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_mlp_train_forward(C.byref(self._cfg(True)), self._table, x.data_ptr(), count, self.out.data_ptr(),
                                                       scratch.data_ptr(), scratch.numel() * 8, self.device.index, self._stream()))
        self._calls += 1

    def _backward(self, x, d_out, count, want_dx, param_grads):
        if not want_dx and not param_grads:
            return None
        d_out = d_out.contiguous()                     # an expanded gradient (out.sum().backward()) is staged; the loss heads' are dense
        self._check("the gradient of out", d_out, (count, self.out_dim))
        scratch = self._scratch_for(self._need)
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_mlp_train_backward(C.byref(self._cfg(param_grads)), self._table, x.data_ptr(), d_out.data_ptr(), count,
                                                        self.d_x.data_ptr() if want_dx else None, scratch.data_ptr(), scratch.numel() * 8,
                                                        self.device.index, self._stream()))
        return self.d_x[:count] if want_dx else None

    def __repr__(self):
        sizes = [self.in_dim] + [m.out_features for m in self.linears]
        return (f"MlpTrainer({'-'.join(str(s) for s in sizes)}, batch_size={self.batch_size}, device={str(self.device)!r}, "
                f"accumulate={self.accumulate})")
