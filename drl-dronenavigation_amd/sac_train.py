"""The training pass of the SAC networks on the device and the Polyak update of the target critics (include/dronenav.h
dn_sac_train_forward / dn_sac_train_backward, dn_polyak_update).

What a SAC gradient step does between the replay minibatch, the loss heads and the optimisers: the forward of the actor (latent_pi with
the heads mu | log_std) or of all critics at once (over obs and actions as two tensors, never concatenated) with the hidden activations
saved, and the backward from the gradients of the head outputs to every weight and bias gradient and, where asked, to the inputs --
float32 grade on the bf16 matrix cores, bit-reproducible, plain launches; and target <- (1 - tau) target + tau source in one launch.  The
nn.Linear parameters are read in place; the gradients land in static tensors that are the parameters' .grad, which is what
optim.ClippedAdam reads.  The sampler, the loss heads and the optimisers are replay.ReplaySampler, sac.* and optim.ClippedAdam.
"""
import ctypes as C

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi
from ._fleetnorm import DeviceScratch, LossHead
from .mlp_train import MAX_BATCH

_ACTIVATIONS = {"tanh": (_capi.TRAIN_ACT_TANH, nn.Tanh), "relu": (_capi.TRAIN_ACT_RELU, nn.ReLU)}


class _SacTrainFunction(torch.autograd.Function):
    """forward: dn_sac_train_forward; backward: the one dn_sac_train_backward call, which writes the parameter gradients itself.  The
    parameters are inputs only so that the outputs require grad; their gradients are returned as None."""

    @staticmethod
    def forward(ctx, x0, x1, owner, count, param_grads, *params):
        owner._forward(x0, x1, count)
        ctx.owner, ctx.count, ctx.call, ctx.param_grads, ctx.n_params = owner, count, owner._calls, param_grads, len(params)
        ctx.two = x1 is not None
        ctx.save_for_backward(*((x0, x1) if ctx.two else (x0,)))
        return owner._views(count)

    @staticmethod
    @once_differentiable                               # the saved activations are plain buffers: there is no double backward
    def backward(ctx, *d_out):
        owner = ctx.owner
        owner._stale(ctx)
        x0, x1 = ctx.saved_tensors if ctx.two else (ctx.saved_tensors[0], None)
        want0, want1 = ctx.needs_input_grad[0], ctx.two and ctx.needs_input_grad[1]
        d_x0, d_x1 = owner._backward(x0, x1, d_out, ctx.count, want0, want1, ctx.param_grads)
        return (d_x0, d_x1, None, None, None) + (None,) * ctx.n_params


def _trunk(who, name, seq, act_cls):
    """The nn.Linear modules of a trunk built as Linear, act, Linear, act, ...; anything else is refused under `name`."""
    mods = list(seq)
    pairs = f"Linear, {act_cls.__name__} pairs"
    if not mods or len(mods) % 2 or any(not isinstance(lin, nn.Linear) or not isinstance(act, act_cls) for lin, act in zip(mods[0::2], mods[1::2])):
        raise ValueError(f"{who}: {name} must be {pairs}, got {[type(m).__name__ for m in mods]}")
    return mods[0::2]


class SacTrainer(LossHead):
    """nets: 1..4 networks of identical dimensions that share their input (the twin critics; one for the actor).  A network is a list of
    its nn.Linear modules in order, 2..4 with the head counted once; the last element is the head, an nn.Linear or a tuple of two
    (the actor's mu and log_std, read in place as one head).  float32, dense, on one GPU; layer 0 reads 1..64 columns, every hidden width
    is a multiple of 32 in 32..512, a head part has 1..32 outputs and the parts at most 32 together.
    activation: "relu" or "tanh", after every layer but the head.  in_split: None, or (in0, in1): layer 0 reads two tensors side by
    side, x0 [count, in0] and x1 [count, in1] -- obs and actions, never concatenated.  squeeze: outputs of one column come back as
    [count].  accumulate: add each gradient to its tensor instead of overwriting it.  grads=False: a forward-only instance (the target
    critics): no gradient tensors are made, no .grad is touched and every call returns detached outputs.
    for_actor(actor): latent_pi + (mu, log_std) of a SacActor; for_critics(critic): every q_network of a SacCritic.

    Static tensors: grads, one per parameter in the order (weight, bias) per layer and part, network by network, installed as that
    parameter's .grad here and again at every call that finds another tensor there; outs, one [batch_size, out] per network and part;
    d_x0, d_x1.
    outs = trainer(x0, x1=None, param_grads=True): a tuple of n_nets * parts tensors, network-major, views of the static tensors that
    the next call overwrites, connected to autograd: backward makes the one dn_sac_train_backward call with the incoming gradients.  The
    kernel overwrites the parameter gradients (adds, with accumulate=True); x0 and x1 receive a gradient only where they require one.
    param_grads=False: only the inputs' gradients are formed (the actor loss's pass through the critics).  An instance holds one set of
    saved activations: backward must come before the next call (RuntimeError otherwise); there is no double backward.  Under
    torch.no_grad() the outputs are detached, nothing is pending and no .grad is touched.
    Capturable after one eager call: the scratch is made here, for batch_size rows, and never grows."""
    _NAME, _NOUN = "SacTrainer", "rows"

    def __init__(self, nets, batch_size, device=None, *, activation="relu", in_split=None, squeeze=False, accumulate=False, grads=True):
        me = self._NAME
        if activation not in _ACTIVATIONS:
            raise ValueError(f"{me}: activation must be 'relu' or 'tanh', got {activation!r}")
        nets = [list(n) for n in nets]
        if not 1 <= len(nets) <= _capi.TRAIN_MAX_NETS:
            raise ValueError(f"{me}: nets must hold 1..{_capi.TRAIN_MAX_NETS} networks, got {len(nets)}")
        top = _capi.TRAIN_MAX_LAYERS
        entries = []                                   # per network: [(name, module)], the head's parts last
        for c, net in enumerate(nets):
            if not 2 <= len(net) <= top:
                raise ValueError(f"{me}: nets[{c}] must hold 2..{top} layers, the head last and counted once, got {len(net)}")
            head = net[-1]
            parts = list(head) if isinstance(head, (tuple, list)) else [head]
            if not 1 <= len(parts) <= _capi.TRAIN_MAX_PARTS:
                raise ValueError(f"{me}: nets[{c}]'s head must be an nn.Linear or a tuple of two, got {len(parts)} parts")
            named = [(f"nets[{c}][{i}]", m) for i, m in enumerate(net[:-1])]
            named += [(f"nets[{c}][{len(net) - 1}]" + (f"[{p}]" if len(parts) > 1 else ""), m) for p, m in enumerate(parts)]
            for name, m in named:
                if not isinstance(m, nn.Linear):
                    raise ValueError(f"{me}: {name} must be an nn.Linear, got {type(m).__name__}")
                if m.bias is None:
                    raise ValueError(f"{me}: {name} has no bias; the kernels add one")
                for what, p in (("weight", m.weight), ("bias", m.bias)):
                    if p.dtype != torch.float32:
                        raise ValueError(f"{me}: {name}.{what} must be torch.float32, got {p.dtype}")
                    if not p.is_contiguous():
                        raise ValueError(f"{me}: {name}.{what} must be dense (strides {p.stride()}); the kernels read it in place")
            entries.append(named)
        self._count("batch_size", batch_size, MAX_BATCH)
        n_layers, n_parts = len(nets[0]), len(entries[0]) - len(nets[0]) + 1
        hidden = [m for _, m in entries[0][:n_layers - 1]]
        heads = [m for _, m in entries[0][n_layers - 1:]]
        in_dim = hidden[0].in_features
        if in_split is None:
            in_split = (in_dim, 0)
        in0, in1 = (int(v) for v in in_split)
        if not 1 <= in0 <= 64 or not 0 <= in1 <= 63 or in0 + in1 > 64:
            raise ValueError(f"{me}: in_split must be (1..64, 0..63) with at most 64 columns together, got {tuple(in_split)}")
        if in0 + in1 != in_dim:
            raise ValueError(f"{me}: nets[0][0].in_features must be in_split's {in0} + {in1} = {in0 + in1}, got {in_dim}")
        for i, m in enumerate(hidden):
            if not 32 <= m.out_features <= 512 or m.out_features % 32:
                raise ValueError(f"{me}: nets[0][{i}].out_features, a hidden width, must be a multiple of 32 in 32..512, got {m.out_features}")
        for i in range(1, n_layers - 1):
            if hidden[i].in_features != hidden[i - 1].out_features:
                raise ValueError(f"{me}: nets[0][{i}].in_features must be nets[0][{i - 1}].out_features = {hidden[i - 1].out_features}, "
                                 f"got {hidden[i].in_features}")
        for (name, _), m in zip(entries[0][n_layers - 1:], heads):
            if not 1 <= m.out_features <= 32:
                raise ValueError(f"{me}: {name}.out_features, a head part's, must be in 1..32, got {m.out_features}")
            if m.in_features != hidden[-1].out_features:
                raise ValueError(f"{me}: {name}.in_features must be nets[0][{n_layers - 2}].out_features = {hidden[-1].out_features}, got {m.in_features}")
        if sum(m.out_features for m in heads) > 32:
            raise ValueError(f"{me}: the head's parts must have at most 32 outputs together, got {[m.out_features for m in heads]}")
        dims = [(m.in_features, m.out_features) for _, m in entries[0]]
        for c, named in enumerate(entries):
            mine = [(m.in_features, m.out_features) for _, m in named]
            if mine != dims:
                raise ValueError(f"{me}: nets[{c}] has the layers {mine}, nets[0] has {dims}; the networks of a group have one shape")
        modules = [m for named in entries for _, m in named]
        params = [p for m in modules for p in (m.weight, m.bias)]
        for named in entries:
            for name, m in named:
                for what, p in (("weight", m.weight), ("bias", m.bias)):
                    if p.device.type != "cuda":
                        raise ValueError(f"{me}: {name}.{what} is on {p.device}; the parameters must be on a GPU, there is no CPU path")
                    if p.device != params[0].device:
                        raise ValueError(f"{me}: {name}.{what} is on {p.device}, nets[0][0].weight on {params[0].device}; one device")
        if device is not None and torch.device(device).type == "cuda" and torch.device(device).index not in (None, params[0].device.index):
            raise ValueError(f"{me}: device {device} is not the parameters' {params[0].device}")
        super().__init__(params[0].device if device is None else device)
        self.nets, self.modules, self.params, self.batch_size = nets, modules, params, batch_size
        self.activation, self.accumulate, self.squeeze, self.with_grads = activation, bool(accumulate), bool(squeeze), bool(grads)
        self.n_nets, self.n_layers, self.n_parts, self.in0, self.in1 = len(nets), n_layers, n_parts, in0, in1
        self.out_dims = [m.out_features for m in heads]
        f32 = dict(dtype=torch.float32, device=self.device)
        self.grads = [torch.zeros_like(p) for p in params] if self.with_grads else []
        self.outs = [torch.zeros((batch_size, o), **f32) for _ in range(self.n_nets) for o in self.out_dims]
        self._out_table = (C.c_void_p * len(self.outs))(*[t.data_ptr() for t in self.outs])
        if self.with_grads:
            self.d_x0 = torch.zeros((batch_size, in0), **f32)
            self.d_x1 = torch.zeros((batch_size, in1), **f32) if in1 else None
            self._zeros = [torch.zeros_like(t) for t in self.outs]     # stands for the gradient of an output that nothing used
            self._install()
        ptr = lambda i, k: self.grads[2 * i + k].data_ptr() if self.with_grads else None      # noqa: E731
        self._table = (_capi.DnMlpTrainLayer * len(modules))(*[
            _capi.DnMlpTrainLayer(m.weight.data_ptr(), m.bias.data_ptr(), ptr(i, 0), ptr(i, 1), m.in_features, m.out_features)
            for i, m in enumerate(modules)])
        self._need = int(self._lib.dn_sac_train_scratch_bytes(C.byref(self._cfg(True)), self._table, batch_size))
        self._scratch_for(self._need)                  # of a full minibatch, made here: a capture never sees it grow

    @classmethod
    def for_actor(cls, actor, batch_size, device=None, **kw):
        """latent_pi + (mu, log_std) of a SacActor: mean, log_std_raw = trainer(obs); the clamp stays the loss head's."""
        return cls([_trunk(cls._NAME, "actor.latent_pi", actor.latent_pi, nn.ReLU) + [(actor.mu, actor.log_std)]], batch_size, device, **kw)

    @classmethod
    def for_critics(cls, critic, batch_size, device=None, act_dim=4, **kw):
        """Every q_network of a SacCritic: q = trainer(obs, actions), a tuple of n_critics tensors [count]."""
        nets = []
        for c, q in enumerate(critic.q_networks):
            mods = list(q)
            if not mods or not isinstance(mods[-1], nn.Linear):
                raise ValueError(f"{cls._NAME}: critic.q_networks[{c}] must end in its nn.Linear head, got {[type(m).__name__ for m in mods]}")
            nets.append(_trunk(cls._NAME, f"critic.q_networks[{c}]'s trunk", mods[:-1], nn.ReLU) + [mods[-1]])
        kw.setdefault("in_split", (nets[0][0].in_features - act_dim, act_dim) if nets else None)
        kw.setdefault("squeeze", True)
        return cls(nets, batch_size, device, **kw)

    def _cfg(self, param_grads):
        flags = (_capi.TRAIN_ACCUMULATE if self.accumulate else 0) | (0 if param_grads else _capi.TRAIN_NO_PARAM_GRADS)
        return _capi.DnSacTrainConfig(self.n_nets, self.n_layers, self.n_parts, _ACTIVATIONS[self.activation][0], self.in0, self.in1, flags, 0)

    def _install(self):
        for p, g in zip(self.params, self.grads):
            if p.grad is not g:
                p.grad = g

    def _views(self, count):
        return tuple(t[:count, 0] if self.squeeze and t.shape[1] == 1 else t[:count] for t in self.outs)

    def __call__(self, x0, x1=None, param_grads=True):
        count = self._rows("x0", x0, self.in0)
        if self.in1:
            self._check("x1", x1, (count, self.in1))
        elif x1 is not None:
            raise ValueError(f"{self._NAME}: x1 was given, but the networks read one tensor (in_split is {(self.in0, self.in1)})")
        if not self.with_grads or not torch.is_grad_enabled():
            self._forward(x0, x1, count)
            return tuple(t.detach() for t in self._views(count))
        param_grads = bool(param_grads)
        if param_grads:
            self._install()
        return _SacTrainFunction.apply(x0, x1, self, count, param_grads, *(self.params if param_grads else ()))

    def _refresh(self):
        for i, m in enumerate(self.modules):           # the parameters are read where they are now: load_state_dict keeps them, .to() does not
            self._table[i].weight, self._table[i].bias = m.weight.data_ptr(), m.bias.data_ptr()

    def _forward(self, x0, x1, count):
        self._refresh()
        scratch = self._scratch_for(self._need)
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_sac_train_forward(C.byref(self._cfg(True)), self._table, x0.data_ptr(), x1.data_ptr() if self.in1 else None,
                                                       count, self._out_table, scratch.data_ptr(), scratch.numel() * 8, self.device.index,
                                                       self._stream()))
        self._calls += 1

    def _backward(self, x0, x1, d_out, count, want0, want1, param_grads):
        if not want0 and not want1 and not param_grads:
            return None, None
        dense = []
        for i, (d, o) in enumerate(zip(d_out, self.outs)):
            d = self._zeros[i][:count] if d is None else d.reshape(count, o.shape[1]).contiguous()
            self._check(f"the gradient of output {i}", d, (count, o.shape[1]))
            dense.append(d)
        table = (C.c_void_p * len(dense))(*[d.data_ptr() for d in dense])
        scratch = self._scratch_for(self._need)
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_sac_train_backward(C.byref(self._cfg(param_grads)), self._table, x0.data_ptr(),
                                                        x1.data_ptr() if self.in1 else None, table, count, self.d_x0.data_ptr() if want0 else None,
                                                        self.d_x1.data_ptr() if want1 else None, scratch.data_ptr(), scratch.numel() * 8,
                                                        self.device.index, self._stream()))
        return (self.d_x0[:count] if want0 else None), (self.d_x1[:count] if want1 else None)

    def __repr__(self):
        sizes = [f"{self.in0}+{self.in1}"] + [str(m.out_features) for m in self.modules[:self.n_layers - 1]] + [str(tuple(self.out_dims))]
        return (f"SacTrainer({self.n_nets} x {'-'.join(sizes)}, {self.activation}, batch_size={self.batch_size}, device={str(self.device)!r}, "
                f"accumulate={self.accumulate}, grads={self.with_grads})")


class PolyakUpdate(DeviceScratch):
    """target_i <- (1 - tau) target_i + tau source_i over up to 32 pairs of float32 tensors in one launch (dn_polyak_update): each element
    is widened to float64, two products and one add, rounded once.  source_params, target_params: the parameters of the critics and of
    their targets, pair by pair, dense, on one GPU; tau a float in [0, 1].  step() reads the tensors where they are now.  Capturable."""
    _NAME, _NOUN = "PolyakUpdate", "parameters"

    def __init__(self, source_params, target_params, tau=0.005, device=None):
        me = self._NAME
        source, target = list(source_params), list(target_params)
        if len(source) != len(target):
            raise ValueError(f"{me}: {len(source)} source tensors against {len(target)} target tensors; they go pair by pair")
        if not 1 <= len(source) <= _capi.ADAM_MAX_TENSORS:
            raise ValueError(f"{me}: a call takes 1..{_capi.ADAM_MAX_TENSORS} tensors, got {len(source)}; make one update per group")
        tau = float(tau)
        if not 0.0 <= tau <= 1.0:
            raise ValueError(f"{me}: tau must be in [0, 1], got {tau!r}")
        for i, (s, t) in enumerate(zip(source, target)):
            for what, p in ((f"source_params[{i}]", s), (f"target_params[{i}]", t)):
                if not isinstance(p, torch.Tensor):
                    raise ValueError(f"{me}: {what} must be a tensor, got {type(p).__name__}")
                if p.dtype != torch.float32:
                    raise ValueError(f"{me}: {what} must be torch.float32, got {p.dtype}")
                if not p.is_contiguous():
                    raise ValueError(f"{me}: {what} must be dense (strides {p.stride()}); the kernel updates it in place")
            if s.shape != t.shape or s.numel() < 1:
                raise ValueError(f"{me}: source_params[{i}] has the shape {list(s.shape)}, target_params[{i}] {list(t.shape)}; a pair has one shape, not empty")
            if s is t or (s.device == t.device and s.data_ptr() == t.data_ptr()):
                raise ValueError(f"{me}: source_params[{i}] is target_params[{i}]; a target is a tensor of its own")
        for i, p in enumerate(source + target):
            if p.device.type != "cuda":
                raise ValueError(f"{me}: {'source' if i < len(source) else 'target'}_params[{i % len(source)}] is on {p.device}; the tensors must be "
                                 "on a GPU, there is no CPU path")
            if p.device != source[0].device:
                raise ValueError(f"{me}: the tensors are on {p.device} and {source[0].device}; one device")
        super().__init__(source[0].device if device is None else device)
        self.source, self.target, self.tau = source, target, tau
        n = len(source)
        self._src, self._dst = (C.c_void_p * n)(), (C.c_void_p * n)()
        self._counts = (C.c_int64 * n)(*[s.numel() for s in source])

    def _refresh(self):
        for i, (s, t) in enumerate(zip(self.source, self.target)):
            self._src[i], self._dst[i] = s.data_ptr(), t.data_ptr()

    def step(self):
        self._refresh()
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_polyak_update(len(self.source), self._src, self._dst, self._counts, self.tau, self.device.index,
                                                   self._stream()))

    def __repr__(self):
        return f"PolyakUpdate({len(self.source)} tensors, tau={self.tau}, device={str(self.device)!r})"
