"""The PPO optimiser step on the device (include/dronenav.h dn_adam_step).

What SB3's PPO.train [from recall] puts between loss.backward() and the next minibatch -- clip_grad_norm_(parameters, max_grad_norm) and
torch.optim.Adam(eps=1e-5).step() -- as one C call of two launches over up to 32 tensors: the global gradient norm in float64 with a
summation order that depends on the tensor sizes alone, the clip coefficient, and Adam's update with every input widened once and every
output rounded once.  The learning rate and the step count live in device memory, so a captured training step follows a schedule.  The
networks' backward and the learner loop stay the caller's.
"""
import ctypes as C
import math

import torch

from . import _capi
from ._fleetnorm import DeviceScratch

STAT_NAMES = ("grad_norm", "clip_coef", "lr", "step")


def _running_product(beta, step):
    """beta ** step as the device forms it: `step` IEEE products in sequence.  The walk ends early where a product no longer moves:
    at 0.0, or at the subnormal that rounds back to itself."""
    c = 1.0
    for _ in range(step):
        nxt = c * beta
        if nxt == c:
            break
        c = nxt
    return c


class ClippedAdam(DeviceScratch):
    """params: an iterable of at most 32 float32, dense leaf tensors on one GPU (net.parameters() works; there is no CPU path); lr, betas,
    eps: torch.optim.Adam's, with SB3's eps; max_grad_norm: the bound of the global gradient norm, None or <= 0 for no clip;
    zero_grads: zero every gradient in the same call, after it is read (zero_grad(set_to_none=False) at no launch of its own).

    step(): the one C call.  Every parameter must have a dense .grad on the device (ValueError otherwise).
    zero_grad(): zeroes the existing gradients in place -- never sets them to None, see below.
    Owned tensors: exp_avg and exp_avg_sq (lists, a tensor per parameter); lr float64 [1], state float64 [4] = (step, beta1 ** step,
    beta2 ** step, 0) with the powers as running products, stats float64 [4] = (grad_norm before the clip, clip_coef, lr, step).
    opt.lr.fill_(x), or set_lr(x), is how a schedule changes the rate, also between replays of a captured graph; stats_dict() copies stats
    to the host.
    Capturable after one eager call (the scratch is made there).  The call captures the addresses of the gradients, so at replay the
    gradients must be the same tensors: copy fresh values into them, and clear them with zero_grad() here, the model's
    zero_grad(set_to_none=False), or zero_grads=True -- not with torch's default zero_grad(), which drops them.
    state_dict() / load_state_dict() use torch.optim.Adam's layout (state[i] = step, exp_avg, exp_avg_sq; param_groups with lr, betas,
    eps), so a checkpoint made by SB3's optimiser continues here and the other way round."""
    _NAME, _NOUN = "ClippedAdam", "the parameters"

    def __init__(self, params, *, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5, zero_grads=False):
        params = list(params)
        top = _capi.ADAM_MAX_TENSORS
        if not 1 <= len(params) <= top:
            raise ValueError(f"ClippedAdam takes 1..{top} tensors, got {len(params)}")
        for i, p in enumerate(params):
            if not isinstance(p, torch.Tensor):
                raise ValueError(f"ClippedAdam: params[{i}] must be a tensor, got {type(p).__name__}")
            if p.dtype != torch.float32:
                raise ValueError(f"ClippedAdam: params[{i}] must be torch.float32, got {p.dtype}")
            if not p.is_contiguous():
                raise ValueError(f"ClippedAdam: params[{i}] must be dense (strides {p.stride()}); the kernel updates it in place")
            if p.numel() < 1:
                raise ValueError(f"ClippedAdam: params[{i}] is empty")
            if not p.is_leaf:
                raise ValueError(f"ClippedAdam: params[{i}] must be a leaf tensor")
        for i, p in enumerate(params):
            if p.device.type != "cuda":
                raise ValueError(f"ClippedAdam: params[{i}] is on {p.device}; the parameters must be on a GPU, there is no CPU path")
            if p.device != params[0].device:
                raise ValueError(f"ClippedAdam: params[{i}] is on {p.device}, params[0] on {params[0].device}; one device a call")
        lr, eps = float(lr), float(eps)
        beta1, beta2 = (float(b) for b in betas)
        if not math.isfinite(lr):
            raise ValueError(f"ClippedAdam.lr must be finite, got {lr!r}")
        for name, b in (("betas[0]", beta1), ("betas[1]", beta2)):
            if not 0.0 <= b < 1.0:
                raise ValueError(f"ClippedAdam.{name} must be in [0, 1), got {b!r}")
        if not (math.isfinite(eps) and eps >= 0.0):
            raise ValueError(f"ClippedAdam.eps must be finite and >= 0, got {eps!r}")
        max_grad_norm = 0.0 if max_grad_norm is None else float(max_grad_norm)
        if not math.isfinite(max_grad_norm):
            raise ValueError(f"ClippedAdam.max_grad_norm must be finite (None or <= 0: no clip), got {max_grad_norm!r}")
        super().__init__(params[0].device)
        self.params, self.betas, self.eps, self.max_grad_norm, self.zero_grads = params, (beta1, beta2), eps, max_grad_norm, bool(zero_grads)
        self.exp_avg = [torch.zeros_like(p) for p in params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in params]
        f64 = dict(dtype=torch.float64, device=self.device)
        self.lr = torch.full((1,), lr, **f64)
        self.state = torch.tensor([0.0, 1.0, 1.0, 0.0], **f64)
        self.stats = torch.zeros(4, **f64)
        n = len(params)
        self._cfg = _capi.DnAdamConfig(beta1, beta2, eps, max_grad_norm, n, _capi.ADAM_ZERO_GRADS if self.zero_grads else 0)
        self._table = (_capi.DnAdamTensor * n)(*[_capi.DnAdamTensor(p.data_ptr(), None, m.data_ptr(), v.data_ptr(), p.numel())
                                                 for p, m, v in zip(params, self.exp_avg, self.exp_avg_sq)])
        self._need = int(self._lib.dn_adam_scratch_bytes((C.c_int64 * n)(*[p.numel() for p in params]), n))

    def step(self):
        table = self._table
        for i, p in enumerate(self.params):
            g = p.grad
            if g is None:
                raise ValueError(f"ClippedAdam.step: params[{i}].grad is None; every parameter takes part in the global norm")
            if g.device != self.device or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape:
                raise ValueError(f"ClippedAdam.step: params[{i}].grad must be dense torch.float32 {list(p.shape)} on {self.device}, got "
                                 f"{g.dtype} {list(g.shape)} on {g.device}, strides {g.stride()}")
            table[i].param, table[i].grad = p.data_ptr(), g.data_ptr()
            table[i].exp_avg, table[i].exp_avg_sq = self.exp_avg[i].data_ptr(), self.exp_avg_sq[i].data_ptr()
        scratch = self._scratch_for(self._need)
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_adam_step(C.byref(self._cfg), table, self.lr.data_ptr(), self.state.data_ptr(), self.stats.data_ptr(),
                                               scratch.data_ptr(), scratch.numel() * 8, self.device.index, self._stream()))

    def zero_grad(self):
        """Zeroes the existing gradients in place; a parameter without one is left without one."""
        grads = [p.grad for p in self.params if p.grad is not None]
        if grads:
            torch._foreach_zero_(grads)

    def set_lr(self, lr):
        self.lr.fill_(float(lr))

    def stats_dict(self):
        """The statistics of the last step on the host: the gradient norm before the clip, the clip coefficient, lr and the step count."""
        return dict(zip(STAT_NAMES, self.stats.cpu().tolist()))

    def state_dict(self):
        step, lr = float(self.state[0]), float(self.lr)
        state = {i: dict(step=torch.tensor(step, dtype=torch.float32), exp_avg=m.clone(), exp_avg_sq=v.clone())
                 for i, (m, v) in enumerate(zip(self.exp_avg, self.exp_avg_sq))} if step > 0 else {}
        group = dict(lr=lr, betas=self.betas, eps=self.eps, weight_decay=0, amsgrad=False, maximize=False, foreach=None, capturable=False,
                     differentiable=False, fused=None, decoupled_weight_decay=False, params=list(range(len(self.params))))
        return dict(state=state, param_groups=[group])

    def load_state_dict(self, sd):
        groups, state = sd["param_groups"], sd["state"]
        n = len(self.params)
        if len(groups) != 1 or len(groups[0]["params"]) != n:
            raise ValueError(f"ClippedAdam.load_state_dict: one parameter group of {n} tensors is wanted, got {len(groups)} group(s) of "
                             f"{[len(g['params']) for g in groups]}")
        g = groups[0]
        if g.get("weight_decay", 0) or g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("ClippedAdam.load_state_dict: weight_decay, amsgrad and maximize are not supported")
        beta1, beta2 = (float(b) for b in g["betas"])
        if (beta1, beta2) != self.betas or float(g["eps"]) != self.eps:
            raise ValueError(f"ClippedAdam.load_state_dict: betas {g['betas']} and eps {g['eps']} of the checkpoint are not this optimiser's "
                             f"{self.betas}, {self.eps}: they are host values of the C call")
        if state and sorted(state) != list(range(n)):
            raise ValueError(f"ClippedAdam.load_state_dict: state must hold the entries 0..{n - 1} or none, got {sorted(state)}")
        steps = {float(s["step"]) for s in state.values()}
        if len(steps) > 1 or any(s < 0 or s != int(s) for s in steps):
            raise ValueError(f"ClippedAdam.load_state_dict: one whole step count for every tensor is wanted, got {sorted(steps)}")
        step = int(steps.pop()) if steps else 0
        for i in range(n):
            for mine, key in ((self.exp_avg[i], "exp_avg"), (self.exp_avg_sq[i], "exp_avg_sq")):
                if state:
                    if tuple(state[i][key].shape) != tuple(mine.shape):
                        raise ValueError(f"ClippedAdam.load_state_dict: state[{i}][{key!r}] has shape {list(state[i][key].shape)}, "
                                         f"params[{i}] {list(mine.shape)}")
                    mine.copy_(state[i][key])
                else:
                    mine.zero_()
        self.lr.fill_(float(g["lr"]))
        self.state.copy_(torch.tensor([float(step), _running_product(beta1, step), _running_product(beta2, step), 0.0], dtype=torch.float64))

    def __repr__(self):
        return (f"ClippedAdam({len(self.params)} tensors, {sum(p.numel() for p in self.params)} elements, device={str(self.device)!r}, "
                f"betas={self.betas}, eps={self.eps:g}, max_grad_norm={self.max_grad_norm:g}, zero_grads={self.zero_grads})")
