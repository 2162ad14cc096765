"""The PPO loss head on the device (include/dronenav.h dn_ppo_loss).

SB3's PPO.train body [from recall] between the three head outputs of MlpActorCritic (action_net, log_std, value_net) and the scalar
loss: one C call of two launches maps (action means, log_std, values, a minibatch) to the loss, SB3's logged statistics and the gradients
with respect to the three head outputs, in float64 with a summation order that depends on the batch shape alone.  An autograd function
hands those gradients on, so loss.backward() continues into the caller's networks.  The networks' own forward and backward, the optimiser
and the learner loop stay the caller's.
"""
import ctypes as C
import math

import torch
from torch.autograd.function import once_differentiable

from . import _capi
from ._fleetnorm import LossHead

STAT_NAMES = ("loss", "policy_gradient_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")      # SB3's logger keys; stats[6:8] are 0


class _PpoLossFunction(torch.autograd.Function):
    """forward: the one C call, which also leaves the gradients in the owner's static buffers; backward: those buffers times grad_output."""

    @staticmethod
    def forward(ctx, mean, log_std, values, owner, count, mb):
        owner._launch(mean, log_std, values, count, mb)
        ctx.owner, ctx.count, ctx.call = owner, count, owner._calls
        return owner.loss.view(())

    @staticmethod
    @once_differentiable                               # the stored gradients are plain buffers: there is no double backward
    def backward(ctx, grad_output):
        owner, n = ctx.owner, ctx.count
        owner._stale(ctx)
        return grad_output * owner.d_mean[:n], grad_output * owner.d_log_std, grad_output * owner.d_value[:n], None, None, None


class PpoLoss(LossHead):
    """batch_size: the most rows of a call (SB3's batch_size); act_dim: 1..8 action columns; device: a GPU (there is no CPU path);
    clip_range > 0; clip_range_vf: None (no value clip, SB3's default) or > 0; ent_coef, vf_coef >= 0.  All four are host values: a
    captured graph keeps the ones it was captured with.

    loss = ppo(mean, log_std, values, mb): mean [count, act_dim], log_std [act_dim], values [count], float32, dense, on the device,
    count <= batch_size; mb: what MinibatchSampler.gather returns, or any dict with "actions" [count, act_dim], "log_probs", "advantages",
    "returns" [count] and, with the value clip, "values" [count].  Returns the 0-dim float32 loss, a view of the static `loss` tensor that
    the next call overwrites; loss.backward() hands the stored gradients, times grad_output, to mean, log_std and values.  Backward must
    come before the next forward (RuntimeError otherwise); there is no double backward.
    Static tensors: d_mean [batch_size, act_dim], d_log_std [act_dim], d_value [batch_size], loss [1], log_probs [batch_size] (the new
    log-probabilities, [:count] valid), stats float64 [8] (loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction, 0, 0);
    stats_dict() copies stats to the host under SB3's names.  Capturable after one eager call (the scratch is made there)."""
    _NAME, _NOUN = "PpoLoss", "a minibatch"

    def __init__(self, batch_size, act_dim, device, *, clip_range=0.2, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5):
        self._count("batch_size", batch_size, (1 << 31) - 1)
        self._count("act_dim", act_dim, _capi.PPO_MAX_ACT)
        clip_range = float(clip_range)
        if not (math.isfinite(clip_range) and clip_range > 0.0):
            raise ValueError(f"PpoLoss.clip_range must be finite and > 0, got {clip_range!r}")
        if clip_range_vf is not None:
            clip_range_vf = float(clip_range_vf)
            if not (math.isfinite(clip_range_vf) and clip_range_vf > 0.0):
                raise ValueError(f"PpoLoss.clip_range_vf must be None (no value clip) or finite and > 0, got {clip_range_vf!r}")
        for name, v in (("ent_coef", ent_coef), ("vf_coef", vf_coef)):
            if not (math.isfinite(float(v)) and float(v) >= 0.0):
                raise ValueError(f"PpoLoss.{name} must be finite and >= 0, got {v!r}")
        super().__init__(device)
        self.batch_size, self.act_dim = batch_size, act_dim
        self.clip_range, self.clip_range_vf, self.ent_coef, self.vf_coef = clip_range, clip_range_vf, float(ent_coef), float(vf_coef)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.d_mean, self.d_log_std = torch.zeros((batch_size, act_dim), **f32), torch.zeros(act_dim, **f32)
        self.d_value, self.log_probs, self.loss = torch.zeros(batch_size, **f32), torch.zeros(batch_size, **f32), torch.zeros(1, **f32)
        self.stats = torch.zeros(8, dtype=torch.float64, device=self.device)

    def __call__(self, mean, log_std, values, mb):
        count = self._rows("mean", mean, self.act_dim)
        self._check("log_std", log_std, (self.act_dim,))
        self._check("values", values, (count,))
        need = ("actions", "log_probs", "advantages", "returns") + (("values",) if self.clip_range_vf is not None else ())
        for key in need:
            if not isinstance(mb, dict) or key not in mb:
                raise ValueError(f"PpoLoss: mb[{key!r}] is missing; the minibatch must hold {', '.join(need)}")
            self._check(f"mb[{key!r}]", mb[key], (count, self.act_dim) if key == "actions" else (count,))
        return _PpoLossFunction.apply(mean, log_std, values, self, count, {key: mb[key] for key in need})

    def _launch(self, mean, log_std, values, count, mb):
        cfg = _capi.DnPpoLossConfig(self.clip_range, self.clip_range_vf if self.clip_range_vf is not None else 0.0, self.ent_coef, self.vf_coef,
                                    self.act_dim, 0)
        scratch = self._scratch_for(self._lib.dn_ppo_loss_scratch_bytes(self.batch_size, self.act_dim))     # of a full minibatch: it grows once
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_ppo_loss(C.byref(cfg), count, mean.data_ptr(), log_std.data_ptr(), values.data_ptr(),
                                              mb["actions"].data_ptr(), mb["log_probs"].data_ptr(), mb["advantages"].data_ptr(),
                                              mb["returns"].data_ptr(), mb["values"].data_ptr() if self.clip_range_vf is not None else None,
                                              self.d_mean.data_ptr(), self.d_log_std.data_ptr(), self.d_value.data_ptr(),
                                              self.log_probs.data_ptr(), self.loss.data_ptr(), self.stats.data_ptr(), scratch.data_ptr(),
                                              scratch.numel() * 8, self.device.index, self._stream()))
        self._calls += 1

    def stats_dict(self):
        """The statistics of the last call on the host, under the names SB3's logger gives them (train/...)."""
        return dict(zip(STAT_NAMES, self.stats.cpu().tolist()))

    def __repr__(self):
        return (f"PpoLoss(batch_size={self.batch_size}, act_dim={self.act_dim}, device={str(self.device)!r}, clip_range={self.clip_range:g}, "
                f"clip_range_vf={self.clip_range_vf!r}, ent_coef={self.ent_coef:g}, vf_coef={self.vf_coef:g})")
