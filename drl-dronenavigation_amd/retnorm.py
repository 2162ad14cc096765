"""A fleet-wide running return normaliser for rewards (include/dronenav.h dn_retnorm).

The reward half of SB3's VecNormalize (norm_reward=True) [from recall]: one discounted return per drone, ONE RunningMeanStd of those returns
over the whole fleet (the arithmetic of Sol/Model/Environments/normalize.py:10-47 with the N returns of a step as the batch), and the
reward divided by the returns' standard deviation.  Per step: returns = returns * gamma + r; the statistics are updated with the N
returns; out = clip(r / sqrt(var + epsilon), +-clip) with the updated variance (no mean is subtracted); returns = 0 where done.  Kernels
of their own, after the step; statistics and returns float64 on the device, so a captured graph keeps them moving.  The reference's
per-drone NormalizeReward (norm_rew) keeps one statistic per drone and runs inside the one-wave option kernel; this one leaves the step
kernels alone.  Each rank keeps its own statistics: there is no collective.
"""
import ctypes as C

import torch

from . import _capi
from ._fleetnorm import FleetNormalizer


class ReturnNormalizer(FleetNormalizer):
    """num_envs: the fleet; device: a GPU (there is no CPU path); gamma: the discount of the returns, the normaliser's own (SB3's default
    0.99); clip: +-clip bounds the output (math.inf: none); epsilon: added to the variance.

    update_normalize(rewards, dones, out=None): `rewards` [N] (one step) or [K, N] (K steps in sequence: step t is scaled with the
    statistics after steps 0..t) float32 and `dones` uint8 of the same shape, on the device; returns `out` (a new tensor when None;
    `out=rewards` works in place).  normalize(rewards, out=None) leaves statistics and returns alone (evaluation).  update(rewards, dones)
    moves them without an output.  Tensors that are not dense are staged through a dense copy.

    stats: the device float64 tensor [3]: count, mean, var.  returns: the device float64 tensor [N].  state_dict() / load_state_dict()
    copy both, so a round trip is exact.  reset() is RunningMeanStd.__init__ and zero returns; reset_returns() zeroes the returns only."""
    _NAME, _NOUN = "ReturnNormalizer", "rewards"

    def __init__(self, num_envs, device, *, gamma=0.99, clip=10.0, epsilon=1e-8):
        if isinstance(num_envs, bool) or not isinstance(num_envs, int) or num_envs < 1:
            raise ValueError(f"ReturnNormalizer.num_envs must be an integer >= 1, got {num_envs!r}")
        gamma, clip, epsilon = float(gamma), float(clip), float(epsilon)
        if not 0.0 <= gamma <= 1.0:
            raise ValueError(f"ReturnNormalizer.gamma must be in [0, 1], got {gamma!r}")
        super().__init__(device, clip, epsilon)
        self.num_envs, self.gamma = num_envs, gamma
        self._cfg = _capi.DnRetnormConfig(gamma, epsilon, clip, 0)
        self.stats = torch.empty(3, dtype=torch.float64, device=self.device)
        self.returns = torch.empty(num_envs, dtype=torch.float64, device=self.device)
        self.reset()

    def _init(self, stats):
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_retnorm_init(self.stats.data_ptr() if stats else None, self.returns.data_ptr(), self.num_envs,
                                                  self.device.index, self._stream()))

    def reset(self):
        """count = 1e-4, mean = 0, var = 1 (RunningMeanStd.__init__) and returns = 0."""
        self._init(True)

    def reset_returns(self):
        """returns = 0; the statistics stay (VecNormalize.reset [from recall])."""
        self._init(False)

    count = property(lambda self: self.stats[0])
    mean = property(lambda self: self.stats[1])
    var = property(lambda self: self.stats[2])

    def state_dict(self):
        return {"stats": self.stats.clone(), "returns": self.returns.clone(), "num_envs": self.num_envs, "gamma": self.gamma,
                "clip": self.clip, "epsilon": self.epsilon}

    def load_state_dict(self, state):
        if int(state["num_envs"]) != self.num_envs:
            raise ValueError(f"the state is of {state['num_envs']} envs, this normaliser of {self.num_envs}")
        for name, mine in (("stats", self.stats), ("returns", self.returns)):
            s = torch.as_tensor(state[name])
            if s.dtype != torch.float64 or tuple(s.shape) != tuple(mine.shape):
                raise ValueError(f"{name} must be float64 [{mine.shape[0]}], got {s.dtype} {tuple(s.shape)}")
        self.stats.copy_(torch.as_tensor(state["stats"]))
        self.returns.copy_(torch.as_tensor(state["returns"]))

    def _run(self, rewards, dones, out, update, want_out=True):
        n = self.num_envs
        self._check_source(rewards)
        if rewards.dim() not in (1, 2) or rewards.shape[-1] != n or rewards.numel() == 0:
            raise ValueError(f"rewards must be [{n}] or [K, {n}] with K >= 1, got {tuple(rewards.shape)}")
        k = 1 if rewards.dim() == 1 else rewards.shape[0]
        if update and (not isinstance(dones, torch.Tensor) or dones.device != self.device or dones.dtype != torch.uint8
                       or dones.shape != rewards.shape):
            raise ValueError("dones must be a uint8 tensor of the shape of rewards on the same device")
        out, src, dst = self._stage(rewards, out, want_out)
        flags = scratch = None
        if update:
            flags = dones if dones.is_contiguous() else dones.contiguous()
            scratch = self._scratch_for(self._lib.dn_retnorm_scratch_bytes(k, n))
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_retnorm(C.byref(self._cfg), self.stats.data_ptr(), self.returns.data_ptr(), k, n, src.data_ptr(),
                                             None if flags is None else flags.data_ptr(), None if dst is None else dst.data_ptr(),
                                             int(update), None if scratch is None else scratch.data_ptr(),
                                             0 if scratch is None else scratch.numel() * 8, self.device.index, self._stream()))
        return self._finish(out, dst)

    def update_normalize(self, rewards, dones, out=None):
        return self._run(rewards, dones, out, True)

    def normalize(self, rewards, out=None):
        return self._run(rewards, None, out, False)

    def update(self, rewards, dones):
        self._run(rewards, dones, None, True, want_out=False)

    def __repr__(self):
        return (f"ReturnNormalizer(num_envs={self.num_envs}, device={str(self.device)!r}, gamma={self.gamma:g}, clip={self._clip_text()}, "
                f"epsilon={self.epsilon:g})")
