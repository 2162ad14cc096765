"""The SAC loss heads on the device (include/dronenav.h dn_sac_policy, dn_sac_policy_backward, dn_sac_critic_loss, dn_sac_actor_loss).

SB3's SAC.train body [from recall] between the networks' head outputs and the scalar losses: SacPolicyHead is the squashed Gaussian's
reparametrised sample with its log-probability, SacCriticLoss the TD target and the critics' loss, SacActorLoss the actor loss and the
entropy-coefficient loss -- each a small C call of plain launches, in float64 with a summation order that depends on the shapes alone.
Autograd functions hand the gradients on, so critic_loss.backward() and actor_loss.backward() continue into the caller's networks.  The
networks' own forward and backward, the optimisers (optim.ClippedAdam(eps=1e-8, max_grad_norm=None)), the Polyak update and the learner
loop stay the caller's.
"""
import ctypes as C
import math

import torch
from torch.autograd.function import once_differentiable

from . import _capi
from ._fleetnorm import LossHead

CRITIC_STAT_NAMES = ("critic_loss", "ent_coef", "target_q_mean")       # then q_mean_0 .. q_mean_{n_critics - 1}; SB3's logger keys first
ACTOR_STAT_NAMES = ("actor_loss", "ent_coef_loss", "ent_coef", "log_prob_mean", "q_pi_min_mean")


def _ent_coef(cls, v):
    """None = a learned coefficient (log_ent_coef is read on the device); else SB3's fixed one."""
    if v is None:
        return None
    v = float(v)
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"{cls}.ent_coef must be None (learned: log_ent_coef is read) or finite and >= 0, got {v!r}")
    return v


class _SacHead(LossHead):
    """What the three heads share beyond LossHead: the checks of a list of per-critic tensors and of log_ent_coef, and the table of
    per-critic pointers."""

    def _check_list(self, name, ts, count):
        if not isinstance(ts, (list, tuple)) or len(ts) != self.n_critics:
            raise ValueError(f"{self._NAME}: {name} must be a list of {self.n_critics} tensors (n_critics), got {type(ts).__name__}"
                             + (f" of {len(ts)}" if isinstance(ts, (list, tuple)) else ""))
        for c, t in enumerate(ts):
            self._check(f"{name}[{c}]", t, [(count,), (count, 1)])

    def _check_log_ent_coef(self, log_ent_coef):
        if self.ent_coef is None:
            if log_ent_coef is None:
                raise ValueError(f"{self._NAME}: log_ent_coef is required: the coefficient is learned (ent_coef=None)")
            self._check("log_ent_coef", log_ent_coef, [(1,), ()])
        elif log_ent_coef is not None:
            raise ValueError(f"{self._NAME}: log_ent_coef must be None with the fixed ent_coef={self.ent_coef:g}")

    @staticmethod
    def _table(tensors):
        return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


# ---- the squashed policy head ------------------------------------------------------------------------------------------------------------
class _SacPolicyFunction(torch.autograd.Function):
    """forward: the one C call into the owner's static outputs; backward: the one backward call, which recomputes from the saved inputs."""

    @staticmethod
    def forward(ctx, mean, log_std, noise, owner, count):
        owner._forward(mean, log_std, noise, count)
        ctx.save_for_backward(mean, log_std, noise)
        ctx.owner, ctx.count, ctx.call = owner, count, owner._calls
        ctx.set_materialize_grads(False)               # an output nobody used has no gradient: NULL, which the kernel reads as zero
        return owner.actions[:count], owner.log_prob[:count]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_actions, g_log_prob):
        owner, n = ctx.owner, ctx.count
        owner._stale(ctx)
        mean, log_std, noise = ctx.saved_tensors
        owner._backward(mean, log_std, noise, g_actions, g_log_prob, n)
        # copies: autograd may keep what it is handed as a leaf's .grad, and the static buffers are the next call's
        return owner.d_mean[:n].clone(), owner.d_log_std[:n].clone(), None, None, None


class SacPolicyHead(_SacHead):
    """batch_size: the most rows of a call; act_dim: 1..8 action columns; device: a GPU (there is no CPU path); log_std_min < log_std_max:
    the clamp of the log_std head (SB3's -20, 2).  Host values: a captured graph keeps the ones it was captured with.

    actions, log_prob = head(mean, log_std, noise): mean, log_std (the head's raw output, before the clamp) and noise (the caller's
    torch.randn draw) [count, act_dim], float32, dense, on the device, count <= batch_size.  actions [count, act_dim] in (-1, 1) and
    log_prob [count] are views of the static `actions` and `log_prob` tensors, which the next call overwrites.  Differentiable in mean and
    log_std: backward makes one C call, which recomputes the element from the saved inputs (nothing is kept in float32 between forward and
    backward), into the static d_mean and d_log_std [batch_size, act_dim], and hands copies of them on.  Backward must come before the next
    forward (RuntimeError otherwise); there is no double backward.
    One SAC gradient step needs TWO instances: one for obs, whose outputs carry the gradient, and one for next_obs (under no_grad), whose
    outputs are still read while the first one's backward runs.  Capturable."""
    _NAME, _NOUN = "SacPolicyHead", "a batch"

    def __init__(self, batch_size, act_dim, device, *, log_std_min=-20.0, log_std_max=2.0):
        self._count("batch_size", batch_size, (1 << 31) - 1)
        self._count("act_dim", act_dim, _capi.SAC_MAX_ACT)
        log_std_min, log_std_max = float(log_std_min), float(log_std_max)
        if not (math.isfinite(log_std_min) and math.isfinite(log_std_max) and log_std_min < log_std_max):
            raise ValueError(f"SacPolicyHead.log_std_min and log_std_max must be finite with log_std_min < log_std_max, got {log_std_min!r}, {log_std_max!r}")
        super().__init__(device)
        self.batch_size, self.act_dim, self.log_std_min, self.log_std_max = batch_size, act_dim, log_std_min, log_std_max
        f32 = dict(dtype=torch.float32, device=self.device)
        self.actions, self.log_prob = torch.zeros((batch_size, act_dim), **f32), torch.zeros(batch_size, **f32)
        self.d_mean, self.d_log_std = torch.zeros((batch_size, act_dim), **f32), torch.zeros((batch_size, act_dim), **f32)

    def _cfg(self):
        return _capi.DnSacConfig(0.0, 0.0, 0.0, self.log_std_min, self.log_std_max, self.act_dim, 1, 0)

    def __call__(self, mean, log_std, noise):
        count = self._rows("mean", mean, self.act_dim)
        for name, t in (("log_std", log_std), ("noise", noise)):
            self._check(name, t, (count, self.act_dim))
        return _SacPolicyFunction.apply(mean, log_std, noise, self, count)

    def _forward(self, mean, log_std, noise, count):
        cfg = self._cfg()
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_sac_policy(C.byref(cfg), count, mean.data_ptr(), log_std.data_ptr(), noise.data_ptr(), self.actions.data_ptr(),
                                                self.log_prob.data_ptr(), self.device.index, self._stream()))
        self._calls += 1

    def _backward(self, mean, log_std, noise, g_actions, g_log_prob, count):
        cfg = self._cfg()
        g_actions = None if g_actions is None else g_actions.contiguous()
        g_log_prob = None if g_log_prob is None else g_log_prob.contiguous()
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_sac_policy_backward(C.byref(cfg), count, mean.data_ptr(), log_std.data_ptr(), noise.data_ptr(),
                                                         None if g_actions is None else g_actions.data_ptr(),
                                                         None if g_log_prob is None else g_log_prob.data_ptr(), self.d_mean.data_ptr(),
                                                         self.d_log_std.data_ptr(), self.device.index, self._stream()))

    def __repr__(self):
        return (f"SacPolicyHead(batch_size={self.batch_size}, act_dim={self.act_dim}, device={str(self.device)!r}, log_std_min={self.log_std_min:g}, "
                f"log_std_max={self.log_std_max:g})")


# ---- the critic loss ---------------------------------------------------------------------------------------------------------------------
class _SacCriticFunction(torch.autograd.Function):
    """forward: the one C call, which also leaves d_q_c in the owner's static buffers; backward: those buffers times grad_output."""

    @staticmethod
    def forward(ctx, owner, count, rest, *q):
        owner._launch(q, count, *rest)
        ctx.owner, ctx.count, ctx.call, ctx.shapes = owner, count, owner._calls, [t.shape for t in q]
        return owner.loss.view(())

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        owner, n = ctx.owner, ctx.count
        owner._stale(ctx)
        return (None, None, None) + tuple((grad_output * owner.d_q[c, :n]).view(s) for c, s in enumerate(ctx.shapes))


class SacCriticLoss(_SacHead):
    """batch_size: the most rows of a call; device: a GPU (there is no CPU path); n_critics: 1..4 (SB3's 2); gamma in [0, 1]; ent_coef: None =
    learned (log_ent_coef, a float32 tensor [1] on the device, is read by the kernel when it runs) or SB3's fixed coefficient >= 0.

    loss = crit(q_list, next_q_list, next_log_prob, batch, log_ent_coef=None): q_list the n_critics outputs Q_c(obs, actions), next_q_list
    the target critics' Qtarget_c(next_obs, a_next), each [count] or dense [count, 1]; next_log_prob [count]; batch what
    ReplaySampler.sample() returns, of which "rewards" and "dones" [count] are read.  Returns the 0-dim float32
    critic_loss = 0.5 sum_c mean((q_c - y)^2), y = rewards + (1 - dones) gamma (min_c next_q_c - alpha next_log_prob): a view of the static
    `loss` that the next call overwrites; loss.backward() hands d_q_c = (q_c - y) / count, times grad_output, to each q_c.  The target
    side gets no gradient, as under SB3's no_grad.  Backward must come before the next forward; there is no double backward.
    Static tensors: d_q [n_critics, batch_size], target_q [batch_size] (float32(y), for logging), loss [1], stats float64 [8]
    (critic_loss, ent_coef, mean y, mean q_0 .. q_3, 0); stats_dict() copies them to the host.  alpha is read when the kernel runs: a
    caller who steps the coefficient's optimiser after the actor loss reproduces SB3's order.  Capturable after one eager call."""
    _NAME, _NOUN = "SacCriticLoss", "a batch"

    def __init__(self, batch_size, device, *, n_critics=2, gamma=0.99, ent_coef=None):
        self._count("batch_size", batch_size, (1 << 31) - 1)
        self._count("n_critics", n_critics, _capi.SAC_MAX_CRITICS)
        gamma = float(gamma)
        if not (math.isfinite(gamma) and 0.0 <= gamma <= 1.0):
            raise ValueError(f"SacCriticLoss.gamma must be finite and in [0, 1], got {gamma!r}")
        ent_coef = _ent_coef("SacCriticLoss", ent_coef)
        super().__init__(device)
        self.batch_size, self.n_critics, self.gamma, self.ent_coef = batch_size, n_critics, gamma, ent_coef
        f32 = dict(dtype=torch.float32, device=self.device)
        self.d_q, self.target_q, self.loss = torch.zeros((n_critics, batch_size), **f32), torch.zeros(batch_size, **f32), torch.zeros(1, **f32)
        self.stats = torch.zeros(8, dtype=torch.float64, device=self.device)

    def __call__(self, q_list, next_q_list, next_log_prob, batch, log_ent_coef=None):
        count = self._rows("next_log_prob", next_log_prob)
        self._check_list("q_list", q_list, count)
        self._check_list("next_q_list", next_q_list, count)
        for key in ("rewards", "dones"):
            if not isinstance(batch, dict) or key not in batch:
                raise ValueError(f"SacCriticLoss: batch[{key!r}] is missing; the batch must hold rewards, dones")
            self._check(f"batch[{key!r}]", batch[key], (count,))
        self._check_log_ent_coef(log_ent_coef)
        rest = (tuple(t.detach() for t in next_q_list), next_log_prob.detach(), batch["rewards"], batch["dones"], log_ent_coef)
        return _SacCriticFunction.apply(self, count, rest, *q_list)

    def _launch(self, q, count, next_q, next_log_prob, rewards, dones, log_ent_coef):
        C_ = self.n_critics
        cfg = _capi.DnSacConfig(self.gamma, 0.0, self.ent_coef if self.ent_coef is not None else 0.0, 0.0, 0.0, 1, C_, 0)
        scratch = self._scratch_for(self._lib.dn_sac_loss_scratch_bytes(self.batch_size, C_))       # of a full batch: it grows once
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_sac_critic_loss(C.byref(cfg), count, self._table(q), self._table(next_q), next_log_prob.data_ptr(),
                                                     rewards.data_ptr(), dones.data_ptr(), None if log_ent_coef is None else log_ent_coef.data_ptr(),
                                                     self._table([self.d_q[c] for c in range(C_)]), self.target_q.data_ptr(), self.loss.data_ptr(),
                                                     self.stats.data_ptr(), scratch.data_ptr(), scratch.numel() * 8, self.device.index,
                                                     self._stream()))
        self._calls += 1

    def stats_dict(self):
        """The statistics of the last call on the host: SB3's logger names (train/critic_loss, train/ent_coef), the mean target and the mean
        of each critic's Q values."""
        s = self.stats.cpu().tolist()
        return dict(zip(CRITIC_STAT_NAMES + tuple(f"q_mean_{c}" for c in range(self.n_critics)), s[:3 + self.n_critics]))

    def __repr__(self):
        return (f"SacCriticLoss(batch_size={self.batch_size}, device={str(self.device)!r}, n_critics={self.n_critics}, gamma={self.gamma:g}, "
                f"ent_coef={self.ent_coef!r})")


# ---- the actor and entropy-coefficient loss ----------------------------------------------------------------------------------------------
class _SacActorFunction(torch.autograd.Function):
    """forward: the one C call, which also leaves the gradients in the owner's static buffers; backward: those buffers times the two
    grad_outputs."""

    @staticmethod
    def forward(ctx, owner, count, log_prob, log_ent_coef, *q_pi):
        owner._launch(log_prob, log_ent_coef, q_pi, count)
        ctx.owner, ctx.count, ctx.call, ctx.shapes = owner, count, owner._calls, [t.shape for t in q_pi]
        ctx.learned = log_ent_coef is not None
        ctx.coef_shape = log_ent_coef.shape if ctx.learned else None
        ctx.set_materialize_grads(False)
        actor_loss, ent_coef_loss = owner.actor_loss.view(()), owner.ent_coef_loss.view(())
        if not ctx.learned:
            ctx.mark_non_differentiable(ent_coef_loss)
        return actor_loss, ent_coef_loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g_actor, g_ent):
        owner, n = ctx.owner, ctx.count
        owner._stale(ctx)
        d_lp = None if g_actor is None else g_actor * owner.d_log_prob[:n]
        d_q = tuple(None if g_actor is None else (g_actor * owner.d_q_pi[c, :n]).view(s) for c, s in enumerate(ctx.shapes))
        d_coef = None if g_ent is None or not ctx.learned else (g_ent * owner.d_log_ent_coef).view(ctx.coef_shape)
        return (None, None, d_lp, d_coef) + d_q


class SacActorLoss(_SacHead):
    """batch_size: the most rows of a call; device: a GPU (there is no CPU path); n_critics: 1..4; target_entropy: finite (SB3's "auto" is
    -act_dim); ent_coef: None = learned (log_ent_coef [1] on the device is read by the kernel) or SB3's fixed coefficient >= 0.

    actor_loss, ent_coef_loss = act(log_prob, q_pi_list, log_ent_coef=None): log_prob [count] of SacPolicyHead on obs; q_pi_list the
    n_critics outputs Q_c(obs, a_pi), each [count] or dense [count, 1].  Two 0-dim float32 views of static tensors that the next call
    overwrites: actor_loss = mean(alpha log_prob - min_c q_pi_c) with alpha = exp(log_ent_coef) detached, and
    ent_coef_loss = -log_ent_coef mean(log_prob + target_entropy) with log_prob detached (0, without gradient, for a fixed coefficient).
    actor_loss.backward() hands alpha / count to log_prob and -1 / count to the smallest q_pi_c of each row (a tie: the lowest c);
    ent_coef_loss.backward() hands -mean(log_prob + target_entropy) to log_ent_coef; (actor_loss + ent_coef_loss).backward() does both.
    Backward must come before the next forward; there is no double backward.
    Static tensors: d_log_prob [batch_size], d_q_pi [n_critics, batch_size], d_log_ent_coef [1], actor_loss [1], ent_coef_loss [1], stats
    float64 [8] (actor_loss, ent_coef_loss, ent_coef, mean log_prob, mean min_c q_pi_c, d_log_ent_coef, 0, 0); stats_dict() copies them
    to the host.  alpha is read when the kernel runs: a caller who steps the coefficient's optimiser after this loss reproduces SB3's order.
    Capturable after one eager call."""
    _NAME, _NOUN = "SacActorLoss", "a batch"

    def __init__(self, batch_size, device, *, n_critics=2, target_entropy, ent_coef=None):
        self._count("batch_size", batch_size, (1 << 31) - 1)
        self._count("n_critics", n_critics, _capi.SAC_MAX_CRITICS)
        target_entropy = float(target_entropy)
        if not math.isfinite(target_entropy):
            raise ValueError(f"SacActorLoss.target_entropy must be finite, got {target_entropy!r}")
        ent_coef = _ent_coef("SacActorLoss", ent_coef)
        super().__init__(device)
        self.batch_size, self.n_critics, self.target_entropy, self.ent_coef = batch_size, n_critics, target_entropy, ent_coef
        f32 = dict(dtype=torch.float32, device=self.device)
        self.d_log_prob, self.d_q_pi = torch.zeros(batch_size, **f32), torch.zeros((n_critics, batch_size), **f32)
        self.d_log_ent_coef, self.actor_loss, self.ent_coef_loss = torch.zeros(1, **f32), torch.zeros(1, **f32), torch.zeros(1, **f32)
        self.stats = torch.zeros(8, dtype=torch.float64, device=self.device)

    def __call__(self, log_prob, q_pi_list, log_ent_coef=None):
        count = self._rows("log_prob", log_prob)
        self._check_list("q_pi_list", q_pi_list, count)
        self._check_log_ent_coef(log_ent_coef)
        return _SacActorFunction.apply(self, count, log_prob, log_ent_coef, *q_pi_list)

    def _launch(self, log_prob, log_ent_coef, q_pi, count):
        C_ = self.n_critics
        cfg = _capi.DnSacConfig(0.0, self.target_entropy, self.ent_coef if self.ent_coef is not None else 0.0, 0.0, 0.0, 1, C_, 0)
        scratch = self._scratch_for(self._lib.dn_sac_loss_scratch_bytes(self.batch_size, C_))       # of a full batch: it grows once
        learned = log_ent_coef is not None
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_sac_actor_loss(C.byref(cfg), count, log_prob.data_ptr(), self._table(q_pi),
                                                    log_ent_coef.data_ptr() if learned else None, self.d_log_prob.data_ptr(),
                                                    self._table([self.d_q_pi[c] for c in range(C_)]),
                                                    self.d_log_ent_coef.data_ptr() if learned else None, self.actor_loss.data_ptr(),
                                                    self.ent_coef_loss.data_ptr(), self.stats.data_ptr(), scratch.data_ptr(), scratch.numel() * 8,
                                                    self.device.index, self._stream()))
        self._calls += 1

    def stats_dict(self):
        """The statistics of the last call on the host: SB3's logger names (train/actor_loss, train/ent_coef_loss, train/ent_coef), the mean
        log-probability and the mean of the smallest Q value."""
        return dict(zip(ACTOR_STAT_NAMES, self.stats.cpu().tolist()))

    def __repr__(self):
        return (f"SacActorLoss(batch_size={self.batch_size}, device={str(self.device)!r}, n_critics={self.n_critics}, "
                f"target_entropy={self.target_entropy:g}, ent_coef={self.ent_coef!r})")
