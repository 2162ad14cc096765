"""PPO minibatches on the device (include/dronenav.h dn_minibatch).

The reading half of SB3's RolloutBuffer, get(batch_size) [from recall]: swap-and-flatten, one random permutation per epoch, the gathered
minibatches, and PPO's per-minibatch advantage normalisation -- on the step-major [n_steps, N, ...] tensors the collectors return,
without a flattened copy, with a keyed permutation whose bits are pinned (csrc/dn_permute.h) and a float64 normalisation whose summation
order depends on the minibatch's size alone.  Sample s is drone s // n_steps at step s % n_steps, SB3's order.  Kernels of their own; the
learner stays the caller's.  Each rank shuffles its own shard: there is no collective.
"""
import ctypes as C
import math

import torch

from . import _capi
from ._fleetnorm import DeviceScratch

MAX_WIDTH = 64
DTYPES = (torch.float32, torch.int32)


def permutation(m, seed, epoch):
    """pi(0) .. pi(m - 1) of the epoch's keyed permutation of [0, m) as a CPU int64 tensor (dn_minibatch_permutation: host code, needs no
    GPU): sample pi(i) is what slot i of the epoch gathers."""
    out = torch.empty(int(m), dtype=torch.int64)
    _capi.check(_capi.load().dn_minibatch_permutation(_u64("seed", seed), _u64("epoch", epoch), int(m), 0, int(m), out.data_ptr()))
    return out


def _u64(name, v):
    if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 1 << 64:
        raise ValueError(f"MinibatchSampler: {name} must be an integer in [0, 2^64), got {v!r}")
    return v


def _field_spec(name, spec):
    """(trailing shape, dtype, width) of one declared field, or the ValueError that names it."""
    try:
        shape, dtype = spec
        shape = tuple(int(d) for d in shape)
    except (TypeError, ValueError):
        raise ValueError(f"MinibatchSampler: field {name!r} must be (trailing_shape, dtype), got {spec!r}") from None
    if dtype not in DTYPES:
        why = " (one byte a cell: the kernel copies 32-bit words; convert it, or index it with the returned indices)" if dtype == torch.uint8 else ""
        raise ValueError(f"MinibatchSampler: field {name!r} must be float32 or int32, got {dtype}{why}")
    width = math.prod(shape)
    if not 1 <= width <= MAX_WIDTH or any(d < 1 for d in shape):
        raise ValueError(f"MinibatchSampler: field {name!r} has {width} columns a row ({shape}); the kernel takes 1..{MAX_WIDTH}")
    return shape, dtype, width


def _check_tensor(name, t, lead, shape, dtype, device=None):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"MinibatchSampler: field {name!r} must be a tensor, got {type(t).__name__}")
    if tuple(t.shape) != lead + shape or t.dtype != dtype or (device is not None and t.device != device):
        where = "" if device is None else f" on {device}"
        raise ValueError(f"MinibatchSampler: field {name!r} must be {dtype} {list(lead + shape)}{where}, got {t.dtype} {list(t.shape)} on {t.device}")
    if not t.is_contiguous():
        raise ValueError(f"MinibatchSampler: field {name!r} must be dense [n_steps, num_envs, ...] (strides {t.stride()}); the kernel reads it in "
                         "place and stages nothing")


class MinibatchSampler(DeviceScratch):
    """n_steps, num_envs: the rollout's shape, M = n_steps * num_envs samples (<= 2^31 - 1); batch_size: rows of a minibatch (SB3's
    batch_size; the last one of an epoch is shorter); fields: {name: (trailing_shape, dtype)}, dtype float32 or int32, 1..64 columns a row,
    at most 8 fields; device: a GPU (there is no CPU path); seed: the key of the permutations; normalize: the name of the field to normalise
    (PPO's (a - mean) / (std + epsilon) over the minibatch, unbiased std, skipped for a minibatch of one row), or None.

    gather(rollout, epoch, start, count=None, *, indices=None, epoch_offset=None): rows start .. start + count of the epoch's permutation
    (count: up to batch_size, default what is left of the epoch), or the samples `indices` (device int64, start = 0; values outside [0, M)
    are clamped).  `rollout` is the dict collect() returns, or any dict with the declared tensors, dense [n_steps, num_envs, *trailing] on
    the device.  Returns {name: [count, *trailing]} views of the sampler's static output tensors -- the next call overwrites them -- plus
    "indices", the samples taken (int64).  epoch_offset, a device int64 [1], is added to `epoch` on the device: a captured graph that also
    increments it reshuffles on every replay.
    epoch(rollout, epoch): a generator over the minibatches of one epoch.  permutation(epoch): the epoch's samples in order, on the CPU."""
    _NAME, _NOUN = "MinibatchSampler", "a minibatch"

    def __init__(self, n_steps, num_envs, batch_size, fields, device, *, seed=0, normalize="advantages", epsilon=1e-8):
        for name, v in (("n_steps", n_steps), ("num_envs", num_envs), ("batch_size", batch_size)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"MinibatchSampler.{name} must be an integer >= 1, got {v!r}")
        if n_steps * num_envs > (1 << 31) - 1:
            raise ValueError(f"MinibatchSampler: {n_steps} x {num_envs} samples are more than the 2^31 - 1 of a buffer")
        if not isinstance(fields, dict) or not 1 <= len(fields) <= _capi.MINIBATCH_MAX_FIELDS:
            raise ValueError(f"MinibatchSampler.fields must be a dict of 1..{_capi.MINIBATCH_MAX_FIELDS} fields, got "
                             f"{len(fields) if isinstance(fields, dict) else type(fields).__name__}")
        self.fields = {name: _field_spec(name, spec) for name, spec in fields.items()}
        if "indices" in self.fields:
            raise ValueError("MinibatchSampler: 'indices' names the samples a minibatch took and cannot be a field")
        if normalize is not None:
            if normalize not in self.fields:
                raise ValueError(f"MinibatchSampler.normalize names {normalize!r}, which is not a field (None: no normalisation)")
            if self.fields[normalize][1:] != (torch.float32, 1):
                raise ValueError(f"MinibatchSampler.normalize: field {normalize!r} must be float32 with one column a row")
        epsilon = float(epsilon)
        if not epsilon >= 0.0:
            raise ValueError(f"MinibatchSampler.epsilon must be >= 0, got {epsilon!r}")
        self.seed = _u64("seed", seed)
        super().__init__(device)
        self.n_steps, self.num_envs, self.batch_size = n_steps, num_envs, min(batch_size, n_steps * num_envs)
        self.num_samples, self.normalize, self.epsilon = n_steps * num_envs, normalize, epsilon
        self.out = {name: torch.empty((self.batch_size,) + shape, dtype=dtype, device=self.device)
                    for name, (shape, dtype, _) in self.fields.items()}
        self._indices = torch.empty(self.batch_size, dtype=torch.int64, device=self.device)

    @classmethod
    def for_rollout(cls, rollout, batch_size, fields=("obs", "actions", "values", "log_probs", "advantages", "returns"), **kw):
        """The sampler of a rollout dict: shapes, dtypes and the device are read from the named tensors."""
        fields = tuple(fields)
        if not fields:
            raise ValueError("MinibatchSampler.for_rollout: no field is named")
        for name in fields:
            if name not in rollout or not isinstance(rollout[name], torch.Tensor) or rollout[name].dim() < 2:
                raise ValueError(f"MinibatchSampler: field {name!r} must be a tensor [n_steps, num_envs, ...] of the rollout")
        lead = tuple(rollout[fields[0]].shape[:2])
        spec = {name: (tuple(rollout[name].shape[2:]), rollout[name].dtype) for name in fields}
        for name, (shape, dtype) in spec.items():
            _field_spec(name, (shape, dtype))
            _check_tensor(name, rollout[name], lead, shape, dtype)
        kw.setdefault("normalize", "advantages" if "advantages" in fields else None)
        return cls(int(lead[0]), int(lead[1]), batch_size, spec, rollout[fields[0]].device, **kw)

    def permutation(self, epoch):
        return permutation(self.num_samples, self.seed, epoch)

    def gather(self, rollout, epoch, start, count=None, *, indices=None, epoch_offset=None):
        m, dev = self.num_samples, self.device
        if indices is not None:
            if (not isinstance(indices, torch.Tensor) or indices.device != dev or indices.dtype != torch.int64 or indices.dim() != 1
                    or not indices.is_contiguous() or not 1 <= indices.numel() <= self.batch_size):
                raise ValueError(f"indices must be a dense int64 tensor [1..{self.batch_size}] on {dev}")
            if start != 0 or count not in (None, indices.numel()):
                raise ValueError("with indices, start must be 0 and count None or their number")
            count = indices.numel()
        elif count is None:
            count = min(self.batch_size, m - start)
        if isinstance(count, bool) or not isinstance(count, int) or not 1 <= count <= self.batch_size or start < 0 or start + count > m:
            raise ValueError(f"start and count must select 1..{self.batch_size} of the {m} slots of an epoch, got start {start!r}, count {count!r}")
        if epoch_offset is not None and (not isinstance(epoch_offset, torch.Tensor) or epoch_offset.device != dev
                                         or epoch_offset.dtype != torch.int64 or epoch_offset.numel() != 1):
            raise ValueError(f"epoch_offset must be an int64 tensor of one element on {dev}")
        lead = (self.n_steps, self.num_envs)
        fd = (_capi.DnMinibatchField * _capi.MINIBATCH_MAX_FIELDS)()
        for i, (name, (shape, dtype, width)) in enumerate(self.fields.items()):
            if name not in rollout:
                raise ValueError(f"MinibatchSampler: field {name!r} is not in the rollout")
            _check_tensor(name, rollout[name], lead, shape, dtype, dev)
            fd[i] = _capi.DnMinibatchField(rollout[name].data_ptr(), self.out[name].data_ptr(), width, int(name == self.normalize))
        cfg = _capi.DnMinibatchConfig(self.seed, _u64("epoch", epoch), self.epsilon, len(self.fields), 0)
        scratch = self._scratch_for(self._lib.dn_minibatch_scratch_bytes(self.batch_size))      # of a full minibatch: it grows once
        with torch.cuda.device(dev):
            _capi.check(self._lib.dn_minibatch(C.byref(cfg), fd, self.n_steps, self.num_envs, start, count,
                                               None if indices is None else indices.data_ptr(),
                                               None if epoch_offset is None else epoch_offset.data_ptr(), self._indices.data_ptr(),
                                               scratch.data_ptr(), scratch.numel() * 8, dev.index, self._stream()))
        got = {name: t[:count] for name, t in self.out.items()}
        got["indices"] = self._indices[:count]
        return got

    def epoch(self, rollout, epoch, *, epoch_offset=None):
        """The minibatches of one epoch in order: start = 0, batch_size, ...; the last one has what is left.  Every dict holds views of the
        same static tensors: use a minibatch before asking for the next."""
        for start in range(0, self.num_samples, self.batch_size):
            yield self.gather(rollout, epoch, start, epoch_offset=epoch_offset)

    def __repr__(self):
        return (f"MinibatchSampler(n_steps={self.n_steps}, num_envs={self.num_envs}, batch_size={self.batch_size}, fields={list(self.fields)}, "
                f"device={str(self.device)!r}, seed={self.seed}, normalize={self.normalize!r}, epsilon={self.epsilon:g})")
