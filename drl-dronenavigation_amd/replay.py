"""SAC replay minibatches on the device (include/dronenav.h dn_replay_sample).

SB3's ReplayBuffer.sample(batch_size) [from recall] on the buffers the off-policy collector fills: per row a slot and a drone drawn
uniformly with replacement, the gathered transition, the terminal observation where the episode ended, and dones * (1 - timeouts) -- one
launch into static tensors, with a keyed draw whose bits are pinned (csrc/dn_replay_draw.h) and which the host can repeat.  It reads
collector.ReplayBuffer and collector.RingReplayBuffer in place.  A kernel of its own; the learner stays the caller's.  Each rank samples
its own buffer: there is no collective.
"""
import ctypes as C

import torch

from . import _capi
from ._fleetnorm import DeviceScratch
from .collector import ReplayBuffer, RingReplayBuffer

# layout -> the six sources in dn_replay_source's order: (the buffer's attribute, dtype, extra leading rows, has a trailing dimension)
_F32, _U8 = torch.float32, torch.uint8
_SOURCES = {
    _capi.REPLAY_PLAIN: (("obs", _F32, 0, "obs"), ("next_obs", _F32, 0, "obs"), ("actions", _F32, 0, "act"), ("rewards", _F32, 0, None),
                         ("dones", _F32, 0, None), ("timeouts", _F32, 0, None)),
    _capi.REPLAY_RING: (("obs_ring", _F32, 1, "obs"), ("terminal_obs", _F32, 0, "obs"), ("actions", _F32, 0, "act"), ("rewards", _F32, 0, None),
                        ("done_flags", _U8, 0, None), ("timeout_flags", _U8, 0, None)),
}


def _u64(name, v):
    if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 1 << 64:
        raise ValueError(f"ReplaySampler: {name} must be an integer in [0, 2^64), got {v!r}")
    return v


def _count(name, v, most):
    if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= most:
        raise ValueError(f"ReplaySampler: {name} must be an integer in 1..{most}, got {v!r}")
    return v


def window(buffer):
    """(valid, skip) of a buffer as its own sample() reads pos / full: the slots 0 .. valid - 1, or with skip >= 0 (a full ring mid-cycle,
    whose slot `pos` is being replaced) 0 .. valid without slot skip.  valid == 0: the buffer is empty."""
    if isinstance(buffer, RingReplayBuffer) and buffer.full:
        return (buffer.buffer_size - 1, buffer.pos) if buffer.pos else (buffer.buffer_size, -1)
    return (buffer.buffer_size if buffer.full else buffer.pos), -1


class ReplaySampler(DeviceScratch):
    """buffer: a collector.ReplayBuffer or collector.RingReplayBuffer on a GPU (there is no CPU path), read in place; batch_size: the rows
    of the static outputs (SB3's batch_size, or gradient_steps * batch_size: row j does not depend on the number of rows, so one call
    draws that many independent batches); seed: the key of the draws.

    sample(count=None, *, draw=None, indices=None): `count` rows (default batch_size) of draw number `draw` (default: a host counter,
    `self.draw`, which then advances by one) from the window buffer.pos / buffer.full give at the call, or the transitions `indices`
    (device int64 flat indices slot * num_envs + env; out-of-range slots and drones are clamped).  Returns {"obs", "next_obs", "actions",
    "rewards", "dones", "indices"}: views of the sampler's static tensors, which the next call overwrites; rows count.. are left alone.
    Raises RuntimeError on an empty buffer.  draw_offset, a device int64 [1], is added to the draw number on the device: after one eager
    call, sample() can be captured in a graph, and a graph that also increments draw_offset draws afresh on every replay.  A captured
    graph holds the window it was captured with.
    indices(draw, count=None): the flat indices of the same draw on the CPU (dn_replay_indices: host code, needs no GPU)."""
    _NAME, _NOUN = "ReplaySampler", "a batch"

    def __init__(self, buffer, batch_size, *, seed=0):
        if not isinstance(buffer, (ReplayBuffer, RingReplayBuffer)):
            raise TypeError(f"ReplaySampler reads a collector.ReplayBuffer or collector.RingReplayBuffer, got {type(buffer).__name__}")
        self.layout = _capi.REPLAY_RING if isinstance(buffer, RingReplayBuffer) else _capi.REPLAY_PLAIN
        self.batch_size = _count("batch_size", batch_size, (1 << 31) - 1)
        self.seed = _u64("seed", seed)
        first = getattr(buffer, _SOURCES[self.layout][0][0])
        if not isinstance(first, torch.Tensor) or first.dim() != 3:
            raise ValueError(f"ReplaySampler: field {_SOURCES[self.layout][0][0]!r} must be a tensor [slots, num_envs, obs_dim]")
        self.buffer, self.buffer_size, self.num_envs = buffer, int(buffer.buffer_size), int(buffer.num_envs)
        self.obs_dim, self.act_dim = int(first.shape[2]), int(buffer.actions.shape[-1]) if isinstance(buffer.actions, torch.Tensor) else 0
        if not 1 <= self.obs_dim <= _capi.REPLAY_MAX_OBS or not 1 <= self.act_dim <= _capi.REPLAY_MAX_ACT:
            raise ValueError(f"ReplaySampler: rows of {self.obs_dim} observation and {self.act_dim} action columns; the kernel takes "
                             f"1..{_capi.REPLAY_MAX_OBS} and 1..{_capi.REPLAY_MAX_ACT}")
        self._sources(first.device)
        super().__init__(first.device)
        f32, dev, b = torch.float32, self.device, self.batch_size
        self.out = dict(obs=torch.empty((b, self.obs_dim), dtype=f32, device=dev), next_obs=torch.empty((b, self.obs_dim), dtype=f32, device=dev),
                        actions=torch.empty((b, self.act_dim), dtype=f32, device=dev), rewards=torch.empty(b, dtype=f32, device=dev),
                        dones=torch.empty(b, dtype=f32, device=dev), indices=torch.empty(b, dtype=torch.int64, device=dev))
        self.draw_offset = torch.zeros(1, dtype=torch.int64, device=dev)
        self.draw = 0

    def _sources(self, device):
        """dn_replay_source of the buffer's tensors as they are now, each checked: dtype, device, shape, density."""
        ptrs = []
        for name, dtype, extra, trailing in _SOURCES[self.layout]:
            t = getattr(self.buffer, name)
            shape = (self.buffer_size + extra, self.num_envs) + ({"obs": (self.obs_dim,), "act": (self.act_dim,), None: ()}[trailing])
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"ReplaySampler: field {name!r} must be a tensor, got {type(t).__name__}")
            if tuple(t.shape) != shape or t.dtype != dtype or t.device != device:
                raise ValueError(f"ReplaySampler: field {name!r} must be {dtype} {list(shape)} on {device}, got {t.dtype} {list(t.shape)} on {t.device}")
            if not t.is_contiguous():
                raise ValueError(f"ReplaySampler: field {name!r} must be dense (strides {t.stride()}); the kernel reads it in place and stages nothing")
            ptrs.append(t.data_ptr())
        return _capi.DnReplaySource(*ptrs)

    def _window(self):
        valid, skip = window(self.buffer)
        if valid == 0:
            raise RuntimeError("the replay buffer is empty")
        return valid, skip

    def indices(self, draw, count=None):
        count = self.batch_size if count is None else _count("count", count, self.batch_size)
        valid, skip = self._window()
        out = torch.empty(count, dtype=torch.int64)
        _capi.check(self._lib.dn_replay_indices(self.seed, _u64("draw", draw), valid, self.num_envs, skip, 0, count, out.data_ptr()))
        return out

    def sample(self, count=None, *, draw=None, indices=None):
        dev = self.device
        if indices is not None:
            if (not isinstance(indices, torch.Tensor) or indices.device != dev or indices.dtype != torch.int64 or indices.dim() != 1
                    or not indices.is_contiguous() or not 1 <= indices.numel() <= self.batch_size):
                raise ValueError(f"indices must be a dense int64 tensor [1..{self.batch_size}] on {dev}")
            if draw is not None or count not in (None, indices.numel()):
                raise ValueError("with indices, draw must be None and count None or their number")
            count = indices.numel()
        count = self.batch_size if count is None else _count("count", count, self.batch_size)
        valid, skip = self._window()
        src = self._sources(dev)
        if indices is None:
            if draw is None:
                draw, self.draw = self.draw, (self.draw + 1) & ((1 << 64) - 1)
            _u64("draw", draw)
        cfg = _capi.DnReplayConfig(self.seed, draw or 0, self.buffer_size, self.num_envs, valid, skip, self.obs_dim, self.act_dim, self.layout, 0)
        o = self.out
        with torch.cuda.device(dev):
            _capi.check(self._lib.dn_replay_sample(C.byref(cfg), C.byref(src), count, None if indices is None else indices.data_ptr(),
                                                   self.draw_offset.data_ptr() if indices is None else None, o["obs"].data_ptr(),
                                                   o["next_obs"].data_ptr(), o["actions"].data_ptr(), o["rewards"].data_ptr(),
                                                   o["dones"].data_ptr(), o["indices"].data_ptr(), dev.index, self._stream()))
        return {k: v[:count] for k, v in o.items()}

    def __repr__(self):
        return (f"ReplaySampler({type(self.buffer).__name__}(buffer_size={self.buffer_size}, num_envs={self.num_envs}), batch_size={self.batch_size}, "
                f"device={str(self.device)!r}, seed={self.seed})")
