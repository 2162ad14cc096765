"""A fleet-wide running normaliser for policy and critic input rows (include/dronenav.h dn_rownorm).

The 13 observation columns pass through the per-drone NormalizeObservation inside the step kernels; the privileged rows, cat(obs, goal)
and the history rows reach the networks raw -- rotor speeds of order 1e4 beside columns of order 1.  A RowNormalizer keeps ONE
RunningMeanStd over the whole fleet for one kind of row (the arithmetic of Sol/Model/Environments/normalize.py:10-47 with the N rows of a
step as the batch) and normalises the rows with it, in SB3's VecNormalize order [from recall]: update with the step's rows, then normalise
them with the updated statistics; terminal rows are normalised only.  Kernels of their own, after the step; statistics float64 on the
device, so a captured graph keeps them moving.  Each rank keeps its own statistics: there is no collective (at 32 768 drones per rank
they agree closely; a delta-tracking merge is a later change).
"""
import ctypes as C

import torch

from . import _capi
from ._fleetnorm import FleetNormalizer

MAX_WIDTH = 64


class RowNormalizer(FleetNormalizer):
    """width: columns of a row, 1..64; device: a GPU (there is no CPU path); clip: +-clip bounds the output (math.inf: none); epsilon:
    added to the variance.

    update_normalize(rows, out=None): `rows` [N, W] (one step) or [K, N, W] (K steps in sequence: step t is normalised with the statistics
    after steps 0..t) float32 on the device; returns `out` (a new tensor when None; `out=rows` works in place).  normalize(rows, out=None)
    leaves the statistics alone.  update(rows) moves them without an output.  Rows that are not dense (a column slice of a wider buffer)
    are staged through a dense copy: the kernels take dense rows.

    stats: the device float64 tensor [1 + 2 W]: count, mean[W], var[W].  state_dict() / load_state_dict() copy it, so a round trip is exact."""
    _NAME, _NOUN = "RowNormalizer", "rows"

    def __init__(self, width, device, *, clip=10.0, epsilon=1e-8):
        if isinstance(width, bool) or not isinstance(width, int) or not 1 <= width <= MAX_WIDTH:
            raise ValueError(f"RowNormalizer.width must be an integer in 1..{MAX_WIDTH}, got {width!r}")
        super().__init__(device, clip, epsilon)
        self.width = width
        self._cfg = _capi.DnRownormConfig(width, self.clip, self.epsilon)
        self.stats = torch.empty(1 + 2 * width, dtype=torch.float64, device=self.device)
        self.reset()

    def reset(self):
        """count = 1e-4, mean = 0, var = 1 (RunningMeanStd.__init__)."""
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_rownorm_init(C.byref(self._cfg), self.stats.data_ptr(), self.device.index, self._stream()))

    count = property(lambda self: self.stats[0])
    mean = property(lambda self: self.stats[1:1 + self.width])
    var = property(lambda self: self.stats[1 + self.width:])

    def state_dict(self):
        return {"stats": self.stats.clone(), "width": self.width, "clip": self.clip, "epsilon": self.epsilon}

    def load_state_dict(self, state):
        if int(state["width"]) != self.width:
            raise ValueError(f"the state is of width {state['width']}, this normaliser of width {self.width}")
        s = torch.as_tensor(state["stats"])
        if s.dtype != torch.float64 or tuple(s.shape) != tuple(self.stats.shape):
            raise ValueError(f"stats must be float64 [{self.stats.shape[0]}], got {s.dtype} {tuple(s.shape)}")
        self.stats.copy_(s)

    def _run(self, rows, out, update, want_out=True):
        self._check_source(rows)
        if rows.dim() not in (2, 3) or rows.shape[-1] != self.width or rows.numel() == 0:
            raise ValueError(f"rows must be [N, {self.width}] or [K, N, {self.width}] with N >= 1, got {tuple(rows.shape)}")
        k, n = (1, rows.shape[0]) if rows.dim() == 2 else (rows.shape[0], rows.shape[1])
        out, src, dst = self._stage(rows, out, want_out)
        scratch = self._scratch_for(self._lib.dn_rownorm_scratch_bytes(k, n, self.width))
        with torch.cuda.device(self.device):
            _capi.check(self._lib.dn_rownorm(C.byref(self._cfg), self.stats.data_ptr(), k, n, src.data_ptr(),
                                             None if dst is None else dst.data_ptr(), int(update), scratch.data_ptr(), scratch.numel() * 8,
                                             self.device.index, self._stream()))
        return self._finish(out, dst)

    def update_normalize(self, rows, out=None):
        return self._run(rows, out, True)

    def normalize(self, rows, out=None):
        return self._run(rows, out, False)

    def update(self, rows):
        self._run(rows, None, True, want_out=False)

    def __repr__(self):
        return f"RowNormalizer(width={self.width}, device={str(self.device)!r}, clip={self._clip_text()}, epsilon={self.epsilon:g})"
