"""What the classes that call the env-free kernels share on the Python side.  DeviceScratch (rownorm.RowNormalizer,
retnorm.ReturnNormalizer, minibatch.MinibatchSampler, optim.ClippedAdam, replay.ReplaySampler, and through LossHead ppo.PpoLoss and the
three heads of sac): the device, the stream and the scratch with its capture guard.  FleetNormalizer, what the two fleet-wide normalisers
share beyond that: the clip and epsilon checks and the staging of tensors that are not dense.  LossHead, what the four loss heads share
beyond it: the checks of a constructor count, of the rows of a call and of a tensor by argument name, and the call counter with its
stale-backward refusal.  Shapes, state and the C calls are the classes' own."""
import ctypes as C
import math

import torch

from . import _capi


class DeviceScratch:
    _NAME = _NOUN = None        # the class and its input as the messages name them: "RowNormalizer", "rows"

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"{self._NAME} needs a GPU device, got {device}; there is no CPU path")
        self.device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        self._lib = _capi.load()
        self._scratch = None

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _scratch_for(self, need):
        """The scratch tensor of at least `need` bytes (what dn_*_scratch_bytes answered: <= 0 is its refusal)."""
        if need <= 0:
            _capi.check(int(need))
        if self._scratch is None or self._scratch.numel() * 8 < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self._NAME}: the scratch would have to grow inside a graph capture; call it once with {self._NOUN} of "
                                   "this size before capturing")
            self._scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
        return self._scratch


class LossHead(DeviceScratch):
    """A head keeps batch_size (the most rows of a call) and counts its forward calls in _calls: the autograd functions note the count at
    forward, and _stale refuses a backward that comes after a later forward."""

    def __init__(self, device):
        super().__init__(device)
        self._calls = 0

    def _count(self, name, v, top):
        """A constructor argument that is an integer in 1..top; usable before __init__."""
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= top:
            raise ValueError(f"{self._NAME}.{name} must be an integer in 1..{top}, got {v!r}")

    def _check(self, name, t, shapes):
        """t: a dense float32 tensor on the device of `shapes`, one shape or a list of them."""
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{self._NAME}: {name} must be a tensor, got {type(t).__name__}")
        shapes = shapes if isinstance(shapes, list) else [shapes]
        if tuple(t.shape) not in shapes or t.dtype != torch.float32 or t.device != self.device:
            want = " or ".join(str(list(s)) for s in shapes)
            raise ValueError(f"{self._NAME}: {name} must be torch.float32 {want} on {self.device}, got {t.dtype} {list(t.shape)} on {t.device}")
        if not t.is_contiguous():
            raise ValueError(f"{self._NAME}: {name} must be dense (strides {t.stride()}); the kernel reads it in place and stages nothing")

    def _rows(self, name, t, *cols):
        """count, the rows of a call, from its leading tensor t [count, *cols]: 1..batch_size of them, and t passes _check."""
        if not isinstance(t, torch.Tensor) or t.dim() != 1 + len(cols):
            raise ValueError(f"{self._NAME}: {name} must be a tensor [{', '.join(['count'] + [str(c) for c in cols])}]")
        count = int(t.shape[0])
        if not 1 <= count <= self.batch_size:
            raise ValueError(f"{self._NAME}: {name} has {count} rows; a call takes 1..{self.batch_size} (batch_size)")
        self._check(name, t, (count,) + cols)
        return count

    def _stale(self, ctx):
        if ctx.call != self._calls:
            raise RuntimeError(f"{self._NAME}: backward of call {ctx.call} after call {self._calls}: the gradients live in static buffers that the "
                               "later forward has overwritten; call backward() before the next forward")


class FleetNormalizer(DeviceScratch):
    def __init__(self, device, clip, epsilon):
        clip, epsilon = float(clip), float(epsilon)
        if not clip > 0.0:
            raise ValueError(f"{self._NAME}.clip must be > 0 (math.inf for no clip), got {clip!r}")
        if not epsilon >= 0.0:
            raise ValueError(f"{self._NAME}.epsilon must be >= 0, got {epsilon!r}")
        super().__init__(device)
        self.clip, self.epsilon = clip, epsilon

    def _check_source(self, x):
        if not isinstance(x, torch.Tensor) or x.device != self.device or x.dtype != torch.float32:
            raise ValueError(f"{self._NOUN} must be a float32 tensor on {self.device}; there is no CPU path")

    def _stage(self, x, out, want_out):
        """(out, the dense source, the dense destination): `out` is made when None and wanted; the kernels take dense tensors, so a
        strided source goes through a dense copy, and a strided `out` is written in that copy (or a dense buffer) and filled by _finish."""
        if want_out:
            if out is None:
                out = torch.empty(x.shape, dtype=torch.float32, device=self.device)
            elif not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32 or out.shape != x.shape:
                raise ValueError(f"out must be a float32 tensor of the shape of {self._NOUN} on the same device")
        src = x if x.is_contiguous() else x.contiguous()
        if out is None or out.is_contiguous():
            dst = out
        else:
            dst = src if src is not x else torch.empty(x.shape, dtype=torch.float32, device=self.device)
        return out, src, dst

    @staticmethod
    def _finish(out, dst):
        if out is not None and dst is not out:
            out.copy_(dst)
        return out

    def _clip_text(self):
        return "inf" if math.isinf(self.clip) else f"{self.clip:g}"
