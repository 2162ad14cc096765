"""What the tests of the networks' training pass share (tests/test_mlp_train_cpu.py, tests/test_gpu_mlp_train.py): the networks and batches
of the issue, the float64 reference through torch autograd on the CPU (computed once per case), the scratch formula restated, and the
ctypes tables of a call.  A plain module like tests/mlp_support.py -- pytest does not collect it."""
import ctypes as C
import functools

import torch

import mlp_support as ms

R = 1024                                 # DN_MLP_TRAIN_CHUNK, restated: test_mlp_train_cpu.py holds it to the header
BOUND = 1e-4                             # the project's float32-grade bar (dn_mlp_forward grade 1)

WIDTHS = (16, 17, 32, 48, 49, 64)        # layer-0 widths beside 13: both sides of the 16-column K-step and of the 32-column staged step
NETS = ((13, 512, 512, 256, 4), (13, 512, 512, 256, 1), (52, 512, 512, 256, 1), (21, 512, 512, 256, 4), (64, 32, 32), (1, 32, 1),
        (17, 64, 64, 8), (33, 96, 160, 32)) + tuple((w, 512, 512, 256, 4) for w in WIDTHS)
BATCHES = (1, 31, 32, 33, 64, 65, R - 1, R, R + 1, 2 * R + 5)
EVERY_BATCH = (NETS[0], NETS[7])         # every batch on these two; every network at 33, R + 1 and 2 R + 5
CASES = tuple(sorted({(n, b) for n in EVERY_BATCH for b in BATCHES} | {(n, b) for n in NETS for b in (33, R + 1, 2 * R + 5)},
                     key=lambda c: (NETS.index(c[0]), c[1])))


def case_id(case):
    return "-".join(str(s) for s in case[0]) + f"@{case[1]}"


@functools.lru_cache(maxsize=None)
def layers_of(sizes):
    """[(W, b)] float32 on the CPU by mlp_support.random_layers' rule (that function itself for its in-512-512-256-out shape)."""
    seed = 1000 + NETS.index(sizes) if sizes in NETS else 999
    if len(sizes) == 5 and sizes[1:4] == (512, 512, 256):
        return ms.random_layers(sizes[0], sizes[4], seed)
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn((b, a), generator=g) * (1.4 / max(a, 16) ** 0.5), 0.1 * torch.randn((b,), generator=g))
            for a, b in zip(sizes[:-1], sizes[1:])]


@functools.lru_cache(maxsize=None)
def _inputs_full(sizes):
    g = torch.Generator().manual_seed(77 + len(sizes) + 13 * sizes[0])
    top = max(BATCHES)
    return torch.randn((top, sizes[0]), generator=g), torch.randn((top, sizes[-1]), generator=g)


def inputs(sizes, batch):
    """x ~ N(0, 1) and d_out ~ N(0, 1) / batch; the rows of a smaller batch are the leading rows of a larger one."""
    x, d = _inputs_full(sizes)
    return x[:batch].contiguous(), (d[:batch] / batch).contiguous()


def reference_of(layers, x, d_out):
    """out, [d_weight_0, d_bias_0, ...] and d_x of the float32 parameters and inputs evaluated in float64 (mlp_support.f64 is the forward)."""
    lay = [(w.double().requires_grad_(), b.double().requires_grad_()) for w, b in layers]
    xd = x.double().requires_grad_()
    out = ms.f64(lay, xd)
    out.backward(d_out.double())
    return out.detach(), [t.grad for pair in lay for t in pair], xd.grad


@functools.lru_cache(maxsize=None)
def reference(sizes, batch):
    return reference_of(layers_of(sizes), *inputs(sizes, batch))


def scratch_bytes(sizes, batch):
    """The header's formula, restated."""
    r = lambda b: (b + 255) // 256 * 256      # noqa: E731
    chunks = (batch - 1) // R + 1
    pairs = list(zip(sizes[:-1], sizes[1:]))
    return (sum(2 * r(4 * batch * o) for _, o in pairs[:-1]) + sum(r(4 * chunks * o * i) for i, o in pairs)
            + sum(r(8 * chunks * o) for _, o in pairs))


def tables(K, sizes, ptrs=None, flags=0):
    """(cfg, layer table) for a network of these sizes; ptrs: [(weight, bias, d_weight, d_bias)] addresses, default a dummy non-NULL one."""
    n = len(sizes) - 1
    ptrs = ptrs or [(4096, 4096, 4096, 4096)] * n
    table = (K.DnMlpTrainLayer * n)(*[K.DnMlpTrainLayer(*p, i, o) for p, i, o in zip(ptrs, sizes[:-1], sizes[1:])])
    return K.DnMlpTrainConfig(n, K.TRAIN_ACT_TANH, flags, 0), table


def byref(x):
    return C.byref(x)
