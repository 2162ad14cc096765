"""What the tests of the LSTM layer share (tests/test_lstm_cpu.py, tests/test_gpu_lstm.py): the layers, shapes and episode-start patterns
of the cases, torch.nn.LSTM's default initialisation from fixed seeds, the inputs, the float64 reference through torch.nn.LSTM(...).double()
on the CPU stepped with the masking of include/dronenav.h (computed once per case), the scratch formula restated, and the ctypes tables
of a call.  A plain module like tests/mlp_train_support.py -- pytest does not collect it."""
import functools

import torch

R = 1024                                 # DN_MLP_TRAIN_CHUNK, restated: test_mlp_train_cpu.py holds it to the header
BOUND = 1e-4                             # the project's float32-grade bar (dn_mlp_forward grade 1)

LAYERS = ((13, 256), (1, 32), (17, 96), (64, 64), (33, 160), (13, 512))          # (I, H)
SHAPES = ((1, 1), (1, 33), (2, 31), (5, 129), (5, 205), (3, 683))                # (T, B): the last two are 1025 and 2049 rows
PATTERNS = ("none", "first", "random", "step")
# every shape on the first two layers, every layer at (5, 129) and (5, 205)
PAIRS = tuple(sorted({(l, s) for l in LAYERS[:2] for s in SHAPES} | {(l, s) for l in LAYERS for s in ((5, 129), (5, 205))},
                     key=lambda p: (LAYERS.index(p[0]), SHAPES.index(p[1]))))


def case_id(case):
    (i, h), (t, b), pattern = case
    return f"{i}-{h}@{t}x{b}-{pattern}"


@functools.lru_cache(maxsize=None)
def params_of(layer):
    """(weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0) float32 on the CPU: torch.nn.LSTM's default initialisation, seeded by the layer."""
    with torch.random.fork_rng():
        torch.manual_seed(2000 + LAYERS.index(layer) if layer in LAYERS else 1999)
        lstm = torch.nn.LSTM(*layer)
    return tuple(getattr(lstm, n).detach().clone() for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"))


def starts_of(shape, pattern):
    """episode_starts uint8 [T, B], or None: none; all ones at t = 0; each cell set with probability 0.2; one step (T // 2) with every row
    set."""
    t, b = shape
    if pattern == "none":
        return None
    s = torch.zeros((t, b), dtype=torch.uint8)
    if pattern == "first":
        s[0] = 1
    elif pattern == "random":
        g = torch.Generator().manual_seed(31 + 7 * t + b)
        s = (torch.rand((t, b), generator=g) < 0.2).to(torch.uint8)
    else:
        s[t // 2] = 1
    return s


CASES = tuple((l, s, p) for l, s in PAIRS for p in PATTERNS)


def all_start(shape, pattern):
    """Every row of hprev is masked away: T = 1 with every row's episode starting -- the rollout step in which every drone resets.  d_w_hh
    is identically zero there (in the float64 reference too), so the tests ask for exact zeros instead of the relative bound."""
    s = starts_of(shape, pattern)
    return s is not None and shape[0] == 1 and bool(s.all())


@functools.lru_cache(maxsize=None)
def inputs(layer, shape):
    """x ~ N(0, 1) [T, B, I], d_hseq ~ N(0, 1) / (T B) [T, B, H], and an initial state h0, c0 ~ N(0, 1) / 2 [B, H]."""
    (i, h), (t, b) = layer, shape
    g = torch.Generator().manual_seed(77 + 13 * i + h + 1000 * t + b)
    return (torch.randn((t, b, i), generator=g), torch.randn((t, b, h), generator=g) / (t * b), 0.5 * torch.randn((b, h), generator=g),
            0.5 * torch.randn((b, h), generator=g))


def lstm64(params):
    """torch.nn.LSTM(I, H).double() on the CPU holding the float32 parameters."""
    w_ih = params[0]
    lstm = torch.nn.LSTM(w_ih.shape[1], w_ih.shape[0] // 4).double()
    with torch.no_grad():
        for n, p in zip(("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"), params):
            getattr(lstm, n).copy_(p.double())
    return lstm


def sequence64(lstm, x, starts, h0, c0):
    """(h_seq, c_seq) float64 [T, B, H], stepped with the masking of the header: both states times 1 - episode_start before the step."""
    h, c = h0, c0
    hs, cs = [], []
    for t in range(x.shape[0]):
        if starts is not None:
            keep = (1 - starts[t].double()).unsqueeze(1)
            h, c = h * keep, c * keep
        _, (h, c) = lstm(x[t:t + 1], (h.unsqueeze(0), c.unsqueeze(0)))
        h, c = h[0], c[0]
        hs.append(h)
        cs.append(c)
    return torch.stack(hs), torch.stack(cs)


def reference_of(params, x, starts, h0, c0, d_hseq):
    """h_seq, c_seq, [d_w_ih, d_w_hh, d_b_ih, d_b_hh] and d_x of the float32 parameters and inputs, evaluated in float64 with autograd
    over the whole sequence."""
    lstm = lstm64(params)
    xd = x.double().requires_grad_()
    hs, cs = sequence64(lstm, xd, starts, h0.double(), c0.double())
    hs.backward(d_hseq.double())
    return hs.detach(), cs.detach(), [getattr(lstm, n).grad for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")], xd.grad


@functools.lru_cache(maxsize=None)
def reference(case):
    layer, shape, pattern = case
    x, d, h0, c0 = inputs(layer, shape)
    return reference_of(params_of(layer), x, starts_of(shape, pattern), h0, c0, d)


def teacher_forced(params, x, starts, h0, c0, h_seq, c_seq):
    """(h, c) float64 [T, B, H]: step t of the float64 cell from the states given in h_seq[t - 1], c_seq[t - 1] (h0, c0 at t = 0), all
    steps as the rows of one cell call."""
    t, b, _ = x.shape
    hp = torch.cat((h0.unsqueeze(0), h_seq[:-1])).double()
    cp = torch.cat((c0.unsqueeze(0), c_seq[:-1])).double()
    if starts is not None:
        keep = (1 - starts.double()).unsqueeze(2)
        hp, cp = hp * keep, cp * keep
    with torch.no_grad():
        _, (h, c) = lstm64(params)(x.double().reshape(1, t * b, -1), (hp.reshape(1, t * b, -1), cp.reshape(1, t * b, -1)))
    return h.reshape(t, b, -1), c.reshape(t, b, -1)


def scratch_regions(layer, shape):
    """The header's regions, restated: [(name, bytes)] in order."""
    (i, h), (t, b) = layer, shape
    r = lambda n: (n + 255) // 256 * 256      # noqa: E731
    chunks = (t * b - 1) // R + 1
    return [("gates", r(16 * t * b * h)), ("carry_h", r(4 * b * h)), ("carry_c", r(4 * b * h)), ("wpart", r(16 * chunks * h * (i + h))),
            ("bpart", r(32 * chunks * h))]


def scratch_bytes(layer, shape):
    return sum(n for _, n in scratch_regions(layer, shape))


def gates_bytes(layer, shape):
    return scratch_regions(layer, shape)[0][1]


def tables(K, layer, ptrs=None, flags=0):
    """(cfg, params) of a call; ptrs: the eight addresses of dn_lstm_params, default a dummy non-NULL one."""
    return K.DnLstmConfig(layer[0], layer[1], flags, 0), K.DnLstmParams(*(ptrs or [4096] * 8))
