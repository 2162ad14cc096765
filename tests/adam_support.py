"""What the tests of the optimiser step (include/dronenav.h dn_adam_step) share and what needs no GPU: the reference -- the arithmetic of
the header in NumPy float64, with math.fsum for the norm --, the case generator, the bounds, and a helper that places every tensor
inside a larger buffer with sentinel words on both sides.  A plain module: pytest does not collect it and does not rewrite its asserts,
so every assert here carries its own message."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constant(name):
    """A #define of include/dronenav.h: the chunk size is stated there once."""
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dronenav.h")).read(), flags=re.S)
    return int(re.search(r"#define %s (\d+)\b" % name, code).group(1))


CHUNK = header_constant("DN_ADAM_CHUNK")
MAX_TENSORS = header_constant("DN_ADAM_MAX_TENSORS")
BETAS, EPS, LR, MAX_GRAD_NORM = (0.9, 0.999), 1e-5, 3e-4, 0.5
STATE0 = (0.0, 1.0, 1.0, 0.0)
STEPS = 5

# 13 -> 32 -> 32 -> 32 actor and critic trunks, a 4-column action head, log_std, a value head: MlpActorCritic(pi=(32,) * 3, vf=(32,) * 3)
SMALL_NET = (416, 32, 1024, 32, 1024, 32, 128, 4, 4, 416, 32, 1024, 32, 1024, 32, 32, 1)
# 32 tensors: single elements, the edges of the 16-byte word, of the wave (256 elements), of the chunk, and several chunks
MIXED_32 = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3000, 1, 513, 6, 4096, 4097, 100, 31, 33,
            1000, 12, 999, 17)
COUNT_LISTS = ((1,), (3,), (4,), (5,), (1023,), (1024,), (1025,), (4097,), (1, 1024, 5, 2049), SMALL_NET, MIXED_32)
DATA_SETS = ("under", "over", "zero", "noclip")        # coef exactly 1; norm about 3 x over; zero gradients; max_grad_norm = 0
assert len(SMALL_NET) == 17 and len(MIXED_32) == MAX_TENSORS, "the count lists of the issue"


def chunks(counts):
    return sum(-(-int(c) // CHUNK) for c in counts)


def max_grad_norm_of(data_set):
    return 0.0 if data_set == "noclip" else MAX_GRAD_NORM


def case(counts, data_set, seed=0):
    """(p, m, v) float32 lists, and STEPS lists of float32 gradients whose global norm is 0.1 ("under"), 3 ("over", "noclip") times
    MAX_GRAD_NORM, or zero.  With zero gradients the moments start at zero, so that the parameters must not move."""
    rng = np.random.default_rng([seed, len(counts), sum(counts), DATA_SETS.index(data_set)])
    f32 = np.float32
    p = [rng.normal(0.0, 0.3, c).astype(f32) for c in counts]
    if data_set == "zero":
        m, v = [np.zeros(c, f32) for c in counts], [np.zeros(c, f32) for c in counts]
    else:
        m = [rng.normal(0.0, 1e-3, c).astype(f32) for c in counts]
        v = [(rng.normal(0.0, 1e-3, c) ** 2).astype(f32) for c in counts]
    grads = []
    for k in range(STEPS):
        g = [rng.normal(0.0, 1.0, c) for c in counts]
        norm = math.sqrt(sum(float((x * x).sum()) for x in g))
        want = {"under": 0.1, "over": 3.0, "noclip": 3.0, "zero": 0.0}[data_set] * MAX_GRAD_NORM * (1.0 + 0.1 * k)
        grads.append([(x * (want / norm)).astype(f32) for x in g])
    return p, m, v, grads


def reference(p, g, m, v, lr, state, *, betas=BETAS, eps=EPS, max_grad_norm=MAX_GRAD_NORM):
    """One step of the header's arithmetic in float64 on lists of arrays: (p', m', v') unrounded, the state after it, the statistics."""
    beta1, beta2 = betas
    p, g, m, v = ([np.asarray(x, np.float64) for x in t] for t in (p, g, m, v))
    squares = [x * x for x in g]                       # exact: the square of a float32 has 48 bits
    if all(np.isfinite(s).all() for s in squares):
        total = math.sqrt(math.fsum(np.concatenate(squares).tolist()))
    else:
        total = math.sqrt(float(sum(sq.sum() for sq in squares)))
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.float64(max_grad_norm) / (np.float64(total) + 1e-6)
        coef = (1.0 if c > 1.0 else float(c)) if max_grad_norm > 0.0 else 1.0
        step, c1, c2 = state[0] + 1.0, state[1] * beta1, state[2] * beta2
        bc1, bc2 = 1.0 - c1, 1.0 - c2
        out_p, out_m, out_v = [], [], []
        for pi, gi, mi, vi in zip(p, g, m, v):
            gs = gi * coef
            m1 = mi + (gs - mi) * (1.0 - beta1)
            v1 = vi * beta2 + (1.0 - beta2) * gs * gs
            out_p.append(pi - (lr / bc1) * (m1 / (np.sqrt(v1) / math.sqrt(bc2) + eps)))
            out_m.append(m1)
            out_v.append(v1)
    return out_p, out_m, out_v, (step, c1, c2, 0.0), (total, coef, lr, step)


def ulps_off(got, ref):
    """|got - ref| in float32 ulps of ref, per element; 0 where within 2^-40 absolute, or where both are NaN."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = np.abs(got - ref)
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        d = np.where(diff <= 2.0 ** -40, 0.0, diff / ulp)
    return np.where(np.isnan(got) & np.isnan(ref), 0.0, np.where(np.isnan(d), np.inf, d))


def check_step(got, ref, tag):
    """got: (p, m, v lists of float32 arrays, state [4], stats [4]) of the device after a step; ref: reference() on what the device held
    before it.  p, m, v within one float32 ulp or 2^-40; stats[0] within 2^-40 relative; the rest of stats within 2^-40 relative too;
    the state bit-equal.  Returns the largest distance in ulps."""
    worst = 0.0
    for name, a, b in zip("pmv", got[:3], ref[:3]):
        for i, (x, y) in enumerate(zip(a, b)):
            d = float(ulps_off(x, y).max())
            assert d <= 1.0, f"{tag}: {name}[{i}] is {d:.3g} float32 ulps from the reference"
            worst = max(worst, d)
    state, stats = np.asarray(got[3], np.float64), np.asarray(got[4], np.float64)
    assert state.tobytes() == np.asarray(ref[3], np.float64).tobytes(), f"{tag}: state {state.tolist()} is not {list(ref[3])} bit for bit"
    for j, name in enumerate(("total", "coef", "lr", "step")):
        want = ref[4][j]
        if math.isnan(want):
            assert math.isnan(stats[j]), f"{tag}: stats {name} {stats[j]!r}, the reference has NaN"
        else:
            assert abs(stats[j] - want) <= 2.0 ** -40 * abs(want), f"{tag}: stats {name} {stats[j]!r} against {want!r}"
    return worst


# ---- tensors between sentinels ----------------------------------------------------------------------------------------------------------
SENTINEL = 0x7FC12345                                  # a NaN no arithmetic produces
PAD = 8                                                # elements either side: a multiple of four, so `offset` alone sets the alignment


def place(torch, values, offset, device):
    """(buffer, view): `values` (a float32 array) at element PAD + offset of a buffer filled with SENTINEL.  The allocator aligns the
    buffer far beyond 16 bytes, so offset 0 gives a 16-byte aligned view and offset 1 one that is 4 bytes past it."""
    n = len(values)
    buf = torch.full((PAD + offset + n + PAD,), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)
    view = buf[PAD + offset: PAD + offset + n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32)))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * (offset % 4) and view.is_contiguous(), "place: alignment"
    return buf, view


def sentinels_intact(torch, buf, offset, n):
    w = buf.view(torch.int32)
    return bool((w[:PAD + offset] == SENTINEL).all()) and bool((w[PAD + offset + n:] == SENTINEL).all())
