#!/usr/bin/env python3
"""Device time of dn_rownorm (csrc/dn_rownorm.hip) beside two references, written to profiles/time_rownorm.txt:
    python3 profiles/time_rownorm.py [reps] [output file]
Rows are N(0, 1) columns at mixed scales with a rotor-speed column (14468 +- 1), a constant and a zero column.  Shapes: 32 768 drones x
W = 21 / 52 / 64 at K = 1 and K = 32, and 2 097 152 drones x 52 at K = 1.  Per shape, interleaved launch by launch, the median of `reps`
(default 25):
  kernel   one dn_rownorm call with update = 1, out of place: three launches (block moments, merge, normalise)
  moments  the same with out = NULL: the first two launches alone
  apply    update = 0: the normalise launch alone, on the statistics as they are
  copy     dn_stream_copy of the same algorithmic bytes: the rows are read twice (moments, normalise) and written once, 12 K N W bytes; the
           copy moves half of that in and half out
  torch    the float64 torch composition it replaces, eager (per step: mean, population variance, the update, the clipped output)
dn_rownorm takes no env, so the launch-event hook of the step kernels does not reach it: every figure is one pair of events around INNER
back-to-back calls on the stream, over INNER -- kernel and copy alike (as profiles/time_history.py does).  The kernel's statistics are held
against the torch composition's (1e-9) and its output against the float64 expression on its own statistics (float32 ulp) on every shape.
Last, RolloutCollector.collect() at 32 768 drones, n_steps = 32, value_input="privileged" with a fused float32-grade critic on the 52
columns, with and without value_norm."""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import drl_dronenavigation_amd as pkg  # noqa: E402
from drl_dronenavigation_amd import _capi, tracks  # noqa: E402
from drl_dronenavigation_amd.collector import RolloutCollector  # noqa: E402
from drl_dronenavigation_amd.policy_mfma import FusedMlpValue  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 25
target = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "time_rownorm.txt")
dev = torch.device("cuda:0")
lib = _capi.load()
lines = []
CLIP, EPS = 10.0, 1e-8


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) * 1e3 / inner


def med(xs):
    return statistics.median(xs)


def stream():
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def make_rows(K, n, W, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    scales = 10.0 ** ((torch.arange(W, device=dev) % 7) - 3.0)
    x = torch.randn((K, n, W), generator=g, device=dev) * scales + 5.0 * scales
    x[..., W - 3] = 14468.0 + torch.randn((K, n), generator=g, device=dev)
    x[..., W - 2] = 3.25
    x[..., W - 1] = 0.0
    return x


def torch_update_normalize(stats, rows, out, W):
    """The composition a user writes today: float64 statistics, one step after the other."""
    count, mean, var = stats[0], stats[1:1 + W], stats[1 + W:]
    for t in range(rows.shape[0]):
        x = rows[t].double()
        n = x.shape[0]
        bm, bv = x.mean(dim=0), x.var(dim=0, unbiased=False)
        delta = bm - mean
        tot = count + n
        new_mean = mean + delta * n / tot
        m2 = var * count + bv * n + delta * delta * count * n / tot
        mean, var, count = new_mean, m2 / tot, tot
        out[t] = ((x - mean) / torch.sqrt(var + EPS)).clamp(-CLIP, CLIP).float()
    return torch.cat((count.reshape(1), mean, var))


def ulps(got, want64):
    a, b = got.view(torch.int32).long(), want64.float().view(torch.int32).long()
    a, b = torch.where(a < 0, -(a & 0x7FFFFFFF), a), torch.where(b < 0, -(b & 0x7FFFFFFF), b)
    return int((a - b).abs().max())


say(f"device {torch.cuda.get_device_name(0)}, reps {reps}")
worst_ulp = 0
for n, K, W in [(32768, K, W) for K in (1, 32) for W in (21, 52, 64)] + [(2097152, 1, 52)]:
    inner = 10 if n * K <= 32768 else 3 if K == 1 else 1
    rows = make_rows(K, n, W, 1000 * W + K)
    out, out_t = torch.empty_like(rows), torch.empty_like(rows)
    norm = pkg.RowNormalizer(W, dev, clip=CLIP, epsilon=EPS)
    norm.update(make_rows(1, n, W, 7)[0])                          # away from the prior
    start = norm.stats.clone()
    cfg = _capi.DnRownormConfig(W, CLIP, EPS)
    sb = lib.dn_rownorm_scratch_bytes(K, n, W)
    scratch = torch.empty(sb // 8, dtype=torch.float64, device=dev)

    def call(o, update):
        _capi.check(lib.dn_rownorm(C.byref(cfg), norm.stats.data_ptr(), K, n, rows.data_ptr(), o, update, scratch.data_ptr(), sb, 0, stream()))

    # one checked call from the common start
    call(out.data_ptr(), 1)
    want_stats = torch_update_normalize(start, rows, out_t, W)
    got = norm.stats.clone()
    err_m = float(((got[1:1 + W] - want_stats[1:1 + W]).abs() / (want_stats[1:1 + W].abs() + want_stats[1 + W:].sqrt())).max())
    err_v = float(((got[1 + W:] - want_stats[1 + W:]).abs() / want_stats[1 + W:]).max())
    agree = bool(got[0] == want_stats[0]) and err_m <= 1e-9 and err_v <= 1e-9
    ref = ((rows[K - 1].double() - got[1:1 + W]) / torch.sqrt(got[1 + W:] + EPS)).clamp(-CLIP, CLIP)
    u = ulps(out[K - 1], ref)
    worst_ulp = max(worst_ulp, u)
    if not agree or u > 3:
        say(f"W={W} N={n} K={K}: MISMATCH -- statistics vs torch: mean {err_m:.3e} var {err_v:.3e} (bar 1e-9), output {u} ulp (bar 3)")

    nbytes = 12 * K * n * W
    half = nbytes // 2 // 16 * 16
    src, dst = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
    fns = {"kernel": lambda: call(out.data_ptr(), 1), "moments": lambda: call(None, 1), "apply": lambda: call(out.data_ptr(), 0),
           "copy": lambda: _capi.check(lib.dn_stream_copy(dst.data_ptr(), src.data_ptr(), half, 0, stream())),
           "torch": lambda: torch_update_normalize(start, rows, out_t, W)}
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, 1 if k == "torch" else inner))
    m = {k: med(v) for k, v in t.items()}
    say(f"W={W} N={n} K={K} algorithmic {nbytes / 1e6:.1f} MB | kernel {m['kernel']:.2f} us ({nbytes / m['kernel'] / 1e3:.0f} GB/s) = moments "
        f"{m['moments']:.2f} + apply {m['apply']:.2f} | copy {m['copy']:.2f} us ({nbytes / m['copy'] / 1e3:.0f} GB/s) | torch float64 "
        f"{m['torch']:.1f} us | kernel / copy {m['kernel'] / m['copy']:.2f} | torch / kernel {m['torch'] / m['kernel']:.1f} | "
        f"statistics vs torch: mean {err_m:.1e} var {err_v:.1e} | output {u} ulp")
    del rows, out, out_t, scratch, src, dst, norm
    torch.cuda.empty_cache()
say(f"largest distance of the output from the float64 expression on the kernel's own statistics: {worst_ulp} float32 ulp (bar 3)")

n, T = 32768, 32
common = dict(normalize_obs=True, max_steps=64, seed=1, device=dev)
policy_w = (0.05 * torch.randn((13, 4), device=dev))


def policy(obs):
    x = torch.nan_to_num(obs).clamp(-5, 5)
    return 0.0922 + 0.01 * torch.tanh(x @ policy_w), x[:, 0], -(x * x).sum(dim=1)


for use_graph in (False, True):
    cols, t = {}, {}
    for name in ("raw", "value_norm"):
        env = pkg.DroneVecEnv(tracks.reaching(), n, privileged=pkg.PrivilegedObservation(), **common)
        critic = FusedMlpValue(pkg.MlpValue(52).to(dev), n, dev, grade="fp32")
        kw = dict(value_norm=pkg.RowNormalizer(52, dev)) if name == "value_norm" else {}
        cols[name] = RolloutCollector(env, policy, T, value_fn=critic, value_input="privileged", use_graph=use_graph, **kw)
        t[name] = []
        for _ in range(3):
            cols[name].collect()
    torch.cuda.synchronize(dev)
    for _ in range(reps):
        for name, col in cols.items():
            t[name].append(timed(col.collect, 1) / 1e3)
    say(f"RolloutCollector.collect() N={n} n_steps={T} value_input='privileged', fused fp32-grade critic on 52 columns, use_graph={use_graph}: "
        f"raw rows {med(t['raw']):.2f} ms | value_norm {med(t['value_norm']):.2f} ms | ratio {med(t['value_norm']) / med(t['raw']):.3f}")
    for col in cols.values():
        col.env.close()
os.makedirs(os.path.dirname(os.path.abspath(target)), exist_ok=True)
with open(target, "w") as f:
    f.write("\n".join(lines) + "\n")
