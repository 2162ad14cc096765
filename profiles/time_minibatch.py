#!/usr/bin/env python3
"""Device time of one PPO epoch of minibatches through dn_minibatch (csrc/dn_minibatch.hip) beside the torch composition it replaces,
written to profiles/time_minibatch.txt:
    python3 profiles/time_minibatch.py [reps] [output file]
The workload: n_steps = 32, 32 768 drones (M = 1 048 576 samples), batch_size = 65 536 (16 minibatches an epoch), SB3's six fields --
obs (13 columns), actions (4), values, log_probs, advantages, returns -- and the same with a 64-column history field in place of obs.
Per shape, interleaved epoch by epoch, the median and the range of `reps` (default 15) timings, each one pair of events around INNER
back-to-back epochs on the stream, over INNER:
  kernel eager   MinibatchSampler.epoch(): 16 dn_minibatch calls of three launches (gather + block moments, merge, division)
  kernel graph   the same epoch and epoch_offset += 1 captured once and replayed
  kernel 4-byte  eager, with every source moved by one 4-byte word: the 4-byte path where the aligned tensors take 16-byte words
  torch          torch.randperm, then per minibatch the slice of the permutation, one indexing launch per field on the flattened
                 arrays, and (a - mean) / (std + 1e-8) in float32 -- eager, on the same tensors
  flatten        what the torch composition needs once per ROLLOUT before its first epoch, and dn_minibatch does not: the
                 transpose(0, 1).reshape(M, ...) copy of every field
  copy           dn_stream_copy of the epoch's algorithmic bytes, half in and half out: per sample every field word read and written once
                 (8 bytes a word), the sample index written (8 bytes) and the advantage read and written once more by the division (8)
Before the timings the kernel's epoch is held against the torch gather with the kernel's own permutation: the copied fields bit for bit,
the advantages against the float64 torch expression (one float32 ulp of it, or 2^-40)."""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import drl_dronenavigation_amd as pkg  # noqa: E402
from drl_dronenavigation_amd import _capi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
target = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "time_minibatch.txt")
dev = torch.device("cuda:0")
lib = _capi.load()
lines = []
T, N, BATCH, INNER, SEED = 32, 32768, 65536, 5, 3
M = T * N


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


def stream():
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def spread(xs):
    return f"{statistics.median(xs):.1f} us ({min(xs):.1f}-{max(xs):.1f})"


def moved(x):
    """The same words one 4-byte word further on: dense, 4 bytes off every 16-byte boundary."""
    return torch.empty(x.numel() + 1, dtype=x.dtype, device=dev)[1:].view(x.shape).copy_(x)


say(f"device {torch.cuda.get_device_name(0)}, reps {reps}, {INNER} epochs per timing; n_steps {T}, drones {N}, batch_size {BATCH}: {M // BATCH} minibatches "
    "an epoch")
for first, width in (("obs", 13), ("history", 64)):
    g = torch.Generator(device=dev).manual_seed(width)
    shapes = {first: (width,), "actions": (4,), "values": (), "log_probs": (), "advantages": (), "returns": ()}
    out = {k: torch.randn((T, N) + s, generator=g, device=dev) for k, s in shapes.items()}
    out["advantages"].mul_(2.0).add_(0.3)
    words = sum(torch.Size(s).numel() for s in shapes.values())
    nbytes = M * (8 * words + 16)
    sampler = pkg.MinibatchSampler.for_rollout(out, BATCH, fields=tuple(shapes), seed=SEED)
    slow = pkg.MinibatchSampler.for_rollout(out, BATCH, fields=tuple(shapes), seed=SEED)
    out_moved = {k: moved(v) for k, v in out.items()}
    offset = torch.zeros(1, dtype=torch.int64, device=dev)

    def flatten():
        return {k: v.transpose(0, 1).reshape((M,) + tuple(v.shape[2:])) for k, v in out.items()}

    flat = flatten()
    assert all(v.data_ptr() != out[k].data_ptr() for k, v in flat.items())

    def torch_epoch():
        perm = torch.randperm(M, device=dev)
        for start in range(0, M, BATCH):
            idx = perm[start:start + BATCH]
            mb = {k: v[idx] for k, v in flat.items()}
            a = mb["advantages"]
            mb["advantages"] = (a - a.mean()) / (a.std() + 1e-8)
        return mb

    def kernel_epoch(s=sampler, src=out, epoch_offset=None):
        for mb in s.epoch(src, 7, epoch_offset=epoch_offset):
            pass
        return mb

    # the kernel's epoch against the torch gather with the kernel's own permutation
    perm = sampler.permutation(7).to(dev)
    bit_equal, worst = True, 0
    for i, mb in enumerate(sampler.epoch(out, 7)):
        idx = perm[i * BATCH:(i + 1) * BATCH]
        bit_equal &= bool(torch.equal(mb["indices"], idx))
        for k in shapes:
            if k != "advantages":
                bit_equal &= bool(torch.equal(mb[k].view(torch.int32), flat[k][idx].view(torch.int32)))
        a = flat["advantages"][idx].double()
        want = (a - a.mean()) / (a.std() + 1e-8)
        w32 = want.abs().float()
        tol = (torch.nextafter(w32, torch.full_like(w32, float("inf"))) - w32).double().clamp(min=2.0 ** -40)
        worst = max(worst, float(((mb["advantages"].double() - want).abs() / tol).max()))
    if not bit_equal or worst > 1.0:
        say(f"{first} {width}: MISMATCH -- copied fields bit-equal {bit_equal}, advantages {worst:.2f} of a float32 ulp (or 2^-40) from the float64 "
            "torch expression (bar 1)")

    kernel_epoch()
    kernel_epoch(slow, out_moved)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kernel_epoch(epoch_offset=offset)
        offset.add_(1)
    half = nbytes // 2 // 16 * 16
    src, dst = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
    fns = {"eager": kernel_epoch, "graph": graph.replay, "4-byte": lambda: kernel_epoch(slow, out_moved), "torch": torch_epoch,
           "flatten": flatten, "copy": lambda: _capi.check(lib.dn_stream_copy(dst.data_ptr(), src.data_ptr(), half, 0, stream()))}
    t = {k: [] for k in fns}
    for fn in fns.values():                                        # every path once more before the timed window
        fn()
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, INNER))
    m = {k: statistics.median(v) for k, v in t.items()}
    best = min(m["eager"], m["graph"])
    say(f"{first} {width} columns, {words} words a sample, algorithmic {nbytes / 1e6:.1f} MB an epoch | kernel eager {spread(t['eager'])} = "
        f"{nbytes / m['eager'] / 1e3:.0f} GB/s | kernel graph {spread(t['graph'])} = {nbytes / m['graph'] / 1e3:.0f} GB/s | kernel 4-byte path eager "
        f"{spread(t['4-byte'])} | torch {spread(t['torch'])} = {nbytes / m['torch'] / 1e3:.0f} GB/s | flatten once per rollout {spread(t['flatten'])} | "
        f"copy {spread(t['copy'])} = {nbytes / m['copy'] / 1e3:.0f} GB/s")
    say(f"    torch / kernel eager {m['torch'] / m['eager']:.2f} | torch / kernel graph {m['torch'] / m['graph']:.2f} | kernel graph / copy "
        f"{m['graph'] / m['copy']:.2f} | 4-byte / 16-byte path {m['4-byte'] / m['eager']:.2f} | the faster path: "
        f"{'the kernels' if best < m['torch'] else 'the torch composition'}, by {max(best, m['torch']) / min(best, m['torch']):.2f}x an epoch "
        f"(the flatten, {m['flatten'] / m['torch']:.2f} of a torch epoch, not counted) | copied fields bit-equal to the torch gather {bit_equal}, "
        f"advantages within {worst:.2f} float32 ulp of the float64 torch expression")
    del out, out_moved, flat, sampler, slow, graph, src, dst
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(target)), exist_ok=True)
with open(target, "w") as f:
    f.write("\n".join(lines) + "\n")
