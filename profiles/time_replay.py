#!/usr/bin/env python3
"""Device time of one SAC replay minibatch through dn_replay_sample (csrc/dn_replay.hip) beside the torch composition it stands next to,
written to profiles/time_replay.txt:
    python3 profiles/time_replay.py [reps] [output file]
The workload: a RingReplayBuffer of 64 slots x 32 768 drones (13 observation and 4 action columns), full, at pos = 0 (a cycle boundary:
all 64 slots) and at pos = 17 (mid-cycle: slot 17 is skipped); batches of 256 rows (SB3's default) and of 65 536.
Per shape, interleaved call by call, the median and the range of `reps` (default 15) timings, each one pair of events around INNER
back-to-back calls on the stream, over INNER:
  kernel eager    ReplaySampler.sample(): one dn_replay_sample call, one launch
  kernel graph    the same call captured once and replayed
  graph + offset  the same with draw_offset += 1 in the graph (two nodes): what a learner that draws afresh on every replay runs
  torch           RingReplayBuffer.sample() on the same buffer, unchanged: two torch.randint, the skip, seven indexing gathers, a where,
                  the flag conversions and a multiply -- eager
  copy            dn_stream_copy of the call's algorithmic bytes, half in and half out: per row 2 D + A + 1 words and two flag bytes read,
                  2 D + A + 2 words and the int64 index written
Before the timings the kernel's output is held bit for bit against torch indexing with the kernel's own indices, and the indices against
dn_replay_indices."""
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
target = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "time_replay.txt")
dev = torch.device("cuda:0")
lib = _capi.load()
lines = []
T, N, D, A, SEED = 64, 32768, 13, 4, 3


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
    return f"{statistics.median(xs):.2f} us ({min(xs):.2f}-{max(xs):.2f})"


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


g = torch.Generator(device=dev).manual_seed(SEED)
buf = pkg.RingReplayBuffer(T, N, D, A, dev)
buf.obs_ring.copy_(torch.randn(buf.obs_ring.shape, generator=g, device=dev))
buf.terminal_obs.copy_(torch.randn(buf.terminal_obs.shape, generator=g, device=dev))
buf.actions.copy_(torch.rand(buf.actions.shape, generator=g, device=dev) * 2 - 1)
buf.rewards.copy_(torch.randn(buf.rewards.shape, generator=g, device=dev))
buf.done_flags.copy_(torch.rand(buf.done_flags.shape, generator=g, device=dev) < 0.05)
buf.timeout_flags.copy_(buf.done_flags.bool() & (torch.rand(buf.done_flags.shape, generator=g, device=dev) < 0.5))
buf.full = True
say(f"device {torch.cuda.get_device_name(0)}, reps {reps}; RingReplayBuffer {T} slots x {N} drones, {D} + {A} columns, full")
for pos in (0, 17):
    buf.pos = pos
    for batch, inner in ((256, 200), (65536, 50)):
        sampler = pkg.ReplaySampler(buf, batch, seed=SEED)
        nbytes = batch * (4 * (2 * D + A + 1) + 2 + 4 * (2 * D + A + 2) + 8)

        # the kernel's output against torch indexing with the kernel's own indices
        got = sampler.sample(draw=7)
        idx = got["indices"]
        ti, ei = idx // N, idx % N
        done = buf.done_flags[ti, ei].bool()
        want = dict(obs=buf.obs_ring[ti, ei], next_obs=torch.where(done[:, None], buf.terminal_obs[ti, ei], buf.obs_ring[ti + 1, ei]),
                    actions=buf.actions[ti, ei], rewards=buf.rewards[ti, ei], dones=done.float() * (1.0 - buf.timeout_flags[ti, ei].float()))
        bit_equal = all(bool(torch.equal(bits(got[k]), bits(v))) for k, v in want.items())
        bit_equal &= bool(torch.equal(idx.cpu(), sampler.indices(7))) and (pos == 0 or not bool((ti == pos).any()))
        if not bit_equal:
            say(f"pos {pos}, batch {batch}: MISMATCH -- the kernel's rows are not torch indexing at the kernel's own indices")

        torch.cuda.synchronize(dev)
        graph, graph_offset = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            sampler.sample(draw=0)
        with torch.cuda.graph(graph_offset):
            sampler.sample(draw=0)
            sampler.draw_offset.add_(1)
        half = max(nbytes // 2 // 16 * 16, 16)
        src, dst = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
        fns = {"eager": sampler.sample, "graph": graph.replay, "graph+offset": graph_offset.replay, "torch": lambda: buf.sample(batch),
               "copy": lambda: _capi.check(lib.dn_stream_copy(dst.data_ptr(), src.data_ptr(), half, 0, stream()))}
        t = {k: [] for k in fns}
        for fn in fns.values():                                    # every path once more before the timed window
            for _ in range(10):
                fn()
        for _ in range(reps):
            for k, fn in fns.items():
                t[k].append(timed(fn, inner))
        m = {k: statistics.median(v) for k, v in t.items()}
        best = min(m["eager"], m["graph"])
        say(f"pos {pos:2d}, batch {batch:5d}, algorithmic {nbytes / 1e3:.1f} kB a call, {inner} calls per timing | kernel eager {spread(t['eager'])} | "
            f"kernel graph {spread(t['graph'])} = {nbytes / m['graph'] / 1e3:.1f} GB/s | graph + offset {spread(t['graph+offset'])} | "
            f"torch {spread(t['torch'])} | copy {spread(t['copy'])}")
        say(f"    torch / kernel eager {m['torch'] / m['eager']:.2f} | torch / kernel graph {m['torch'] / m['graph']:.2f} | kernel graph / copy "
            f"{m['graph'] / m['copy']:.2f} | the faster path: {'the kernel' if best < m['torch'] else 'the torch composition'}, by "
            f"{max(best, m['torch']) / min(best, m['torch']):.2f}x a call | rows bit-equal to torch indexing at the kernel's indices {bit_equal}")
        del sampler, graph, graph_offset, src, dst
torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(target)), exist_ok=True)
with open(target, "w") as f:
    f.write("\n".join(lines) + "\n")
