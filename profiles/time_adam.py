#!/usr/bin/env python3
"""Device time of the PPO optimiser step through dn_adam_step (csrc/dn_adam.hip, optim.ClippedAdam) beside what it replaces --
torch.nn.utils.clip_grad_norm_(parameters, 0.5) + torch.optim.Adam(eps=1e-5).step() --, written to profiles/time_adam.txt:
    python3 profiles/time_adam.py [reps] [output file] [trace]
The workloads: the 17 parameter tensors of MlpActorCritic() (13 -> 512 -> 512 -> 256 twice, the heads, log_std), and those plus the 8 of
an MlpValue(52), 25 tensors; float32 gradients that stay the same from call to call.  Per workload, interleaved timing by timing, the
median and the range of `reps` (default 15) timings, each one pair of events around INNER back-to-back calls on the stream, over INNER:
  kernel eager         opt.step(): one C call, two launches
  kernel graph         the same captured once and replayed
  torch eager          clip_grad_norm_ + Adam.step(), torch's default (foreach) form
  torch fused eager    clip_grad_norm_ + Adam(fused=True).step()
  torch graph          clip_grad_norm_ + Adam(capturable=True).step() captured once and replayed
  torch fused graph    clip_grad_norm_ + Adam(fused=True, capturable=True).step() captured once and replayed
Every optimiser has its own copy of the parameters.  A leg that torch refuses to capture is reported as such, not left out silently.
Bytes are what the algorithm needs: 28 per element (p, g, m, v read, p, m, v written; the norm's read of g is counted once), against the
HBM3E peak of 8.0 TB/s.  With a third argument `trace` only the kernel eager leg runs, for a kernel trace taken in a run of its own."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import drl_dronenavigation_amd as pkg  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
target = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "time_adam.txt")
trace_only = len(sys.argv) > 3 and sys.argv[3] == "trace"
dev = torch.device("cuda:0")
lines = []
INNER, MAX_GRAD_NORM, LR, EPS, HBM_PEAK = 10, 0.5, 3e-4, 1e-5, 8.0e12


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


def spread(xs):
    return f"{statistics.median(xs):.1f} us ({min(xs):.1f}-{max(xs):.1f})"


def captured(step):
    """step() warmed up three times on a side stream, as torch asks before capturing an optimiser, then captured."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph


def copies(params, grads):
    out = [p.detach().clone() for p in params]
    for q, g in zip(out, grads):
        q.grad = g.clone()
    return out


def torch_leg(params, **kw):
    opt = torch.optim.Adam(params, lr=LR, eps=EPS, **kw)

    def step():
        torch.nn.utils.clip_grad_norm_(params, MAX_GRAD_NORM)
        opt.step()
    return step


say(f"device {torch.cuda.get_device_name(0)}, reps {reps}, {INNER} calls per timing; max_grad_norm {MAX_GRAD_NORM}, lr {LR}, eps {EPS}")
torch.manual_seed(0)
actor_critic, value = pkg.MlpActorCritic().to(dev), pkg.MlpValue(52).to(dev)
for name, params in (("MlpActorCritic()", list(actor_critic.parameters())),
                     ("MlpActorCritic() + MlpValue(52)", list(actor_critic.parameters()) + list(value.parameters()))):
    gen = torch.Generator(device=dev).manual_seed(len(params))
    grads = [1e-2 * torch.randn(p.shape, generator=gen, device=dev) for p in params]
    elements = sum(p.numel() for p in params)
    mine = copies(params, grads)
    opt = pkg.ClippedAdam(mine, lr=LR, eps=EPS, max_grad_norm=MAX_GRAD_NORM)
    opt.step()                                                  # the scratch is made outside the capture
    torch.cuda.synchronize(dev)
    stats = opt.stats_dict()
    fns = {"kernel eager": opt.step}
    refused = {}
    if not trace_only:
        fns["kernel graph"] = captured(opt.step).replay
        fns["torch eager"] = torch_leg(copies(params, grads))
        fns["torch fused eager"] = torch_leg(copies(params, grads), fused=True)
        for leg, kw in (("torch graph", dict(capturable=True)), ("torch fused graph", dict(fused=True, capturable=True))):
            try:
                fns[leg] = captured(torch_leg(copies(params, grads), **kw)).replay
            except Exception as e:                              # noqa: BLE001  (reported below, next to the numbers)
                refused[leg] = f"{type(e).__name__}: {str(e).splitlines()[0][:160]}"
                torch.cuda.synchronize(dev)
    t = {k: [] for k in fns}
    for fn in fns.values():                                     # every path once more before the timed window
        fn()
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, INNER))
    m = {k: statistics.median(v) for k, v in t.items()}
    say(f"{name}: {len(params)} tensors, {elements} float32, {pkg.optim.ClippedAdam.__name__} scratch {opt._need} B; gradient norm "
        f"{stats['grad_norm']:.3f}, clip coefficient {stats['clip_coef']:.3f}")
    say("    " + " | ".join(f"{k} {spread(v)}" for k, v in t.items()))
    for leg, why in refused.items():
        say(f"    {leg}: torch did not capture it ({why})")
    for k in ("kernel eager", "kernel graph"):
        if k in m:
            say(f"    {k}: {28 * elements} B needed, {28 * elements / (m[k] * 1e-6) / 1e12:.3f} TB/s, "
                f"{100.0 * 28 * elements / (m[k] * 1e-6) / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak (32 B an element with the zeroing)")
    if not trace_only:
        say("    torch over kernel: " + " | ".join(f"{k} / kernel {'graph' if 'graph' in k else 'eager'} "
                                                   f"{m[k] / m['kernel graph' if 'graph' in k else 'kernel eager']:.2f}"
                                                   for k in m if k.startswith("torch")))
    del fns, opt
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(target)), exist_ok=True)
with open(target, "w") as f:
    f.write("\n".join(lines) + "\n")
