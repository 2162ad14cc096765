#!/usr/bin/env python3
"""Device time of the PPO loss head through dn_ppo_loss (csrc/dn_ppo_loss.hip, ppo.PpoLoss) beside the float32 torch composition it
replaces, written to profiles/time_ppo_loss.txt:
    python3 profiles/time_ppo_loss.py [reps] [output file]
The workload: one minibatch of B in {4096, 65536} rows, A = 4 action columns, clip_range 0.2, the value clip on (0.2), ent_coef 0.01,
vf_coef 0.5; mean [B, 4], log_std [4] and values [B] are leaf tensors that ask for a gradient, so what is timed is the loss forward plus
the backward to the three head outputs and nothing of a network.  Per shape, interleaved call by call, the median and the range of `reps`
(default 15) timings, each one pair of events around INNER back-to-back forward + backward calls on the stream, over INNER:
  kernel eager   loss = ppo(mean, log_std, values, mb); loss.backward(): two launches forward, and autograd's three products of the stored
                 gradients with grad_output
  kernel graph   the same captured once and replayed
  torch eager    SB3's PPO.train body [from recall] in float32 torch and loss.backward(), on the same tensors
  torch graph    the same captured once and replayed
Before the timings both paths are held against the float64 torch composition on the CPU: the largest error of the three gradients, over
the largest gradient."""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import drl_dronenavigation_amd as pkg  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
target = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "time_ppo_loss.txt")
dev = torch.device("cuda:0")
lines = []
A, INNER, CLIP, CLIP_VF, ENT, VF = 4, 10, 0.2, 0.2, 0.01, 0.5
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


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


def composition(mean, log_std, values, mb):
    """SB3 PPO.train's loss [from recall], in the dtype of its tensors."""
    z = (mb["actions"] - mean) * torch.exp(-log_std)
    logp = (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(-1)
    ratio = torch.exp(logp - mb["log_probs"])
    adv = mb["advantages"]
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP)).mean()
    vpred = mb["values"] + torch.clamp(values - mb["values"], -CLIP_VF, CLIP_VF)
    value_loss = ((mb["returns"] - vpred) ** 2).mean()
    entropy_loss = -(0.5 + HALF_LOG_2PI + log_std).sum()
    with torch.no_grad():                                       # SB3 logs these two every minibatch
        lr = logp - mb["log_probs"]
        logged = torch.mean((ratio - 1.0) - lr), torch.mean((torch.abs(ratio - 1.0) > CLIP).float())
    return policy_loss + ENT * entropy_loss + VF * value_loss, logged


def captured(step):
    """step() warmed up on a side stream, as torch asks before a capture with autograd in it, then captured."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph


say(f"device {torch.cuda.get_device_name(0)}, reps {reps}, {INNER} forward + backward calls per timing; act_dim {A}, clip_range {CLIP}, "
    f"clip_range_vf {CLIP_VF}, ent_coef {ENT}, vf_coef {VF}")
for B in (4096, 65536):
    g = torch.Generator(device=dev).manual_seed(B)
    rn = lambda *s: torch.randn(s, generator=g, device=dev)  # noqa: E731
    mean, log_std = (0.09 + 0.01 * rn(B, A)).requires_grad_(), (-2.0 + 0.3 * rn(A)).requires_grad_()
    actions = (mean + torch.exp(log_std) * rn(B, A)).detach()
    with torch.no_grad():
        zz = (actions - mean) * torch.exp(-log_std)
        logp = (-0.5 * zz * zz - log_std - HALF_LOG_2PI).sum(-1)
    returns = 2.0 * rn(B)
    old_values = returns + 0.5 * rn(B)
    mb = dict(actions=actions, log_probs=logp + 0.15 * rn(B), advantages=rn(B), returns=returns, values=old_values)
    values = (old_values + 0.3 * rn(B)).requires_grad_()
    leaves = (mean, log_std, values)
    ppo = pkg.PpoLoss(B, A, dev, clip_range=CLIP, clip_range_vf=CLIP_VF, ent_coef=ENT, vf_coef=VF)

    def kernel_step():
        for t in leaves:
            t.grad = None
        ppo(mean, log_std, values, mb).backward()

    def torch_step():
        for t in leaves:
            t.grad = None
        composition(mean, log_std, values, mb)[0].backward()

    # both paths against the float64 composition on the CPU
    leaves64 = [t.detach().double().cpu().requires_grad_() for t in leaves]
    composition(*leaves64, {k: v.double().cpu() for k, v in mb.items()})[0].backward()
    top = max(float(t.grad.abs().max()) for t in leaves64)
    err = {}
    for name, step in (("kernel", kernel_step), ("torch", torch_step)):
        step()
        torch.cuda.synchronize(dev)
        err[name] = max(float((t.grad.double().cpu() - t64.grad).abs().max()) for t, t64 in zip(leaves, leaves64)) / top
    clip_fraction = float(ppo.stats[5])

    graphs = {"kernel": captured(kernel_step), "torch": captured(torch_step)}
    fns = {"kernel eager": kernel_step, "kernel graph": graphs["kernel"].replay, "torch eager": torch_step, "torch graph": graphs["torch"].replay}
    t = {k: [] for k in fns}
    for fn in fns.values():                                     # every path once more before the timed window
        fn()
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, INNER))
    m = {k: statistics.median(v) for k, v in t.items()}
    say(f"B {B}, clip fraction {clip_fraction:.2f} | " + " | ".join(f"{k} {spread(v)}" for k, v in t.items()))
    say(f"    torch / kernel eager {m['torch eager'] / m['kernel eager']:.2f} | torch / kernel graph {m['torch graph'] / m['kernel graph']:.2f} | "
        f"gradients against the float64 composition, of the largest: kernel {err['kernel']:.2e}, torch {err['torch']:.2e}")
    del graphs, ppo
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(target)), exist_ok=True)
with open(target, "w") as f:
    f.write("\n".join(lines) + "\n")
