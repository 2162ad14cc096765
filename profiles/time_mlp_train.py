#!/usr/bin/env python3
"""Device time of the networks' training pass through dn_mlp_train_forward / dn_mlp_train_backward (csrc/dn_mlp_train.hip,
mlp_train.MlpTrainer) beside what it replaces -- the float32 torch composition, nn.Sequential forward + backward, on the same tensors --,
written to profiles/time_mlp_train.txt:
    python3 profiles/time_mlp_train.py [reps] [output file]
One pass is forward + backward of the actor network of MlpActorCritic() (13-512-512-256-4) and of its critic (13-512-512-256-1), each
from a fixed gradient of its head output, the parameter gradients overwritten (kernel) or accumulated into static tensors (torch).  Per
batch (4 096 and 65 536 rows), interleaved timing by timing, the median and the range of `reps` (default 15) timings, each one pair of
events around INNER back-to-back passes on the stream, over INNER:
  kernel eager    MlpTrainer(x).backward(d_out) for both networks: 4 + 4 forward launches, 8 + 8 backward launches, autograd around them
  kernel graph    the same captured once and replayed
  torch eager     Sequential(x).backward(d_out) for both networks
  torch graph     the same captured once and replayed (reported as refused where torch does not capture it)
and both paths' gradient errors against the float64 evaluation of the same float32 parameters and inputs (torch float64 on the device):
the forward error max |out - out64|, and the largest max |g - g64| / max |g64| over the gradient tensors.
FLOP are the algorithm's: 2 rows in out per product, three products per layer less layer 0's data gradient."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from torch import nn  # noqa: E402

import drl_dronenavigation_amd as pkg  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
target = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "time_mlp_train.txt")
dev = torch.device("cuda:0")
lines = []
PEAK_BF16 = 2.5e15


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


def errors(got_out, got_grads, seq, x, d_out):
    """against the float64 evaluation on the device"""
    seq64 = nn.Sequential(*[nn.Linear(m.in_features, m.out_features) if isinstance(m, nn.Linear) else nn.Tanh() for m in seq]).to(dev).double()
    with torch.no_grad():
        for a, b in zip(seq64.parameters(), seq.parameters()):
            a.copy_(b.double())
    out64 = seq64(x.double())
    g64 = torch.autograd.grad(out64, list(seq64.parameters()), d_out.double())
    fwd = float((got_out.double() - out64).abs().max())
    grad = max(float((g.double() - r).abs().max() / r.abs().max()) for g, r in zip(got_grads, g64))
    return fwd, grad


say(f"device {torch.cuda.get_device_name(0)}, reps {reps}; MlpActorCritic(): actor 13-512-512-256-4 and critic 13-512-512-256-1, float32")
torch.manual_seed(0)
net = pkg.MlpActorCritic().to(dev)
with torch.no_grad():
    for p in net.parameters():
        p.add_(0.02 * torch.randn_like(p))
actor_seq, critic_seq = nn.Sequential(*net.pi, net.action_net), nn.Sequential(*net.vf, net.value_net)
products = sum(m.in_features * m.out_features for s in (actor_seq, critic_seq) for m in s if isinstance(m, nn.Linear))
first = sum(s[0].in_features * s[0].out_features for s in (actor_seq, critic_seq))
for rows, inner in ((4096, 10), (65536, 3)):
    gen = torch.Generator(device=dev).manual_seed(rows)
    x = torch.randn((rows, 13), generator=gen, device=dev)
    d_a = torch.randn((rows, 4), generator=gen, device=dev) / rows
    d_c = torch.randn((rows, 1), generator=gen, device=dev) / rows
    actor, critic = pkg.MlpTrainer.for_actor(net, rows), pkg.MlpTrainer.for_critic(net, rows)

    def kernel_pass():
        actor(x).backward(d_a)
        critic(x).backward(d_c)

    kernel_pass()
    torch.cuda.synchronize(dev)
    k_err = [errors(t.out[:rows], t.grads, s, x, d) for t, s, d in ((actor, actor_seq, d_a), (critic, critic_seq, d_c))]
    t_err = []
    for s, d in ((actor_seq, d_a), (critic_seq, d_c)):
        out = s(x)
        t_err.append(errors(out.detach(), torch.autograd.grad(out, list(s.parameters()), d), s, x, d))
    # the torch legs run on parameters of their own: MlpTrainer holds the .grad of the originals
    t_actor, t_critic = (nn.Sequential(*[nn.Linear(m.in_features, m.out_features) if isinstance(m, nn.Linear) else nn.Tanh() for m in s]).to(dev)
                         for s in (actor_seq, critic_seq))
    t_actor.load_state_dict(actor_seq.state_dict())
    t_critic.load_state_dict(critic_seq.state_dict())

    def torch_pass():
        t_actor(x).backward(d_a)
        t_critic(x).backward(d_c)

    torch_pass()
    fns = {"kernel eager": kernel_pass, "kernel graph": captured(kernel_pass).replay, "torch eager": torch_pass}
    refused = {}
    try:
        fns["torch graph"] = captured(torch_pass).replay
    except Exception as e:                                      # noqa: BLE001  (reported below, next to the numbers)
        refused["torch graph"] = f"{type(e).__name__}: {str(e).splitlines()[0][:160]}"
        torch.cuda.synchronize(dev)
    t = {k: [] for k in fns}
    for fn in fns.values():
        fn()
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, inner))
    m = {k: statistics.median(v) for k, v in t.items()}
    flop = 2.0 * rows * (3 * products - first)
    say(f"{rows} rows, {inner} passes per timing, {flop / 1e9:.1f} GFLOP a pass; MlpTrainer scratch {actor._need + critic._need} B")
    say("    " + " | ".join(f"{k} {spread(v)}" for k, v in t.items()))
    for leg, why in refused.items():
        say(f"    {leg}: torch did not capture it ({why})")
    say("    " + " | ".join(f"{k} {flop / (v * 1e-6) / 1e12:.1f} TFLOP/s" for k, v in m.items())
        + f"; the kernel issues 3 MFMAs a product: {100.0 * 3 * flop / (m['kernel graph'] * 1e-6) / PEAK_BF16:.1f} % of the 2.5 PFLOP/s bf16 peak")
    say("    torch over kernel: " + " | ".join(f"{k} / kernel {k.split()[1]} {m[k] / m['kernel ' + k.split()[1]]:.2f}" for k in m if k.startswith("torch")))
    for name, (kf, kg), (tf, tg) in zip(("actor", "critic"), k_err, t_err):
        say(f"    {name} against float64: forward error kernel {kf:.3e}, torch {tf:.3e}; largest normalised gradient error kernel {kg:.3e}, torch {tg:.3e}")
    del fns, actor, critic
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(target)), exist_ok=True)
with open(target, "w") as f:
    f.write("\n".join(lines) + "\n")
