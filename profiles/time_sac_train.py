#!/usr/bin/env python3
"""Device time of the SAC networks' training pass through dn_sac_train_forward / dn_sac_train_backward (csrc/dn_sac_train.hip,
sac_train.SacTrainer) and of dn_polyak_update beside what they replace -- the float32 torch modules on the same tensors --, written to
profiles/time_sac_train.txt:
    python3 profiles/time_sac_train.py [reps] [output file]
One pass is every network pass of one SAC gradient step of SacActor() (13-256-256, heads 4 | 4) and SacCritic()
(2 x 17-256-256-128-1) from fixed gradients of the head outputs, without the loss heads and the optimisers:
  no grad    actor(next_obs); target(next_obs, a_next)
  critics    critic(obs, actions) forward + backward to the parameters
  actor      actor(obs) forward; critic(obs, a_pi) forward + backward to a_pi alone; actor backward to the parameters from (d_mean, d_log_std)
  polyak     target <- (1 - tau) target + tau critic
Per batch (256 and 65 536 rows, the shapes of time_sac_loss.txt), interleaved timing by timing, the median and the range of `reps`
(default 15) timings, each one pair of events around INNER back-to-back passes on the stream, over INNER:
  kernel eager / kernel graph    SacTrainer x 3 + PolyakUpdate, eager and captured once and replayed
  torch eager / torch graph      the modules, torch.cat for the critics' input, _foreach_mul_ / _foreach_add_ for the Polyak update"""
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import drl_dronenavigation_amd as pkg  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
target_file = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "time_sac_train.txt")
dev = torch.device("cuda:0")
lines = []


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
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph.replay


say(f"device {torch.cuda.get_device_name(dev)}, reps {reps}; SacActor() 13-256-256-(4 | 4) and SacCritic() 2 x 17-256-256-128-1, float32, ReLU")
for batch, inner in ((256, 20), (65536, 3)):
    torch.manual_seed(1)
    actor, critic = pkg.SacActor().to(dev), pkg.SacCritic().to(dev)
    target = copy.deepcopy(critic).requires_grad_(False)
    obs, next_obs = torch.randn(batch, 13, device=dev), torch.randn(batch, 13, device=dev)
    actions, a_next = torch.rand(batch, 4, device=dev) * 2 - 1, torch.rand(batch, 4, device=dev) * 2 - 1
    a_pi = (torch.rand(batch, 4, device=dev) * 2 - 1).requires_grad_()
    d_q = [torch.randn(batch, device=dev) / batch for _ in range(2)]
    d_head = [torch.randn(batch, 4, device=dev) / batch for _ in range(2)]
    actor_t, critic_t = pkg.SacTrainer.for_actor(actor, batch), pkg.SacTrainer.for_critics(critic, batch)
    target_t = pkg.SacTrainer.for_critics(target, batch, grads=False)
    polyak = pkg.PolyakUpdate(critic_t.params, list(target.parameters()), 0.005)
    t_params, c_params = list(target.parameters()), list(critic.parameters())

    def kernel_pass():
        with torch.no_grad():
            actor_t(next_obs)
            target_t(next_obs, a_next)
        heads = actor_t(obs)
        torch.autograd.backward(list(critic_t(obs, actions)), d_q)
        torch.autograd.backward(list(critic_t(obs, a_pi, param_grads=False)), d_q)
        torch.autograd.backward(list(heads), d_head)
        polyak.step()

    def torch_pass():
        with torch.no_grad():
            zn = actor.latent_pi(next_obs)
            actor.mu(zn), actor.log_std(zn)
            target(next_obs, a_next)
        z = actor.latent_pi(obs)
        heads = [actor.mu(z), actor.log_std(z)]
        torch.autograd.backward(list(critic(obs, actions)), d_q)
        torch.autograd.grad(list(critic(obs, a_pi)), [a_pi], d_q)
        torch.autograd.backward(heads, d_head)
        with torch.no_grad():
            torch._foreach_mul_(t_params, 1.0 - 0.005)
            torch._foreach_add_(t_params, c_params, alpha=0.005)

    kernel_pass()
    torch_pass()
    paths = {"kernel eager": kernel_pass, "torch eager": torch_pass}
    for name, step in (("kernel graph", kernel_pass), ("torch graph", torch_pass)):
        try:
            paths[name] = captured(step)
        except Exception as e:  # noqa: BLE001
            say(f"    {name}: capture refused ({type(e).__name__}: {str(e)[:80]})")
    times = {k: [] for k in paths}
    for _ in range(reps):
        for k, fn in paths.items():
            times[k].append(timed(fn, inner))
    say(f"{batch} rows, {inner} passes per timing")
    say("    " + " | ".join(f"{k} {spread(v)}" for k, v in times.items()))
    med = {k: statistics.median(v) for k, v in times.items()}
    say("    torch over kernel: " + " | ".join(f"{a} / {b} {med[a] / med[b]:.2f}" for a, b in (("torch eager", "kernel eager"), ("torch graph", "kernel graph"))
                                              if a in med and b in med))
with open(target_file, "w") as f:
    f.write("\n".join(lines) + "\n")
