#!/usr/bin/env python3
"""Device time of the SAC loss heads (csrc/dn_sac_loss.hip, sac.SacPolicyHead / SacCriticLoss / SacActorLoss) beside the float32 torch
composition they replace, written to profiles/time_sac_loss.txt:
    python3 profiles/time_sac_loss.py [reps] [output file]
The workload: one full loss pass of a SAC gradient step over B in {256, 65536} rows, A = 4 action columns, C = 2 critics, gamma 0.99,
target_entropy -4, a learned ent_coef -- the policy head on obs (with gradient) and on next_obs (without), the critic loss with its
backward to q_c, and the actor and entropy-coefficient loss with their backward to mean and log_std through the head and to log_ent_coef.
The networks are replaced by leaf tensors (mean, log_std, q_c) and, where a critic must see the actions, by a fixed linear stand-in
q = actions @ w_c + b_c, the same in both paths, so what is timed is the losses and nothing of a network.  Per shape, interleaved call by
call, the median and the range of `reps` (default 15) timings, each one pair of events around INNER back-to-back passes, over INNER:
  kernel eager   the three heads and their autograd glue
  kernel graph   the same captured once and replayed
  torch eager    SacActor.squash and SB3's SAC.train expressions [from recall] in float32 torch, on the same tensors
  torch graph    the same captured once and replayed
Before the timings both paths are held against the float64 composition on the CPU: the largest error of the gradients, over the largest
gradient."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import drl_dronenavigation_amd as pkg  # noqa: E402
from drl_dronenavigation_amd.policy import LOG_STD_MAX, LOG_STD_MIN, SacActor  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
target = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "time_sac_loss.txt")
dev = torch.device("cuda:0")
lines = []
A, C, INNER, GAMMA, TARGET_ENTROPY = 4, 2, 10, 0.99, -4.0


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


def composition(t, squash):
    """SB3 SAC.train's losses [from recall] in the dtype of the tensors of t: (critic_loss, actor_loss + ent_coef_loss)."""
    a_pi, lp = squash(t["mean"], t["log_std"], t["eps"])
    lec = t["lec"]
    ent_coef = torch.exp(lec.detach())
    ent_coef_loss = -(lec * (lp + TARGET_ENTROPY).detach()).mean()
    with torch.no_grad():
        a_n, lp_n = squash(t["mean_n"], t["log_std_n"], t["eps_n"])
        nq = torch.min(torch.stack([a_n @ w + b for w, b in zip(t["w_t"], t["b"])]), dim=0).values
        y = t["rewards"] + (1.0 - t["dones"]) * GAMMA * (nq - ent_coef * lp_n)
    critic_loss = 0.5 * sum(((q - y) ** 2).mean() for q in t["q"])
    q_pi = torch.min(torch.stack([a_pi @ w + b for w, b in zip(t["w"], t["b"])]), dim=0).values
    return critic_loss, (ent_coef * lp - q_pi).mean() + ent_coef_loss


def literal(mean, raw, eps):
    return SacActor.squash(mean, torch.clamp(raw, LOG_STD_MIN, LOG_STD_MAX), eps)


def stable(mean, raw, eps):
    """The forms of include/dronenav.h, for the float64 yardstick."""
    ls = torch.clamp(raw, LOG_STD_MIN, LOG_STD_MAX)
    pre = mean + torch.exp(ls) * eps
    t = torch.exp(-2.0 * pre.abs())
    J = 4.0 * t / ((1.0 + t) * (1.0 + t))
    return torch.tanh(pre), (-0.5 * eps * eps - ls - 0.9189385332046727 - torch.log(J + 1e-6)).sum(-1)


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


say(f"device {torch.cuda.get_device_name(0)}, reps {reps}, {INNER} full loss passes per timing; act_dim {A}, n_critics {C}, gamma {GAMMA}, "
    f"target_entropy {TARGET_ENTROPY}, learned ent_coef")
for B in (256, 65536):
    g = torch.Generator(device=dev).manual_seed(B)
    rn = lambda *s: torch.randn(s, generator=g, device=dev)  # noqa: E731
    t = dict(mean=rn(B, A).requires_grad_(), log_std=(-1.25 + 0.9 * rn(B, A)).requires_grad_(), eps=rn(B, A), mean_n=rn(B, A),
             log_std_n=-1.25 + 0.9 * rn(B, A), eps_n=rn(B, A), q=[(5.0 + 2.0 * rn(B)).requires_grad_() for _ in range(C)],
             w=[rn(A) for _ in range(C)], w_t=[rn(A) for _ in range(C)], b=[rn(1) for _ in range(C)], rewards=rn(B),
             dones=(torch.rand(B, generator=g, device=dev) < 0.3).float(), lec=torch.log(torch.full((1,), 0.3, device=dev)).requires_grad_())
    leaves = [t["mean"], t["log_std"], t["lec"]] + t["q"]
    head, head_n = pkg.SacPolicyHead(B, A, dev), pkg.SacPolicyHead(B, A, dev)
    crit = pkg.SacCriticLoss(B, dev, n_critics=C, gamma=GAMMA)
    act = pkg.SacActorLoss(B, dev, n_critics=C, target_entropy=TARGET_ENTROPY)
    batch = dict(rewards=t["rewards"], dones=t["dones"])

    def kernel_step():
        for x in leaves:
            x.grad = None
        a_pi, lp = head(t["mean"], t["log_std"], t["eps"])
        with torch.no_grad():
            a_n, lp_n = head_n(t["mean_n"], t["log_std_n"], t["eps_n"])
            next_q = [a_n @ w + b for w, b in zip(t["w_t"], t["b"])]
        crit(t["q"], next_q, lp_n, batch, t["lec"]).backward()
        actor_loss, ent_coef_loss = act(lp, [a_pi @ w + b for w, b in zip(t["w"], t["b"])], t["lec"])
        (actor_loss + ent_coef_loss).backward()

    def torch_step():
        for x in leaves:
            x.grad = None
        critic_loss, rest = composition(t, literal)
        critic_loss.backward()
        rest.backward()

    # both paths against the float64 composition on the CPU
    t64 = {k: ([x.detach().double().cpu() for x in v] if isinstance(v, list) else v.detach().double().cpu()) for k, v in t.items()}
    for k in ("mean", "log_std", "lec"):
        t64[k].requires_grad_()
    for x in t64["q"]:
        x.requires_grad_()
    leaves64 = [t64["mean"], t64["log_std"], t64["lec"]] + t64["q"]
    critic_loss, rest = composition(t64, stable)
    critic_loss.backward()
    rest.backward()
    top = max(float(x.grad.abs().max()) for x in leaves64)
    err = {}
    for name, step in (("kernel", kernel_step), ("torch", torch_step)):
        step()
        torch.cuda.synchronize(dev)
        err[name] = max(float((x.grad.double().cpu() - x64.grad).abs().max()) for x, x64 in zip(leaves, leaves64)) / top

    graphs = {"kernel": captured(kernel_step), "torch": captured(torch_step)}
    fns = {"kernel eager": kernel_step, "kernel graph": graphs["kernel"].replay, "torch eager": torch_step, "torch graph": graphs["torch"].replay}
    times = {k: [] for k in fns}
    for fn in fns.values():                                     # every path once more before the timed window
        fn()
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(timed(fn, INNER))
    m = {k: statistics.median(v) for k, v in times.items()}
    say(f"B {B} | " + " | ".join(f"{k} {spread(v)}" for k, v in times.items()))
    say(f"    torch / kernel eager {m['torch eager'] / m['kernel eager']:.2f} | torch / kernel graph {m['torch graph'] / m['kernel graph']:.2f} | "
        f"gradients against the float64 composition, of the largest: kernel {err['kernel']:.2e}, torch {err['torch']:.2e}")
    del graphs, head, head_n, crit, act
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(target)), exist_ok=True)
with open(target, "w") as f:
    f.write("\n".join(lines) + "\n")
