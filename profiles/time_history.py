#!/usr/bin/env python3
"""Device time of dn_stack_history (csrc/dn_history.hip) beside two references, written to profiles/time_history.txt:
    python3 profiles/time_history.py [reps]
Inputs are an env's own outputs (reaching track, the normaliser on, max_steps=64, uniform actions in [-1, 1]).  The fleet starts together,
so the time limit ends its episodes together: the K = 64 launch holds one such step (done rate 1 / 64), the single step timed holds none
(the measured done rate is printed; the microbenchmark below ends 3 % of the episodes at every step).  Configurations F = 4, A = 3 (W = 64) and F = 3, A = 2 with the 8 goal columns (W = 56), at
N = 32 768 with K = 1 and K = 64 and at N = 2 097 152 with K = 1.  Per configuration, interleaved launch by launch, the median of `reps`
(default 25):
  kernel   one dn_stack_history launch with terminal rows
  copy     dn_stream_copy of the same algorithmic bytes: per drone-step reads of 52 + 16 + 1 + 4 E and writes of 4 W bytes, the terminal
           parts (52 + 4 E read, 4 W written) weighted by the measured done rate, and `prev` (4 W) once per drone and launch; the copy
           moves half of that sum in and half out
  torch    the torch composition it replaces (cat / where per step; for K = 64 the Python loop over K)
dn_stack_history takes no env, so the launch-event hook of the step kernels does not reach it: every figure is one pair of events around
INNER back-to-back launches on the stream, over INNER -- kernel and copy alike, so both carry the same dispatch gap (kernel-only times of
the kernel forms: profiles/microbench/history_forms.hip).  Last, RolloutCollector.collect() at 32 768 drones, n_steps = 32, a fused
float16-grade policy (deterministic actions) on W = 64 rows: policy_input="history" against the same collector over an env that stacks with the torch composition."""
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
from drl_dronenavigation_amd.policy_mfma import FusedMlpPolicy  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 25
dev = torch.device("cuda:0")
lib = _capi.load()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def torch_stack(P, o, a, d, tau, x, xt, F, A):
    """One step of the rule in torch: (row, terminal row -- valid where done)."""
    n, oe, ae = P.shape[0], 13 * F, 13 * F + 4 * A
    so, sa = P[:, 13:oe], P[:, oe + 4:ae]
    tail = [] if x is None else [x]
    pad = P.shape[1] - ae - (0 if x is None else x.shape[1])
    z = [torch.zeros((n, pad), dtype=P.dtype, device=P.device)] if pad else []
    act = [sa, a] if A else []
    cont = torch.cat([so, o] + act + tail + z, dim=1)
    fresh = torch.cat([torch.zeros_like(so), o, torch.zeros((n, 4 * A), dtype=P.dtype, device=P.device)] + tail + z, dim=1)
    term = torch.cat([so, tau] + act + ([] if xt is None else [xt]) + z, dim=1)
    return torch.where(d.bool()[:, None], fresh, cont), term


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


say(f"device {torch.cuda.get_device_name(0)}, reps {reps}")
for n, K in ((32768, 1), (32768, 64), (2097152, 1)):
    inner = 10 if n * K <= 32768 else 3 if K == 1 else 1
    for F, A, goal in ((4, 3, False), (3, 2, True)):
        hist = pkg.HistoryObservation(frames=F, actions=A, goal=goal)
        E, W = hist.extra_dim, hist.width()
        kw = dict(goal=pkg.GoalObservation(frame="world")) if goal else {}
        env = pkg.DroneVecEnv(tracks.reaching(), n, normalize_obs=True, max_steps=64, seed=1, device=dev, history=hist, **kw)
        env.reset_tensor()
        warm = torch.rand((40, n, 4), device=dev) * 2 - 1 if n <= 32768 else torch.rand((1, n, 4), device=dev) * 2 - 1
        for w in warm:                                   # spread the episode ends over the steps
            env.step_tensor(w)
        acts = torch.rand((K, n, 4), device=dev) * 2 - 1
        if K == 1:
            o, _, d, info = env.step_tensor(acts[0])
            out = dict(obs=o[None], done=d[None], terminal_obs=info["terminal_obs"][None])
            if goal:
                out.update(goal=info["goal"][None], terminal_goal=info["terminal_goal"][None])
            out = {k: v.clone() for k, v in out.items()}
        else:
            out = env.rollout_tensor(acts, want_terminal=True)
        prev = torch.randn((n, W), device=dev)
        rows, trows = torch.empty((K, n, W), device=dev), torch.empty((K, n, W), device=dev)
        rate = float(out["done"].float().mean())
        cfg = hist.to_c()
        x, xt = (out["goal"], out["terminal_goal"]) if goal else (None, None)
        ptr = [t.data_ptr() if t is not None else None for t in (prev, out["obs"], acts, out["done"], out["terminal_obs"], x, xt, rows, trows)]

        def kernel():
            _capi.check(lib.dn_stack_history(C.byref(cfg), K, n, *ptr, 0, stream()))

        algo = K * n * (52 + 16 + 1 + 4 * E + 4 * W + rate * (52 + 4 * E + 4 * W)) + n * 4 * W
        half = int(algo / 2) // 16 * 16
        src, dst = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)

        def copy():
            _capi.check(lib.dn_stream_copy(dst.data_ptr(), src.data_ptr(), half, 0, stream()))

        def composed():
            P = prev
            for t in range(K):
                rows[t], trows[t] = torch_stack(P, out["obs"][t], acts[t], out["done"][t], out["terminal_obs"][t],
                                                None if x is None else x[t], None if xt is None else xt[t], F, A)
                P = rows[t]

        composed()
        want = rows.clone()
        kernel()
        torch.cuda.synchronize(dev)
        assert torch.equal(rows.view(torch.int32), want.view(torch.int32)), "the torch composition and the kernel disagree"
        t = {"kernel": [], "copy": [], "torch": []}
        for _ in range(reps):
            t["kernel"].append(timed(kernel, inner))
            t["copy"].append(timed(copy, inner))
            t["torch"].append(timed(composed, 1))
        k_us, c_us, t_us = med(t["kernel"]), med(t["copy"]), med(t["torch"])
        say(f"F={F} A={A} E={E} W={W} N={n} K={K} done rate {rate:.4f} algorithmic {algo / 1e6:.1f} MB | kernel {k_us:.2f} us "
            f"({algo / k_us / 1e3:.0f} GB/s) | copy {c_us:.2f} us ({algo / c_us / 1e3:.0f} GB/s) | torch {t_us:.1f} us | "
            f"kernel / copy {k_us / c_us:.2f} | torch / kernel {t_us / k_us:.1f}")
        env.close()
        del env, out, rows, trows, prev, acts, warm, src, dst, want
        torch.cuda.empty_cache()


class TorchHistoryEnv(pkg.DroneVecEnv):
    """The env without the option, its history rows composed in torch after every step: what a user writes today."""

    def __init__(self, *args, frames, actions, **kw):
        super().__init__(*args, **kw)
        self._fa = (frames, actions)
        w = (13 * frames + 4 * actions + 3) // 4 * 4
        self.history = torch.zeros((self.num_envs, w), dtype=torch.float32, device=self.device)
        self._term_hist = torch.zeros_like(self.history)

    def reset_tensor(self):
        obs = super().reset_tensor()
        if getattr(self, "_fa", None) is not None:
            F, A = self._fa
            self.history.zero_()
            self.history[:, 13 * (F - 1):13 * F] = obs
        return obs

    def step_tensor(self, actions, want_terminal=True):
        obs, reward, done, info = super().step_tensor(actions, want_terminal)
        row, term = torch_stack(self.history, obs, actions, done, info["terminal_obs"], None, None, *self._fa)
        self.history.copy_(row)
        self._term_hist.copy_(term)
        info.update(history=self.history, terminal_history=self._term_hist)
        return obs, reward, done, info


n, T = 32768, 32
net = pkg.MlpActorCritic(obs_dim=64).to(dev)
common = dict(normalize_obs=True, max_steps=64, seed=1, device=dev)
envs = {"kernel": pkg.DroneVecEnv(tracks.reaching(), n, history=pkg.HistoryObservation(frames=4, actions=3), **common),
        "torch": TorchHistoryEnv(tracks.reaching(), n, frames=4, actions=3, **common)}
for use_graph in (False, True):
    cols, t = {}, {}
    for name, env in envs.items():
        pol = FusedMlpPolicy(net, n, dev, grade="fp16")
        cols[name] = RolloutCollector(env, lambda x, pol=pol: pol(x, deterministic=True), T, policy_input="history", use_graph=use_graph)
        t[name] = []
        for _ in range(3):
            cols[name].collect()
    torch.cuda.synchronize(dev)
    for _ in range(reps):
        for name, col in cols.items():
            t[name].append(timed(col.collect, 1) / 1e3)
    say(f"RolloutCollector.collect() N={n} n_steps={T} W=64 fused fp16 policy, use_graph={use_graph}: policy_input='history' "
        f"{med(t['kernel']):.2f} ms | torch composition {med(t['torch']):.2f} ms | ratio {med(t['torch']) / med(t['kernel']):.2f}")
with open(os.path.join(ROOT, "profiles", "time_history.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
