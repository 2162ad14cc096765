#!/usr/bin/env python3
"""Device time of the LSTM layer through dn_lstm_forward / dn_lstm_backward (csrc/dn_lstm.hip, lstm_train.LstmTrainer / LstmStepper)
beside what it replaces -- float32 torch.nn.LSTM on the same tensors --, written to profiles/time_lstm.txt:
    python3 profiles/time_lstm.py [reps] [output file]
  forward + backward at (I, H, T, B) = (13, 256, 32, 1024) and (13, 64, 32, 4096), to the four parameter gradients and d_x, from a fixed
    gradient of h_seq, with episode starts in one cell of five; torch steps its nn.LSTM over the sequence with both states multiplied by
    1 - episode_start before every step (what sb3_contrib's _process_sequence does when a sequence holds starts), the kernels take the
    sequence in one call;
  the rollout step at 32 768 drones, (I, H) = (13, 256) and (13, 64): one T = 1 forward that updates the resident state in place.
Interleaved timing by timing, the median and the range of `reps` (default 15) timings, each one pair of events around INNER back-to-back
passes on the stream, over INNER: kernel eager / kernel graph (captured once and replayed) and torch eager / torch graph.
The largest errors of tests/test_gpu_lstm.py, which that file prints, are recorded at the end when the caller hands them over in the
environment (LSTM_ERRORS, one line of text)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import drl_dronenavigation_amd as pkg  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
target_file = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "time_lstm.txt")
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


def measure(title, kernel_pass, torch_pass, inner):
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
    say(f"{title}, {inner} passes per timing")
    say("    " + " | ".join(f"{k} {spread(v)}" for k, v in times.items()))
    med = {k: statistics.median(v) for k, v in times.items()}
    say("    torch over kernel: " + " | ".join(f"{a} / {b} {med[a] / med[b]:.2f}" for a, b in (("torch eager", "kernel eager"), ("torch graph", "kernel graph"))
                                              if a in med and b in med))


say(f"device {torch.cuda.get_device_name(dev)}, reps {reps}; torch.nn.LSTM(I, H), one layer, float32, default initialisation")
for I, H, T, B in ((13, 256, 32, 1024), (13, 64, 32, 4096)):
    torch.manual_seed(1)
    lstm = torch.nn.LSTM(I, H).to(dev)
    x = torch.randn(T, B, I, device=dev).requires_grad_()
    starts = (torch.rand(T, B, device=dev) < 0.2).to(torch.uint8)
    keep = (1.0 - starts.float()).unsqueeze(2)
    h0, c0 = 0.5 * torch.randn(B, H, device=dev), 0.5 * torch.randn(B, H, device=dev)
    d_hseq = torch.randn(T, B, H, device=dev) / (T * B)
    trainer = pkg.LstmTrainer(lstm, T, B)

    def kernel_pass():
        trainer(x, starts, h0, c0).backward(d_hseq)

    def torch_pass():
        h, c, hs = h0.unsqueeze(0), c0.unsqueeze(0), []
        for t in range(T):
            out, (h, c) = lstm(x[t:t + 1], (h * keep[t], c * keep[t]))
            hs.append(out)
        torch.cat(hs).backward(d_hseq)

    measure(f"forward + backward, I {I}, H {H}, T {T}, B {B}", kernel_pass, torch_pass, 3)
    x.grad = None

for I, H in ((13, 256), (13, 64)):
    N = 32768
    torch.manual_seed(2)
    lstm = torch.nn.LSTM(I, H).to(dev)
    x = torch.randn(N, I, device=dev)
    starts = (torch.rand(N, device=dev) < 0.01).to(torch.uint8)
    keep = (1.0 - starts.float()).unsqueeze(1)
    stepper = pkg.LstmStepper(lstm, N, dev)
    state = [torch.zeros(1, N, H, device=dev), torch.zeros(1, N, H, device=dev)]

    def kernel_step():
        stepper.step(x, starts)

    def torch_step():
        with torch.no_grad():
            _, (h, c) = lstm(x.unsqueeze(0), (state[0] * keep, state[1] * keep))
            state[0].copy_(h)
            state[1].copy_(c)

    measure(f"rollout step, I {I}, H {H}, {N} drones", kernel_step, torch_step, 10)

if os.environ.get("LSTM_ERRORS"):
    say("largest errors of tests/test_gpu_lstm.py against float64 (bar 1e-4): " + os.environ["LSTM_ERRORS"])
with open(target_file, "w") as f:
    f.write("\n".join(lines) + "\n")
