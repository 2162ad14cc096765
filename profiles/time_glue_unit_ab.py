#!/usr/bin/env python3
"""Device time of the three rollout-glue kernels whose text the glue unit changed, the parent commit's library against this build:
    python3 profiles/time_glue_unit_ab.py PARENT_LIBRARY [rounds] [output file]    the table, written to profiles/time_glue_unit_ab.txt
    python3 profiles/time_glue_unit_ab.py run                                     one timed run of one build (DN_LIB_PATH picks it)
A round is one run of the parent's library and one of this build, each a fresh child process; the rounds alternate the two on one device.
A run times dn_pack_done, dn_compact_done (5 % of the fleet finished, the records of tests/rollout_glue_support.py) and dn_policy_sample at
32 768 and 2 097 152 drones, each as the eager call and as the same call captured once in a graph and replayed (at the small fleet the
eager line is the host's launch path, the graph line the device's): per line REPS timings, each one pair of events around INNER
back-to-back calls on the stream, over INNER; the run's figure is their median.  This build's median of run medians is held to the spread of the parent's own run medians."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
FLEETS, REPS, SEED = (32768, 2097152), 15, 3


def run():
    import numpy as np
    import torch

    import drl_dronenavigation_amd as pkg
    import rollout_glue_support as R
    from drl_dronenavigation_amd import _capi, tracks

    dev = torch.device("cuda:0")
    lib = _capi.load()
    to = lambda a: torch.from_numpy(np.array(a, order="C")).to(dev)  # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) * 1e3 / inner

    figures = {}
    for n in FLEETS:
        inner = 200 if n <= 65536 else 20
        tobs, ep_ret, ep_len, trunc, found = (to(x) for x in R.pack_inputs(n))
        mask = to(R.mask_words(R.done_bits(n, 0.05), n))
        idx, cnt, packed = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros((n, 16), device=dev)
        env = pkg.DroneVecEnv(tracks.reaching(), n, device=dev)
        env.reset_tensor()
        mean, ls = torch.randn((n, 4), generator=torch.Generator(device=dev).manual_seed(SEED), device=dev), (C.c_float * 4)(-1.0, -2.0, -0.5, -3.0)
        a, c, lp = torch.empty((n, 4), device=dev), torch.empty((n, 4), device=dev), torch.empty(n, device=dev)
        fns = {
            "dn_pack_done": lambda: _capi.check(lib.dn_pack_done(mask.data_ptr(), n, tobs.data_ptr(), ep_ret.data_ptr(), ep_len.data_ptr(), trunc.data_ptr(),
                                                                 found.data_ptr(), idx.data_ptr(), cnt.data_ptr(), packed.data_ptr(), 0, stream())),
            "dn_compact_done": lambda: _capi.check(lib.dn_compact_done(mask.data_ptr(), n, idx.data_ptr(), cnt.data_ptr(), 0, stream())),
            "dn_policy_sample": lambda: _capi.check(lib.dn_policy_sample(env._handle, mean.data_ptr(), ls, SEED, 0, a.data_ptr(), c.data_ptr(),
                                                                         lp.data_ptr(), stream())),
        }
        for fn in list(fns.values()):                              # every path before the timed window and before its capture
            for _ in range(10):
                fn()
        torch.cuda.synchronize(dev)
        for k, fn in list(fns.items()):                            # the same call captured once and replayed: the device's time
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                fn()
            fns[k + " graph"] = graph.replay
        t = {k: [] for k in fns}
        for _ in range(REPS):
            for k, fn in fns.items():
                t[k].append(timed(fn, inner))
        for k, v in t.items():
            figures[f"{k} N={n}"] = [statistics.median(v), min(v), max(v)]
        env.close()
    print("FIGURES " + json.dumps(figures), flush=True)


def table(parent_library, rounds, target):
    sides = {"parent": dict(os.environ, DN_LIB_PATH=os.path.abspath(parent_library)),
             "this build": {k: v for k, v in os.environ.items() if k != "DN_LIB_PATH"}}
    runs = {s: [] for s in sides}
    for r in range(rounds):
        for s, env in sides.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "run"], env=env, check=True, timeout=300, capture_output=True, text=True).stdout
            runs[s].append(json.loads(next(line for line in out.splitlines() if line.startswith("FIGURES "))[8:]))
            print(f"round {r + 1}, {s}: done", flush=True)
    lines = [f"# dn_pack_done, dn_compact_done and dn_policy_sample, the parent commit's library (through DN_LIB_PATH) against this build: {rounds} rounds of one run",
             f"# each, alternated on one device.  us a call.  A run's figure is its median of {REPS} timings.  'parent runs': the smallest and largest of the parent's",
             "# run medians, the spread this build's median of run medians is held to; 'parent timings': the parent's smallest and largest single timing.",
             "| line | parent median | parent runs | parent timings | this build median | this build runs | inside parent runs / timings |", "|---|---|---|---|---|---|---|"]
    ok = True
    for line in runs["parent"][0]:
        p, q = [x[line] for x in runs["parent"]], [x[line] for x in runs["this build"]]
        pm, qm = [x[0] for x in p], [x[0] for x in q]
        med = statistics.median(qm)
        in_runs, in_timings = min(pm) <= med <= max(pm), min(x[1] for x in p) <= med <= max(x[2] for x in p)
        ok &= in_runs
        lines.append(f"| {line} | {statistics.median(pm):.2f} | {min(pm):.2f} - {max(pm):.2f} | {min(x[1] for x in p):.2f} - {max(x[2] for x in p):.2f} | {med:.2f} | "
                     f"{min(qm):.2f} - {max(qm):.2f} | {'yes' if in_runs else 'no'} / {'yes' if in_timings else 'no'} |")
    lines.append("# run medians in the order parent [..] this build [..]:")
    for line in runs["parent"][0]:
        lines.append(f"#   {line} {[round(x[line][0], 2) for x in runs['parent']]} {[round(x[line][0], 2) for x in runs['this build']]}")
    print("\n".join(lines))
    with open(target, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1] == "run":
        sys.exit(run())
    sys.exit(table(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 8,
                   sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "time_glue_unit_ab.txt")))
