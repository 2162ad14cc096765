#!/usr/bin/env python3
"""Device time of the step kernels with and without the privileged rows (dn_enable_privileged), interleaved A/B:
    python3 profiles/time_privileged.py [reps] [configs]    (configs: a comma list of sens, priv-obs, priv-all; default all)
The A/B against another tree (no privileged rows) runs `sens` from a checkout of each tree in turn.
Each launch is timed by the two events dn_set_launch_events attaches to its own dispatch (the kernel alone, as a kernel trace sees it);
per configuration the median over `reps` launches, the configurations interleaved launch by launch.  At 32 768 and 262 144 drones, the fused
launch (K = 64, us per vector step) and the single step (us per launch):
  sens       zero_damping=True, dynamics randomisation (every range +-20 %), gusty wind (steady speed [0.5, 6] m/s, sigma = (0.8, 0.3) m/s,
             tau = 0.25 s), ActuatorModel(latency=(0, 8)) and SensorModel(latency=(0, 8), bias=0.02): the sensor family, what a sim-to-real
             user runs without the feature (profiles/time_sensor.py's sens+lat+bias)
  priv-obs   the same with PrivilegedObservation(groups=("obs",)): the privileged family, 64 + 4 bytes stored per drone-step
  priv-all   the same with every group: 208 bytes stored per drone-step and a 64-byte reload of the bias
The fused launch is timed twice: `fused` without want_terminal (no terminal_obs / ep_return / ep_length / done_mask, and step rows only:
no terminal rows are bound) and `fused_term` with want_terminal=True (those four outputs in every configuration, and the terminal rows
bound as well), which is what a collector that bootstraps truncated episodes runs.  The single steps are step_tensor's default,
want_terminal=True: both row buffers bound.
Uniform actions in [-1, 1] with max_steps=64: episodes end (and redraw) throughout."""
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import drl_dronenavigation_amd as pkg  # noqa: E402
from drl_dronenavigation_amd import _capi, tracks  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 25
dev = torch.device("cuda:0")
lib = _capi.load()
STEADY = dict(speed=(0.5, 6.0), azimuth=(-math.pi, math.pi), vertical=(-0.5, 0.5))
GUST = dict(gust_sigma=(0.8, 0.3), gust_tau=0.25)
RANGE = (0.8, 1.2)
GROUPS = {"priv-obs": ("obs",), "priv-all": ("obs", "dyn", "wind", "act", "sens")}


def make(name, n):
    kw = dict(max_steps=64, seed=1, device=dev, wind=pkg.WindDisturbance(**STEADY, **GUST),
              dynamics=pkg.DynamicsRandomization(mass=RANGE, inertia=RANGE, kf=RANGE, km=RANGE), actuator=pkg.ActuatorModel(latency=(0, 8)),
              sensor=pkg.SensorModel(latency=(0, 8), bias=0.02))
    if name in GROUPS:
        kw["privileged"] = pkg.PrivilegedObservation(groups=GROUPS[name])
    os.environ["DN_WAVES"] = "1"
    try:
        return pkg.DroneVecEnv(tracks.reaching(), n, normalize_obs=True, zero_damping=True, **kw)
    finally:
        os.environ.pop("DN_WAVES", None)


def timed(env, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); e1.record()                                 # torch only reads the times of events it saw recorded
    torch.cuda.synchronize(dev)
    _capi.check(lib.dn_set_launch_events(env._handle, C.c_void_p(e0.cuda_event), C.c_void_p(e1.cuda_event)))
    fn()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) * 1e3


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
results = {"library": os.path.relpath(_capi.library_path(), ROOT), "device": torch.cuda.get_device_name(0), "reps": reps, "sizes": {}}
names = tuple(sys.argv[2].split(",")) if len(sys.argv) > 2 else ("sens", "priv-obs", "priv-all")
for n in (32768, 262144):
    K = 64
    envs = {nm: make(nm, n) for nm in names}
    for e in envs.values():
        e.reset_tensor()
    acts = torch.rand((K, n, 4), device=dev) * 2 - 1
    one = acts[0].contiguous()
    # one set of output buffers for every env (the launches are serial), from an env that hands out the privileged rows if there is one
    widest = envs[[nm for nm in names if nm in GROUPS][-1] if any(nm in GROUPS for nm in names) else names[0]]
    out, out_term = widest.rollout_tensor(acts), widest.rollout_tensor(acts, want_terminal=True)
    for e in envs.values():                                  # warm-up
        e.rollout_tensor(acts, out=out)
        e.rollout_tensor(acts, out=out_term)
        e.step_tensor(one)
    torch.cuda.synchronize(dev)
    t = {nm: {"fused": [], "fused_term": [], "single": []} for nm in names}
    for _ in range(reps):
        for nm, e in envs.items():
            t[nm]["fused"].append(timed(e, lambda: e.rollout_tensor(acts, out=out)) / K)
            t[nm]["fused_term"].append(timed(e, lambda: e.rollout_tensor(acts, out=out_term)) / K)
            t[nm]["single"].append(timed(e, lambda: e.step_tensor(one)))
    row = {}
    for nm, e in envs.items():
        row[nm] = {"waves_fused": e.kernel_waves(fused=True), "waves_single": e.kernel_waves(fused=False),
                   "fused_k64_us_per_step": round(statistics.median(t[nm]["fused"]), 4),
                   "fused_term_k64_us_per_step": round(statistics.median(t[nm]["fused_term"]), 4),
                   "single_us_per_launch": round(statistics.median(t[nm]["single"]), 3)}
    if "sens" in envs:
        for kind, key in (("fused", "fused_k64_us_per_step"), ("fused_term", "fused_term_k64_us_per_step"), ("single", "single_us_per_launch")):
            for nm in GROUPS:
                if nm in envs:
                    row[f"{nm}_over_sens_{kind}"] = round(row[nm][key] / row["sens"][key], 4)
    results["sizes"][str(n)] = row
    print(json.dumps({str(n): row}), flush=True)
    for e in envs.values():
        e.close()
    del out, out_term, acts, one
    torch.cuda.empty_cache()
print(json.dumps(results))
