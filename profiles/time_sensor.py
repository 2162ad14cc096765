#!/usr/bin/env python3
"""Device time of the step kernels with and without the per-drone sensor model (dn_enable_sensor), interleaved A/B:
    python3 profiles/time_sensor.py [reps] [configs]    (configs: a comma list of act, sens-off, sens+lat, sens+lat+bias, opt, ref; default all)
The A/B against another tree (no sensor model) runs `act,opt,ref` from a checkout of each tree in turn.
Each launch is timed by the two events dn_set_launch_events attaches to its own dispatch (the kernel alone, as a kernel trace sees it);
per configuration the median over `reps` launches, the configurations interleaved launch by launch.  At 32 768 and 262 144 drones, the fused
launch (K = 64, us per vector step) and the single step (us per launch):
  act            zero_damping=True, dynamics randomisation (every range +-20 %), gusty wind (steady speed [0.5, 6] m/s, sigma = (0.8, 0.3)
                 m/s, tau = 0.25 s) and ActuatorModel(latency=(0, 8)): the actuator family, what a sim-to-real user runs without the sensor
  sens-off       the same with SensorModel(): the sensor family with latency [0, 0] and zero bias (both branches off)
  sens+lat       the same with sensor latency [0, 8]: one 64-byte row store and one gathered 64-byte row load per drone-step
  sens+lat+bias  the same with a bias amplitude of 0.02 on every column as well: one more 64-byte load and 13 adds per drone-step
  opt          zero_damping=True, DN_WAVES=1, no feature: the one-wave option kernel
  ref          the reference configuration (normaliser on), dn_create's own shape pick
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


def make(name, n):
    kw = dict(max_steps=64, seed=1, device=dev)
    if name == "ref":
        os.environ.pop("DN_WAVES", None)
        return pkg.DroneVecEnv(tracks.reaching(), n, normalize_obs=True, **kw)
    os.environ["DN_WAVES"] = "1"
    if name != "opt":
        kw["wind"] = pkg.WindDisturbance(**STEADY, **GUST)
        kw["dynamics"] = pkg.DynamicsRandomization(mass=RANGE, inertia=RANGE, kf=RANGE, km=RANGE)
        kw["actuator"] = pkg.ActuatorModel(latency=(0, 8))
    if name == "sens-off":
        kw["sensor"] = pkg.SensorModel()
    elif name == "sens+lat":
        kw["sensor"] = pkg.SensorModel(latency=(0, 8))
    elif name == "sens+lat+bias":
        kw["sensor"] = pkg.SensorModel(latency=(0, 8), bias=0.02)
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


results = {"library": _capi.library_path(), "device": torch.cuda.get_device_name(0), "reps": reps, "sizes": {}}
names = tuple(sys.argv[2].split(",")) if len(sys.argv) > 2 else ("act", "sens-off", "sens+lat", "sens+lat+bias", "opt", "ref")
for n in (32768, 262144):
    K = 64
    envs = {nm: make(nm, n) for nm in names}
    for e in envs.values():
        e.reset_tensor()
    acts = torch.rand((K, n, 4), device=dev) * 2 - 1
    one = acts[0].contiguous()
    out = next(iter(envs.values())).rollout_tensor(acts)                   # one set of output buffers for every env (the launches are serial)
    for e in envs.values():                                  # warm-up
        e.rollout_tensor(acts, out=out)
        e.step_tensor(one)
    torch.cuda.synchronize(dev)
    t = {nm: {"fused": [], "single": []} for nm in names}
    for _ in range(reps):
        for nm, e in envs.items():
            t[nm]["fused"].append(timed(e, lambda: e.rollout_tensor(acts, out=out)) / K)
            t[nm]["single"].append(timed(e, lambda: e.step_tensor(one)))
    row = {}
    for nm, e in envs.items():
        row[nm] = {"waves_fused": e.kernel_waves(fused=True), "waves_single": e.kernel_waves(fused=False),
                   "fused_k64_us_per_step": round(statistics.median(t[nm]["fused"]), 4),
                   "single_us_per_launch": round(statistics.median(t[nm]["single"]), 3)}
    if "act" in envs:
        for kind, key in (("fused", "fused_k64_us_per_step"), ("single", "single_us_per_launch")):
            for nm in ("sens-off", "sens+lat", "sens+lat+bias"):
                if nm in envs:
                    row[f"{nm}_over_act_{kind}"] = round(row[nm][key] / row["act"][key], 4)
    results["sizes"][str(n)] = row
    print(json.dumps({str(n): row}), flush=True)
    for e in envs.values():
        e.close()
    del out, acts, one
    torch.cuda.empty_cache()
print(json.dumps(results))
