"""What the tests of the per-drone models (dynamics, wind, actuator, sensor, privileged observations) share and what needs neither a
GPU nor torch nor scipy: numpy and oracle.oracle alone.  A plain module like tests/rigid_body_ref.py -- pytest does not collect it and
does not rewrite its asserts, so every assert here carries its own message.  tests/gpu_support.py holds what needs torch and the package.

Sections: constants; action streams; Philox, noise, ulp distance, bit view; the documented draws as the GPU tests restate them; the
sensor's delivery rule and the float64 normaliser; what the package's model objects carry, for the oracle; the draws as the oracle
tests restate them; the actuator and sensor configurations the oracle files cover on the CPU and the GPU files fly; GPU outputs
against the oracle's."""
import ctypes as C
import math
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                   # as tests/conftest.py does: the module also imports outside a pytest run
    sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402

# ---- constants ------------------------------------------------------------------------------------------------------------------
DT = 1.0 / 240.0
WIDE = [-1e4, -1e4, -1e4, 1e4, 1e4, 1e4]
STATE_KEYS = ("pos", "quat", "vel", "ang_v", "prev_vel", "prev_ang_v", "cur_pos", "d", "d_prev", "idx", "steps", "just_found", "ep_ret",
              "ep_len", "rms_mean", "rms_var", "rms_count", "rms_m2", "last_rpm", "ep_ret_lo")
BODY_KEYS = tuple(k for k in STATE_KEYS if not k.startswith("rms_"))       # the state outside the normaliser's statistics
STATE_F32 = ("pos", "quat", "vel", "ang_v", "prev_vel", "prev_ang_v", "cur_pos", "d", "d_prev")
BODY = dict(mass=(0.7, 1.3), inertia=(0.7, 1.3), kf=(0.8, 1.2), km=(0.7, 1.3))
ZERO = dict(speed=(0.0, 0.0), azimuth=(0.0, 0.0), vertical=(0.0, 0.0), gust_sigma=(0.0, 0.0))
GUSTY = dict(speed=(0.5, 6.0), azimuth=(-math.pi, math.pi), vertical=(-0.5, 0.5), gust_sigma=(0.8, 0.3), gust_tau=0.25)
NOISE = dict(obs_noise_sigma=0.01, act_noise_sigma=0.001)
HOVER_FILL = (0.0922, 0.0922, 0.0922, 0.0922)         # normalised hover
FULL = dict(latency=(0, 8), motor_tau=(0.02, 0.15), fill=HOVER_FILL)       # the actuator model with latency and lag on together
AMPS = (0.02, 0.02, 0.03, 0.01, 0.01, 0.04, 0.05, 0.05, 0.05, 0.1, 0.1, 0.1, 0.02)
SENSOR = dict(latency=(0, 8), bias=AMPS)
RTOL = ATOL = 1e-5          # the project's observation bar
# pwm2rpm over the PWM range [20000, 65535] (env_utils.py:39, :58): the span of the speeds the chain can command
RPM_SPAN = 0.2685 * (65535.0 - 20000.0)
# float32-compute filter against its float64 definition.  A priori: three float32 roundings of values below 21 667 (a r, (1 - a) c and
# their sum; ulp 2^-9 = 1.95e-3 above 16 384) of half an ulp each plus the relative 2^-24 of float32(1 - a) on a term below 21 667
# (another ~0.65 ulp), then the float32 store of the float64 definition itself (half an ulp): <= 2.7 ulp = 5.2e-3 rpm = 4.3e-7 span.
LAG_F32_BOUND = 4.3e-7
# ... and as measured on one MI355X (test_gpu_actuator.test_motor_lag_matches_the_oracles_pieces[f32], 512 drones x 40 steps, tau in
# [0.02, 0.15]): see that test's docstring; the bar is about 2x the measured maximum and inside the a-priori bound.
LAG_F32_STEP = 3.0e-7
# float32-compute rpm after a 5-step launch against the float64 oracle run from the launch's first state.  c depends only on the
# action and its float64-drawn noise, so it is the same on both sides and every step adds at most LAG_F32_BOUND: a priori
# 5 x 4.3e-7 = 2.15e-6 of RPM_SPAN.  Measured on one MI355X over the eight float32 cells of
# test_gpu_actuator_oracle.test_every_instantiation_with_latency_and_lag_matches_oracle: see its docstring; the bar is about 2x the
# measured maximum.
LAG_F32_LAUNCH_BOUND = 5 * LAG_F32_BOUND
LAG_F32_LAUNCH = 1.0e-6
# the float32-compute gust's distance from the float64 definition, in units of its sigma: measured on one MI355X over the eight
# float32 wind cells of test_gpu_dynamics_wind_oracle (150 000 drone-steps each), at most 3.97e-7 after a teacher-forced step (about
# one float32 ulp of a gust near 1.3 sigma) and 1.19e-6 after a 5-step launch; the bars are ~2x that
GUST_F32_STEP = 8e-7
GUST_F32_LAUNCH = 2.5e-6


# ---- action streams (two different streams: no test switches from one to the other) -----------------------------------------------
def _mixed(rng, n):
    bang = rng.uniform(-1, 1, (n, 4))
    hover = 0.0922 + 0.003 * rng.standard_normal((n, 4))
    return np.where((np.arange(n) % 2 == 0)[:, None], bang, hover).astype(np.float32)


def actions_mixed(rng, n):
    """Even drones: bang-bang U(-1,1) (crash within tens of steps, BASELINE config 2's stream); odd drones:
    hover + noise, 0.0922 + 0.003 N(0,1) (long flights, truncation, gate passes); one step in eight the two
    regimes swap so that hovering drones get kicked."""
    bang = rng.uniform(-1, 1, (n, 4))
    hover = 0.0922 + 0.003 * rng.standard_normal((n, 4))
    swap = rng.random((n, 1)) < 0.125
    even = (np.arange(n) % 2 == 0)[:, None]
    a = np.where(even ^ swap, bang, hover)
    return a.astype(np.float32)


# ---- Philox, noise, ulp distance, bit view ----------------------------------------------------------------------------------------
def philox(gid, step, stream, seed):
    """The four words of one Philox4x32-10 call on (seed; gid, step, stream), as float64 (exact: each is below 2^32)."""
    out = (C.c_uint32 * 4)()
    O.lib().orc_philox4x32(gid & 0xFFFFFFFF, gid >> 32, step & 0xFFFFFFFF, stream | ((step >> 32) << 8), seed & 0xFFFFFFFF, seed >> 32, out)
    return np.array(list(out), dtype=np.float64)


def unit(r):
    return (r + 0.5) / 4294967296.0


def _noise(seed, gid0, n, step, stream):
    """orc_noise4 of drones gid0 .. gid0 + n - 1: [n, 4] float32 (Box-Muller on the C library's log / sqrt / cos / sin)."""
    out = np.zeros((n, 4), np.float32)
    O.lib().orc_noise4_many(seed, gid0, n, step, stream, out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def ulps(a, b):
    """Distance in float32 ulps (same-sign values; 0 and -0 are 0 apart)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def f32(x):
    return float(np.float32(x))


# ---- the documented draws, as the GPU tests restate them (on the package's model objects) -------------------------------------------
def _dyn_draw(d, gid, step, seed):
    """The documented draw: one Philox4x32-10 call on (seed; gid, step, stream 13), s_j = lo + (hi - lo)(r_j + 0.5) / 2^32 in float64."""
    r = philox(gid, step, 13, seed)
    lo = np.array([np.float32(d.mass[0]), np.float32(d.inertia[0]), np.float32(d.kf[0]), np.float32(d.km[0])], dtype=np.float64)
    hi = np.array([np.float32(d.mass[1]), np.float32(d.inertia[1]), np.float32(d.kf[1]), np.float32(d.km[1])], dtype=np.float64)
    return (lo + (hi - lo) * ((r + 0.5) / 4294967296.0)).astype(np.float32)


def _mean_draw(w, gid, step, seed):
    """The documented steady draw: one Philox4x32-10 call on (seed; gid, step, stream 14), float64, stored as float32."""
    u = (philox(gid, step, 14, seed)[:3] + 0.5) / 4294967296.0
    f = lambda r: (float(np.float32(r[0])), float(np.float32(r[1])))      # noqa: E731
    (s0, s1), (a0, a1), (v0, v1) = f(w.speed), f(w.azimuth), f(w.vertical)
    s, th, v = s0 + (s1 - s0) * u[0], a0 + (a1 - a0) * u[1], v0 + (v1 - v0) * u[2]
    return np.array([s * math.cos(th), s * math.sin(th), v, 0.0], dtype=np.float32)


def _sigma3(w):
    return np.array([w.gust_sigma[0], w.gust_sigma[0], w.gust_sigma[1], 0.0], np.float32)


def _act_draw(act, gid, step, seed):
    """The documented episode-start draw: one Philox4x32-10 call on (seed; gid, step, stream 17) -> (d, float32 a)."""
    u = (philox(gid, step, 17, seed)[:2] + 0.5) / 4294967296.0
    lo, hi = act.latency
    d = min(lo + int(math.floor((hi - lo + 1) * u[0])), hi)
    t0, t1 = float(np.float32(act.motor_tau[0])), float(np.float32(act.motor_tau[1]))
    tau = t0 + (t1 - t0) * u[1]
    return d, (np.float32(math.exp(-DT / tau)) if tau > 0.0 else np.float32(0.0))


def _sens_draw(model, gid, step, seed):
    """The documented episode-start draw: four Philox4x32-10 calls on (seed; gid, step, streams 18..21), u_m = (r + 0.5) / 2^32 with
    m = 4 q + c: b_j = float32(amp_j (2 u_j - 1)) in float64, d = lo + floor((hi - lo + 1) u_13) clamped to hi."""
    u = (np.concatenate([philox(gid, step, 18 + q, seed) for q in range(4)]) + 0.5) / 4294967296.0
    amp = np.asarray(model.bias, np.float32).astype(np.float64)
    lo, hi = model.latency
    return min(lo + int(math.floor((hi - lo + 1) * u[13])), hi), (amp * (2.0 * u[:13] - 1.0)).astype(np.float32)


# ---- the sensor's delivery rule and the float64 normaliser ------------------------------------------------------------------------
class Delivery:
    """The host's statement of the rule.  hist[i, j] = the pre-bias row o_{k - j} of drone i, k[i] = control steps of its episode."""

    def __init__(self, model, n, seed, gid0):
        self.model, self.n, self.seed, self.gid0 = model, n, seed, gid0
        self.d = np.zeros(n, np.int64)
        self.b = np.zeros((n, 13), np.float32)
        self.hist = np.zeros((n, 9, 13), np.float32)
        self.k = np.zeros(n, np.int64)
        self.seen, self.young, self.ends = set(), 0, 0
        self.bias_on = any(v > 0.0 for v in model.bias)      # all-zero amplitudes: no add at all (-0.0f + 0.0f would flip a sign bit)

    def _plus_bias(self, o, rows):
        return o + self.b[rows] if self.bias_on else o.copy()

    def start(self, rows, o0, step):
        """Episodes of `rows` start at vector step `step` with pre-bias reset rows o0: returns float32(o_0 + b_new)."""
        for i, r in zip(rows, o0):
            self.d[i], self.b[i] = _sens_draw(self.model, self.gid0 + int(i), step, self.seed)
            self.hist[i] = 0.0
            self.hist[i, 0] = r
            self.k[i] = 0
        return self._plus_bias(np.asarray(o0, np.float32), rows)

    def step(self, o):
        """The pre-bias step rows o (also the terminal rows) of all drones: returns y."""
        self.hist = np.roll(self.hist, 1, axis=1)
        self.hist[:, 0] = o
        self.k += 1
        dd = np.minimum(self.d, self.k)
        self.seen.update(np.unique(self.d).tolist())
        self.young += int((self.k < self.d).sum())
        return self._plus_bias(self.hist[np.arange(self.n), dd], np.arange(self.n))


class Rms64:
    """gymnasium's NormalizeObservation on a batch of one, float64: RunningMeanStd.update then (x - mean) / sqrt(var + 1e-8)."""

    def __init__(self, n):
        self.mean, self.var, self.count = np.zeros((n, 13)), np.ones((n, 13)), np.full(n, 1e-4)

    def __call__(self, x, rows=None):
        rows = np.arange(len(self.count)) if rows is None else rows
        x = np.asarray(x, np.float64)
        mean, var, count = self.mean[rows], self.var[rows], self.count[rows][:, None]
        delta, tot = x - mean, count + 1.0
        mean = mean + delta / tot
        var = (var * count + delta * delta * count / tot) / tot
        self.mean[rows], self.var[rows], self.count[rows] = mean, var, tot[:, 0]
        return (x - mean) / np.sqrt(var + 1e-8)


class Worst:
    def __init__(self):
        self.excess, self.abs = 0.0, 0.0

    def close(self, got, want, tag):
        err = np.abs(got.astype(np.float64) - want)
        self.abs = max(self.abs, float(err.max(initial=0.0)))
        self.excess = max(self.excess, float((err / (ATOL + RTOL * np.abs(want))).max(initial=0.0)))
        assert self.excess <= 1.0, (tag, self.abs, self.excess)


# ---- what the package's model objects carry (the oracle reads the attributes only) ---------------------------------------------------
def dyn(mass=(1.0, 1.0), inertia=(1.0, 1.0), kf=(1.0, 1.0), km=(1.0, 1.0), resample=True):
    """What the package's DynamicsRandomization carries."""
    return SimpleNamespace(mass=mass, inertia=inertia, kf=kf, km=km, resample=resample)


def wind(speed=(0.0, 0.0), azimuth=(0.0, 2.0 * math.pi), vertical=(0.0, 0.0), gust_sigma=(0.0, 0.0), gust_tau=0.5,
         coeff=(5.5626e-3, 6.2490e-3), resample=True):
    """What the package's WindDisturbance carries."""
    return SimpleNamespace(speed=speed, azimuth=azimuth, vertical=vertical, gust_sigma=gust_sigma, gust_tau=gust_tau, coeff=coeff,
                           resample=resample)


def act(latency=(0, 0), motor_tau=(0.0, 0.0), fill=(0.0, 0.0, 0.0, 0.0), resample=True):
    """What the package's ActuatorModel carries."""
    return SimpleNamespace(latency=latency, motor_tau=motor_tau, fill=fill, resample=resample)


def sens(latency=(0, 0), bias=0.0, resample=True):
    """What the package's SensorModel carries."""
    b = (float(bias),) * 13 if isinstance(bias, (int, float)) else tuple(float(v) for v in bias)
    return SimpleNamespace(latency=tuple(latency), bias=b, resample=resample)


WIDE_BODY = dyn(**BODY)
GUSTY_WIND = wind(**GUSTY)

# ---- oracle-side tracks and cases --------------------------------------------------------------------------------------------------
CIRCLE6 = dict(waypoints=[[math.cos(a), math.sin(a), 1.0] for a in np.linspace(0, 2 * np.pi, 7)], spawn=[1.0, 0.0, 1.0],
               dim=[-2.0, -2.0, 0.0, 2.0, 2.0, 2.0], circle=True)
LOW = dict(waypoints=[[0.0, 1.0, 0.4], [-1.0, 0.0, 0.8], [0.0, -1.0, 0.4]], spawn=[1.0, 0.0, 0.05], dim=[-2.0, -2.0, 0.0, 2.0, 2.0, 2.0],
           circle=False, cylinder=False)
RACE = dict(waypoints=[[(x + 0.0) / 5, y / 5, (z + 3) / 5] for x, y, z in
                       [[-2.5, 4.5, 3], [10, 3.5, 1], [8, -4.5, 1], [-4.5, -6, 2], [-5, -5, 2], [5, -1, 3], [2.5, 6, 3], [-2.5, 4.5, 3]]],
            dim=[-4, -4, 0, 4, 4, 4])
_ANG = np.linspace(0, 2 * np.pi, 5, endpoint=True)
CIRCLE4 = dict(waypoints=np.stack([0.0 + 1.0 * np.cos(_ANG), 0.0 + 1.0 * np.sin(_ANG), np.full(5, 1.0)], axis=1)[1:], spawn=[1.0, 0.0, 1.0],
               dim=[-2.0, -2.0, 0.0, 2.0, 2.0, 2.0])
LOW_TRACK = (np.array(LOW["waypoints"]), np.array([LOW["spawn"]]), np.array(LOW["dim"]), False)
PHYSICS = {"pyb": 0, "pyb_gnd": 1, "pyb_drag": 2, "pyb_dw": 3, "pyb_gnd_drag_dw": 4}
ACTION_TYPES = {"thrust": 0, "rpm": 1, "pid": 2, "vel": 3, "one_d_rpm": 4, "one_d_pid": 5}
CASES = [(p, a, False) for p in range(5) for a in range(6)] + [(0, 0, True), (4, 2, True)]       # physics x action type x random spawn


def config(track, **kw):
    t = dict(track)
    opts = dict(circle=t.pop("circle"), cylinder=t.pop("cylinder", True))
    opts.update(kw)
    return O.make_config(t["waypoints"], t["spawn"], t["dim"], **opts)


def free_body(n, actuator, seed=3, max_steps=1 << 20, **kw):
    opts = dict(circle=False, cylinder=False, threshold=0.0, max_steps=max_steps, normalize_actions=False, normalize_obs=False, seed=seed)
    opts.update(kw)
    cfg = O.make_config([[5e3, 5e3, 5e3]], [0.0, 0.0, 1.0], WIDE, **opts)
    return O.OracleVecEnv(cfg, n, actuator=actuator)


def same_step(ra, rb, tag):
    for k in ra:
        assert ra[k].tobytes() == rb[k].tobytes(), (tag, k)


def stagger(ora, rng, hi=40):
    ora.envs["steps"] = rng.integers(0, hi, ora.n).astype(np.int32)


# ---- the draws, as the oracle tests restate them (the header's formulas on orc_philox4x32 words) -----------------------------------
def normals(gid, step, stream, seed):
    """orc_noise4's definition restated: Box-Muller in float64 on the four Philox words, rounded to float32."""
    r = philox(gid, step, stream, seed)
    z = []
    for h in range(2):
        rad = math.sqrt(-2.0 * math.log(unit(r[2 * h])))
        ang = 2.0 * math.pi * unit(r[2 * h + 1])
        z += [f32(rad * math.cos(ang)), f32(rad * math.sin(ang))]
    return z


def want_scales(d, gid, step, seed):
    r = philox(gid, step, 13, seed)
    return [f32(f32(lo) + (f32(hi) - f32(lo)) * unit(r[j])) for j, (lo, hi) in enumerate((d.mass, d.inertia, d.kf, d.km))]


def want_mean(w, gid, step, seed):
    r = philox(gid, step, 14, seed)
    s = f32(w.speed[0]) + (f32(w.speed[1]) - f32(w.speed[0])) * unit(r[0])
    th = f32(w.azimuth[0]) + (f32(w.azimuth[1]) - f32(w.azimuth[0])) * unit(r[1])
    v = f32(w.vertical[0]) + (f32(w.vertical[1]) - f32(w.vertical[0])) * unit(r[2])
    return [f32(s * math.cos(th)), f32(s * math.sin(th)), f32(v), 0.0]


def want_gust_start(w, gid, step, seed):
    z = normals(gid, step, 16, seed)
    sx, sz = np.float32(w.gust_sigma[0]), np.float32(w.gust_sigma[1])
    return [float(sx * np.float32(z[0])), float(sx * np.float32(z[1])), float(sz * np.float32(z[2])), 0.0]


def want_gust_step(w, g, gid, step, seed):
    a = math.exp(-DT / f32(w.gust_tau))
    root = math.sqrt(1.0 - a * a)
    b = [f32(w.gust_sigma[0]) * root, f32(w.gust_sigma[0]) * root, f32(w.gust_sigma[1]) * root]
    z = normals(gid, step, 15, seed)
    return [f32(a * float(g[j]) + b[j] * z[j]) for j in range(3)] + [0.0]


# ---- the actuator configurations: tests/test_oracle_actuator.py shows on the oracle alone that they reach the cases that ---------------
# ---- tests/test_gpu_actuator_oracle.py claims to test, and that file flies them on the device -------------------------------------
# a. every instantiation (the sensor files fly the same shapes)
INST = dict(n=1000, T=150, K=5, max_steps=40, rng=7)
INST_CELLS = [(dt, norm, noise, mode) for dt in ("f64", "f32") for norm in (0, 1) for noise in (0, 1) for mode in ("step", "rollout")]


def act_inst_seed(dt, norm, noise):
    return 5000 + norm * 4 + noise * 2 + (dt == "f32")


# b. options.  (physics, normalize_actions, extra options, features on)
LAG_OPTION_CELLS = [("pyb", True, {}, "both"), ("pyb_gnd", True, {}, "both"), ("pyb_drag", True, {}, "both"), ("pyb_dw", True, {}, "both"),
                    ("pyb_gnd_drag_dw", True, {}, "both"), ("pyb_gnd_drag_dw", True, {}, "none"), ("pyb_gnd_drag_dw", False, {}, "both"),
                    ("pyb", True, dict(random_spawn=True), "both"), ("pyb", True, dict(clip_rew=True, norm_rew=True), "both"),
                    ("pyb_drag", True, dict(zero_damping=True), "both"), ("pyb", True, dict(include_distance=False), "both")]
LAT_OPTION_CELLS = [("pyb_gnd_drag_dw", "rpm"), ("pyb", "rpm"), ("pyb", "pid"), ("pyb", "vel"), ("pyb_drag", "one_d_rpm"),
                    ("pyb", "one_d_pid"), ("pyb_gnd_drag_dw", "pid")]          # the non-THRUST pairs of test_gpu_dynamics_wind_oracle's
ACT_OPT = dict(n=1024, T=100, seed=31, rng=5)
RAW_FILL = (0.07, 0.07, 0.07, 0.07)                    # newton per rotor (normalize_actions off): a little above hover's 0.066
LAT_FILL = (0.1, -0.2, 0.05, 0.3)


def option_setup(physics, act_name, normalize_actions, extra):
    """(waypoints, spawn, dim, circle, kw shared by DroneVecEnv and make_config, the actuator's kw) of one option cell."""
    kw = dict(max_steps=60, normalize_obs=False, seed=ACT_OPT["seed"], **extra)
    if extra.get("random_spawn"):
        wp, spawn, dim, circle = np.array(CIRCLE6["waypoints"])[1:], np.array([CIRCLE6["spawn"]]), np.array(CIRCLE6["dim"]), True
        kw.update(max_steps=25, cylinder=False, ground_contact=False)
    else:
        wp, spawn, dim, circle = LOW_TRACK
        kw.update(ground_contact=False, cylinder=False, normalize_actions=normalize_actions)
    if act_name == "thrust":
        model = dict(FULL, fill=HOVER_FILL if normalize_actions else RAW_FILL)
    else:
        model = dict(latency=(0, 8), fill=LAT_FILL)
    return wp, spawn, dim, circle, kw, model


def option_actions(rng, n, act_name, normalize_actions):
    if act_name != "thrust":
        return rng.uniform(-1, 1, (n, 4)).astype(np.float32)
    return actions_mixed(rng, n) if normalize_actions else rng.uniform(0.02, 0.16, (n, 4)).astype(np.float32)


# c. free-running fused launches; d. short launches and set values
ACT_FREE = dict(n=4096, K=64, launches=4, max_steps=100, seed=0xAC7, rng=64)
FREE_WHERE = {"gid-past-2^33": ((1 << 33) + 12345, 0), "step-across-2^32": (0, (1 << 32) - 100)}
SHORT = dict(n=2048, Ks=(1, 3, 7, 8, 9, 8, 1, 7, 3, 9, 1, 8, 9, 7, 3, 1, 9, 8, 3, 7), max_steps=30, seed=0x5A0, rng=11)
ACT_SETV = dict(n=2048, K=20, launches=4, max_steps=15, seed=77, rng=12)


def act_track_oracle(track, n, actuator, dw, **kw):
    """The oracle side of gpu_support.make_pair for the circle4 (`tracks.circle(1, 4, 1)`) and race (`tracks.reaching()`) tracks:
    float32 state, the normaliser on unless told, ground contact off (what DN_GROUND_CONTACT_AUTO resolves to on both)."""
    t = CIRCLE4 if track == "circle4" else dict(RACE, spawn=RACE["waypoints"][0])
    kw.setdefault("normalize_obs", True)
    cfg = O.make_config(t["waypoints"], t["spawn"], t["dim"], circle=track == "circle4", f32_state=True, ground_contact=False, **kw)
    return O.OracleVecEnv(cfg, n, threads=8, dynamics=dyn(**BODY) if dw else None, wind=wind(**GUSTY) if dw else None,
                          actuator=act(**actuator))


def act_inst_oracle(dt, norm, noise):
    return act_track_oracle("circle4", INST["n"], FULL, bool(norm), max_steps=INST["max_steps"], normalize_obs=bool(norm),
                            seed=act_inst_seed(dt, norm, noise), **(NOISE if noise else {}))


def short_set_values(rng, n):
    """d. the values written by set_actuator: latency 8 for half the drones / random valid values."""
    return dict(latency=rng.integers(0, 9, n).astype(np.int32), coeff=rng.uniform(0.3, 0.99, n).astype(np.float32),
                rpm=rng.uniform(9500.0, 21000.0, (n, 4)).astype(np.float32), history=rng.uniform(-1, 1, (n, 8, 4)).astype(np.float32))


# ---- the sensor configurations: tests/test_oracle_sensor.py covers them, tests/test_gpu_sensor_oracle.py flies them -------------------
# a. every instantiation: the shapes of INST; the norm cells carry dynamics + wind + actuator, the raw cells the sensor alone
def sens_inst_seed(dt, norm, noise):
    return 7000 + norm * 4 + noise * 2 + (dt == "f32")


def sens_track_oracle(track, n, sensor, full, **kw):
    """act_track_oracle with the sensor; full: dynamics + wind + the FULL actuator ride along, else the sensor is alone."""
    ora = act_track_oracle(track, n, FULL if full else {}, full, **kw)
    if not full:
        ora.enable_actuator(None)
    ora.enable_sensor(None if sensor is None else sens(**sensor))
    return ora


def sens_inst_oracle(dt, norm, noise, n=None):
    return sens_track_oracle("circle4", INST["n"] if n is None else n, SENSOR, bool(norm), max_steps=INST["max_steps"],
                             normalize_obs=bool(norm), seed=sens_inst_seed(dt, norm, noise), **(NOISE if noise else {}))


# b. options: the 18 cells of the actuator file with the sensor on top, two (three) with the sensor and nothing else, one with the
# normaliser.  (physics, action type, normalize_actions, extra options, features: both | none | sensor)
SENS_OPTION_CELLS = ([(p, "thrust", na, e, f) for p, na, e, f in LAG_OPTION_CELLS] + [(p, a, False, {}, "both") for p, a in LAT_OPTION_CELLS]
                     + [("pyb", "thrust", True, {}, "sensor"), ("pyb_gnd_drag_dw", "pid", False, {}, "sensor"),
                        ("pyb", "thrust", True, dict(random_spawn=True), "sensor"), ("pyb_gnd", "thrust", True, dict(normalize_obs=True), "both")])
SENS_OPTION_IDS = [f"{p}-{a}-{'norm' if na else 'raw'}-{'-'.join(e) or 'plain'}-{f}" for p, a, na, e, f in SENS_OPTION_CELLS]
SENS_OPT = dict(ACT_OPT, seed=47)


def option_cell(cell):
    """(waypoints, spawn, dim, circle, kw shared by DroneVecEnv and make_config, the actuator's kw or None, dynamics + wind on) of a cell."""
    physics, act_name, normalized, extra, feat = SENS_OPTION_CELLS[cell]
    extra = dict(extra)
    norm_obs = extra.pop("normalize_obs", False)
    wp, spawn, dim, circle, kw, model = option_setup(physics, act_name, normalized, extra)
    kw.update(normalize_obs=norm_obs, seed=SENS_OPT["seed"])
    return wp, spawn, dim, circle, kw, (None if feat == "sensor" else model), feat == "both"


def option_oracle(cell, n, ground_contact=None):
    physics, act_name = SENS_OPTION_CELLS[cell][:2]
    wp, spawn, dim, circle, kw, model, both = option_cell(cell)
    if ground_contact is not None:
        kw = dict(kw, ground_contact=ground_contact)
    cfg = O.make_config(wp, spawn.ravel(), dim, circle=circle, f32_state=True, physics=PHYSICS[physics],
                        action_type=ACTION_TYPES[act_name], **kw)
    return O.OracleVecEnv(cfg, n, threads=8, dynamics=dyn(**BODY) if both else None, wind=wind(**GUSTY) if both else None,
                          actuator=None if model is None else act(**model), sensor=sens(**SENSOR))


# c. free-running launches; d. tile shapes; e. set values; f. late enable and re-enable
SENS_FREE = dict(ACT_FREE, seed=0x5E75)
SHAPES = (1, 63, 65, 191)
# dn_step_many refuses K > 1 unless num_envs % 4 == 0, so the K = 20 launches cannot run at SHAPES: those fly the same number of steps as
# single steps, and the nearest fleet sizes a launch accepts (still one partial tile each) fly the launches
LAUNCH_SHAPES = (4, 60, 68, 188)
SHAPE = dict(singles=14, K=20, launches=2, max_steps=6, seed=0x7A9, rng=21)
SENS_SETV = dict(n=1500, K=20, launches=4, max_steps=15, seed=79, rng=13)
REENABLE = dict(n=1000, pre=30, K=20, launches=3, max_steps=40, seed=91, rng=17, second=dict(latency=(2, 5), bias=tuple(2.0 * a for a in AMPS)))


def shape_oracle(n):
    return sens_track_oracle("circle4", n, dict(SENSOR, resample=False), False, max_steps=SHAPE["max_steps"], normalize_obs=False,
                             seed=SHAPE["seed"], **NOISE)


def shape_plan(n):
    """d. the (K, single step?) sequence of a shape: 14 single steps, then two launches of 20 where dn_step_many takes the fleet size,
    40 more single steps where it does not."""
    tail = [(SHAPE["K"], False)] * SHAPE["launches"] if n % 4 == 0 else [(1, True)] * (SHAPE["K"] * SHAPE["launches"])
    return [(1, True)] * SHAPE["singles"] + tail


def shape_values(n):
    """d. what set_sensor writes: latency i mod 9, a bias row that names its drone and column."""
    i = np.arange(n)
    return dict(latency=(i % 9).astype(np.int32),
                bias=(0.01 * ((i[:, None] * 13 + np.arange(13)[None, :]) % 17 - 8)).astype(np.float32))


def setv_oracle(n=None):
    return sens_track_oracle("circle4", SENS_SETV["n"] if n is None else n, dict(SENSOR, resample=False), False,
                             max_steps=SENS_SETV["max_steps"], normalize_obs=False, seed=SENS_SETV["seed"])


def set_values(rng, n):
    """e. random valid latency / bias / history for set_sensor."""
    return dict(latency=rng.integers(0, 9, n).astype(np.int32), bias=rng.uniform(-0.1, 0.1, (n, 13)).astype(np.float32),
                history=rng.uniform(-1, 1, (n, 9, 13)).astype(np.float32))


def setv_start(rng, n):
    """e. the staggered episode step counters (so that written history entries are inside the episode and get delivered), then the values."""
    return rng.integers(0, SENS_SETV["max_steps"], n).astype(np.int32), set_values(rng, n)


def reenable_oracle(n=None):
    """f. starts WITHOUT the sensor (enable_sensor comes later), dynamics + wind + actuator on."""
    return sens_track_oracle("circle4", REENABLE["n"] if n is None else n, None, True, max_steps=REENABLE["max_steps"], normalize_obs=False,
                             seed=REENABLE["seed"], **NOISE)


# ---- GPU outputs against the oracle's (what they are given answers .cpu().numpy(): device tensors, or numpy arrays wrapped to) ---------
def gpu_state_to_oracle(st, envs, step_count):
    """Teacher forcing: load the GPU's float32 state into the oracle's float64 variables."""
    for k in ("pos", "quat", "vel", "ang_v", "prev_vel", "prev_ang_v", "cur_pos", "d", "d_prev", "idx", "steps",
              "just_found", "ep_ret", "ep_len", "rms_mean", "rms_var", "rms_count", "rr_returns", "rr_mean", "rr_var",
              "rr_count", "pid"):
        envs[k] = st[k]
    envs["ep_ret"] = st["ep_ret"].astype(np.float64) + st["ep_ret_lo"].astype(np.float64)    # Monitor's running return: a float32 pair
    envs["last_clipped_action"] = st["last_rpm"]
    envs["cur_vel"] = st["vel"]
    envs["cur_ang_v"] = st["ang_v"]
    envs["is_done"] = 0
    envs["step_count"] = step_count


def compare_step(out, ref, tag, obs_atol=1e-5, rew_atol=1e-5):
    """rew_atol: 1e-5 teacher-forced.  Free-running comparisons (both sides keep their own float32 state) pass 1e-4:
    a stored distance may differ by one float32 ulp (1.2e-7) and the reward carries 3000 (d_prev - d) / 25 = 120x that."""
    obs, rew, done, info = out
    assert np.array_equal(done.cpu().numpy(), ref["done"]), f"{tag}: done"
    assert np.array_equal(info["truncated"].cpu().numpy(), ref["truncated"]), f"{tag}: TimeLimit.truncated"
    assert np.array_equal(info["found_targets"].cpu().numpy(), ref["found_targets"]), f"{tag}: waypoint index"
    k = obs.shape[1]                       # 12 columns when include_distance is off
    np.testing.assert_allclose(obs.cpu().numpy(), ref["obs"][:, :k], rtol=0, atol=obs_atol, err_msg=f"{tag}: obs")
    # reward carries 3000*(d_prev - d)/25: 1e-5 relative + 1e-5 absolute
    np.testing.assert_allclose(rew.cpu().numpy(), ref["reward"], rtol=1e-5, atol=rew_atol, err_msg=f"{tag}: reward")
    dn = ref["done"].astype(bool)
    if dn.any():
        np.testing.assert_allclose(info["terminal_obs"].cpu().numpy()[dn], ref["terminal_obs"][dn][:, :k], rtol=0,
                                   atol=obs_atol, err_msg=f"{tag}: terminal_observation")
        assert np.array_equal(info["ep_length"].cpu().numpy()[dn], ref["ep_len"][dn]), f"{tag}: episode l"
        np.testing.assert_allclose(info["ep_return"].cpu().numpy()[dn], ref["ep_ret"][dn], rtol=1e-5, atol=1e-4,
                                   err_msg=f"{tag}: episode r")
    return int(dn.sum())


def _step_mismatch(out, ref, obs_atol, rew_atol):
    """Per-drone mismatch mask of one step (the checks of compare_step, drone by drone)."""
    obs, rew, done, info = out
    k = obs.shape[1]
    bad = done.cpu().numpy() != ref["done"]
    bad |= info["truncated"].cpu().numpy() != ref["truncated"]
    bad |= info["found_targets"].cpu().numpy() != ref["found_targets"]
    bad |= ~(np.abs(obs.cpu().numpy().astype(np.float64) - ref["obs"][:, :k]) <= obs_atol).all(axis=1)
    r = ref["reward"].astype(np.float64)
    bad |= ~(np.abs(rew.cpu().numpy().astype(np.float64) - r) <= rew_atol + 1e-5 * np.abs(r))
    dn = ref["done"].astype(bool) & ~bad
    if dn.any():
        t_ok = (np.abs(info["terminal_obs"].cpu().numpy().astype(np.float64) - ref["terminal_obs"][:, :k]) <= obs_atol).all(axis=1)
        l_ok = info["ep_length"].cpu().numpy() == ref["ep_len"]
        e = ref["ep_ret"].astype(np.float64)
        r_ok = np.abs(info["ep_return"].cpu().numpy().astype(np.float64) - e) <= 1e-4 + 1e-5 * np.abs(e)
        bad |= dn & ~(t_ok & l_ok & r_ok)
    return bad
