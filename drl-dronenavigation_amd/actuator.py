"""Per-drone actuator model (include/dronenav.h dn_enable_actuator): command latency and first-order motor lag.

Latency: a drone with latency d flies, at a control step it enters with episode step counter s, the action commanded d vector steps
ago (s >= d) or `fill` (s < d: a fresh episode's pipeline holds no command of that episode yet).  Motor lag: the rotor speeds r
follow the speeds c the action chain commands as r <- a r + (1 - a) c with a = exp(-dt / tau), dt = 1/240 s; an episode starts with
the chain's speeds for `fill`.  Both are drawn per drone at every episode start or set by DroneVecEnv.set_actuator.
"""
import dataclasses
import math

from . import _capi

MAX_LATENCY = 8         # DN_MAX_LATENCY: control steps (33 ms at 240 Hz)


@dataclasses.dataclass(frozen=True)
class ActuatorModel:
    """latency: integer range [lo, hi] of control steps, 0 <= lo <= hi <= 8.  motor_tau: range [lo, hi] of the motor time constant in
    seconds, finite, 0 <= lo <= hi; (0, 0) turns the lag off, any other range needs act="thrust".  fill: the action (4 finite numbers) a
    fresh episode's pipeline holds; with the default zeros and normalised actions a drone starts every episode with rotors at the
    centre of the action box.  resample=True draws latency and time constant at every episode start (keyed by seed / global drone id /
    vector step: shard-invariant); False keeps what DroneVecEnv.set_actuator wrote (latency 0, no lag until then)."""
    latency: tuple = (0, 0)
    motor_tau: tuple = (0.0, 0.0)
    fill: tuple = (0.0, 0.0, 0.0, 0.0)
    resample: bool = True

    def __post_init__(self):
        try:
            lo, hi = self.latency
            if isinstance(lo, bool) or isinstance(hi, bool) or int(lo) != lo or int(hi) != hi:
                raise ValueError
            lo, hi = int(lo), int(hi)
        except (TypeError, ValueError, OverflowError):
            raise ValueError(f"ActuatorModel.latency must be a pair of integers, got {self.latency!r}") from None
        if not 0 <= lo <= hi <= MAX_LATENCY:
            raise ValueError(f"ActuatorModel.latency = {self.latency!r}: need 0 <= lo <= hi <= {MAX_LATENCY}")
        object.__setattr__(self, "latency", (lo, hi))
        try:
            tlo, thi = (float(v) for v in self.motor_tau)
        except (TypeError, ValueError):
            raise ValueError(f"ActuatorModel.motor_tau must be a pair of numbers, got {self.motor_tau!r}") from None
        if not (math.isfinite(tlo) and math.isfinite(thi)):
            raise ValueError(f"ActuatorModel.motor_tau = {self.motor_tau!r}: both values must be finite")
        if not 0.0 <= tlo <= thi:
            raise ValueError(f"ActuatorModel.motor_tau = {self.motor_tau!r}: need 0 <= lo <= hi")
        object.__setattr__(self, "motor_tau", (tlo, thi))
        try:
            fill = tuple(float(v) for v in self.fill)
        except (TypeError, ValueError):
            raise ValueError(f"ActuatorModel.fill must be four numbers, got {self.fill!r}") from None
        if len(fill) != 4 or not all(math.isfinite(v) for v in fill):
            raise ValueError(f"ActuatorModel.fill = {self.fill!r}: need four finite numbers")
        object.__setattr__(self, "fill", fill)
        object.__setattr__(self, "resample", bool(self.resample))

    def to_c(self):
        """The dn_actuator_config this describes."""
        c = _capi.DnActuatorConfig()
        c.latency[:] = self.latency
        c.motor_tau[:] = self.motor_tau
        c.fill[:] = self.fill
        c.resample = int(self.resample)
        c.reserved = 0
        return c

    @classmethod
    def from_c(cls, c):
        return cls(latency=tuple(c.latency), motor_tau=tuple(c.motor_tau), fill=tuple(c.fill), resample=bool(c.resample))
