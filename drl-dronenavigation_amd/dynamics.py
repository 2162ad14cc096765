"""Per-drone dynamics randomisation (include/dronenav.h dn_enable_dynamics): the ranges of the body's scale factors.

Each drone's simulated body is the cf2x with its mass, inertia (all three axes together), thrust coefficient KF and drag-torque
coefficient KM multiplied by per-drone factors.  The action chain, the hover rpm and the PID loop keep the nominal constants (the
flight stack models the drone it was tuned for), so a policy trained over the ranges meets bodies it does not know exactly.
"""
import dataclasses
import math

from . import _capi

_FIELDS = ("mass", "inertia", "kf", "km")


@dataclasses.dataclass(frozen=True)
class DynamicsRandomization:
    """Scale ranges [lo, hi] (0 < lo <= hi, finite) relative to the nominal body.  resample=True draws new scales uniformly from the
    ranges at every episode start (reset and auto-reset, keyed by seed / global drone id / vector step: shard-invariant); False keeps
    the scales DroneVecEnv.set_dynamics wrote (1 until then)."""
    mass: tuple = (1.0, 1.0)
    inertia: tuple = (1.0, 1.0)
    kf: tuple = (1.0, 1.0)
    km: tuple = (1.0, 1.0)
    resample: bool = True

    def __post_init__(self):
        for name in _FIELDS:
            r = getattr(self, name)
            try:
                lo, hi = (float(v) for v in r)
            except (TypeError, ValueError):
                raise ValueError(f"DynamicsRandomization.{name} must be a (lo, hi) pair of numbers, got {r!r}") from None
            if not (math.isfinite(lo) and math.isfinite(hi)):
                raise ValueError(f"DynamicsRandomization.{name} = {r!r}: lo and hi must be finite")
            if not lo > 0.0:
                raise ValueError(f"DynamicsRandomization.{name} = {r!r}: lo must be > 0")
            if not lo <= hi:
                raise ValueError(f"DynamicsRandomization.{name} = {r!r}: lo must be <= hi")
            object.__setattr__(self, name, (lo, hi))
        object.__setattr__(self, "resample", bool(self.resample))

    def to_c(self):
        """The dn_dynamics_config this describes."""
        c = _capi.DnDynamicsConfig()
        for name in _FIELDS:
            getattr(c, name)[:] = getattr(self, name)
        c.resample = int(self.resample)
        c.reserved = 0
        return c

    @classmethod
    def from_c(cls, c):
        return cls(mass=tuple(c.mass), inertia=tuple(c.inertia), kf=tuple(c.kf), km=tuple(c.km), resample=bool(c.resample))
