"""Per-drone wind (include/dronenav.h dn_enable_wind): a steady wind drawn per episode and Ornstein-Uhlenbeck gusts.

Each drone is pushed by F_w = (k_xy w_x, k_xy w_y, k_z w_z) at its centre of mass, w = wbar + g in the world frame: wbar is drawn
at every episode start (speed, azimuth and vertical component uniform on their ranges) or set by DroneVecEnv.set_wind; g is an
Ornstein-Uhlenbeck process with correlation time gust_tau and stationary standard deviation (gust_sigma[0], gust_sigma[0],
gust_sigma[1]).  The default coefficients are the cf2x rotor-drag coefficients at hover (a 5 m/s wind is about 1.03 m/s^2).
"""
import dataclasses
import math

from . import _capi

_PAIRS = ("speed", "azimuth", "vertical", "gust_sigma", "coeff")


@dataclasses.dataclass(frozen=True)
class WindDisturbance:
    """speed, azimuth, vertical: ranges [lo, hi] (finite, lo <= hi; speed lo >= 0) of the steady wind, in m/s and radians (azimuth =
    the direction the air moves toward).  gust_sigma (xy, z) >= 0 m/s and gust_tau > 0 s: the gust process (sigma = (0, 0) turns it
    off).  coeff (k_xy, k_z) >= 0 N s / m.  resample=True draws a new steady wind at every episode start (keyed by seed / global
    drone id / vector step: shard-invariant); False keeps what DroneVecEnv.set_wind wrote (0 until then)."""
    speed: tuple = (0.0, 0.0)
    azimuth: tuple = (0.0, 2.0 * math.pi)
    vertical: tuple = (0.0, 0.0)
    gust_sigma: tuple = (0.0, 0.0)
    gust_tau: float = 0.5
    coeff: tuple = (5.5626e-3, 6.2490e-3)
    resample: bool = True

    def __post_init__(self):
        for name in _PAIRS:
            r = getattr(self, name)
            try:
                lo, hi = (float(v) for v in r)
            except (TypeError, ValueError):
                raise ValueError(f"WindDisturbance.{name} must be a pair of numbers, got {r!r}") from None
            if not (math.isfinite(lo) and math.isfinite(hi)):
                raise ValueError(f"WindDisturbance.{name} = {r!r}: both values must be finite")
            if name in ("speed", "azimuth", "vertical") and not lo <= hi:
                raise ValueError(f"WindDisturbance.{name} = {r!r}: lo must be <= hi")
            if name == "speed" and not lo >= 0.0:
                raise ValueError(f"WindDisturbance.speed = {r!r}: lo must be >= 0")
            if name in ("gust_sigma", "coeff") and not (lo >= 0.0 and hi >= 0.0):
                raise ValueError(f"WindDisturbance.{name} = {r!r}: both values must be >= 0")
            object.__setattr__(self, name, (lo, hi))
        try:
            tau = float(self.gust_tau)
        except (TypeError, ValueError):
            raise ValueError(f"WindDisturbance.gust_tau must be a number, got {self.gust_tau!r}") from None
        if not (math.isfinite(tau) and tau > 0.0):
            raise ValueError(f"WindDisturbance.gust_tau = {tau!r}: must be finite and > 0")
        object.__setattr__(self, "gust_tau", tau)
        object.__setattr__(self, "resample", bool(self.resample))

    def to_c(self):
        """The dn_wind_config this describes."""
        c = _capi.DnWindConfig()
        for name in _PAIRS:
            getattr(c, name)[:] = getattr(self, name)
        c.gust_tau = self.gust_tau
        c.resample = int(self.resample)
        c.reserved = 0
        return c

    @classmethod
    def from_c(cls, c):
        return cls(speed=tuple(c.speed), azimuth=tuple(c.azimuth), vertical=tuple(c.vertical), gust_sigma=tuple(c.gust_sigma),
                   gust_tau=c.gust_tau, coeff=tuple(c.coeff), resample=bool(c.resample))
