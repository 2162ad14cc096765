"""Per-drone sensor model (include/dronenav.h dn_enable_sensor): observation latency and a per-episode constant bias.

A drone with latency d is shown, after the k-th control step of its episode, the pre-normaliser observation row of min(d, k) steps
ago plus its bias row b: y_k = float32(o_{k - min(d, k)} + b).  A fresh episode's pipeline holds its own reset observation; the reset
row itself leaves undelayed with the new episode's bias.  The normaliser (normalize_obs) is fed the delivered rows.  Nothing feeds back
into the flight: state, reward and episode ends are those of the env without the sensor model.  Both are drawn per drone at every
episode start or set by DroneVecEnv.set_sensor.
"""
import dataclasses
import math

from . import _capi
from .actuator import MAX_LATENCY

OBS_DIM = 13


@dataclasses.dataclass(frozen=True)
class SensorModel:
    """latency: integer range [lo, hi] of control steps, 0 <= lo <= hi <= 8.  bias: the amplitude per observation column (13 finite
    numbers >= 0, or one number for all columns) in observation-column units: b_j is uniform in [-bias_j, bias_j];
    DroneVecEnv.observation_scale() converts from physical units.  resample=True draws latency and bias at every episode start (keyed
    by seed / global drone id / vector step: shard-invariant); with it, latency (0, 0) and an all-zero bias each switch their half off.
    resample=False keeps what DroneVecEnv.set_sensor wrote (latency 0, bias 0 until then)."""
    latency: tuple = (0, 0)
    bias: tuple = (0.0,) * OBS_DIM
    resample: bool = True

    def __post_init__(self):
        try:
            lo, hi = self.latency
            if isinstance(lo, bool) or isinstance(hi, bool) or int(lo) != lo or int(hi) != hi:
                raise ValueError
            lo, hi = int(lo), int(hi)
        except (TypeError, ValueError, OverflowError):
            raise ValueError(f"SensorModel.latency must be a pair of integers, got {self.latency!r}") from None
        if not 0 <= lo <= hi <= MAX_LATENCY:
            raise ValueError(f"SensorModel.latency = {self.latency!r}: need 0 <= lo <= hi <= {MAX_LATENCY}")
        object.__setattr__(self, "latency", (lo, hi))
        try:
            if isinstance(self.bias, bool):
                raise TypeError
            bias = (float(self.bias),) * OBS_DIM if isinstance(self.bias, (int, float)) else tuple(float(v) for v in self.bias)
        except (TypeError, ValueError):
            raise ValueError(f"SensorModel.bias must be one number or {OBS_DIM} numbers, got {self.bias!r}") from None
        if len(bias) != OBS_DIM or not all(math.isfinite(v) and v >= 0.0 for v in bias):
            raise ValueError(f"SensorModel.bias = {self.bias!r}: need {OBS_DIM} finite numbers >= 0")
        object.__setattr__(self, "bias", bias)
        object.__setattr__(self, "resample", bool(self.resample))

    def to_c(self):
        """The dn_sensor_config this describes."""
        c = _capi.DnSensorConfig()
        c.latency[:] = self.latency
        c.bias_amp[:] = self.bias
        c.resample = int(self.resample)
        c.reserved = 0
        return c

    @classmethod
    def from_c(cls, c):
        return cls(latency=tuple(c.latency), bias=tuple(c.bias_amp), resample=bool(c.resample))
