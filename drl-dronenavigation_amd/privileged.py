"""Privileged observations (include/dronenav.h dn_enable_privileged): the ground truth the per-drone models hide from the policy.

For an asymmetric actor-critic or a teacher-student setup the critic / teacher sees, per drone and step, one row of PRIV_DIM = 52
float32: the true observation (before observation noise, sensor model and normaliser) and the values the four models drew for the
episode -- body scales, wind, actuator, sensor -- while the actor keeps the degraded observation row.  The step kernels write the rows
themselves, inside a fused K-step launch too, where episodes restart and parameters are redrawn.  A step row describes the state the
step leaves (a restarted drone: the new episode); a terminal row, written only where an episode ended, describes the terminal state
with the finished episode's parameters.  A model that is off reads as its neutral value (scales 1, everything else 0); a group that is
not selected is not written at all.  Nothing feeds back into the flight.
"""
import dataclasses

from . import _capi

PRIV_DIM = 52
# group name -> its bit in dn_privileged_config.groups
PRIV_GROUPS = {"obs": 1, "dyn": 2, "wind": 4, "act": 8, "sens": 16}
# the named columns of a row
PRIV_SLICES = {
    "obs": slice(0, 13),            # the true observation (13..15 are 0)
    "scales": slice(16, 20),        # s_m, s_I, s_kf, s_km
    "wind_mean": slice(20, 23),     # wbar (23 is 0)
    "wind_gust": slice(24, 27),     # g (27 is 0)
    "rpm": slice(28, 32),           # the effective rotor speeds r
    "act_latency": slice(32, 33),   # the actuator's latency d
    "act_coeff": slice(33, 34),     # the motor lag coefficient a
    "sens_latency": slice(34, 35),  # the sensor's latency d
    "steps": slice(35, 36),         # the episode step counter (terminal row: the finished episode's length)
    "bias": slice(36, 49),          # the sensor bias b (49..51 are 0)
}
# the columns each group writes
PRIV_GROUP_COLUMNS = {
    "obs": tuple(range(0, 16)) + (35,),
    "dyn": tuple(range(16, 20)),
    "wind": tuple(range(20, 28)),
    "act": tuple(range(28, 34)),
    "sens": (34,) + tuple(range(36, 52)),
}


@dataclasses.dataclass(frozen=True)
class PrivilegedObservation:
    """groups: which column groups the kernels write, a non-empty sequence of "obs", "dyn", "wind", "act", "sens" (PRIV_GROUPS).  The
    default is all five; groups=("obs",) costs 64 bytes per drone and step instead of 208."""
    groups: tuple = ("obs", "dyn", "wind", "act", "sens")

    def __post_init__(self):
        if isinstance(self.groups, str):
            raise ValueError(f"PrivilegedObservation.groups must be a sequence of group names, got {self.groups!r}")
        try:
            groups = tuple(self.groups)
        except TypeError:
            raise ValueError(f"PrivilegedObservation.groups must be a sequence of group names, got {self.groups!r}") from None
        for g in groups:
            if not isinstance(g, str) or g not in PRIV_GROUPS:
                raise ValueError(f"PrivilegedObservation.groups: unknown group {g!r} (known: {', '.join(PRIV_GROUPS)})")
        if not groups:
            raise ValueError("PrivilegedObservation.groups must name at least one group")
        object.__setattr__(self, "groups", tuple(g for g in PRIV_GROUPS if g in groups))    # canonical order, no repeats

    @property
    def mask(self):
        m = 0
        for g in self.groups:
            m |= PRIV_GROUPS[g]
        return m

    def columns(self):
        """The columns of a row the kernels write with these groups, ascending."""
        return sorted(c for g in self.groups for c in PRIV_GROUP_COLUMNS[g])

    def column_runs(self):
        """columns() as ascending (start, stop) runs of adjacent columns: one run with every group, at most three otherwise."""
        runs = []
        for c in self.columns():
            if runs and runs[-1][1] == c:
                runs[-1][1] = c + 1
            else:
                runs.append([c, c + 1])
        return [tuple(r) for r in runs]

    def to_c(self):
        """The dn_privileged_config this describes."""
        c = _capi.DnPrivilegedConfig()
        c.groups = self.mask
        c.reserved = 0
        return c

    @classmethod
    def from_c(cls, c):
        if c.groups & ~sum(PRIV_GROUPS.values()):
            raise ValueError(f"dn_privileged_config.groups = {c.groups:#x} has unknown bits")
        return cls(groups=tuple(g for g, bit in PRIV_GROUPS.items() if c.groups & bit))
