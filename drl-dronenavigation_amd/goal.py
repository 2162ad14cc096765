"""Goal observations (include/dronenav.h dn_enable_goal): where the drone is supposed to fly, as the policy may see it.

The 13 observation columns carry the drone's own state and one scalar distance, but no direction to the target.  With
DroneVecEnv(goal=GoalObservation(...)) the step kernels write, per drone and step -- inside a fused K-step launch too --, one row of
GOAL_DIM = 8 float32: the vector to the current target waypoint and the segment after it, both over max_target_dist, in the world frame
or in the body frame of the observation's own Euler columns.  The row is built from the DELIVERED observation (after observation noise
and the sensor model's latency and bias, before the normaliser), so it hands the policy nothing the sensor model hides; the waypoint
index is the true one.  A step row describes what the step leaves (a restarted drone: the reset row against waypoint 0); a terminal
row, written only where an episode ended, describes the terminal row against the waypoint the episode ended on.  The rows are neither
normalised nor clipped, and nothing feeds back into the flight.
"""
import dataclasses

from . import _capi

GOAL_DIM = 8
# frame name -> dn_goal_config.frame
GOAL_FRAMES = {"world": 0, "body": 1}
# the named columns of a row
GOAL_SLICES = {
    "to_target": slice(0, 3),       # e = (wp[i] - p_hat) / max_target_dist
    "index": slice(3, 4),           # i, as a float32 number
    "next_segment": slice(4, 7),    # n = (wp[i+1] - wp[i]) / max_target_dist, zeros at the last waypoint
    "has_next": slice(7, 8),        # 1 where i + 1 < W, else 0
}


@dataclasses.dataclass(frozen=True)
class GoalObservation:
    """frame: "world" (the default) or "body" -- the two vectors of a row multiplied by R^T, R = Rz(yaw) Ry(pitch) Rx(roll) of the
    delivered Euler columns."""
    frame: str = "world"

    def __post_init__(self):
        if not isinstance(self.frame, str) or self.frame not in GOAL_FRAMES:
            raise ValueError(f"GoalObservation.frame must be one of {', '.join(map(repr, GOAL_FRAMES))}, got {self.frame!r}")

    def to_c(self):
        """The dn_goal_config this describes."""
        c = _capi.DnGoalConfig()
        c.frame = GOAL_FRAMES[self.frame]
        c.reserved = 0
        return c

    @classmethod
    def from_c(cls, c):
        for name, value in GOAL_FRAMES.items():
            if c.frame == value:
                return cls(frame=name)
        raise ValueError(f"dn_goal_config.frame = {c.frame} is not a known frame")
