"""Observation and action history rows (include/dronenav.h dn_stack_history): the policy's input under latency and lag.

With command latency, motor lag and observation latency the 13 observation columns of one instant are no Markov state: a feed-forward
policy needs a short history of observations and of its own actions.  With DroneVecEnv(history=HistoryObservation(...)) a kernel of its
own assembles, after every step -- and for all K steps of a fused launch --, one row of W float32 per drone: `frames` observation frames
oldest first (SB3's VecFrameStack order), `actions` action frames oldest first, the 8 goal columns of the step with goal=True, zero
padding to a multiple of 4.  Where an episode ends the row restarts from zero frames with the reset observation as its newest frame, and
the terminal row (the old stack with the terminal observation) is written beside it.  Every word is a copy: nothing is normalised or
rescaled, and nothing feeds back into the flight.
"""
import dataclasses

from . import _capi
from .goal import GOAL_DIM

MAX_WIDTH = 64          # the widest row the policy kernels take


@dataclasses.dataclass(frozen=True)
class HistoryObservation:
    """frames: observation frames in a row, 1..4; actions: previous actions in a row, 0..4; goal: append the env's 8 goal columns (the env
    needs goal=GoalObservation(...)).  The row width 4 * ceil((13 frames + 4 actions + extra) / 4) must not exceed 64."""
    frames: int = 3
    actions: int = 2
    goal: bool = False

    def __post_init__(self):
        for name, lo, hi in (("frames", 1, 4), ("actions", 0, 4)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f"HistoryObservation.{name} must be an integer in {lo}..{hi}, got {v!r}")
        if not isinstance(self.goal, bool):
            raise ValueError(f"HistoryObservation.goal must be True or False, got {self.goal!r}")
        self.width(self.extra_dim)

    @property
    def extra_dim(self):
        """Extra columns the env itself supplies: the goal row or none."""
        return GOAL_DIM if self.goal else 0

    def width(self, extra_dim=None):
        """W for `extra_dim` extra columns (default: the env's own, 8 with goal=True): the rule of dn_history_width."""
        e = self.extra_dim if extra_dim is None else extra_dim
        if isinstance(e, bool) or not isinstance(e, int) or e < 0:
            raise ValueError(f"extra_dim must be an integer >= 0, got {e!r}")
        w = (13 * self.frames + 4 * self.actions + e + 3) // 4 * 4
        if w > MAX_WIDTH:
            raise ValueError(f"a history row of 13 x {self.frames} + 4 x {self.actions} + {e} columns is wider than {MAX_WIDTH}, "
                             "the policy kernels' limit")
        return w

    def to_c(self, extra_dim=None):
        """The dn_history_config this describes."""
        c = _capi.DnHistoryConfig()
        c.frames, c.actions, c.reserved = self.frames, self.actions, 0
        c.extra_dim = self.extra_dim if extra_dim is None else int(extra_dim)
        return c
