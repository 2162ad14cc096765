"""What the support modules of the two loss heads share (tests/ppo_loss_support.py, tests/sac_loss_support.py, which hand every name on under
their own; pytest does not collect it; needs numpy only): the shapes that both heads are tested at, and how an output is measured against
a reference -- one float32 ulp, 2^-40, and the distance in units of a tolerance.  The data, the references and the tolerances built
from these are each head's own."""
import math

import numpy as np

BLOCK_ROWS = 1024                       # DN_ROWNORM_BLOCK_ROWS
BATCHES = (1, 2, 63, 65, 1024, 1025, 2049)
ACT_DIMS = (1, 3, 4, 8)
COVERED_FROM = 63                       # below this many rows a data set cannot promise its shares (a batch of one has one branch)
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
EPS40 = 2.0 ** -40


def ulp32(want):
    """One float32 ulp at the reference value."""
    w32 = np.abs(np.asarray(want, np.float64)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.nextafter(w32, np.float32(np.inf)) - w32).astype(np.float64)


def distance(got, want, tol):
    """The largest |got - want| / tol over the cells where the reference is finite; where it is not, got must be NaN in the same cells.
    Returns (distance, the NaN patterns agree)."""
    got, want, tol = (np.asarray(x, np.float64) for x in (got, want, tol))
    got, want, tol = np.broadcast_arrays(got, want, tol)
    fin = np.isfinite(want)
    same = bool(np.array_equal(np.isnan(got), np.isnan(want)))
    if not fin.any():
        return 0.0, same
    err = np.abs(got[fin] - want[fin])
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(err == 0.0, 0.0, err / tol[fin]))), same             # a bound of 0 (a clip fraction of 0) asks for equality
