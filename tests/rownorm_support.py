"""What the row-normaliser tests share (tests/test_rownorm_cpu.py, tests/test_gpu_rownorm.py): the reference in NumPy float64 -- the
literal update of Sol/Model/Environments/normalize.py:10-47 with np.mean / np.var of a step's rows as the batch moments, and the literal
output expression -- and the test data.  A plain module like tests/history_support.py: pytest does not collect it.  NumPy only."""
import numpy as np

ROTOR = 14468.0             # a rotor-speed column: 14468 +- 1 loses five digits in a raw-moment form
CONSTANT = 3.25
BLOCK_ROWS = 1024           # csrc/dn_internal.h DN_ROWNORM_BLOCK_ROWS


def update_from_moments(mean, var, count, batch_mean, batch_var, batch_count):
    """update_mean_var_count_from_moments, normalize.py:19-47, literally: (mean, var, count) after the batch.  The caller forms the batch
    moments, np.mean / np.var in its own shape, so that NumPy sums in the order it always has."""
    delta = batch_mean - mean
    tot_count = count + batch_count
    new_mean = mean + delta * batch_count / tot_count
    m_a = var * count
    m_b = batch_var * batch_count
    M2 = m_a + m_b + np.square(delta) * count * batch_count / tot_count
    return new_mean, M2 / tot_count, tot_count


class RunningMeanStd:
    """normalize.py:10-47, batch form."""

    def __init__(self, width):
        self.mean = np.zeros(width, np.float64)
        self.var = np.ones(width, np.float64)
        self.count = 1e-4

    def update(self, x):
        x = np.asarray(x, np.float64)
        self.mean, self.var, self.count = update_from_moments(self.mean, self.var, self.count, np.mean(x, axis=0), np.var(x, axis=0), x.shape[0])

    def stats(self):
        return np.concatenate(([self.count], self.mean, self.var))


def normalize(x, mean, var, epsilon=1e-8, clip=10.0):
    """The output expression in float64 (x float32 or float64); NaN stays NaN, as np.clip leaves it."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.clip((np.asarray(x, np.float64) - mean) / np.sqrt(var + epsilon), -clip, clip)


def special_columns(width):
    """(rotor, constant, zero) column indices; a row of fewer than 3 columns keeps the rotor column (the hard one) first."""
    if width >= 3:
        return width - 3, width - 2, width - 1
    return (0, None, None) if width == 1 else (0, 1, None)


def make_rows(rng, k, n, width):
    """[k, n, width] float32: N(0, 1) columns at scales 1e-3 .. 1e3 with offsets, and the three special columns."""
    scales = 10.0 ** ((np.arange(width) % 7) - 3.0)
    offsets = np.where(np.arange(width) % 3 == 0, 5.0, -0.25) * scales
    x = rng.standard_normal((k, n, width)) * scales + offsets
    rotor, const, zero = special_columns(width)
    x[..., rotor] = ROTOR + rng.standard_normal((k, n))
    if const is not None:
        x[..., const] = CONSTANT
    if zero is not None:
        x[..., zero] = 0.0
    return x.astype(np.float32)


def ulp_distance(got, want64):
    """Distance in float32 ulps between float32 `got` and the float64 `want64` rounded to float32 (finite cells only)."""
    want = want64.astype(np.float32)
    a = got.view(np.int32).astype(np.int64)
    b = want.view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)          # sign-magnitude -> a monotone integer line (+0 and -0 coincide)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)
