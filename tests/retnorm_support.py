"""What the return-normaliser tests share (tests/test_retnorm_cpu.py, tests/test_gpu_retnorm.py): the reference in NumPy float64 -- the
reward half of SB3's VecNormalize [from recall] in its four literal steps, on the literal RunningMeanStd update of
Sol/Model/Environments/normalize.py:10-47 with np.mean / np.var of a step's returns as the batch moments -- and the test data.  A plain
module like tests/rownorm_support.py: pytest does not collect it.  NumPy only."""
import numpy as np

# csrc/dn_internal.h DN_ROWNORM_BLOCK_ROWS; the float32 ulp distance; the literal update, which both references share
from rownorm_support import BLOCK_ROWS, ulp_distance, update_from_moments  # noqa: F401

FLEETS = (1, 63, 64, 65, 1000, 2 * BLOCK_ROWS + 1)      # the last: three blocks, the third of one drone
STEPS = (1, 3, 9, 17)


class ReturnNormalizer:
    """VecNormalize(norm_reward=True), the reward half: one discounted return per env, one RunningMeanStd of the returns."""

    def __init__(self, n, gamma=0.99, clip=10.0, epsilon=1e-8):
        self.gamma, self.clip, self.epsilon = gamma, clip, epsilon
        self.count, self.mean, self.var = 1e-4, 0.0, 1.0
        self.returns = np.zeros(n, np.float64)

    def _update(self, x):
        """normalize.py:19-47, batch form, on a vector of scalars."""
        self.mean, self.var, self.count = update_from_moments(self.mean, self.var, self.count, np.mean(x), np.var(x), x.shape[0])

    def step(self, r, d):
        """r float32 [n], d uint8 [n] -> the scaled, clipped reward in float64."""
        self.returns = self.returns * self.gamma + r            # 1. float32 widens to float64; a product, then a sum
        self._update(self.returns)                              # 2.
        out = scale(r, self.var, self.epsilon, self.clip)       # 3. with the updated variance; no mean is subtracted
        self.returns[d != 0] = 0.0                              # 4.
        return out

    def stats(self):
        return np.array([self.count, self.mean, self.var], np.float64)


def scale(r, var, epsilon=1e-8, clip=10.0):
    """The output expression in float64 (r float32 or float64); NaN stays NaN, as np.clip leaves it."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.clip(np.asarray(r, np.float64) / np.sqrt(var + epsilon), -clip, clip)


def make_rewards(rng, k, n):
    """([k, n] float32 rewards 3 N(0, 1) - 0.5, [k, n] uint8 done flags with probability 0.05 per cell)."""
    r = (3.0 * rng.standard_normal((k, n)) - 0.5).astype(np.float32)
    d = (rng.random((k, n)) < 0.05).astype(np.uint8)
    return r, d


def clip_case(n=1000, clip=1.0):
    """The clip case of the output test: three calls of three single steps.  Returns ([(r [3, n], d [3, n])] * 3, the fraction of the
    cells of calls two and three that lie beyond the clip on the reference)."""
    rng = np.random.default_rng(4)
    ref = ReturnNormalizer(n, clip=clip)
    calls, beyond = [], 0
    for call in range(3):
        r, d = make_rewards(rng, 3, n)
        calls.append((r, d))
        for t in range(3):
            ref.step(r[t], d[t])
            if call >= 1:
                beyond += int((np.abs(scale(r[t], ref.var, ref.epsilon, np.inf)) > clip).sum())
    return calls, beyond / (6 * n)
