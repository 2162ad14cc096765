"""What the minibatch tests share and what needs NumPy alone (pytest does not collect it): the keyed permutation written from the text of
include/dronenav.h in uint32 / uint64 NumPy, the sample-to-row rule, the float64 reference of the advantage normalisation, and the test
data."""
import numpy as np

BLOCK_ROWS = 1024                       # DN_ROWNORM_BLOCK_ROWS
SIZES = (1, 2, 3, 4, 5, 17, 64, 1000, 1025, 4097, 65537)
SEEDS = (0, 7, 2 ** 64 - 1)
EPOCHS = (0, 1, 2 ** 40)
U64 = (1 << 64) - 1


def _fmix32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def round_keys(seed, epoch):
    """Six round keys: the high halves of six splitmix64 outputs from the state seed ^ (epoch * 0xD1342543DE82EF95), all mod 2^64."""
    x = (seed ^ (epoch * 0xD1342543DE82EF95 & U64)) & U64
    keys = []
    for _ in range(6):
        x = (x + 0x9E3779B97F4A7C15) & U64
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & U64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & U64
        z ^= z >> 31
        keys.append(z >> 32)
    return keys


def permutation(m, seed, epoch, start=0, count=None):
    """pi(start) .. pi(start + count - 1) of [0, m) as int64, and the most walk iterations any element needed."""
    count = m - start if count is None else count
    b = max(1, int(m - 1).bit_length())
    h = max(1, (b + 1) // 2)
    mask = np.uint32((1 << h) - 1)
    keys = [np.uint32(k) for k in round_keys(seed, epoch)]
    sh, back = np.uint32(h), np.uint32(32 - h)

    def one_pass(v):
        left, right = (v >> sh) & mask, v & mask
        for k in keys:
            f = _fmix32(right + k) >> back
            left, right = right, (left ^ f) & mask
        return (left << sh) | right

    v = np.arange(start, start + count, dtype=np.uint32)
    todo = np.ones(count, bool)
    walks = 0
    with np.errstate(over="ignore"):
        while todo.any():
            v[todo] = one_pass(v[todo])
            todo &= v >= m
            walks += 1
    return v.astype(np.int64), walks


def source_rows(samples, n_steps, n_envs):
    """Sample s is drone s // n_steps at step s % n_steps (swap-and-flatten order); its row in the step-major buffer."""
    s = np.asarray(samples, np.int64)
    return (s % n_steps) * n_envs + s // n_steps


def gather(x, samples):
    """The rows of step-major x [n_steps, n_envs, ...] the samples name, bit for bit."""
    n_steps, n_envs = x.shape[:2]
    return x.reshape((n_steps * n_envs,) + x.shape[2:])[source_rows(samples, n_steps, n_envs)]


def normalize(a, epsilon=1e-8, reverse=False):
    """(a - mean) / (std + epsilon) in float64 with the unbiased std; a batch of one is returned as it is.  reverse: the moments summed in
    the opposite order."""
    x = np.asarray(a, np.float32).astype(np.float64)
    if len(x) == 1:
        return x
    y = x[::-1].copy() if reverse else x
    mean = np.mean(y)
    std = np.std(y, ddof=1)
    return (x - mean) / (std + epsilon)


def noisy_advantages(rng, shape):
    """2 N(0, 1) + 0.3 as float32."""
    return (2.0 * rng.standard_normal(shape) + 0.3).astype(np.float32)


def offset_advantages(rng, shape):
    """4096 + j 2^-10 for integers |j| <= 16384 (exact in float32; standard deviation about 9.2, so that |mean| 2^-50 / std stays under
    the 2^-40 of tolerance() with a factor of two to spare).  x^2 is about 2^24 against a variance of 85: E[x^2] - E[x]^2 loses five to
    six digits in float64 and all but one in float32 (one ulp of x^2 is 2), while the shifted form loses none -- all its sums are exact
    here."""
    return (4096.0 + rng.integers(-16384, 16385, shape) * 2.0 ** -10).astype(np.float32)


DATA = {"noisy": noisy_advantages, "offset": offset_advantages}


def tolerance(want):
    """Per cell: one float32 ulp of the reference value or 2^-40 absolute, whichever is larger.  The first term is the single rounding to
    float32 plus the last float64 bits of mean and std, which depend on the summation order; the second covers outputs near zero, where
    the relative error of a - mean is unbounded: its absolute error is below |mean| 2^-50 / std, under 2^-40 for both data sets."""
    w32 = np.abs(want).astype(np.float32)
    ulp = (np.nextafter(w32, np.float32(np.inf)) - w32).astype(np.float64)
    return np.maximum(ulp, 2.0 ** -40)
