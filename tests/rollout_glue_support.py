"""What the rollout-glue tests share (tests/test_rollout_glue_cpu.py, tests/test_gpu_rollout_glue.py): the plain statement of each small
kernel between the policy and the step -- dn_gae, dn_add_bootstrap, dn_policy_sample, dn_squashed_sample, dn_pack_done / dn_compact_done
-- in numpy, the shapes the tests run them at, and their inputs.  numpy only.  A plain module like tests/mlp_support.py -- pytest does
not collect it and does not rewrite its asserts.

The float32 forms round every operation on its own, as the kernels do (the library is built with -ffp-contract=off), so the kernels are
held to them bit for bit; the float64 forms are what the float32 forms are measured against."""
import functools

import numpy as np

FLEETS = (1, 63, 64, 65, 255, 256, 257, 1000)           # the 64-drone tile (one Philox counter per tile) and the 256-lane workgroup, +-1
GAE_SHAPES = ((1, 1), (1, 257), (2, 255), (7, 256), (33, 1), (128, 64))       # (T, N)
PACK_SIZES = (1, 63, 64, 65, 4097, 65535, 65536, 65537, 131073)               # the 64-drone word, the 65 536-drone workgroup, a third one
GAMMA_LAMBDA = ((0.99, 0.95), (1.0, 1.0), (0.0, 0.95), (0.99, 0.0))
START_DENSITIES = (0.0, 0.05, 1.0)
LOG_STD_ROWS = ((-20.0, -5.5, 0.0, 2.0), (-1.0, -2.0, -0.5, -3.0), (0.3, -0.7, 1.9, -19.5))
MEAN_SCALES = (0.1, 1.0, 10.0, 100.0)                   # per action column
PACK_DENSITIES = (1.0, 0.5, 0.003, 0.0)
HALF_LOG_2PI = 0.91893853320467274178
SNAN_INT, QNAN_INT = 0x7F800001, 0x7FC00001             # int32 episode lengths whose float reinterpretation is a signalling / a quiet NaN
PATTERN = 0x7FC12345                                    # the guard cells' bits: a quiet NaN no kernel here produces (mlp_support's)

_F = np.float32


# ---- GAE ----------------------------------------------------------------------------------------------------------------------------
def gae32(r, v, d, lv, ld, gamma, lam):
    """The float32 recursion in the kernel's operation order, all drones of a step at once: [T, N] rewards, values, start flags; [N] last
    values and flags.  Returns (adv, ret)."""
    r, v, lv = np.asarray(r, _F), np.asarray(v, _F), np.asarray(lv, _F)
    d, ld = np.asarray(d).astype(_F), np.asarray(ld).astype(_F)
    g32, gl32, one = _F(gamma), _F(float(gamma) * float(lam)), _F(1.0)
    adv, ret = np.empty_like(r), np.empty_like(r)
    last, nnt, nv = np.zeros(r.shape[1], _F), one - ld, lv
    with np.errstate(all="ignore"):
        for t in range(r.shape[0] - 1, -1, -1):
            delta = (r[t] + (g32 * nv) * nnt) - v[t]
            last = delta + (gl32 * nnt) * last
            adv[t], ret[t] = last, last + v[t]
            nnt, nv = one - d[t], v[t]
    return adv, ret


def gae64(r, v, d, lv, ld, gamma, lam):
    """The same recursion in float64 on the same float32 inputs."""
    r, v, lv = np.asarray(r, np.float64), np.asarray(v, np.float64), np.asarray(lv, np.float64)
    d, ld = np.asarray(d).astype(np.float64), np.asarray(ld).astype(np.float64)
    adv, ret = np.empty_like(r), np.empty_like(r)
    last, nnt, nv = np.zeros(r.shape[1]), 1.0 - ld, lv
    with np.errstate(all="ignore"):
        for t in range(r.shape[0] - 1, -1, -1):
            delta = (r[t] + (gamma * nv) * nnt) - v[t]
            last = delta + (gamma * lam * nnt) * last
            adv[t], ret[t] = last, last + v[t]
            nnt, nv = 1.0 - d[t], v[t]
    return adv, ret


@functools.lru_cache(None)
def gae_inputs(T, N, density, last_all_done=False):
    """(rewards, values, starts, last_values, last_starts) of one case: rewards of the environment's size with a crash penalty here and
    there, values of a critic's size, start flags at `density` (0 and 1 give none and all, the last flags included)."""
    rng = np.random.default_rng(1000 * T + N + int(1e4 * density))
    r = rng.standard_normal((T, N)).astype(_F)
    r[rng.random((T, N)) < 0.02] = _F(-10.0)
    v = (3.0 * rng.standard_normal((T, N))).astype(_F)
    d = (rng.random((T, N)) < density).astype(np.uint8)
    lv = (3.0 * rng.standard_normal(N)).astype(_F)
    ld = np.ones(N, np.uint8) if last_all_done else (rng.random(N) < density).astype(np.uint8)
    for a in (r, v, d, lv, ld):
        a.setflags(write=False)
    return r, v, d, lv, ld


def gae_cases():
    """Every (density, last flags all set, gamma, lambda) a shape is run at."""
    for density in START_DENSITIES:
        for last_all in ((False, True) if density == 0.05 else (False,)):
            for gamma, lam in GAMMA_LAMBDA:
                yield density, last_all, gamma, lam


# ---- bootstrap ----------------------------------------------------------------------------------------------------------------------
def bootstrap32(reward, tv, trunc, gamma):
    """float32(r + float32(gamma) * tv) where trunc != 0, the input bits elsewhere."""
    reward, tv = np.asarray(reward, _F), np.asarray(tv, _F)
    out, m = reward.copy(), np.asarray(trunc) != 0
    with np.errstate(all="ignore"):
        out[m] = reward[m] + _F(gamma) * tv[m]
    return out


# ---- the Gaussian policy's draw -----------------------------------------------------------------------------------------------------
def logprob32(z, log_std):
    """sum_j log N(a_j; mu_j, sigma_j) with (a - mu) / sigma = z, in float32 and in the kernel's order: z [n, 4], log_std [4] or [n, 4]."""
    z = np.asarray(z, _F)
    ls = np.broadcast_to(np.asarray(log_std, _F), z.shape)
    c, lp = _F(HALF_LOG_2PI), np.zeros(z.shape[0], _F)
    for j in range(4):
        lp = lp + ((((_F(-0.5) * z[:, j]) * z[:, j]) - ls[:, j]) - c)
    return lp


def logprob64(z, log_std):
    z = np.asarray(z, np.float64)
    return (-0.5 * z * z - np.broadcast_to(np.asarray(log_std, np.float64), z.shape) - HALF_LOG_2PI).sum(1)


def sample64(mean, log_std, z):
    """mean + exp(log_std) z in float64 on the float32 inputs."""
    return np.asarray(mean, np.float64) + np.exp(np.asarray(log_std, np.float64)) * np.asarray(z, np.float64)


def sample_allowance(log_std, z, a):
    """How far a float32 evaluation of mean + expf(log_std) z may be from sample64: one ulp on expf (the device library's documented
    accuracy) and half an ulp on the product, both relative to the product, plus half an ulp of the sum `a`."""
    prod = np.abs(np.exp(np.asarray(log_std, np.float64)) * np.asarray(z, np.float64))
    return 1.5 * 2.0 ** -23 * prod + 0.5 * np.spacing(np.abs(np.asarray(a, _F))).astype(np.float64)


@functools.lru_cache(None)
def means(n):
    """[n, 4] float32 means, column j at scale MEAN_SCALES[j]."""
    m = (np.random.default_rng(77 + n).standard_normal((n, 4)) * np.array(MEAN_SCALES)).astype(_F)
    m.setflags(write=False)
    return m


# ---- the squashed Gaussian (SAC) ------------------------------------------------------------------------------------------------------
def squashed64(mu, log_std, z):
    """tanh(mu + exp(clip(log_std, -20, 2)) z) in float64."""
    return np.tanh(sample64(mu, np.clip(np.asarray(log_std, np.float64), -20.0, 2.0), z))


def squashed_logprob32(z, log_std, a):
    """The float32 form of the squashed log-probability, evaluated from the squashed action itself as SB3 does: logprob32 per dimension
    minus log(1 - a^2 + 1e-6) (numpy's float32 log: the bar on it is relative, not bit for bit)."""
    z, a = np.asarray(z, _F), np.asarray(a, _F)
    ls = np.clip(np.asarray(log_std, _F), _F(-20.0), _F(2.0))
    c, lp = _F(HALF_LOG_2PI), np.zeros(z.shape[0], _F)
    for j in range(4):
        lp = lp + (((((_F(-0.5) * z[:, j]) * z[:, j]) - ls[:, j]) - c) - np.log((_F(1.0) - a[:, j] * a[:, j]) + _F(1e-6)))
    return lp


@functools.lru_cache(None)
def squashed_rows(n):
    """[n, 8] (mu | log_std) rows: random ones, then -- cycling over the fleet from its first drone -- the clamp edges, saturation
    (mu = +-12 at log_std = -20) and denormal-scale means (+-1e-30).  Returns (rows, saturated [n] bool, tiny [n] bool)."""
    rng = np.random.default_rng(500 + n)
    rows = np.concatenate((rng.standard_normal((n, 4)), 1.5 * rng.standard_normal((n, 4)) - 0.5), 1).astype(_F)
    special = [((0.3, -0.2, 0.1, 0.0), 5.0), ((0.3, -0.2, 0.1, 0.0), -30.0), ((12.0, -12.0, 12.0, -12.0), -20.0),
               ((-12.0, 12.0, -12.0, 12.0), -20.0), ((1e-30, -1e-30, 1e-30, -1e-30), -20.0), ((-1e-30, 1e-30, -1e-30, 1e-30), 0.0)]
    kind = np.full(n, -1)
    for i in range(0, n, 3):                              # every third drone, so that random rows stay at every fleet but n = 1
        k = (i // 3) % len(special)
        rows[i, :4], rows[i, 4:], kind[i] = special[k][0], special[k][1], k
    rows.setflags(write=False)
    return rows, (kind == 2) | (kind == 3), (kind == 4) | (kind == 5)


# ---- done compaction ------------------------------------------------------------------------------------------------------------------
def pack_reference(bits, tobs, ep_ret, ep_len, trunc, found):
    """(indices int32 [count], rows uint32 [count, 16]): the finished drones in ascending order and, per drone, terminal_obs[13], the
    episode return, the episode length's bits and truncated | found << 8 -- every word as its bit pattern."""
    idx = np.nonzero(np.asarray(bits))[0].astype(np.int32)
    rows = np.empty((idx.size, 16), np.uint32)
    rows[:, :13] = np.ascontiguousarray(tobs, _F).view(np.uint32).reshape(-1, 13)[idx]
    rows[:, 13] = np.ascontiguousarray(ep_ret, _F).view(np.uint32)[idx]
    rows[:, 14] = np.ascontiguousarray(ep_len, np.int32).view(np.uint32)[idx]
    rows[:, 15] = (np.asarray(trunc)[idx].astype(np.int64) | (np.asarray(found)[idx].astype(np.int64) << 8)).astype(np.uint32)
    return idx, rows


def mask_words(bits, n):
    """The ballot words of `bits` [n] bool as int64 (bit i & 63 of word i >> 6; no bit beyond the fleet)."""
    padded = np.zeros((n + 63) // 64 * 64, np.uint8)
    padded[:n] = np.asarray(bits, np.uint8)[:n]
    return np.packbits(padded, bitorder="little").view(np.int64)


@functools.lru_cache(None)
def pack_inputs(n):
    """(terminal_obs [n, 13], ep_return [n], ep_length [n] int32, truncated [n] uint8, found_targets [n] int32): random records; every
    seventh length is one of the two NaN patterns."""
    rng = np.random.default_rng(9000 + n)
    tobs = rng.standard_normal((n, 13)).astype(_F)
    ep_ret = (50.0 * rng.standard_normal(n)).astype(_F)
    ep_len = rng.integers(1, 4097, n).astype(np.int32)
    ep_len[0::14], ep_len[7::14] = SNAN_INT, QNAN_INT
    trunc = rng.integers(0, 2, n).astype(np.uint8)
    found = rng.integers(0, 65, n).astype(np.int32)
    for a in (tobs, ep_ret, ep_len, trunc, found):
        a.setflags(write=False)
    return tobs, ep_ret, ep_len, trunc, found


def done_bits(n, density):
    """[n] bool at `density` (1 and 0: all and none), the first and the last drone of the fleet flagged whenever any is."""
    if density >= 1.0:
        return np.ones(n, bool)
    b = np.random.default_rng(n + int(1e6 * density)).random(n) < density
    if density > 0.0:
        b[0] = b[-1] = True
    return b


# ---- bits ---------------------------------------------------------------------------------------------------------------------------
def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(u32(a), u32(b))
