"""What the replay tests share and what needs NumPy alone (pytest does not collect it): the keyed draw written from the text of
csrc/dn_replay_draw.h in uint64 NumPy, its known answers, SB3's sample of a transition for both buffer layouts as plain indexing, the
window rule of the two buffers, and the buffer builders."""
import numpy as np

U64 = (1 << 64) - 1
MAX = (1 << 31) - 1
PLAIN, RING = 0, 1                      # DN_REPLAY_PLAIN, DN_REPLAY_RING
FIELDS = ("obs", "next_obs", "actions", "rewards", "dones")


def draw(seed, draw_, s, n, skip, start=0, count=8):
    """(slots, envs) of rows start .. start + count - 1 as int64 arrays."""
    x = (seed ^ (draw_ * 0xD1342543DE82EF95 & U64)) & U64
    j1 = np.arange(start + 1, start + count + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(x) + j1 * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        raw = (((z >> np.uint64(32)) * np.uint64(s)) >> np.uint64(32)).astype(np.int64)
        env = (((z & np.uint64(0xFFFFFFFF)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    slot = raw + ((raw >= skip) if skip >= 0 else 0)
    return slot, env


def flat(seed, draw_, s, n, skip, start=0, count=8):
    slot, env = draw(seed, draw_, s, n, skip, start, count)
    return slot * n + env


# draw(seed, draw, S, N, skip) -> (slots, envs) of the first rows, computed once with the statement above and kept as literals
KNOWN = [
    ((0, 0, 5, 7, -1), [4, 2, 0, 4, 0, 1, 0, 3], [3, 4, 3, 3, 2, 3, 0, 5]),
    ((1, 2, 5, 7, 2), [1, 4, 1, 1, 5, 4, 1, 5], [6, 0, 1, 5, 6, 5, 4, 3]),
    ((U64, U64, MAX, MAX, -1), [1792654871, 2114717153, 1391844100, 1369261991], [784006440, 1865083658, 69374683, 376241447]),
    ((0x0123456789ABCDEF, 1 << 40, 1000, 32768, 0), [317, 660, 884, 341], [7036, 15064, 16824, 30255]),
]

UNIFORM_SEEDS = (0, 1, 0xDEADBEEF, U64)
UNIFORM_DRAWS = (0, 1, 1 << 40)
UNIFORM_SHAPES = ((7, 65), (64, 64), (1000, 1000), (3, 1), (1, 3), (8, 8))
UNIFORM_ROWS = 1 << 20


def chi2_score(counts):
    """(chi^2 - (k - 1)) / sqrt(2 (k - 1)) of observed counts against the uniform distribution over their k cells; 0 for one cell."""
    counts = np.asarray(counts, np.float64)
    k = counts.size
    if k < 2:
        return 0.0
    want = counts.sum() / k
    chi2 = float(((counts - want) ** 2).sum() / want)
    return (chi2 - (k - 1)) / np.sqrt(2.0 * (k - 1))


def window(layout, buffer_size, pos, full):
    """(valid, skip) as ReplayBuffer.sample and RingReplayBuffer._sample_slots read pos / full; valid == 0: the buffer is empty."""
    if layout == PLAIN:
        return (buffer_size if full else pos), -1
    if not full:
        return pos, -1
    return (buffer_size - 1, pos) if pos else (buffer_size, -1)


def clamp(indices, t, n):
    """(slot, env) of caller's flat indices: C's truncating division by n, then each clamped into its range."""
    slots, envs = [], []
    for v in (int(x) for x in np.asarray(indices, np.int64)):                   # Python integers: exact at both ends of int64
        q = abs(v) // n * (1 if v >= 0 else -1)
        slots.append(min(max(q, 0), t - 1))
        envs.append(min(max(v - q * n, 0), n - 1))
    return np.array(slots, np.int64), np.array(envs, np.int64)


def _words(rng, shape):
    """Random int32 bit patterns viewed as float32: NaN payloads, infinities and denormals included."""
    return rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32).view(np.float32)


def _flags(rng, t, n):
    """(done, timeout) uint8 [t][n] with every combination present wherever t * n >= 4, in random places."""
    combo = np.arange(t * n) % 4
    rng.shuffle(combo)
    combo = combo.reshape(t, n)
    return (combo & 1).astype(np.uint8), (combo >> 1).astype(np.uint8)


def build(layout, t, n, d, a, seed=0):
    """The six source arrays of one buffer of `layout`, named as the buffer classes name them."""
    rng = np.random.default_rng([layout, t, n, d, a, seed])
    done, timeout = _flags(rng, t, n)
    if layout == PLAIN:
        return dict(obs=_words(rng, (t, n, d)), next_obs=_words(rng, (t, n, d)), actions=_words(rng, (t, n, a)), rewards=_words(rng, (t, n)),
                    dones=done.astype(np.float32), timeouts=timeout.astype(np.float32))
    return dict(obs_ring=_words(rng, (t + 1, n, d)), terminal_obs=_words(rng, (t, n, d)), actions=_words(rng, (t, n, a)),
                rewards=_words(rng, (t, n)), done_flags=done, timeout_flags=timeout)


def sample(layout, src, slot, env):
    """SB3's view of the transitions (slot, env): plain indexing."""
    if layout == PLAIN:
        dones = src["dones"][slot, env] * (np.float32(1.0) - src["timeouts"][slot, env])
        return dict(obs=src["obs"][slot, env], next_obs=src["next_obs"][slot, env], actions=src["actions"][slot, env],
                    rewards=src["rewards"][slot, env], dones=dones.astype(np.float32))
    done = src["done_flags"][slot, env] != 0
    nxt = np.where(done[:, None], src["terminal_obs"][slot, env].view(np.int32), src["obs_ring"][slot + 1, env].view(np.int32)).view(np.float32)
    dones = (done & (src["timeout_flags"][slot, env] == 0)).astype(np.float32)
    return dict(obs=src["obs_ring"][slot, env], next_obs=nxt, actions=src["actions"][slot, env], rewards=src["rewards"][slot, env], dones=dones)
