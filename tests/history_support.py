"""What the history-row tests share (tests/test_history_cpu.py, tests/test_gpu_history.py): the step rule of dn_stack_history
(include/dronenav.h) as a plain NumPy loop over steps and drones, and the bit-level comparison.  A plain module like
tests/goal_support.py -- pytest does not collect it.  NumPy only."""
import numpy as np

OBS, ACT = 13, 4
# the configurations of the synthetic GPU tests and of the width checks: (frames, actions, extra_dim)
CONFIGS = ((1, 0, 0), (1, 4, 0), (4, 0, 0), (4, 3, 0), (3, 2, 8), (2, 2, 8))


def width(frames, actions, extra_dim):
    """W = 4 ceil((13 F + 4 A + E) / 4), or None where the configuration is refused."""
    if not (1 <= frames <= 4 and 0 <= actions <= 4 and extra_dim >= 0):
        return None
    w = -(-(OBS * frames + ACT * actions + extra_dim) // 4) * 4
    return w if w <= 64 else None


def bits(x):
    """The int32 view of a float32 array: NaN payloads and -0.0 count."""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def stack_reference(cfg, prev, obs, actions, done, terminal_obs, extra, terminal_extra):
    """The sequential definition.  cfg = (F, A, E); obs [K, N, 13], actions [K, N, 4] or None, done [K, N] or None, terminal_obs
    [K, N, 13] or None, extra / terminal_extra [K, N, E] or None, prev [N, W] or None.  Returns (rows, terminal_rows), both [K, N, W]
    float32; terminal_rows is zero where no episode ended.  Works on the bit patterns (uint32), so every word is a copy."""
    F, A, E = cfg
    W = width(F, A, E)
    u = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)      # noqa: E731
    prev, obs, actions, terminal_obs, extra, terminal_extra = map(u, (prev, obs, actions, terminal_obs, extra, terminal_extra))
    K, N = obs.shape[:2]
    rows = np.zeros((K, N, W), np.uint32)
    term = np.zeros((K, N, W), np.uint32)
    zeros = lambda m: np.zeros(m, np.uint32)                                                            # noqa: E731

    def assemble(frames, acts, x):
        row = zeros(W)
        row[:OBS * F] = np.concatenate(frames)
        if A:
            row[OBS * F:OBS * F + ACT * A] = np.concatenate(acts)
        row[OBS * F + ACT * A:OBS * F + ACT * A + E] = x
        return row

    for i in range(N):
        P = zeros(W) if prev is None else prev[i]
        for t in range(K):
            o = obs[t, i]
            a = zeros(ACT) if actions is None else actions[t, i]
            d = done is not None and bool(done[t, i])
            x = zeros(E) if extra is None else extra[t, i]
            # shift(P): P without its oldest observation frame and its oldest action frame
            frames = [P[OBS * j:OBS * (j + 1)] for j in range(1, F)]
            acts = [P[OBS * F + ACT * j:OBS * F + ACT * (j + 1)] for j in range(1, A)]
            if not d:
                row = assemble(frames + [o], acts + [a], x)
            else:
                if terminal_obs is not None:
                    xt = zeros(E) if terminal_extra is None else terminal_extra[t, i]
                    term[t, i] = assemble(frames + [terminal_obs[t, i]], acts + [a], xt)
                row = assemble([zeros(OBS)] * (F - 1) + [o], [zeros(ACT)] * A, x)
            rows[t, i] = row
            P = row
    return rows.view(np.float32), term.view(np.float32)


def random_words(rng, shape):
    """float32 arrays of random BIT PATTERNS (NaNs with payloads, infinities, subnormals and -0.0 among them)."""
    w = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    flat = w.reshape(-1)
    flat[:: 7] = 0x80000000                       # -0.0
    flat[3:: 11] = 0x7FC00001 + (flat[3:: 11] & 0xFFFF)      # quiet NaNs with payloads
    return w.view(np.float32)


def done_patterns(rng, K, N):
    """name -> uint8 [K, N]: the done fields of the issue, with events at lanes 0, 63 and 64 where the fleet has them."""
    lanes = [l for l in (0, 63, 64) if l < N]
    z = lambda: np.zeros((K, N), np.uint8)                  # noqa: E731
    out = {"none": z()}
    for name, steps, who in (("all at step 0", slice(0, 1), slice(None)), ("last step", slice(K - 1, K), lanes),
                             ("two consecutive", slice(max(K - 2, 0), K), lanes), ("every step", slice(None), lanes)):
        out[name] = z()
        out[name][steps, who] = 1
    out["bernoulli"] = (rng.random((K, N)) < 0.3).astype(np.uint8)
    return out
