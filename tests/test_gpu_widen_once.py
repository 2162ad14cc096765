"""The four- and five-wave fused kernels mail their float32 state words already widened (MailL.wide, MailG.we), the observation wave
keeps prev_vel / prev_ang_v widened for the whole launch, and the report wave takes `d_e <= threshold` from a bit of the flag word.
None of that may change a bit: every output of every step, the final state and the normaliser's statistics are held against the
one-wave kernel, on the smallest fleet that has a ragged last tile (132 = 64 + 64 + 4), over chained launches of several lengths so
that episode ends fall on the first and last step of a launch, inside launches and across their boundaries."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gpu_support import pkg as _gpu  # noqa: E402

N = 132                                   # three tiles, the last with 4 rows (dn_step_many needs a multiple of four)
DEV = "cuda:0"
ANG_LIMIT2 = 0.3 * 0.3                    # smoothness_reward's bar on |entry ang_v - prev_ang_v|^2


def _bang(rng, n):
    return rng.uniform(-1, 1, (n, 4)).astype(np.float32)


def _hover(rng, n):
    return (0.0922 + 0.003 * rng.standard_normal((n, 4))).astype(np.float32)


def _envs(monkeypatch, shapes, norm, max_steps):
    from drl_dronenavigation_amd import tracks
    pkg = _gpu()
    envs = {}
    for shape in shapes:
        monkeypatch.setenv("DN_WAVES", shape)
        envs[shape] = pkg.DroneVecEnv(tracks.reaching(), N, device=DEV, normalize_obs=norm, max_steps=max_steps, seed=5)
        assert envs[shape].kernel_waves(fused=True) == int(shape)
    monkeypatch.delenv("DN_WAVES")
    first = {s: e.reset_tensor().clone() for s, e in envs.items()}
    for s in shapes[1:]:
        assert torch.equal(first[shapes[0]], first[s]), ("reset", s)
    return envs


def _same_state(a, b, tag):
    for k in a.dtype.names:               # body, prev_vel / prev_ang_v, Monitor words, rms_mean / rms_var / rms_count
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), (tag, k)


def _pen_ang_fired(state, first_reward):
    """Drones whose angular smoothness penalty applies in the NEXT step, from the one-wave env's state: the step's entry angular
    velocity less its stale copy, beyond the bar by a margin no rounding reaches, and the step not a collision (reward -10)."""
    d = state["ang_v"].astype(np.float64) - state["prev_ang_v"].astype(np.float64)
    return int(((np.sum(d * d, axis=1) > 1.01 * ANG_LIMIT2) & (first_reward != -10.0)).sum())


def _chain(envs, make_actions, seed, lengths, total):
    """Launches of the given lengths, cycled until `total` steps are done, the same actions on every env.  Returns (finished
    drone-steps, drone-steps at a launch's first step with the angular smoothness penalty applied), both read off envs['1']."""
    rng = np.random.default_rng(seed)
    done_n = pen_n = t = j = 0
    while t < total:
        K = min(lengths[j % len(lengths)], total - t)
        j += 1
        acts = torch.from_numpy(np.stack([make_actions(rng, N) for _ in range(K)])).to(DEV)
        entry = envs["1"].get_state()
        outs = {s: {k: v.clone() for k, v in e.rollout_tensor(acts, want_terminal=True).items()} for s, e in envs.items()}
        ref = outs["1"]
        for s, o in outs.items():
            if s == "1":
                continue
            for k in ref:
                if k in ("terminal_obs", "ep_return", "ep_length"):      # written for finished drones only
                    d = ref["done"].bool()
                    assert torch.equal(ref[k][d], o[k][d]), (s, t, K, k)
                else:
                    assert torch.equal(ref[k], o[k]), (s, t, K, k)
        done_n += int(ref["done"].sum())
        pen_n += _pen_ang_fired(entry, ref["reward"][0].cpu().numpy())
        t += K
    st = {s: e.get_state() for s, e in envs.items()}
    stats = {s: e.stats() for s, e in envs.items()}
    for s in envs:
        if s != "1":
            _same_state(st["1"], st[s], s)
            assert stats["1"] == stats[s], s
    for e in envs.values():
        e.close()
    return done_n, pen_n


@pytest.mark.parametrize("norm", [True, False])
def test_widened_mail_is_bit_identical_across_episode_ends(norm, monkeypatch):
    """U(-1, 1) actions (collisions) and max_steps = 7 (truncations), launches of 2, 3, 5 and 20 steps chained for 60 steps: four waves
    with and without the normaliser, five waves with it, against one wave."""
    envs = _envs(monkeypatch, ("1", "4") + (("5",) if norm else ()), norm, max_steps=7)
    done_n, pen_n = _chain(envs, _bang, seed=21, lengths=(2, 3, 5, 20), total=60)
    assert done_n > N                     # every drone was truncated several times over
    # the pen_ang branch of the reward ran (on the one-wave kernel's own state): an error in the carried prev_ang_v could not hide
    assert pen_n > 0


@pytest.mark.parametrize("norm", [True, False])
def test_widened_mail_is_bit_identical_over_long_flights(norm, monkeypatch):
    """Hover-band actions and max_steps = 4096 for 40 steps: no resets, the smoothness copies carried across every iteration of a launch
    and across launch boundaries."""
    envs = _envs(monkeypatch, ("1", "4") + (("5",) if norm else ()), norm, max_steps=4096)
    _chain(envs, _hover, seed=22, lengths=(2, 3, 5, 20), total=40)
