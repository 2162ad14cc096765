"""The five-wave fused step takes its roles from the SIMDs its waves landed on (csrc/dn_role_place.h): a role only says which wave runs
which function, so nothing the step returns or keeps may depend on the placement -- and the placement may differ from launch to launch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gpu_support import pkg as _gpu  # noqa: E402

STEPS = (1, 2, 3, 7)        # the pipeline's fill and drain edges; with max_steps = 3 the time limit falls on the edge of a launch (3) and inside one (7)


LAUNCH_FLEET = {1: 4, 63: 60, 65: 68}      # dn_step_many takes whole groups of four drones: the nearest fleet of the same tile shape


def _run(pkg, track, n, acts, k, singles=False):
    """A fresh environment of the same seed, its reset, one launch of k steps (singles: k single steps): everything rollout_tensor
    (step_tensor) returns, every field of the state blob (the normaliser's statistics included) and the episode statistics, as bytes."""
    env = pkg.DroneVecEnv(track, n, normalize_obs=True, max_steps=3, seed=7, device="cuda:0")
    try:
        env.reset()
        waves = env.kernel_waves(fused=True)
        if singles:
            with pytest.raises(pkg._capi.DroneNavError, match="num_envs % 4 == 0"):
                env.rollout_tensor(acts[:2].contiguous())
            out = {}
            for t in range(k):
                o, r, d, info = env.step_tensor(acts[t])
                out.update({f"obs{t}": o.clone(), f"reward{t}": r.clone(), f"done{t}": d.clone()}, **{f"{name}{t}": v.clone() for name, v in info.items() if v is not None})
        else:
            out = env.rollout_tensor(acts[:k].contiguous(), want_terminal=True)
        torch.cuda.synchronize()
        got = {name: t.cpu().numpy().tobytes() for name, t in out.items()}
        state = env.get_state()              # every field of dn_env_state; the struct's padding bytes are nobody's
        got["state"] = b"".join(np.ascontiguousarray(state[name]).tobytes() for name in state.dtype.names)
        got["stats"] = repr(sorted(env.stats().items()))
    finally:
        env.close()
    return waves, got


SECOND_TILES = "64 (num_cus + 1) + 4"      # one full and one ragged second tile (the workgroups that land beside tiles 0 and 1 on their CUs) beside a full set of first tiles


@pytest.mark.parametrize("n", [1, 63, 64, 65, 640, pytest.param(SECOND_TILES, id="second_tiles")])      # a ragged tile, one tile, two tiles, ten tiles; the shipped second-tile rows
def test_five_waves_give_the_bits_of_one_wave_whatever_the_placement(n, monkeypatch):
    """DN_WAVES=5 against DN_WAVES=1 from the same reset, K in {1, 2, 3, 7}, three runs of the five-wave side.  dn_step_many refuses a
    fleet that is no multiple of four drones, so at n in {1, 63, 65} the refusal is asserted, the K steps fly as single steps at n, and
    the launches fly at the nearest fleet the entry point takes with the same tile shape (4, 60, 68: a ragged tile, a ragged tile, one
    tile and a ragged one).  The last fleet, 16 452 drones on 256 CUs, takes its size from the device the env reports."""
    pkg = _gpu()
    if n == SECOND_TILES:
        from drl_dronenavigation_amd import tracks
        env = pkg.DroneVecEnv(tracks.REGISTRY["reaching"](), 4, normalize_obs=True, device="cuda:0")
        n = 64 * (env.num_cus + 1) + 4
        env.close()
    if n in LAUNCH_FLEET:
        _compare(pkg, n, monkeypatch, singles=True)
        n = LAUNCH_FLEET[n]
    _compare(pkg, n, monkeypatch)


def _compare(pkg, n, monkeypatch, singles=False):
    from drl_dronenavigation_amd import tracks
    track = tracks.REGISTRY["reaching"]()
    gen = torch.Generator().manual_seed(1000 + n)
    acts = (torch.rand((max(STEPS), n, 4), generator=gen) * 2 - 1).to("cuda:0")       # seeded U(-1, 1)
    for k in STEPS:
        monkeypatch.setenv("DN_WAVES", "1")
        waves, want = _run(pkg, track, n, acts, k, singles)
        assert waves == 1
        assert len(want["state"]) > 0 and (singles or set(want) >= {"obs", "reward", "done", "truncated", "found_targets", "terminal_obs", "state", "stats"})
        monkeypatch.setenv("DN_WAVES", "5")
        for run in range(3):                # the same sequence from the same reset: the placement may differ, the bits may not
            waves, got = _run(pkg, track, n, acts, k, singles)
            assert waves == 5
            assert sorted(got) == sorted(want)
            for name in want:
                assert got[name] == want[name], (name, n, k, run)
        if k == 7 and not singles:          # max_steps = 3: episodes did end inside the launch
            assert np.frombuffer(want["done"], np.uint8).any()
    monkeypatch.delenv("DN_WAVES")
