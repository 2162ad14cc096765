"""bench.py's contract beside its headline number: a plain run carries no `--full` legs, reports the K timed steps it was given and
`ms_per_step`, and `--dump-outputs DIR` writes what the last timed step returned -- bit for bit the same arrays on every run with the
same arguments, and the arrays the library returns for the bench's seeded action stream.  The dump helper itself is tested on the CPU."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = {"single_step", "hover_band", "normalize_obs_off", "normalize_obs_on", "hbm_bound_fleet_norm", "hbm_bound_fleet",
             "hbm_copy_ceiling", "other_launch_shapes", "fleet_sweep", "ppo_rollout", "sac_collect", "cpu_baseline", "ppo_rollout_sharded"}


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_output_tests", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample_past_the_cap(tmp_path):
    b = _bench()
    n = 1000
    rng = np.random.default_rng(3)
    arrays = {"obs": rng.standard_normal((n, 13)).astype(np.float32), "reward": rng.standard_normal(n),
              "done": rng.integers(0, 2, n).astype(np.uint8), "found_targets": rng.integers(0, 9, n).astype(np.int32)}
    assert b.dump_outputs(str(tmp_path / "all"), arrays) == sorted(arrays)
    for k, a in arrays.items():
        got = np.load(tmp_path / "all" / f"{k}.npy")
        assert got.dtype in (np.float32, np.float64) and np.array_equal(got, a), k
    cap = 20000                                   # 1000 rows x (52 + 8 + 1 + 4 bytes) do not fit: a sample does
    for d in ("s1", "s2"):
        assert b.dump_outputs(str(tmp_path / d), arrays, max_bytes=cap) == sorted(list(arrays) + ["drone_index"])
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= cap
    idx = np.load(tmp_path / "s1" / "drone_index.npy")
    assert idx.dtype == np.float64 and 100 < len(idx) < n and np.all(np.diff(idx) > 0)
    for k, a in arrays.items():
        got = np.load(tmp_path / "s1" / f"{k}.npy")
        assert np.array_equal(got, a[idx.astype(np.int64)]) and np.array_equal(got, np.load(tmp_path / "s2" / f"{k}.npy")), k


def _run_bench(args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_timed_step_reproducibly(tmp_path):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: the HIP path has no CPU fallback")
    n, K, W, A = 4096, 100, 7, 64                 # K > A and not a multiple of it: the last launch is a partial one
    lines = [_run_bench(["--num-envs", str(n), "--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path / f"run{i}")])
             for i in range(2)]
    pre = lines[0]["config"]["preroll"]["vector_steps"]
    for line in lines:
        assert line["metric"] == "env_steps_per_sec" and line["steps"] == K and line["warmup"] == W and line["ms_per_step"] > 0
        assert abs(line["value"] * line["ms_per_step"] * 1e-3 / n - 1) < 0.05       # value = n K / wall, ms_per_step = wall / K
        assert not FULL_ONLY & set(line), FULL_ONLY & set(line)
        assert line["config"]["preroll"]["vector_steps"] == pre > 0
    names = ["done", "found_targets", "obs", "reward", "truncated"]
    assert sorted(os.listdir(tmp_path / "run0")) == [k + ".npy" for k in names]
    dumped = {k: np.load(tmp_path / "run0" / f"{k}.npy") for k in names}
    for k in names:
        assert dumped[k].dtype == np.float32 and len(dumped[k]) == n, k
        assert np.array_equal(dumped[k].view(np.uint32), np.load(tmp_path / "run1" / f"{k}.npy").view(np.uint32)), k

    # the same stream through the library: seeded actions, reset, pre-roll, warm-up, timed steps, in launches of at most A steps
    import drl_dronenavigation_amd as pkg
    from drl_dronenavigation_amd import tracks
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(1)
    acts = (torch.rand((A, n, 4), generator=g, dtype=torch.float32) * 2 - 1).to(dev)
    env = pkg.DroneVecEnv(tracks.REGISTRY["reaching"](), n, max_steps=4096, normalize_obs=True, compute_dtype="float64", device=dev)
    env.reset_tensor()
    for phase in (pre, W, K):
        done = 0
        while done < phase:
            c = min(A, phase - done)
            out = env.rollout_tensor(acts[:c])
            done += c
    torch.cuda.synchronize(dev)
    ref = {"obs": out["obs"][c - 1], "reward": out["reward"][c - 1], "done": out["done"][c - 1], "truncated": out["truncated"][c - 1],
           "found_targets": out["found_targets"][c - 1]}
    env.close()
    assert 0 < float(dumped["done"].sum()) < n                 # U(-1,1) actions: episodes end every step, never all at once
    for k in names:
        assert np.array_equal(dumped[k], ref[k].cpu().numpy().astype(np.float32)), k
