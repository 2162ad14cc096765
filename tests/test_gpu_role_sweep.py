"""The five-wave fused step under EVERY wave-to-role assignment.  The shipped kernel takes its roles from the SIMDs its waves land on
(csrc/dn_role_place.h); "a role only says which wave runs which function: no result depends on them" is what these tests hold.  The sweep
build of the kernel (-DDN_5W_ROLE_SWEEP on dn_kernels_mw.hip, build.build_variant; never shipped) reads its table, its fallback orders and
its priorities from a device buffer, so a child process that loads it through DN_LIB_PATH forces each of the 120 assignments a tile can
get, in first and in second tiles, whatever the machine's placement, and compares every one, bit for bit, with the one-wave kernels of
the same library; the parent ties that library's reference to the shipped one's.  tests/role_sweep_support.py holds the variant lists,
the flight and the child."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import role_sweep_support as S  # noqa: E402
from gpu_support import pkg as _gpu  # noqa: E402

FLEETS = ["N1", "N2"]       # 132 drones: two tiles and a ragged one, all first tiles | 64 (num_cus + 1) + 4: a full and a ragged second tile as well


@pytest.fixture(scope="module")
def sweep_library(tmp_path_factory):
    """The sweep build, once per file: dn_kernels_mw.hip under -DDN_5W_ROLE_SWEEP beside the default build's other objects.
    DN_ROLE_SWEEP_LIB names one built beforehand (build.build_variant(DIR, "role_sweep", ["-DDN_5W_ROLE_SWEEP"]))."""
    pkg = _gpu()
    t0 = time.perf_counter()
    path = os.environ.get("DN_ROLE_SWEEP_LIB") or pkg.build.build_variant(str(tmp_path_factory.mktemp("role_sweep")), "role_sweep", ["-DDN_5W_ROLE_SWEEP"])
    assert os.path.exists(path), path
    print(f"sweep library {path}: {time.perf_counter() - t0:.1f} s")
    return path


@pytest.fixture(scope="module")
def num_cus():
    pkg = _gpu()
    from drl_dronenavigation_amd import tracks
    env = pkg.DroneVecEnv(tracks.reaching(), 4, normalize_obs=True, device=S.DEV)
    try:
        return env.num_cus
    finally:
        env.close()


def _child(lib, tmp_path, fleet, n, family):
    """One child process on the sweep library: its report.  It exits non-zero on the first variant, launch and tensor that differs."""
    job = {"fleet": fleet, "n": n, "family": family, "report": str(tmp_path / "report.json"), "npz": str(tmp_path / "reference")}
    with open(tmp_path / "job.json", "w") as f:
        json.dump(job, f)
    env_ = dict(os.environ, DN_LIB_PATH=lib)
    for name in ("DN_EXACT_NORM", "DN_WAVES", "DN_WAVES_SINGLE", "DN_5W_ROLE_SWEEP"):
        env_.pop(name, None)
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, os.path.join(S.ROOT, "tests", "role_sweep_support.py"), str(tmp_path / "job.json")],
                         env=env_, timeout=600, capture_output=True, text=True)
    assert out.returncode == 0, f"exit status {out.returncode}: {out.stderr[-3000:]}"
    with open(job["report"]) as f:
        report = json.load(f)
    print(f"{family} at {fleet} = {n} drones: {report['variants']} variants, {report['flights']} flights of K = {S.CHAINS[fleet]}, "
          f"{report['refused']} refusals, {report['forced_tiles']} tiles seen on their forced order, {report['named_tiles']} on a row of the table for "
          f"certain; GPU work {report['seconds']} s, child {time.perf_counter() - t0:.1f} s")
    assert (report["fleet"], report["n"], report["family"], report["library"]) == (fleet, n, family, lib)
    return report


def _n(fleet, num_cus):
    return S.N1 if fleet == "N1" else S.n2(num_cus)


@pytest.mark.parametrize("fleet", FLEETS)
def test_every_forced_assignment_gives_the_bits_of_one_wave(fleet, sweep_library, num_cus, tmp_path):
    """A table that names nothing and the orders (pi, pi rotated by two places) for each of the 120 permutations pi: wave w of a first tile
    runs pi[w], of a second tile pi[(w + 2) % 5], through the device's fallback branch -- every assignment a tile can get, in both kinds
    of tile, with and without noise, launches of K = 2, 3, 7, 20 (N2: 2, 7) chained from one reset.  That each tile ran the order it was
    given is read back from the kernel (dn_debug_role_seen), not assumed."""
    n = _n(fleet, num_cus)
    report = _child(sweep_library, tmp_path, fleet, n, "forced")
    assert report["variants"] == report["flights"] == 2 * 120
    assert report["forced_tiles"] == 2 * 120 * ((n + 63) // 64), "dn_debug_role_seen: every tile of every flight ran the order it was given"


@pytest.mark.parametrize("fleet", FLEETS)
def test_every_ranked_assignment_gives_the_bits_of_one_wave(fleet, sweep_library, num_cus, tmp_path):
    """All four rows of a tile equal to pi (second tile: rotated), the shipped fallback orders: the device's dn_place_rank gives the wave
    of rank r the role pi[r] under the placements the hardware makes."""
    report = _child(sweep_library, tmp_path, fleet, _n(fleet, num_cus), "ranked")
    assert report["variants"] == report["flights"] == 2 * 120
    assert report["forced_tiles"] == 0 and report["named_tiles"] > 0, "dn_debug_role_seen: some tile ran a row of the table, not the fallback order"


@pytest.mark.parametrize("fleet", FLEETS)
def test_no_result_moves_with_a_priority(fleet, sweep_library, num_cus, tmp_path):
    """The shipped table and the forced shipped orders under the priorities 00000, 33333, the shipped 22311 and its mirror 11022.  The
    mail slots are double-buffered on barriers alone: a result that moves with a priority is a missing synchronisation."""
    report = _child(sweep_library, tmp_path, fleet, _n(fleet, num_cus), "priorities")
    assert report["variants"] == report["flights"] == 2 * 8


@pytest.mark.parametrize("fleet", FLEETS)
def test_the_sweep_value_is_parsed_or_refused_whole(fleet, sweep_library, num_cus, tmp_path):
    """Nine words (profiles/sweep_5w_roles.py: the orders default to the shipped ones) and eleven are accepted; ten or twelve words, an
    order with a repeated letter or a dash, a row that is no permutation, a priority past 3 and an empty value return 1 and leave the
    variant before them in force: the launches after the refusals still match the one-wave reference."""
    good, bad = S.parser_cases()
    report = _child(sweep_library, tmp_path, fleet, _n(fleet, num_cus), "parser")
    assert report["variants"] == 2 * len(good) and report["refused"] == 2 * len(good) * len(bad) and report["flights"] == 2 * (2 * len(good) + 1)


@pytest.mark.parametrize("fleet", FLEETS)
def test_the_sweep_library_flies_what_the_shipped_library_flies(fleet, sweep_library, num_cus, tmp_path, monkeypatch):
    """The tie to the shipped binary: this process flies libdronenav.so under DN_WAVES=1 and DN_WAVES=5; both equal, bit for bit, the
    child's one-wave reference and its five-wave flight under the shipped table, orders and priorities."""
    pkg = _gpu()
    assert pkg._capi.library_path() == pkg.build.LIB_PATH, "this test is about the shipped library"
    n, chain = _n(fleet, num_cus), S.CHAINS[fleet]
    _child(sweep_library, tmp_path, fleet, n, "reference")
    acts = S.actions(torch, n, sum(chain))
    for noise in S.NOISES:
        label = "noise" if noise else "plain"
        for waves in (1, 5):
            monkeypatch.setenv("DN_WAVES", str(waves))
            mine = S.to_host(S.fly(pkg, torch, n, chain, noise, acts))
            assert mine["waves"] == waves and mine["num_cus"] == num_cus
            for theirs_waves in (1, 5):
                theirs = np.load(str(tmp_path / "reference") + f".{label}.w{theirs_waves}.npz")
                assert int(theirs["waves"]) == theirs_waves
                assert sorted(theirs.files) == sorted(mine)
                for name in theirs.files:
                    if name != "waves":
                        assert mine[name].tobytes() == theirs[name].tobytes(), (name, label, f"shipped {waves} waves", f"sweep build {theirs_waves} waves")
    monkeypatch.delenv("DN_WAVES")
