"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads and exports every symbol that
include/dronenav.h declares; argument validation and the no-GPU failure are loud; the product never
imports the oracle.  No compute calls (there is no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "drl-dronenavigation_amd")


@pytest.fixture(scope="module")
def pkg():
    import drl_dronenavigation_amd as p
    p.build.build_library()
    return p


def header_symbols():
    src = open(os.path.join(ROOT, "include", "dronenav.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dn_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg._capi.load()
    syms = header_symbols()
    assert len(syms) >= 18
    for s in syms:
        assert hasattr(lib, s), f"libdronenav.so does not export {s}"
    assert set(syms) == set(pkg._capi.PROTOTYPES), "ctypes prototypes and the header disagree"
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._capi.library_path()], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (dn_[a-z_0-9]+)", out))
    assert exported == set(syms), exported ^ set(syms)


def test_struct_layouts_match_header(pkg):
    # sizes computed by hand from include/dronenav.h (natural alignment) ...
    assert C.sizeof(pkg._capi.DnConfig) == 8 + 4 + 4 + 64 * 3 * 8 + 3 * 8 + 6 * 8 + 8 + 8 * 4 + 2 * 4 + 8 + 8 + 4 * 4 + 2 * 4   # ... + random_spawn + zero_damping
    assert C.sizeof(pkg._capi.DnStats) == 7 * 8
    # ... and by the C compiler from the header itself: sizes and the offsets of the trailing fields
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "dronenav.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(dn_config), sizeof(dn_env_state), sizeof(dn_stats), sizeof(dn_mlp_net),
           offsetof(dn_config, random_spawn), offsetof(dn_config, seed), offsetof(dn_env_state, pid),
           offsetof(dn_env_state, rms_mean), offsetof(dn_env_state, ep_ret_lo), offsetof(dn_env_state, rms_m2), DN_ABI_VERSION);
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "abi.c"), os.path.join(td, "abi")
        with open(src, "w") as f:
            f.write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    K = pkg._capi
    assert got == [C.sizeof(K.DnConfig), C.sizeof(K.DnEnvState), C.sizeof(K.DnStats), C.sizeof(K.DnMlpNet),
                   K.DnConfig.random_spawn.offset, K.DnConfig.seed.offset, K.DnEnvState.pid.offset,
                   K.DnEnvState.rms_mean.offset, K.DnEnvState.ep_ret_lo.offset, K.DnEnvState.rms_m2.offset, K.ABI_VERSION], got
    # ABI 10 appended rms_m2 (the normaliser's second moment, verbatim) behind ep_ret_lo: every offset of ABI 9 stands, the struct grew by
    # the field alone, and the numpy view of the blob (vec_env.STATE_DTYPE) places every field where ctypes does
    assert (got[1], got[8], got[9]) == (568, 456, 464) and got[1] - got[9] == 13 * 8, got
    from drl_dronenavigation_amd.vec_env import STATE_DTYPE
    assert STATE_DTYPE.itemsize == got[1] and STATE_DTYPE.names == tuple(f[0] for f in K.DnEnvState._fields_)
    assert all(STATE_DTYPE.fields[name][1] == getattr(K.DnEnvState, name).offset for name in STATE_DTYPE.names)
    assert pkg._capi.load().dn_abi_version() == pkg._capi.ABI_VERSION == 10


def test_config_defaults_follow_the_driver(pkg):
    cfg = pkg._capi.DnConfig()
    pkg._capi.load().dn_config_default(C.byref(cfg))
    assert cfg.threshold == 0.3 and cfg.max_steps == 4096 and cfg.cylinder == 1
    assert cfg.include_distance == 1 and cfg.normalize_actions == 1 and cfg.compute_f32 == 0
    assert cfg.act_noise_sigma == 0 and cfg.obs_noise_sigma == 0
    assert cfg.ground_contact == pkg._capi.GROUND_CONTACT_AUTO == 2


def test_ground_contact_auto_is_on_wherever_the_term_can_fire(pkg):
    """The reference always tests len(p.getContactPoints()) > 0 (PBDroneEnv.py:699).  DN_GROUND_CONTACT_AUTO keeps the
    (approximated) term unless the corridor test provably fires first: off for the circle tracks at z = 1 and the 8-gate
    race track (BASELINE's configs), ON for the registry tracks that spawn at z = 0.1 with the floor inside the 0.3 + 0.2
    corridor, and on whenever the corridor test is off."""
    lib = pkg._capi.load()
    from drl_dronenavigation_amd import tracks
    from drl_dronenavigation_amd.vec_env import make_config

    def resolved(t, **kw):
        cfg = make_config(num_envs=8, target_points=t.targets(), initial_xyzs=t.initial_xyzs, aviary_dim=t.aviary_dim,
                          circle=t.is_circle, **kw)
        return lib.dn_resolve_ground_contact(C.byref(cfg))

    for name in ("circle4", "circle6", "reaching"):
        assert resolved(tracks.REGISTRY[name]()) == 0, name
    for name in ("up", "half_up_forward", "up_circle", "up_sharp_back_turn"):
        assert resolved(tracks.REGISTRY[name]()) == 1, name
    # random_spawn: segment 0 starts at a drawn point up to 0.1 below the lowest waypoint, which the fixed-spawn bound does not cover
    assert resolved(tracks.reaching(), random_spawn=True) == 1
    assert resolved(tracks.reaching(), cylinder=False) == 1             # no corridor: nothing else keeps a drone off the floor
    assert resolved(tracks.circle(1, 4, 1), threshold=0.95) == 1        # a torus fat enough to reach the floor
    assert resolved(tracks.reaching(), ground_contact=True) == 1 and resolved(tracks.up(), ground_contact=False) == 0
    # geometry check of the bound itself: the lowest point of the race track's corridor
    t = tracks.reaching()
    pts = np.vstack([t.initial_xyzs.reshape(1, 3), t.targets()])
    lows = []
    for a, b in zip(pts[:-1], pts[1:]):
        ll = np.linalg.norm(b - a)
        if ll == 0:
            lows.append(a[2] - 0.3)
            continue
        uz = (b - a)[2] / ll
        lows.append(min(a[2] - 0.2 * uz, b[2] + 0.2 * uz) - 0.5)
    assert min(lows) > 0.02 + np.hypot(0.0125, 0.06)                    # margin + the collision cylinder's largest extent below its centre
    cfg = make_config(num_envs=8, target_points=t.targets(), initial_xyzs=t.initial_xyzs, aviary_dim=t.aviary_dim)
    cfg.ground_contact = 3
    assert lib.dn_resolve_ground_contact(C.byref(cfg)) == -1


def test_stream_copy_refuses_what_it_cannot_copy(pkg):
    """dn_stream_copy (the hand-written copy ceiling of bench.py) validates before it touches the device."""
    lib = pkg._capi.load()
    assert lib.dn_stream_copy(None, None, 1024, 0, None) == -1
    assert lib.dn_stream_copy(C.c_void_p(4096), C.c_void_p(8192), 1000, 0, None) == -1      # not a multiple of 16
    assert lib.dn_stream_copy(C.c_void_p(4100), C.c_void_p(8192), 1024, 0, None) == -1      # misaligned
    assert b"16" in lib.dn_last_error()


def test_sparse_info_dicts_answer_the_reference_callbacks():
    """info_mode="sparse" leaves the dicts of running drones unwritten; they must still read like SubprocVecEnv's:
    FoundTargetsCallback does infos[0]["found_targets"] unconditionally (Sol/Utilities/Callbacks.py:59), SB3 does
    info.get("TimeLimit.truncated", False) and info.get("episode")."""
    from drl_dronenavigation_amd.vec_env import _SparseInfo

    class FakeEnv:
        _h_found = np.array([3, 0, 7], np.int32)

    env = FakeEnv()
    infos = [_SparseInfo(env, i) for i in range(3)]
    assert [i["found_targets"] for i in infos] == [3, 0, 7]
    assert infos[0]["TimeLimit.truncated"] is False and infos[1].get("TimeLimit.truncated", True) is False
    assert infos[2].get("episode") is None and "episode" not in infos[2] and "found_targets" in infos[2]
    with pytest.raises(KeyError):
        infos[0]["terminal_observation"]
    infos[1]["episode"] = {"r": 1.0, "l": 2, "t": 0.0}
    infos[1]["TimeLimit.truncated"] = True
    assert infos[1]["TimeLimit.truncated"] is True and set(infos[1].keys()) == {"episode", "TimeLimit.truncated", "found_targets"}
    assert dict(infos[1])["found_targets"] == 0 and len(infos[1]) == 3
    env._h_found[1] = 5                                                  # the next step's host mirror
    infos[1].clear()
    assert infos[1]["found_targets"] == 5 and infos[1]["TimeLimit.truncated"] is False


def test_create_fails_loudly(pkg):
    """Invalid arguments are rejected before any device work; with valid arguments and no GPU the library
    reports DN_ERR_NO_DEVICE instead of falling back to a CPU path."""
    lib = pkg._capi.load()
    from drl_dronenavigation_amd import tracks
    from drl_dronenavigation_amd.vec_env import make_config
    t = tracks.circle(1, 4, 1)
    h = C.c_void_p()
    for bad in (dict(num_envs=0), dict(max_steps=1 << 24), dict(threshold=-1.0), dict(act_noise_sigma=-1.0)):
        kw = dict(num_envs=8, target_points=t.targets(), initial_xyzs=t.initial_xyzs, aviary_dim=t.aviary_dim)
        kw.update(bad)
        rc = lib.dn_create(C.byref(make_config(**kw)), C.byref(h))
        assert rc == -1 and not h.value, bad
        assert lib.dn_last_error()
    cfg = make_config(num_envs=8, target_points=t.targets(), initial_xyzs=t.initial_xyzs, aviary_dim=t.aviary_dim)
    cfg.num_waypoints = 65
    assert lib.dn_create(C.byref(cfg), C.byref(h)) == -1
    if lib.dn_device_count() == 0:
        cfg.num_waypoints = 4
        rc = lib.dn_create(C.byref(cfg), C.byref(h))
        assert rc == -4 and b"no CPU fallback" in lib.dn_last_error()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pkg.DroneVecEnv(t, 8)
    assert lib.dn_step(None, *([None] * 11)) == -1
    assert lib.dn_destroy(None) == 0


def test_state_bytes_capacity_planning(pkg):
    lib = pkg._capi.load()
    n = 32768
    b = lib.dn_state_bytes(n, 0)
    assert 7 * 16 * n <= b <= 7 * 16 * n + 64 * 1024
    assert lib.dn_state_bytes(n, 1) - b >= 27 * 8 * n
    # 288 GB of HBM3E holds > 10^9 drones' state
    assert lib.dn_state_bytes(1 << 30, 0) < 288e9


def test_tracks_match_reference_generators(pkg, golden):
    from drl_dronenavigation_amd import tracks
    g = golden("tracks")
    for n in ["circle4", "circle6", "reaching", "up", "half_up_forward", "up_circle", "up_sharp_back_turn"]:
        t = tracks.REGISTRY[n]()
        assert np.array_equal(t.waypoints, g[n + "_waypoints"]), n
        assert np.array_equal(t.initial_xyzs.ravel(), g[n + "_spawn"]), n
        assert np.array_equal(t.aviary_dim, g[n + "_dim"]), n
    assert len(tracks.circle(1, 4, 1).targets()) == 4          # circle tracks drop their first point
    assert len(tracks.dilate_targets(tracks.reaching().waypoints, 2)) == 7 * 3 + 1


def test_product_never_touches_the_oracle():
    """The oracle is test infrastructure: nothing under the package, include/ or the import shim may
    import, load or link it."""
    offenders = []
    files = [os.path.join(ROOT, "drl_dronenavigation_amd.py")]
    for base in (PKG, os.path.join(ROOT, "include")):
        for d, _, fs in os.walk(base):
            files += [os.path.join(d, f) for f in fs if f.endswith((".py", ".h", ".hip", ".cpp"))]
    for f in files:
        txt = open(f).read()
        if re.search(r"\boracle\b|liboracle|dn_oracle|orc_", txt):
            offenders.append(f)
    assert not offenders, offenders
