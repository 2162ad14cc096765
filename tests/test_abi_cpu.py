"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads and exports every symbol that
include/dronenav.h declares; argument validation and the no-GPU failure are loud; the product never
imports the oracle.  No compute calls (there is no GPU here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_support as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "drl-dronenavigation_amd")


@pytest.fixture(scope="module")
def pkg():
    import drl_dronenavigation_amd as p
    p.build.build_library()
    return p


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg._capi.load()
    syms = abi.header_symbols()
    assert len(syms) >= 18
    for s in syms:
        assert hasattr(lib, s), f"libdronenav.so does not export {s}"
    assert syms == set(pkg._capi.PROTOTYPES), "ctypes prototypes and the header disagree"
    exported = abi.exported(pkg._capi.library_path())
    assert exported == syms, exported ^ syms
    abi.check_names(*syms)
    assert abi.header_arity() == {name: len(args) for name, (_, args) in pkg._capi.PROTOTYPES.items()}


def test_every_mirror_matches_the_header_field_by_field(pkg):
    """Every ctypes.Structure of _capi.py against the header struct its name derives: size, and every field's offset and size."""
    got, mirrors = abi.compiled(), abi.mirrors()
    assert len(mirrors) >= 22 and sum(len(c._fields_) for c in mirrors.values()) >= 164       # the structs and fields of ABI 10
    assert set(mirrors) == set(got.sizes) == set(got.fields)
    for cls in mirrors.values():
        abi.check_layout(cls, C.sizeof(cls))


def test_every_header_struct_has_a_mirror(pkg):
    structs = abi.header_structs()
    assert "dn_config" in structs and "dn_env" not in structs and len(structs) >= 22
    assert structs == set(abi.mirrors()), structs ^ set(abi.mirrors())


MIRRORED_CONSTANTS = {"MAX_WAYPOINTS", "MAX_TRACKS", "OBS_DIM", "ACT_DIM", "ABI_VERSION", "GROUND_CONTACT_AUTO", "MINIBATCH_MAX_FIELDS", "PPO_MAX_ACT",
                      "ADAM_MAX_TENSORS", "ADAM_ZERO_GRADS", "REPLAY_PLAIN", "REPLAY_RING", "REPLAY_MAX_OBS", "REPLAY_MAX_ACT", "SAC_MAX_ACT",
                      "SAC_MAX_CRITICS"}


def test_every_mirrored_constant_and_status_agrees(pkg):
    K, got = pkg._capi, abi.compiled()
    mirrored = {name[3:]: value for name, value in got.constants.items() if hasattr(K, name[3:])}
    assert set(mirrored) == MIRRORED_CONSTANTS, set(mirrored) ^ MIRRORED_CONSTANTS
    for name, value in mirrored.items():
        assert getattr(K, name) == value, name
    assert len(got.status) == 6 and {v: k for k, v in got.status.items()} == K.STATUS_NAMES
    abi.check_version()


def test_struct_layouts_match_header(pkg):
    K = pkg._capi
    # sizes computed by hand from include/dronenav.h (natural alignment) ...
    # ... and by the C compiler from the header itself: sizes and the offsets of the trailing fields
    abi.check_layout(K.DnConfig, 8 + 4 + 4 + 64 * 3 * 8 + 3 * 8 + 6 * 8 + 8 + 8 * 4 + 2 * 4 + 8 + 8 + 4 * 4 + 2 * 4,   # ... + random_spawn + zero_damping
                     seed=1672, random_spawn=1704)
    abi.check_layout(K.DnStats, 7 * 8)
    abi.check_layout(K.DnMlpNet, 9 * 8 + 4 * 4)
    # ABI 10 appended rms_m2 (the normaliser's second moment, verbatim) behind ep_ret_lo: every offset of ABI 9 stands, the struct grew by
    # the field alone
    abi.check_layout(K.DnEnvState, 568, rms_mean=120, pid=384, ep_ret_lo=456, rms_m2=464)
    assert 568 - 464 == 13 * 8
    abi.check_version()


def test_state_dtype_is_the_compiled_record(pkg):
    """vec_env.STATE_DTYPE, the numpy view of the state blob, against the compiled dn_env_state: names in order, offsets, item size and
    every field's size; and the element formats, which the compiler's numbers do not tell."""
    from drl_dronenavigation_amd.vec_env import STATE_DTYPE
    got = abi.compiled()
    state = got.fields["dn_env_state"]
    assert STATE_DTYPE.names == tuple(state) and STATE_DTYPE.itemsize == got.sizes["dn_env_state"] == 568
    assert {n: (STATE_DTYPE.fields[n][1], STATE_DTYPE.fields[n][0].itemsize) for n in STATE_DTYPE.names} == state
    f4 = ("pos", "quat", "vel", "ang_v", "prev_vel", "prev_ang_v", "cur_pos", "d", "d_prev", "ep_ret", "last_rpm", "ep_ret_lo")
    i4 = ("idx", "steps", "just_found", "ep_len")
    f8 = ("rms_mean", "rms_var", "rms_count", "rr_returns", "rr_mean", "rr_var", "rr_count", "pid", "rms_m2")
    assert set(f4 + i4 + f8) == set(STATE_DTYPE.names)
    for names, base in ((f4, "<f4"), (i4, "<i4"), (f8, "<f8")):
        for n in names:
            assert STATE_DTYPE.fields[n][0].base == np.dtype(base), n


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
