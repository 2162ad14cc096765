"""The policy kernels' wide inputs (17 .. 64 columns), the part that needs no GPU: the packed layout of layer 1, the refusals of the
packers and of the C ABI (dn_mlp_forward validates before its first device call), and dn_mlp_ks1 as a stand-alone host program."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mlp_support as S  # noqa: E402
import host_program_support  # noqa: E402


@pytest.fixture(scope="module")
def pkg():
    import drl_dronenavigation_amd as p
    p.build.build_library()
    return p


@pytest.mark.parametrize("grade", S.GRADES)
@pytest.mark.parametrize("in_f", [1, 7, 8, 9, 13, 15, 16, 17, 21, 32, 33, 52, 64])
def test_layer1_fragments_unpack_to_the_weights(pkg, in_f, grade):
    """pack_layer(first=True) read back with the stated rule (mlp_support.unpack_first) gives W: every column where its K-step, lane
    group and slot say, zeros in the padding; in the float32 grade hi + lo gives W to the precision of the bf16 split.  Up to 16 inputs
    the tensor is, byte for byte, the one-K-step layout these kernels always read.  (While layer 1 was one K-step for every width, this
    failed from in_f = 17 on: the columns 16 and up were dropped.)"""
    from drl_dronenavigation_amd import policy_mfma as pm
    rng = np.random.default_rng(100 * in_f)
    w = rng.uniform(-1.0, 1.0, (512, in_f)).astype(np.float32)
    b = rng.uniform(-1.0, 1.0, 512).astype(np.float32)
    packed, bias = pm.pack_layer(torch.from_numpy(w), torch.from_numpy(b), True, scale=pm.TANH_PRESCALE, grade=grade)
    ks1 = S.ksteps(in_f)
    assert tuple(packed.shape) == ((16, 2, ks1, 64, 8) if grade == "fp32" else (16, ks1, 64, 8))
    ws = (w * np.float32(pm.TANH_PRESCALE)).astype(np.float32)
    assert np.array_equal(bias.numpy(), (b * np.float32(pm.TANH_PRESCALE)).astype(np.float32))
    got = S.unpack_first(packed, grade)
    if grade == "fp32":
        hi, lo = got
        assert np.array_equal(hi[:, :in_f], torch.from_numpy(ws).to(torch.bfloat16).float().numpy())
        assert not hi[:, in_f:].any() and not lo[:, in_f:].any()
        # bf16 keeps 8 significant bits, half an ulp is <= 2^-8 of the value: hi = bf16(w) has |w - hi| <= 2^-8 |w|, and
        # lo = bf16(w - hi) has |w - hi - lo| <= 2^-8 |w - hi| <= 2^-16 |w|
        assert (np.abs(hi[:, :in_f].astype(np.float64) + lo[:, :in_f] - ws) <= 2.0 ** -16 * np.abs(ws)).all()
    else:
        dt = torch.float16 if grade == "fp16" else torch.bfloat16
        assert np.array_equal(got[:, :in_f], torch.from_numpy(ws).to(dt).float().numpy())
        assert not got[:, in_f:].any()
    if in_f <= 16:
        want = S.parent_pack_first(w, pm.TANH_PRESCALE, grade)
        assert packed.dtype == want.dtype and packed.shape == want.shape
        assert packed.contiguous().view(torch.uint8).numpy().tobytes() == want.contiguous().view(torch.uint8).numpy().tobytes()


def test_packers_refuse_what_the_kernels_do_not_take(pkg):
    from drl_dronenavigation_amd import policy_mfma as pm
    with pytest.raises(ValueError, match="1..64"):
        pm.pack_mlp(S.random_layers(65, 1, 0), "cpu")
    assert pm.pack_mlp(S.random_layers(64, 1, 0), "cpu")["w1"].shape == (16, 4, 64, 8)
    z = torch.zeros
    sac = lambda in_f: [(z(256, in_f), z(256)), (z(256, 256), z(256)), (z(4, 256), z(4)), (z(4, 256), z(4))]      # noqa: E731
    with pytest.raises(ValueError, match="1..16"):
        pm.pack_sac_actor(sac(17), "cpu")
    assert pm.pack_sac_actor(sac(16), "cpu")["w1"].shape == (8, 1, 64, 8)


def test_exports(pkg):
    for name in ("FusedMlpPolicy", "FusedMlpValue", "MlpValue"):
        assert name in pkg.__all__ and getattr(pkg, name) is not None
    v = pkg.MlpValue(52)
    assert v(torch.zeros(3, 52)).shape == (3,) and v.vf[0].in_features == 52 and v.value_net.out_features == 1


def _dummy_nets(pkg, arch):
    """Two dn_mlp_net whose pointers are non-null, 16-byte aligned and never followed: validation returns before any device call."""
    K = pkg._capi
    arr = (K.DnMlpNet * 2)()
    for n in arr:
        for f in ("w1", "w2", "w3", "wh", "b1", "b2", "b3", "bh", "out"):
            setattr(n, f, 0x1000)
        n.out_dim, n.grade, n.arch = 4, 0, arch
    return arr


def test_dn_mlp_forward_validates_obs_dim_by_arch(pkg):
    K = pkg._capi
    lib = K.load()
    call = lambda arch, d: lib.dn_mlp_forward(C.cast(_dummy_nets(pkg, arch), C.c_void_p), 2, 0x1000, None, 64, d, 0, None)      # noqa: E731
    for arch, bad, rng in ((0, 65, "1..64"), (0, 0, "1..64"), (0, -3, "1..64"), (1, 17, "1..16"), (1, 64, "1..16"), (1, 0, "1..16")):
        assert call(arch, bad) == -1, (arch, bad)                               # DN_ERR_INVALID_ARGUMENT
        msg = lib.dn_last_error().decode()
        assert "obs_dim must be in " + rng in msg, msg


def test_dn_mlp_step_sampled_keeps_its_sixteen_columns(pkg):
    K = pkg._capi
    lib = K.load()
    env = C.create_string_buffer(1 << 20)         # stands in for the opaque env: the call returns at the obs_dim check, before it reads it
    p = C.c_void_p(0x1000)
    log_std = (C.c_float * 4)()
    for d in (17, 21, 64, 0):
        rc = lib.dn_mlp_step_sampled(C.cast(env, C.c_void_p), C.cast(_dummy_nets(pkg, 0), C.c_void_p), 2, p, d, log_std, 0, 0,
                                     *([p] * 12))
        assert rc == -1, d
        assert "obs_dim must be in 1..16" in lib.dn_last_error().decode()


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_ks1_of_every_width(tmp_path, sanitize):
    """tests/tools/check_mlp_ks1.cpp walks obs_dim = -1 .. 70; built with the host compiler against the HIP headers, once plainly and once
    under the address and undefined-behaviour sanitizers, and run as its own process."""
    exe = host_program_support.build("check_mlp_ks1", tmp_path, sanitize=sanitize, hip_headers=True)
    if exe is None:
        pytest.skip("the HIP headers are not installed")
    assert host_program_support.run(exe) == {"cases": 72, "bad": 0}
