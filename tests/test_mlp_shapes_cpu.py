"""The policy kernels' shapes, the part that needs no GPU: the packed layout of the hidden layers and of heads of 1 .. 32 rows, read back
by a rule stated independently of the packer (mlp_support.unpack_hidden), and every refusal of dn_mlp_forward other than obs_dim's
(tests/test_mlp_wide_cpu.py has those): the call validates before its first device call, so the pointers here are never followed."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mlp_support as S  # noqa: E402
from test_mlp_wide_cpu import _dummy_nets  # noqa: E402


@pytest.fixture(scope="module")
def pkg():
    import drl_dronenavigation_amd as p
    p.build.build_library()
    return p


def _check_unpacked(pm, w, b, scale, grade):
    out_f, in_f = w.shape
    packed, bias = pm.pack_layer(torch.from_numpy(w), torch.from_numpy(b), False, scale=scale, grade=grade)
    mt = (out_f + 31) // 32
    assert tuple(packed.shape) == ((mt, 2, in_f // 16, 64, 8) if grade == "fp32" else (mt, in_f // 16, 64, 8))
    ws, bs = (w * np.float32(scale)).astype(np.float32), (b * np.float32(scale)).astype(np.float32)
    assert bias.shape == (32 * mt,) and np.array_equal(bias.numpy()[:out_f], bs) and not bias.numpy()[out_f:].any()
    got = S.unpack_hidden(packed, grade)
    if grade == "fp32":
        hi, lo = got
        assert hi.shape == (32 * mt, in_f)
        assert np.array_equal(hi[:out_f], torch.from_numpy(ws).to(torch.bfloat16).float().numpy())
        assert not hi[out_f:].any() and not lo[out_f:].any()
        # hi = bf16(w): |w - hi| <= 2^-8 |w|; lo = bf16(w - hi): |w - hi - lo| <= 2^-8 |w - hi| <= 2^-16 |w|
        assert (np.abs(hi[:out_f].astype(np.float64) + lo[:out_f] - ws) <= 2.0 ** -16 * np.abs(ws)).all()
    else:
        dt = torch.float16 if grade == "fp16" else torch.bfloat16
        assert got.shape == (32 * mt, in_f)
        assert np.array_equal(got[:out_f], torch.from_numpy(ws).to(dt).float().numpy())
        assert not got[out_f:].any()


@pytest.mark.parametrize("grade", S.GRADES)
@pytest.mark.parametrize("out_f", [1, 2, 5, 17, 32])
def test_head_fragments_unpack_to_the_weights(pkg, out_f, grade):
    """A head of out_f rows on 256 inputs: every weight where its K-step, lane group and slot say, the rows at and beyond out_f zero, and a
    bias of 32 entries (the kernels read all 32) that is zero from out_f on."""
    from drl_dronenavigation_amd import policy_mfma as pm
    rng = np.random.default_rng(7 * out_f)
    w = rng.uniform(-1.0, 1.0, (out_f, 256)).astype(np.float32)
    b = rng.uniform(0.5, 1.0, out_f).astype(np.float32)
    _check_unpacked(pm, w, b, 1.0, grade)                   # one M-tile: the bias it checks has 32 entries


@pytest.mark.parametrize("grade", S.GRADES)
def test_hidden_fragments_unpack_to_the_weights(pkg, grade):
    from drl_dronenavigation_amd import policy_mfma as pm
    rng = np.random.default_rng(512)
    w = rng.uniform(-1.0, 1.0, (512, 512)).astype(np.float32)
    b = rng.uniform(-1.0, 1.0, 512).astype(np.float32)
    _check_unpacked(pm, w, b, pm.TANH_PRESCALE, grade)


def _forward(lib, nets, num_nets=2, obs=0x1000, num_envs=64, obs_dim=13):
    rc = lib.dn_mlp_forward(C.cast(nets, C.c_void_p) if nets is not None else None, num_nets, obs, None, num_envs, obs_dim, 0, None)
    return rc, lib.dn_last_error().decode()


def _set(nets, k, **fields):
    for f, v in fields.items():
        setattr(nets[k], f, v)
    return nets


REQUIRED, ALIGNED = "every weight, bias and output pointer is required", "packed weights must be 16-byte aligned"

REFUSALS = [                                             # (id, arch of the dummies, what to change, keywords of the call, the message)
    ("out_dim_0", 0, lambda a: _set(a, 0, out_dim=0), {}, "net 0: out_dim must be in 1..32"),
    ("out_dim_33", 0, lambda a: _set(a, 1, out_dim=33), {}, "net 1: out_dim must be in 1..32"),
    ("grade_minus_1", 0, lambda a: _set(a, 0, grade=-1), {}, "net 0: grade must be 0 (bf16), 1 (fp32 grade) or 2 (fp16)"),
    ("grade_3", 0, lambda a: _set(a, 1, grade=3), {}, "net 1: grade must be 0 (bf16), 1 (fp32 grade) or 2 (fp16)"),
    ("two_grades", 0, lambda a: _set(a, 1, grade=2), {}, "all networks of one call must share grade and arch"),
    ("two_archs", 0, lambda a: _set(a, 1, arch=1), {}, "all networks of one call must share grade and arch"),
    ("arch_2", 0, lambda a: _set(a, 0, arch=2), {}, "net 0: arch must be 0"),
    ("w2_misaligned", 0, lambda a: _set(a, 1, w2=0x1008), {}, "net 1: " + ALIGNED),
    ("w2_misaligned_by_4", 1, lambda a: _set(a, 0, w2=0x1004), {}, "net 0: " + ALIGNED),
    ("num_nets_0", 0, lambda a: a, dict(num_nets=0), "num_nets must be 1 or 2 (got 0)"),
    ("num_nets_3", 0, lambda a: a, dict(num_nets=3), "num_nets must be 1 or 2 (got 3)"),
    ("num_envs_0", 0, lambda a: a, dict(num_envs=0), "num_envs must be >= 1"),
    ("null_bh", 0, lambda a: _set(a, 1, bh=None), {}, "net 1: " + REQUIRED),
    ("null_out", 1, lambda a: _set(a, 0, out=None), {}, "net 0: " + REQUIRED),
    ("null_obs", 0, lambda a: a, dict(obs=None), "nets and obs are required"),
    # the PPO networks have a third layer, the SAC actor does not: without w3 / b3 the first is refused for the pointer, the second passes
    # the pointer check and is refused only by what validation looks at AFTER it (here: a misaligned wh)
    ("ppo_needs_w3", 0, lambda a: _set(a, 0, w3=None, b3=None, wh=0x1008), {}, "net 0: " + REQUIRED),
    ("sac_takes_no_w3", 1, lambda a: _set(a, 0, w3=None, b3=None, wh=0x1008), {}, "net 0: " + ALIGNED),
    ("sac_takes_no_w3_second_net", 1, lambda a: _set(_set(a, 0, w3=None, b3=None), 1, w3=None, b3=None, out_dim=33), {},
     "net 1: out_dim must be in 1..32"),
]


@pytest.mark.parametrize("arch,change,kw,message", [pytest.param(*r[1:], id=r[0]) for r in REFUSALS])
def test_dn_mlp_forward_refuses(pkg, arch, change, kw, message):
    """Every case returns DN_ERR_INVALID_ARGUMENT with its own message: none gets as far as a device call."""
    lib = pkg._capi.load()
    rc, msg = _forward(lib, change(_dummy_nets(pkg, arch)), **kw)
    assert rc == -1, msg
    assert message in msg, msg


def test_dn_mlp_forward_refuses_null_nets(pkg):
    rc, msg = _forward(pkg._capi.load(), None)
    assert rc == -1 and "nets and obs are required" in msg, msg


def test_the_refusals_are_not_the_dummies_own(pkg):
    """The unchanged dummies pass every check of a PPO pair but one chosen here, the last one validation makes: each refusal above is caused
    by the field it changes."""
    lib = pkg._capi.load()
    for arch in (0, 1):
        rc, msg = _forward(lib, _set(_dummy_nets(pkg, arch), 1, wh=0x1008))
        assert rc == -1 and "net 1: " + ALIGNED in msg, msg
