"""The optimiser step (include/dronenav.h dn_adam_step), the part that needs no GPU: the names are declared, exported and bound; the
layouts of dn_adam_tensor and dn_adam_config, compiled from the header; the scratch-size rule; every refusal of dn_adam_step, which
validates before its first device call, so the pointers here are never followed; the refusals of ClippedAdam that need no device; and the
reference of tests/adam_support.py against an independent statement: torch's own clip_grad_norm_ + torch.optim.Adam on float64 CPU
tensors."""
import ctypes as C
import math
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import abi_support as abi  # noqa: E402
import adam_support as A  # noqa: E402

NAMES = ("dn_adam_scratch_bytes", "dn_adam_step")
INVALID = -1


@pytest.fixture(scope="module")
def pkg():
    import drl_dronenavigation_amd as p
    p.build.build_library()
    return p


def test_the_names_are_declared_exported_and_bound(pkg):
    code = abi.header_text()
    assert re.search(r"#define DN_ADAM_MAX_TENSORS 32\b", code) and re.search(r"#define DN_ADAM_CHUNK \d+\b", code)
    assert re.search(r"typedef struct dn_adam_tensor \{\s*float \*param;\s*float \*grad;\s*float \*exp_avg;\s*float \*exp_avg_sq;\s*"
                     r"int64_t count;\s*\} dn_adam_tensor;", code)
    assert re.search(r"typedef struct dn_adam_config \{\s*double beta1, beta2;\s*double eps;\s*double max_grad_norm;\s*int32_t n_tensors;\s*"
                     r"int32_t flags;\s*\} dn_adam_config;", code)
    abi.check_names(*NAMES)
    assert pkg.ClippedAdam is pkg.optim.ClippedAdam and "ClippedAdam" in pkg.__all__
    abi.check_version()
    assert "dn_adam.hip" in pkg.build.SOURCES


def test_struct_layouts_compiled_from_the_header(pkg):
    """dn_adam_tensor: 40 bytes, param 0, grad 8, exp_avg 16, exp_avg_sq 24, count 32.  dn_adam_config: 40 bytes, beta1 0, beta2 8, eps 16,
    max_grad_norm 24, n_tensors 32, flags 36 -- by the C compiler from the header itself, and the ctypes mirrors agree."""
    abi.check_layout(pkg._capi.DnAdamTensor, 40, param=0, grad=8, exp_avg=16, exp_avg_sq=24, count=32)
    abi.check_layout(pkg._capi.DnAdamConfig, 40, beta1=0, beta2=8, eps=16, max_grad_norm=24, n_tensors=32, flags=36)
    consts = abi.compiled().constants
    assert [consts["DN_ADAM_MAX_TENSORS"], consts["DN_ADAM_CHUNK"], consts["DN_ADAM_ZERO_GRADS"]] == [32, A.CHUNK, 1] and A.MAX_TENSORS == 32
    assert pkg._capi.ADAM_MAX_TENSORS == 32 and pkg._capi.ADAM_ZERO_GRADS == 1
    abi.check_version()


def _scratch_bytes(lib, counts):
    return lib.dn_adam_scratch_bytes((C.c_int64 * max(len(counts), 1))(*counts), len(counts))


def test_scratch_sizes(pkg):
    """8 bytes per chunk of DN_ADAM_CHUNK elements, the last chunk of every tensor short."""
    lib = pkg._capi.load()
    chunk = A.CHUNK
    for counts, want in (((1,), 1), ((chunk,), 1), ((chunk + 1,), 2), ((1, 1, 1), 3), (tuple(range(1, 33)), 32),
                         ((chunk * 3 + 1,) * 32, 128), (A.SMALL_NET, 17 if chunk >= 1024 else None), (A.MIXED_32, None)):
        assert _scratch_bytes(lib, counts) == 8 * A.chunks(counts), counts
        assert want is None or A.chunks(counts) == want, counts
    for counts in ((1,), (1024,), (1025,)):           # the issue's lists as it states them, whatever the header's chunk
        assert _scratch_bytes(lib, counts) == 8 * -(-counts[0] // chunk)
    assert _scratch_bytes(lib, (((1 << 31) - 1) * chunk,)) == 8 * ((1 << 31) - 1)
    assert _scratch_bytes(lib, (1,) * 33) == INVALID and b"n_tensors must be in 1..32 (got 33)" in lib.dn_last_error()
    assert _scratch_bytes(lib, ()) == INVALID and b"n_tensors must be in 1..32 (got 0)" in lib.dn_last_error()
    assert _scratch_bytes(lib, (5, 0, 5)) == INVALID and b"counts[1] must be >= 1 (got 0)" in lib.dn_last_error()
    assert _scratch_bytes(lib, (5, 5, -7)) == INVALID and b"counts[2] must be >= 1 (got -7)" in lib.dn_last_error()
    assert _scratch_bytes(lib, (((1 << 31) - 1) * chunk, 1)) == INVALID and b"at most 2^31 - 1" in lib.dn_last_error()
    assert lib.dn_adam_scratch_bytes(None, 1) == INVALID and b"counts is required" in lib.dn_last_error()


# ---- the refusals of dn_adam_step ---------------------------------------------------------------------------------------------------------
CFG = dict(beta1=0.9, beta2=0.999, eps=1e-5, max_grad_norm=0.5, n_tensors=3, flags=0)
PTRS = dict(lr=0x100000, state=0x200000, stats=0x300000, scratch=0x400000)       # dummy addresses, never followed
COUNTS = (5, 1025, 2049)                               # 1 + 2 + 3 chunks


def _tensors(n, change, counts=COUNTS):
    """n table entries at dummy addresses 16 MiB apart; change: {(index, field): value}."""
    rows = []
    for i in range(n):
        base = 0x10000000 + i * 0x1000000
        row = dict(param=base, grad=base + 0x400000, exp_avg=base + 0x800000, exp_avg_sq=base + 0xC00000, count=counts[i % len(counts)])
        rows.append(row)
    for (i, field), value in change.items():
        rows[i][field] = value
    return rows


def _call(lib, K, *, cfg=CFG, tensors="default", scratch_bytes=1 << 40, change=None, **kw):
    c = None
    if cfg is not None:
        d = dict(cfg, **{k: kw.pop(k) for k in list(kw) if k in CFG})
        c = C.byref(K.DnAdamConfig(d["beta1"], d["beta2"], d["eps"], d["max_grad_norm"], d["n_tensors"], d["flags"]))
        n = d["n_tensors"]
    else:
        n = 3
    table = None
    if tensors == "default":
        rows = _tensors(max(1, min(n, 40)), change or {})
        table = (K.DnAdamTensor * len(rows))(*[K.DnAdamTensor(r["param"], r["grad"], r["exp_avg"], r["exp_avg_sq"], r["count"]) for r in rows])
    p = dict(PTRS, **kw)
    # device 2^20 does not exist: should a case ever pass validation, hipSetDevice refuses it (DN_ERR_HIP) and no kernel sees a dummy pointer
    rc = lib.dn_adam_step(c, table, p["lr"], p["state"], p["stats"], p["scratch"], scratch_bytes, 1 << 20, None)
    return rc, lib.dn_last_error().decode()


REFUSALS = [
    ("null_cfg", dict(cfg=None), "cfg is required"),
    ("null_tensors", dict(tensors=None), "tensors is required"),
    ("null_lr", dict(lr=None), "lr is required"),
    ("null_state", dict(state=None), "state is required"),
    ("null_stats", dict(stats=None), "stats is required"),
    ("null_scratch", dict(scratch=None), "scratch is required"),
    ("n_tensors_0", dict(n_tensors=0), "n_tensors must be in 1..32 (got 0)"),
    ("n_tensors_negative", dict(n_tensors=-1), "n_tensors must be in 1..32 (got -1)"),
    ("n_tensors_33", dict(n_tensors=33), "n_tensors must be in 1..32 (got 33)"),
    ("flags_bit_1", dict(flags=2), "flags has unknown bits"),
    ("flags_bit_31", dict(flags=-(1 << 31)), "flags has unknown bits"),
    ("flags_bits_0_and_4", dict(flags=17), "flags has unknown bits"),
    ("beta1_1", dict(beta1=1.0), "beta1 must be in [0, 1)"),
    ("beta1_negative", dict(beta1=-0.1), "beta1 must be in [0, 1)"),
    ("beta1_nan", dict(beta1=math.nan), "beta1 must be in [0, 1)"),
    ("beta2_1", dict(beta2=1.0), "beta2 must be in [0, 1)"),
    ("beta2_negative", dict(beta2=-1e-9), "beta2 must be in [0, 1)"),
    ("beta2_inf", dict(beta2=math.inf), "beta2 must be in [0, 1)"),
    ("eps_negative", dict(eps=-1e-5), "eps must be finite and >= 0"),
    ("eps_nan", dict(eps=math.nan), "eps must be finite and >= 0"),
    ("eps_inf", dict(eps=math.inf), "eps must be finite and >= 0"),
    ("max_grad_norm_nan", dict(max_grad_norm=math.nan), "max_grad_norm must be finite"),
    ("max_grad_norm_inf", dict(max_grad_norm=math.inf), "max_grad_norm must be finite"),
    ("max_grad_norm_minus_inf", dict(max_grad_norm=-math.inf), "max_grad_norm must be finite"),
    ("null_param", dict(change={(0, "param"): None}), "tensors[0].param is required"),
    ("null_grad", dict(change={(1, "grad"): None}), "tensors[1].grad is required"),
    ("null_exp_avg", dict(change={(2, "exp_avg"): None}), "tensors[2].exp_avg is required"),
    ("null_exp_avg_sq", dict(change={(2, "exp_avg_sq"): None}), "tensors[2].exp_avg_sq is required"),
    ("count_0", dict(change={(1, "count"): 0}), "tensors[1].count must be >= 1 (got 0)"),
    ("count_negative", dict(change={(2, "count"): -5}), "tensors[2].count must be >= 1 (got -5)"),
    ("too_many_chunks", dict(change={(0, "count"): ((1 << 31) - 1) * A.CHUNK}), "at most 2^31 - 1"),
    ("param_misaligned", dict(change={(0, "param"): 0x10000002}), "tensors[0].param must be 4-byte aligned"),
    ("grad_misaligned", dict(change={(2, "grad"): 0x12400001}), "tensors[2].grad must be 4-byte aligned"),
    ("exp_avg_misaligned", dict(change={(1, "exp_avg"): 0x11800003}), "tensors[1].exp_avg must be 4-byte aligned"),
    ("exp_avg_sq_misaligned", dict(change={(1, "exp_avg_sq"): 0x11C00002}), "tensors[1].exp_avg_sq must be 4-byte aligned"),
    ("scratch_one_byte_short", dict(scratch_bytes=8 * A.chunks(COUNTS) - 1), "scratch_bytes is too small"),
    ("scratch_0", dict(scratch_bytes=0), "scratch_bytes is too small"),
    ("scratch_misaligned", dict(scratch=0x400004), "scratch must be 8-byte aligned"),
    ("lr_misaligned", dict(lr=0x100004), "lr must be 8-byte aligned"),
    ("state_misaligned", dict(state=0x200001), "state must be 8-byte aligned"),
    ("stats_misaligned", dict(stats=0x300004), "stats must be 8-byte aligned"),
]


@pytest.mark.parametrize("kw,message", [pytest.param(*r[1:], id=r[0]) for r in REFUSALS])
def test_dn_adam_step_refuses(pkg, kw, message):
    """Every case returns DN_ERR_INVALID_ARGUMENT with a text that names the argument, on dummy pointers: none gets as far as a device
    call."""
    K = pkg._capi
    lib = K.load()
    rc, msg = _call(lib, K, **dict(kw))
    assert rc == INVALID, msg
    assert message in msg, msg


def test_the_refusals_are_not_the_dummies_own(pkg):
    """The unchanged dummy call -- also with the flag, without a clip, with zero betas and eps, 1 and 32 tensors, the exact scratch size
    and tensors 4 bytes off a 16-byte boundary -- passes every check but one chosen here, the last one validation makes: each refusal
    above is caused by what it changes."""
    K = pkg._capi
    lib = K.load()
    for kw in [dict(), dict(flags=1), dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(beta1=0.0, beta2=0.0, eps=0.0), dict(n_tensors=1),
               dict(n_tensors=32), dict(scratch_bytes=8 * A.chunks(COUNTS)), dict(change={(0, "param"): 0x10000004, (1, "grad"): 0x1140000C})]:
        rc, msg = _call(lib, K, **dict(kw, stats=0x300004))
        assert rc == INVALID and "stats must be 8-byte aligned" in msg, (kw, msg)


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------------
def test_python_surface_refuses(pkg):
    """What needs no device: the tensors are CPU tensors, refused after every other check of theirs has passed."""
    O = pkg.ClippedAdam
    z = torch.zeros
    with pytest.raises(ValueError, match="ClippedAdam takes 1..32 tensors, got 33"):
        O([z(3) for _ in range(33)])
    with pytest.raises(ValueError, match="ClippedAdam takes 1..32 tensors, got 0"):
        O([])
    with pytest.raises(ValueError, match=r"params\[1\] must be torch.float32, got torch.float64"):
        O([z(3), z(3, dtype=torch.float64)])
    with pytest.raises(ValueError, match=r"params\[2\] must be torch.float32, got torch.bfloat16"):
        O([z(3), z(3), z(3, dtype=torch.bfloat16)])
    with pytest.raises(ValueError, match=r"params\[1\] must be dense"):
        O([z(3), z(6, 4)[:, :2]])
    with pytest.raises(ValueError, match=r"params\[0\] must be dense"):
        O([z(8)[::2]])
    with pytest.raises(ValueError, match=r"params\[1\] is empty"):
        O([z(3), z(0)])
    with pytest.raises(ValueError, match=r"params\[0\] must be a tensor"):
        O([[0.0, 1.0]])
    with pytest.raises(ValueError, match=r"params\[0\] must be a leaf"):
        O([z(3, requires_grad=True) * 2.0])
    with pytest.raises(ValueError, match=r"params\[0\] is on cpu; the parameters must be on a GPU, there is no CPU path"):
        O([z(3), z(4)])
    with pytest.raises(ValueError, match=r"params\[0\] is on cpu"):
        O(torch.nn.Linear(3, 2).parameters())
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match=r"params\[1\] is on cpu"):
            O([z(3, device="cuda"), z(4)])


def test_running_product_is_a_sequence_of_products(pkg):
    """What load_state_dict rebuilds c1 and c2 with: `step` IEEE products, not pow."""
    f = pkg.optim._running_product
    assert f(0.9, 0) == 1.0 and f(0.9, 1) == 0.9 and f(0.9, 3) == 0.9 * 0.9 * 0.9 and f(0.0, 5) == 0.0
    c = 1.0
    for _ in range(1000):
        c *= 0.999
    assert f(0.999, 1000) == c and abs(c - 0.999 ** 1000) <= 1e-13 * c
    c = 1.0
    for _ in range(100000):
        c *= 0.9
    assert f(0.9, 100000) == f(0.9, 10 ** 9) == c and c < 1e-300       # underflowed: the walk ends early at the value every later product keeps


# ---- the reference --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data_set", A.DATA_SETS)
@pytest.mark.parametrize("counts", [(5,), (1, 1024, 5, 2049), A.SMALL_NET], ids=["one", "four", "net"])
def test_reference_is_torch_in_float64(counts, data_set):
    """The reference over five steps, each fed its own unrounded results, against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam(eps=1e-5)
    on float64 CPU tensors: the clip biting ("over") and not ("under", "zero", and "noclip", where torch is not asked to clip).  Every
    element within 1e-12 of the largest magnitude of its tensor; the gap between the running products and torch's beta ** step, and
    torch's own order of the norm's sum, is what remains."""
    p0, m0, v0, grads = A.case(counts, data_set)
    mgn = A.max_grad_norm_of(data_set)
    params = [torch.nn.Parameter(torch.from_numpy(x.astype(np.float64))) for x in p0]
    opt = torch.optim.Adam(params, lr=A.LR, betas=A.BETAS, eps=A.EPS)
    if data_set != "zero":                             # start torch from the same moments: one step on zero gradients makes its state
        for q in params:
            q.grad = torch.zeros_like(q)
        opt.step()
        for q, x, m, v in zip(params, p0, m0, v0):
            q.data.copy_(torch.from_numpy(x.astype(np.float64)))
            st = opt.state[q]
            st["step"].zero_()
            st["exp_avg"].copy_(torch.from_numpy(m.astype(np.float64)))
            st["exp_avg_sq"].copy_(torch.from_numpy(v.astype(np.float64)))
    p, m, v, state = p0, m0, v0, A.STATE0
    worst = 0.0
    for k, g in enumerate(grads):
        for q, x in zip(params, g):
            q.grad = torch.from_numpy(x.astype(np.float64))
        norm = float(torch.nn.utils.clip_grad_norm_(params, mgn)) if mgn > 0.0 else None
        opt.step()
        p, m, v, state, stats = A.reference(p, g, m, v, A.LR, state, max_grad_norm=mgn)
        assert state[0] == k + 1 and stats[3] == k + 1
        if norm is not None:
            assert abs(stats[0] - norm) <= 1e-12 * norm
        assert (stats[1] < 0.5) == (data_set == "over") and (data_set == "over" or stats[1] == 1.0), (data_set, stats)
        for q, a, b, c in zip(params, p, m, v):
            st = opt.state[q]
            for name, mine, theirs in (("p", a, q.detach().numpy()), ("m", b, st["exp_avg"].numpy()), ("v", c, st["exp_avg_sq"].numpy())):
                top = float(np.abs(theirs).max())
                d = float(np.abs(mine - theirs).max()) / top if top > 0.0 else float(np.abs(mine).max())
                assert d <= 1e-12, (counts, data_set, k, name, d)
                worst = max(worst, d)
    if data_set == "zero":
        assert all(np.array_equal(a, b.astype(np.float64)) for a, b in zip(p, p0)), "zero gradients from zero moments move nothing"
    print(f"{len(counts)} tensors, {data_set}: the reference from torch float64 over {A.STEPS} steps, of the largest of a tensor: {worst:.2e}")


def test_reference_edge_values():
    """One NaN gradient: total and coef NaN, every parameter NaN.  Without a clip it stays in its own element."""
    p, m, v, grads = A.case((5, 1025), "over")
    g = [x.copy() for x in grads[0]]
    g[1][77] = np.nan
    out = A.reference(p, g, m, v, A.LR, A.STATE0)
    assert math.isnan(out[4][0]) and math.isnan(out[4][1]) and all(np.isnan(x).all() for x in out[0])
    out = A.reference(p, g, m, v, A.LR, A.STATE0, max_grad_norm=0.0)
    assert math.isnan(out[4][0]) and out[4][1] == 1.0 and int(sum(np.isnan(x).sum() for x in out[0])) == 1
