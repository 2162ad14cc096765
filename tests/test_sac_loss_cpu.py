"""The SAC loss heads (include/dronenav.h dn_sac_policy, dn_sac_policy_backward, dn_sac_critic_loss, dn_sac_actor_loss), the part that needs
no GPU: the five entry points are declared, exported and bound; the layout of dn_sac_config, compiled from the header; the scratch-size
rule; every refusal of the four calls, which validate before their first device call, so the pointers here are never followed; the
refusals of the Python classes; csrc/dn_sac_math.h as a stand-alone host program, plainly and under the address and undefined-behaviour
sanitizers, with sech^2 and tanh held to 40-digit arithmetic; the header's composition against policy.SacActor.squash in float64 where the
literal form is well conditioned; and the reference of tests/sac_loss_support.py -- the float64 torch composition with autograd -- against
the closed forms of the header restated in NumPy, its coverage of every branch, and its stability under the order of the rows.

Largest seen: sech^2 and tanh 3.1 and 1.6 float64 ulp from 40-digit arithmetic; closed forms from autograd 9e-3 of the bound; the header's
composition from SacActor.squash 0.13 of the bound (8.9e-12)."""
import ctypes as C
import decimal
import math
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import abi_support as abi  # noqa: E402
import host_program_support  # noqa: E402
import sac_loss_support as S  # noqa: E402

NAMES = ("dn_sac_loss_scratch_bytes", "dn_sac_policy", "dn_sac_policy_backward", "dn_sac_critic_loss", "dn_sac_actor_loss")
INVALID = -1


@pytest.fixture(scope="module")
def pkg():
    import drl_dronenavigation_amd as p
    p.build.build_library()
    return p


def test_the_names_are_declared_exported_and_bound(pkg):
    code = abi.header_text()
    assert re.search(r"#define DN_SAC_MAX_ACT 8\b", code) and re.search(r"#define DN_SAC_MAX_CRITICS 4\b", code)
    assert re.search(r"typedef struct dn_sac_config \{\s*double gamma;\s*double target_entropy;\s*double ent_coef;\s*double log_std_min;\s*"
                     r"double log_std_max;\s*int32_t act_dim;\s*int32_t n_critics;\s*int64_t reserved;\s*\} dn_sac_config;", code)
    abi.check_names(*NAMES)
    for name in ("SacPolicyHead", "SacCriticLoss", "SacActorLoss"):
        assert getattr(pkg, name) is getattr(pkg.sac, name) and name in pkg.__all__
    assert pkg.SacCritic is pkg.policy.SacCritic and "SacCritic" in pkg.__all__
    assert "dn_sac_loss.hip" in pkg.build.SOURCES and "dn_sac_math.h" in pkg.build.HEADERS
    abi.check_version()


def test_struct_layout_compiled_from_the_header(pkg):
    """dn_sac_config: 56 bytes, gamma 0, target_entropy 8, ent_coef 16, log_std_min 24, log_std_max 32, act_dim 40, n_critics 44, reserved
    48 -- by the C compiler from the header itself, and the ctypes mirror agrees."""
    abi.check_layout(pkg._capi.DnSacConfig, 56, gamma=0, target_entropy=8, ent_coef=16, log_std_min=24, log_std_max=32, act_dim=40, n_critics=44,
                     reserved=48)
    consts = abi.compiled().constants
    assert (consts["DN_SAC_MAX_ACT"], consts["DN_SAC_MAX_CRITICS"]) == (pkg._capi.SAC_MAX_ACT, pkg._capi.SAC_MAX_CRITICS) == (8, 4)
    abi.check_version()


def test_scratch_sizes(pkg):
    """2 n_critics + 2 float64 sums per block of 1024 rows: one size for both losses."""
    lib = pkg._capi.load()
    for batch in (1, 2, 1024, 1025, 2048, 2049, 65536, (1 << 31) - 1):
        for c in range(1, 5):
            assert lib.dn_sac_loss_scratch_bytes(batch, c) == 8 * (2 * c + 2) * -(-batch // S.BLOCK_ROWS), (batch, c)
    for batch in (0, -1, 1 << 31, 1 << 62):
        assert lib.dn_sac_loss_scratch_bytes(batch, 2) == INVALID, batch
        assert b"batch must be in 1..2^31 - 1" in lib.dn_last_error()
    for c in (0, -1, 5, 1 << 30):
        assert lib.dn_sac_loss_scratch_bytes(100, c) == INVALID, c
        assert b"n_critics must be in 1..4" in lib.dn_last_error()


# ---- the refusals of the four calls ---------------------------------------------------------------------------------------------------------
CFG = dict(gamma=0.99, target_entropy=-4.0, ent_coef=0.2, log_std_min=-20.0, log_std_max=2.0, act_dim=4, n_critics=2, reserved=0)
# dummy addresses 1 MiB apart: 100 rows of 4 columns are 1600 bytes, so nothing overlaps unless a case makes it
P = {k: 0x100000 * (i + 1) for i, k in enumerate(
    ("mean", "log_std", "noise", "actions", "log_prob", "g_actions", "g_log_prob", "d_mean", "d_log_std", "q0", "q1", "q2", "q3", "next_q0",
     "next_q1", "next_q2", "next_q3", "d_q0", "d_q1", "d_q2", "d_q3", "next_log_prob", "rewards", "dones", "log_ent_coef", "target_q", "loss",
     "stats", "scratch", "d_log_prob", "d_log_ent_coef", "ent_coef_loss"))}
TABLES = {"q": "q", "next_q": "next_q", "d_q": "d_q", "q_pi": "q", "d_q_pi": "d_q"}     # a table's entries among the dummies
ARGS = {
    "dn_sac_policy": ("mean", "log_std", "noise", "actions", "log_prob"),
    "dn_sac_policy_backward": ("mean", "log_std", "noise", "g_actions", "g_log_prob", "d_mean", "d_log_std"),
    "dn_sac_critic_loss": ("q", "next_q", "next_log_prob", "rewards", "dones", "log_ent_coef", "d_q", "target_q", "loss", "stats", "scratch"),
    "dn_sac_actor_loss": ("log_prob", "q_pi", "log_ent_coef", "d_log_prob", "d_q_pi", "d_log_ent_coef", "loss", "ent_coef_loss", "stats", "scratch"),
}


def _call(lib, K, fn, *, cfg=CFG, batch=100, scratch_bytes=1 << 40, **kw):
    c = None
    if cfg is not None:
        d = dict(cfg, **{k: kw.pop(k) for k in list(kw) if k in CFG})
        c = C.byref(K.DnSacConfig(*[d[k] for k in CFG]))
    p, keep, argv = dict(P, **kw), [], []
    for name in ARGS[fn]:
        if name in TABLES:
            if name in kw and kw[name] is None:
                argv.append(None)
                continue
            table = (C.c_void_p * 4)(*[p.get(f"{name}{i}", p[f"{TABLES[name]}{i}"]) for i in range(4)])
            keep.append(table)
            argv.append(C.cast(table, C.c_void_p))
        else:
            argv.append(p[name])
    if fn in ("dn_sac_critic_loss", "dn_sac_actor_loss"):
        argv.append(scratch_bytes)
    # device 2^20 does not exist: should a case ever pass validation, hipSetDevice refuses it (DN_ERR_HIP) and no kernel sees a dummy pointer
    rc = getattr(lib, fn)(c, batch, *argv, 1 << 20, None)
    return rc, lib.dn_last_error().decode()


COMMON = [
    ("null_cfg", dict(cfg=None), "cfg is required"),
    ("reserved_1", dict(reserved=1), "reserved must be 0 (got 1)"),
    ("batch_0", dict(batch=0), "batch must be in 1..2^31 - 1 (got 0)"),
    ("batch_negative", dict(batch=-100), "batch must be in 1..2^31 - 1"),
    ("batch_2_to_31", dict(batch=1 << 31), "batch must be in 1..2^31 - 1"),
]
POLICY = [
    ("act_dim_0", dict(act_dim=0), "act_dim must be in 1..8 (got 0)"),
    ("act_dim_9", dict(act_dim=9), "act_dim must be in 1..8 (got 9)"),
    ("log_std_bounds_equal", dict(log_std_min=2.0), "log_std_min < log_std_max (got 2, 2)"),
    ("log_std_bounds_swapped", dict(log_std_min=2.0, log_std_max=-20.0), "log_std_min < log_std_max"),
    ("log_std_min_nan", dict(log_std_min=math.nan), "log_std_min and log_std_max must be finite"),
    ("log_std_min_inf", dict(log_std_min=-math.inf), "log_std_min and log_std_max must be finite"),
    ("log_std_max_inf", dict(log_std_max=math.inf), "log_std_min and log_std_max must be finite"),
    ("mean_misaligned", dict(mean=P["mean"] + 2), "mean must be 4-byte aligned"),
]
LOSSES = [
    ("n_critics_0", dict(n_critics=0), "n_critics must be in 1..4 (got 0)"),
    ("n_critics_5", dict(n_critics=5), "n_critics must be in 1..4 (got 5)"),
    ("ent_coef_negative_when_fixed", dict(ent_coef=-0.1, log_ent_coef=None, d_log_ent_coef=None), "ent_coef must be finite and >= 0 when log_ent_coef is NULL (got -0.1)"),
    ("ent_coef_nan_when_fixed", dict(ent_coef=math.nan, log_ent_coef=None, d_log_ent_coef=None), "ent_coef must be finite and >= 0 when log_ent_coef is NULL"),
    ("ent_coef_inf_when_fixed", dict(ent_coef=math.inf, log_ent_coef=None, d_log_ent_coef=None), "ent_coef must be finite and >= 0 when log_ent_coef is NULL"),
    ("null_stats", dict(stats=None), "stats is required"),
    ("null_scratch", dict(scratch=None), "scratch is required"),
    ("null_loss", dict(loss=None), "loss is required"),
    ("scratch_one_byte_short", dict(scratch_bytes="short"), "scratch_bytes is too small"),
    ("scratch_0", dict(scratch_bytes=0), "scratch_bytes is too small"),
    ("scratch_misaligned", dict(scratch=P["scratch"] + 4), "stats and scratch must be 8-byte aligned"),
    ("stats_misaligned", dict(stats=P["stats"] + 4), "stats and scratch must be 8-byte aligned"),
    ("log_ent_coef_misaligned", dict(log_ent_coef=P["log_ent_coef"] + 2), "log_ent_coef must be 4-byte aligned"),
    ("loss_is_log_ent_coef", dict(loss=P["log_ent_coef"]), "overlaps log_ent_coef"),
    ("stats_on_scratch", dict(stats=P["scratch"] + 8), "stats overlaps scratch"),
]
REFUSALS = {
    "dn_sac_policy": COMMON + POLICY + [("null_" + k, {k: None}, k + " is required") for k in ARGS["dn_sac_policy"]] + [
        ("log_prob_misaligned", dict(log_prob=P["log_prob"] + 1), "log_prob must be 4-byte aligned"),
        ("actions_is_mean", dict(actions=P["mean"]), "actions overlaps mean"),
        ("actions_ends_in_noise", dict(actions=P["noise"] - 1596), "actions overlaps noise"),
        ("log_prob_in_log_std", dict(log_prob=P["log_std"] + 1596), "log_prob overlaps log_std"),
        ("log_prob_in_actions", dict(log_prob=P["actions"] + 800), "actions overlaps log_prob"),
    ],
    "dn_sac_policy_backward": COMMON + POLICY + [("null_" + k, {k: None}, k + " is required") for k in ("mean", "log_std", "noise", "d_mean", "d_log_std")] + [
        ("g_actions_misaligned", dict(g_actions=P["g_actions"] + 2), "g_actions must be 4-byte aligned"),
        ("d_mean_is_g_actions", dict(d_mean=P["g_actions"]), "d_mean overlaps g_actions"),
        ("d_log_std_is_log_std", dict(d_log_std=P["log_std"]), "d_log_std overlaps log_std"),
        ("d_log_std_in_g_log_prob", dict(d_log_std=P["g_log_prob"] - 1596), "d_log_std overlaps g_log_prob"),
        ("d_log_std_is_d_mean", dict(d_log_std=P["d_mean"] + 16), "d_mean overlaps d_log_std"),
    ],
    "dn_sac_critic_loss": COMMON + LOSSES + [("null_" + k, {k: None}, k + " is required")
                                             for k in ("q", "next_q", "d_q", "q1", "next_q0", "d_q1", "next_log_prob", "rewards", "dones", "target_q")] + [
        ("gamma_negative", dict(gamma=-0.1), "gamma must be finite and in [0, 1] (got -0.1)"),
        ("gamma_above_1", dict(gamma=1.5), "gamma must be finite and in [0, 1] (got 1.5)"),
        ("gamma_nan", dict(gamma=math.nan), "gamma must be finite and in [0, 1]"),
        ("q1_misaligned", dict(q1=P["q1"] + 2), "q[1] must be 4-byte aligned"),
        ("d_q0_is_q0", dict(d_q0=P["q0"]), "d_q[0] overlaps q[0]"),
        ("d_q1_in_next_q0", dict(d_q1=P["next_q0"] + 396), "d_q[1] overlaps next_q[0]"),
        ("d_q1_is_d_q0", dict(d_q1=P["d_q0"]), "d_q[0] overlaps d_q[1]"),
        ("target_q_in_rewards", dict(target_q=P["rewards"] - 396), "target_q overlaps rewards"),
        ("target_q_in_d_q1", dict(target_q=P["d_q1"] + 4), "d_q[1] overlaps target_q"),
        ("scratch_ends_in_dones", dict(scratch=P["dones"] - 40), "scratch overlaps dones"),
    ],
    "dn_sac_actor_loss": COMMON + LOSSES + [("null_" + k, {k: None}, k + " is required")
                                            for k in ("q_pi", "d_q_pi", "q1", "d_q0", "log_prob", "d_log_prob", "ent_coef_loss")] + [
        ("target_entropy_nan", dict(target_entropy=math.nan), "target_entropy must be finite"),
        ("target_entropy_inf", dict(target_entropy=math.inf), "target_entropy must be finite"),
        ("d_log_ent_coef_missing_when_learned", dict(d_log_ent_coef=None), "d_log_ent_coef is required with log_ent_coef"),
        ("d_log_ent_coef_given_when_fixed", dict(log_ent_coef=None), "d_log_ent_coef must be NULL without log_ent_coef"),
        ("d_log_prob_is_log_prob", dict(d_log_prob=P["log_prob"]), "d_log_prob overlaps log_prob"),
        ("d_q_pi1_in_q_pi0", dict(d_q1=P["q0"] + 396), "d_q_pi[1] overlaps q_pi[0]"),
        ("d_log_ent_coef_is_log_ent_coef", dict(d_log_ent_coef=P["log_ent_coef"]), "d_log_ent_coef overlaps log_ent_coef"),
        ("ent_coef_loss_is_actor_loss", dict(ent_coef_loss=P["loss"]), "actor_loss overlaps ent_coef_loss"),
        ("d_log_prob_in_d_q_pi0", dict(d_log_prob=P["d_q0"] - 396), "d_log_prob overlaps d_q_pi[0]"),
    ],
}
NAMED = {"dn_sac_actor_loss": {"loss": "actor_loss", "q1": "q_pi[1]", "d_q0": "d_q_pi[0]"},
         "dn_sac_critic_loss": {"q1": "q[1]", "next_q0": "next_q[0]", "d_q1": "d_q[1]"}}


@pytest.mark.parametrize("fn,kw,message", [pytest.param(fn, *r[1:], id=fn[3:] + "-" + r[0]) for fn, rs in REFUSALS.items() for r in rs])
def test_the_calls_refuse(pkg, fn, kw, message):
    """Every case returns DN_ERR_INVALID_ARGUMENT with a text that names the argument, on dummy pointers: none gets as far as a device
    call."""
    K = pkg._capi
    lib = K.load()
    kw = dict(kw)
    if kw.get("scratch_bytes") == "short":
        kw["scratch_bytes"] = lib.dn_sac_loss_scratch_bytes(100, 2) - 1
    if message.endswith(" is required") and message.split()[0] in NAMED.get(fn, {}):
        message = NAMED[fn][message.split()[0]] + " is required"
    rc, msg = _call(lib, K, fn, **kw)
    assert rc == INVALID, msg
    assert message in msg, msg


def test_the_refusals_are_not_the_dummies_own(pkg):
    """The unchanged dummy calls -- also with a fixed coefficient, without the optional gradients, every act_dim and n_critics, a batch of
    one, the exact scratch size, and outputs that end where an input begins -- pass validation and end at hipSetDevice (DN_ERR_HIP, or
    DN_ERR_NO_DEVICE): each refusal above is caused by what it changes."""
    K = pkg._capi
    lib = K.load()
    fixed = dict(log_ent_coef=None, d_log_ent_coef=None)
    cases = {
        "dn_sac_policy": [dict(), dict(batch=1), dict(actions=P["noise"] - 1600)] + [dict(act_dim=a) for a in range(1, 9)],
        "dn_sac_policy_backward": [dict(), dict(g_actions=None), dict(g_log_prob=None), dict(g_actions=None, g_log_prob=None), dict(act_dim=8)],
        "dn_sac_critic_loss": [dict(), dict(log_ent_coef=None), dict(scratch_bytes=lib.dn_sac_loss_scratch_bytes(100, 2)), dict(gamma=0.0), dict(gamma=1.0),
                               dict(target_q=P["rewards"] - 400), dict(ent_coef=-1.0)] + [dict(n_critics=c) for c in range(1, 5)],
        "dn_sac_actor_loss": [dict(), fixed, dict(fixed, ent_coef=0.0), dict(batch=1), dict(ent_coef=math.nan)] + [dict(n_critics=c) for c in range(1, 5)],
    }
    for fn, kws in cases.items():
        for kw in kws:
            rc, msg = _call(lib, K, fn, **kw)
            assert rc in (-2, -4), (fn, kw, rc, msg)


# ---- csrc/dn_sac_math.h as a host program --------------------------------------------------------------------------------------------------
def _ulps(got, exact):
    """|got - exact| in float64 ulp of the exact value (a Decimal)."""
    f = float(exact)
    if f == 0.0:
        return 0.0 if got == 0.0 else math.inf
    return float(abs(decimal.Decimal(got) - exact) / decimal.Decimal(math.ulp(f)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_sac_math_as_a_host_program(tmp_path, sanitize):
    """tests/tools/check_sac_math.cpp includes csrc/dn_sac_math.h alone: built with the host compiler without contraction, as the library
    is, plainly and under the address and undefined-behaviour sanitizers, and run as its own process.
    sech^2 and tanh at 4001 values of pre over [-30, 30] and at 0, -0, +-1e-8, +-1e-3, +-20, 40 are within 8 float64 ulp of 40-digit
    arithmetic (exp 1, 1 + t 0.5, the square 1.5, the quotient 0.5, and a factor 2 for the binade); the elements and their gradients are
    the NumPy statement of the same forms to 2^-40 of their absolute terms; the minimum follows the stated tie and NaN rules."""
    exe = host_program_support.build("check_sac_math", tmp_path, sanitize=sanitize, extra_flags=("-Wall", "-Werror", "-ffp-contract=off"))
    result, lines = host_program_support.run_lines(exe, timeout=120)
    hx = float.fromhex
    worst_j = worst_a = 0.0
    elements, mins = [], []
    with decimal.localcontext() as ctx:
        ctx.prec = 40
        for line in lines[:-1]:
            kind, *v = line.split()
            if kind == "S":
                pre, a, J = (hx(x) for x in v)
                t = (decimal.Decimal(-2) * abs(decimal.Decimal(pre))).exp()
                exact_j = 4 * t / ((1 + t) * (1 + t))
                exact_a = (1 - t) / (1 + t) * (1 if pre >= 0 else -1)
                worst_j, worst_a = max(worst_j, _ulps(J, exact_j)), max(worst_a, _ulps(a, exact_a))
                assert math.copysign(1.0, a) == math.copysign(1.0, pre), line
            elif kind == "E":
                elements.append([hx(x) for x in v])
            else:
                mins.append(([hx(x) for x in v[:4]], hx(v[4]), int(v[5])))
    assert result["squash"] == 4010 and result["elements"] == 4000 == len(elements) and result["mins"] == 9 == len(mins)
    print(f"sech^2 {worst_j:.2f} and tanh {worst_a:.2f} float64 ulp from 40-digit arithmetic")
    assert worst_j <= 8.0 and worst_a <= 8.0, (worst_j, worst_a)

    e = np.array(elements)
    d = dict(mean=e[:, 0:1], log_std=e[:, 1:2], noise=e[:, 2:3], g_actions=e[:, 3:4], g_log_prob=e[:, 4])
    forms = S.policy_closed_forms(d)
    J, std = forms["J"][:, 0], np.exp(np.clip(e[:, 1], S.LOG_STD_MIN, S.LOG_STD_MAX))
    K = 2.0 * forms["actions"][:, 0] * J / (J + S.LOG_EPS)
    dm_terms = np.abs(e[:, 3] * J) + np.abs(e[:, 4] * K)
    bounds = dict(actions=np.abs(forms["actions"][:, 0]), log_prob=0.5 * e[:, 2] ** 2 + np.abs(np.clip(e[:, 1], -20, 2)) + S.HALF_LOG_2PI + np.abs(np.log(J + S.LOG_EPS)),
                  d_mean=dm_terms, d_log_std=dm_terms * np.abs(std * e[:, 2]) + np.abs(e[:, 4]))
    for col, key in ((5, "actions"), (6, "log_prob"), (7, "d_mean"), (8, "d_log_std")):
        want = forms[key][:, 0] if forms[key].ndim == 2 else forms[key]
        assert (np.abs(e[:, col] - want) <= S.EPS40 * bounds[key]).all(), key
    low, high = e[:, 1] < S.LOG_STD_MIN, e[:, 1] > S.LOG_STD_MAX
    assert low.mean() > 0.05 and high.mean() > 0.05 and (e[low | high, 8] == 0.0).all() and (e[7:9, 8] != 0.0).all()      # the bounds pass
    assert (np.abs(e[:, 0] + std * e[:, 2]) > 9.0).mean() > 0.05

    for q, m, pick in mins:
        want = next((c for c, x in enumerate(q) if math.isnan(x)), None)
        if want is None:
            want = q.index(min(q))                              # list.index: the lowest c of a tie
            assert m == min(q)
        else:
            assert math.isnan(m)
        assert pick == want, (q, m, pick)
    assert hx(result["alpha"]) == S.exp_correctly_rounded(-1.2039728164672852)
    assert hx(result["target"]) == 0.5 + (1.0 - 0.0) * 0.99 * (2.0 - 0.25 * -3.0)


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------------
def test_python_surface_refuses(pkg):
    H, Q, A = pkg.SacPolicyHead, pkg.SacCriticLoss, pkg.SacActorLoss
    with pytest.raises(RuntimeError, match="SacPolicyHead needs a GPU device, got cpu; there is no CPU path"):
        H(256, 4, "cpu")
    with pytest.raises(RuntimeError, match="SacCriticLoss needs a GPU device, got cpu; there is no CPU path"):
        Q(256, "cpu", n_critics=2, gamma=0.99, ent_coef=0.2)
    with pytest.raises(RuntimeError, match="SacActorLoss needs a GPU device, got cpu; there is no CPU path"):
        A(256, torch.device("cpu"), target_entropy=-4.0)
    for bad in (dict(batch_size=0), dict(batch_size=2.0), dict(batch_size=True), dict(batch_size=1 << 31), dict(act_dim=0), dict(act_dim=9)):
        args = dict(dict(batch_size=256, act_dim=4), **bad)
        with pytest.raises(ValueError, match="SacPolicyHead." + next(iter(bad))):
            H(args["batch_size"], args["act_dim"], "cpu")
    for kw in (dict(log_std_min=2.0), dict(log_std_min=math.nan), dict(log_std_max=math.inf), dict(log_std_min=3.0, log_std_max=-3.0)):
        with pytest.raises(ValueError, match="SacPolicyHead.log_std_min and log_std_max must be finite with log_std_min < log_std_max"):
            H(256, 4, "cpu", **kw)
    for cls, extra in ((Q, {}), (A, dict(target_entropy=-4.0))):
        for kw in (dict(n_critics=0), dict(n_critics=5), dict(n_critics=2.0), dict(ent_coef=-0.1), dict(ent_coef=math.nan), dict(ent_coef=math.inf)):
            with pytest.raises(ValueError, match=cls.__name__ + "." + next(iter(kw)) + " must be"):
                cls(256, "cpu", **dict(extra, **kw))
        with pytest.raises(ValueError, match=cls.__name__ + ".batch_size must be"):
            cls(0, "cpu", **extra)
    for g in (-0.1, 1.5, math.nan):
        with pytest.raises(ValueError, match="SacCriticLoss.gamma must be finite and in \\[0, 1\\]"):
            Q(256, "cpu", gamma=g)
    for t in (math.nan, math.inf):
        with pytest.raises(ValueError, match="SacActorLoss.target_entropy must be finite"):
            A(256, "cpu", target_entropy=t)
    with pytest.raises(TypeError):
        A(256, "cpu")                                           # target_entropy has no default


def test_python_calls_refuse_their_tensors(pkg):
    """The checks of a call need no device: they run on objects whose device is set by hand, before anything reaches the library."""
    z = torch.zeros
    head = pkg.SacPolicyHead.__new__(pkg.SacPolicyHead)
    head.device, head.batch_size, head.act_dim = torch.device("cpu"), 8, 4

    def refuses(obj, match, *args):
        with pytest.raises(ValueError, match=match):
            obj(*args)

    refuses(head, "mean must be a tensor \\[count, 4\\]", None, z(6, 4), z(6, 4))
    refuses(head, "mean has 9 rows; a call takes 1..8", z(9, 4), z(9, 4), z(9, 4))
    refuses(head, "mean has 0 rows", z(0, 4), z(0, 4), z(0, 4))
    refuses(head, "mean must be torch.float32 \\[6, 4\\]", z(6, 3), z(6, 4), z(6, 4))
    refuses(head, "mean must be dense", z(6, 8)[:, :4], z(6, 4), z(6, 4))
    refuses(head, "log_std must be torch.float32 \\[6, 4\\]", z(6, 4), z(4), z(6, 4))
    refuses(head, "log_std must be torch.float32", z(6, 4), z(6, 4, dtype=torch.float64), z(6, 4))
    refuses(head, "noise must be a tensor", z(6, 4), z(6, 4), None)
    refuses(head, "noise must be dense", z(6, 4), z(6, 4), z(6, 8)[:, ::2])

    crit = pkg.SacCriticLoss.__new__(pkg.SacCriticLoss)
    crit.device, crit.batch_size, crit.n_critics, crit.ent_coef = torch.device("cpu"), 8, 2, None
    q, batch, lec = [z(6), z(6, 1)], dict(rewards=z(6), dones=z(6)), z(1)
    refuses(crit, "next_log_prob must be a tensor \\[count\\]", q, q, z(6, 1), batch, lec)
    refuses(crit, "next_log_prob has 9 rows", q, q, z(9), batch, lec)
    refuses(crit, "q_list must be a list of 2 tensors", [z(6)], q, z(6), batch, lec)
    refuses(crit, "q_list must be a list of 2 tensors", z(2, 6), q, z(6), batch, lec)
    refuses(crit, "q_list\\[1\\] must be torch.float32 \\[6\\] or \\[6, 1\\]", [z(6), z(6, 2)], q, z(6), batch, lec)
    refuses(crit, "next_q_list\\[0\\] must be dense", q, [z(12)[::2], z(6)], z(6), batch, lec)
    refuses(crit, "batch\\['dones'\\] is missing", q, q, z(6), dict(rewards=z(6)), lec)
    refuses(crit, "batch\\['rewards'\\] must be torch.float32 \\[6\\]", q, q, z(6), dict(rewards=z(7), dones=z(6)), lec)
    refuses(crit, "log_ent_coef is required: the coefficient is learned", q, q, z(6), batch, None)
    refuses(crit, "log_ent_coef must be torch.float32 \\[1\\] or \\[\\]", q, q, z(6), batch, z(2))
    crit.ent_coef = 0.2
    refuses(crit, "log_ent_coef must be None with the fixed ent_coef=0.2", q, q, z(6), batch, lec)

    act = pkg.SacActorLoss.__new__(pkg.SacActorLoss)
    act.device, act.batch_size, act.n_critics, act.ent_coef = torch.device("cpu"), 8, 2, None
    refuses(act, "log_prob must be a tensor \\[count\\]", z(6, 1), q, lec)
    refuses(act, "log_prob has 9 rows", z(9), q, lec)
    refuses(act, "log_prob must be torch.float32", z(6, dtype=torch.float16), q, lec)
    refuses(act, "q_pi_list must be a list of 2 tensors", z(6), [z(6)] * 3, lec)
    refuses(act, "q_pi_list\\[0\\] must be torch.float32 \\[6\\] or \\[6, 1\\]", z(6), [z(7), z(6)], lec)
    refuses(act, "log_ent_coef is required", z(6), q, None)


# ---- the header's composition and SB3's literal one -----------------------------------------------------------------------------------------
def test_the_composition_is_sac_actor_squash_where_that_is_well_conditioned(pkg):
    """policy.SacActor.squash, the literal expression, in float64 on data with log_std >= -5 and |pre| <= 6, against the header's forms:
    log_prob to 2^-40 sum_j |term_j| + sum_j 2^-51 / (J_j + 1e-6), the second part being the literal form's own cancellation in
    1 - a * a; the actions are the same tanh."""
    from drl_dronenavigation_amd.policy import SacActor
    rng = np.random.default_rng(11)
    B, A = 8192, 8
    ls = torch.from_numpy(-5.0 + 6.5 * rng.random((B, A)))
    eps = torch.from_numpy(rng.standard_normal((B, A)))
    pre = torch.from_numpy(12.0 * rng.random((B, A)) - 6.0)
    mean = pre - torch.exp(ls) * eps
    a, lp, m = S.squash_composition(mean, ls, eps)
    assert float(m["pre"].abs().max()) <= 6.0 + 1e-9 and float(ls.min()) >= -5.0
    a_lit, lp_lit = SacActor.squash(mean, ls, eps)
    bound = S.EPS40 * m["terms"].abs().sum(1) + (2.0 ** -51 / (m["J"] + S.LOG_EPS)).sum(1)
    worst = float(((lp - lp_lit).abs() / bound).max())
    print(f"log_prob of the header's forms from SacActor.squash: {float((lp - lp_lit).abs().max()):.2e}, {worst:.3f} of the bound")
    assert worst <= 1.0 and torch.equal(a, a_lit)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", S.BATCHES)
def test_policy_reference_is_the_closed_forms(batch):
    """torch's float64 autograd on the composition against the hand-derived forms of the header in NumPy, to 2^-40 of the mean absolute
    term of each output over the data set."""
    worst = 0.0
    for act_dim in S.ACT_DIMS:
        d = S.policy_data(batch, act_dim)
        ref, forms = S.policy_reference(d), S.policy_closed_forms(d)
        if batch >= S.COVERED_FROM:
            S.check_policy_coverage(ref, (batch, act_dim))
        for k in ("actions", "log_prob", "d_mean", "d_log_std"):
            bound = S.EPS40 * float(np.mean(ref[k + "_terms"]))
            err = float(np.abs(forms[k] - ref[k]).max())
            assert err <= bound, (batch, act_dim, k, err, bound)
            worst = max(worst, err / bound)
        for flags in (dict(use_g_actions=False), dict(use_g_log_prob=False)):      # a NULL gradient is a zero gradient
            d0 = dict(d, **{("g_actions" if "use_g_actions" in flags else "g_log_prob"): np.zeros_like(d["g_actions" if "use_g_actions" in flags else "g_log_prob"])})
            ref0, forms0 = S.policy_reference(d, **flags), S.policy_closed_forms(d0)
            for k in ("d_mean", "d_log_std"):
                assert float(np.abs(forms0[k] - ref0[k]).max()) <= S.EPS40 * float(np.mean(ref[k + "_terms"])), (batch, act_dim, k, flags)
    print(f"B {batch}: closed forms from autograd, {worst:.2e} of the bound")


@pytest.mark.parametrize("batch", S.BATCHES)
def test_loss_references_are_the_closed_forms(batch):
    worst = 0.0
    for C_ in S.CRITICS:
        d = S.loss_data(batch, C_)
        for learned in (True, False):
            for gamma in S.GAMMAS:
                ref, forms = S.critic_reference(d, gamma, learned), S.critic_closed_forms(d, gamma, learned)
                if batch >= S.COVERED_FROM:
                    S.check_loss_coverage(ref, (batch, C_, "critic"), dones=True)
                for k in ("d_q", "target_q"):
                    bound = S.EPS40 * float(np.mean(ref[k + "_terms"]))
                    err = float(np.abs(forms[k] - ref[k]).max())
                    assert err <= bound, (batch, C_, k, err, bound)
                    worst = max(worst, err / bound)
                dist, same = S.distance(forms["stats"], ref["stats"], S.stats_tolerance(ref))
                assert same and dist <= 0.25, (batch, C_, "critic stats", dist)
                assert abs(ref["torch_loss"] - ref["loss"]) <= S.stats_tolerance(ref)[0]
            ref, forms = S.actor_reference(d, learned), S.actor_closed_forms(d, learned)
            if batch >= S.COVERED_FROM:
                S.check_loss_coverage(ref, (batch, C_, "actor"))
            assert np.array_equal(forms["d_q_pi"], ref["d_q_pi"]) and np.abs(forms["d_log_prob"] - ref["d_log_prob"]).max() <= 1e-18
            dist, same = S.distance(forms["stats"], ref["stats"], S.stats_tolerance(ref))
            assert same and dist <= 0.25, (batch, C_, "actor stats", dist)
            assert abs(ref["torch_actor_loss"] - ref["actor_loss"]) <= S.stats_tolerance(ref)[0]
            assert abs(ref["torch_ent_coef_loss"] - ref["ent_coef_loss"]) <= max(S.stats_tolerance(ref)[1], 0.0)
    print(f"B {batch}: closed forms from autograd, {worst:.2e} of the bound")


def test_references_are_stable_under_the_order_of_the_rows():
    """The references with their rows reversed stay within 1e-5 of their own tolerances."""
    worst = 0.0
    for batch in S.BATCHES:
        for act_dim in S.ACT_DIMS:
            d = S.policy_data(batch, act_dim)
            one, two = S.policy_reference(d), S.policy_reference(d, reverse=True)
            for k in ("actions", "log_prob", "d_mean", "d_log_std"):
                dist, same = S.distance(two[k], one[k], S.row_tolerance(one, k))
                assert same and dist <= 1e-5, (batch, act_dim, k, dist)
                worst = max(worst, dist)
        for C_ in S.CRITICS:
            d = S.loss_data(batch, C_)
            one, two = S.critic_reference(d, 0.99, True), S.critic_reference(d, 0.99, True, reverse=True)
            for k, tol in (("d_q", S.row_tolerance(one, "d_q")), ("target_q", S.row_tolerance(one, "target_q")), ("stats", S.stats_tolerance(one))):
                dist, same = S.distance(two[k], one[k], tol)
                assert same and dist <= 1e-5, (batch, C_, k, dist)
                worst = max(worst, dist)
            one, two = S.actor_reference(d, True), S.actor_reference(d, True, reverse=True)
            for k, tol in (("d_log_prob", S.ulp32(one["d_log_prob"])), ("d_q_pi", S.ulp32(one["d_q_pi"])), ("stats", S.stats_tolerance(one))):
                dist, same = S.distance(two[k], one[k], tol)
                assert same and dist <= 1e-5, (batch, C_, k, dist)
                worst = max(worst, dist)
    print(f"the two orders differ by at most {worst:.2e} of the tolerance")


def test_reference_edge_values():
    """One NaN mean element: NaN in that row's outputs only.  One NaN reward: NaN in target_q and d_q of that row and in the loss.  A tie of
    q_pi: the NumPy statement picks the lowest c."""
    d = {k: v.copy() for k, v in S.policy_data(65, 4).items()}
    d["mean"][17, 2] = np.nan
    for got in (S.policy_reference(d), S.policy_closed_forms(d)):
        assert np.isnan(got["log_prob"][17]) and np.isfinite(np.delete(got["log_prob"], 17)).all()
        bad = np.isnan(got["actions"])
        assert bad[17, 2] and bad.sum() == 1
        assert np.isnan(got["d_mean"][17, 2]) and np.isfinite(np.delete(got["d_mean"], 17, axis=0)).all()
    d = {k: (tuple(x.copy() for x in v) if isinstance(v, tuple) else v.copy()) for k, v in S.loss_data(65, 2).items()}
    d["rewards"][9] = np.nan
    for got in (S.critic_reference(d, 0.99, True), S.critic_closed_forms(d, 0.99, True)):
        assert np.isnan(got["loss"]) and np.isnan(got["target_q"][9]) and np.isfinite(np.delete(got["target_q"], 9)).all()
        assert np.isnan(got["d_q"][:, 9]).all() and np.isfinite(np.delete(got["d_q"], 9, axis=1)).all()
    d["q_pi"][1][:] = d["q_pi"][0]
    forms = S.actor_closed_forms(d, True)
    assert (forms["d_q_pi"][0] == -1.0 / 65).all() and (forms["d_q_pi"][1] == 0.0).all()
