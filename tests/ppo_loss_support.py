"""What the PPO loss tests share (pytest does not collect it; needs torch on the CPU only): the test data, the reference -- the arithmetic
of include/dronenav.h dn_ppo_loss written as the plain torch composition in float64 on the CPU, autograd producing the gradients -- the
closed forms of the gradients restated in NumPy, the tolerances, and the reference's own branch-coverage and order-stability checks."""
import decimal
import functools
import math

import numpy as np
import torch

from loss_support import ACT_DIMS, BATCHES, BLOCK_ROWS, COVERED_FROM, EPS40, HALF_LOG_2PI, distance, ulp32  # noqa: F401  (handed on to the tests)

SPREADS = {"first": 0.0, "near": 0.15, "far": 0.5}      # the standard deviation of new - old log-probability: the first epoch, near, far
CLIP_RANGE, CLIP_RANGE_VF = 0.2, 0.2
COEFS = ((0.0, 0.0), (0.01, 0.5))       # (ent_coef, vf_coef): both zero, both nonzero
STATS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")


_EXP = {}


def exp_correctly_rounded(x):
    """exp of a float64 NumPy array, every element rounded correctly (40 decimal digits, then one rounding), remembered per input."""
    key = x.tobytes()
    if key not in _EXP:
        with decimal.localcontext() as ctx:
            ctx.prec = 40
            _EXP[key] = np.array([float(decimal.Decimal(float(v)).exp()) for v in x.ravel()], np.float64).reshape(x.shape)
    return _EXP[key]


def _logp64(mean, log_std, actions):
    ls = log_std.astype(np.float64)
    z = (actions.astype(np.float64) - mean.astype(np.float64)) * exp_correctly_rounded(-ls)
    terms = -0.5 * z * z - ls - HALF_LOG_2PI
    logp = terms[:, 0].copy()
    for j in range(1, terms.shape[1]):                          # j ascending
        logp = logp + terms[:, j]
    return logp, z


@functools.lru_cache(maxsize=None)
def data(batch, act_dim, spread):
    """One data set as float32 NumPy arrays (made once, never written): means 0.09 + 0.01 N, log_std = -2 + 0.3 N, actions drawn from that
    Gaussian, old_log_prob = float32(logp + s N), adv = N, returns = 2 N, old_values = returns + 0.5 N, values = old_values + 0.3 N."""
    rng = np.random.default_rng(100000 * list(SPREADS).index(spread) + 10 * batch + act_dim)
    f32 = np.float32
    mean = (0.09 + 0.01 * rng.standard_normal((batch, act_dim))).astype(f32)
    log_std = (-2.0 + 0.3 * rng.standard_normal(act_dim)).astype(f32)
    actions = (mean + np.exp(log_std.astype(np.float64)) * rng.standard_normal((batch, act_dim))).astype(f32)
    logp, _ = _logp64(mean, log_std, actions)
    d = dict(mean=mean, log_std=log_std, actions=actions, old_log_prob=(logp + SPREADS[spread] * rng.standard_normal(batch)).astype(f32),
             advantages=rng.standard_normal(batch).astype(f32))
    d["returns"] = (2.0 * rng.standard_normal(batch)).astype(f32)
    d["old_values"] = (d["returns"] + 0.5 * rng.standard_normal(batch)).astype(f32)
    d["values"] = (d["old_values"] + 0.3 * rng.standard_normal(batch)).astype(f32)
    for v in d.values():
        v.setflags(write=False)
    return d


def composition(mean, log_std, values, actions, old_log_prob, advantages, returns, old_values, clip_range, clip_range_vf, ent_coef, vf_coef,
                exact_exp=False):
    """SB3 PPO.train's loss [from recall] as the plain torch composition, in the dtype and on the device of its tensors.  Returns the loss
    and a dict of everything the tests read; clip_range_vf None = no value clip (old_values is then not read).
    exact_exp (float64 on the CPU only): the values of exp(-log_std) and of ratio = exp(lr) are the correctly rounded ones, their
    derivatives still torch's.  In the first epoch lr ~ 1e-7 and a row's approx_kl term (ratio - 1) - lr is about lr^2 / 2 ~ 1e-14 beside a
    ratio rounded to 2^-53: the term is a function of the very bits of lr and of the rounding of exp, so a reference that is to be held to
    2^-40 of that term has to state both without an error of its own.  torch's vectorised CPU exp is one ulp off in about 6 % of those
    rows (measured against 40-digit arithmetic; the C library's scalar exp in none), which alone moves approx_kl by 1e8 tolerances, and a
    library exp(-log_std) one ulp off moves the last bit of logp in a quarter of the rows (the kernel forms it with csrc/dn_exp_cr.h)."""
    inv = torch.exp(-log_std)
    if exact_exp:
        inv = inv + (torch.from_numpy(exp_correctly_rounded(-log_std.detach().numpy())) - inv).detach()
    z = (actions - mean) * inv
    terms = -0.5 * z * z - log_std - HALF_LOG_2PI
    logp = terms[:, 0]
    for j in range(1, terms.shape[1]):                          # j ascending, as the header states it (torch's own sum(-1) pairs the columns)
        logp = logp + terms[:, j]
    lr = logp - old_log_prob
    ratio = torch.exp(lr)
    if exact_exp:
        exact = torch.from_numpy(exp_correctly_rounded(lr.detach().numpy()))
        ratio = ratio + (exact - ratio).detach()               # both steps exact: the two differ by an ulp at most
    p1 = advantages * ratio
    p2 = advantages * torch.clamp(ratio, 1.0 - clip_range, 1.0 + clip_range)
    pmin = torch.min(p1, p2)
    policy_loss = -pmin.mean()
    clipped = (torch.abs(ratio - 1.0) > clip_range).to(ratio.dtype)
    with torch.no_grad():
        kl = (ratio - 1.0) - lr
    if clip_range_vf is None:
        vpred, inside = values, torch.ones_like(values)
    else:
        step = values - old_values
        vpred = old_values + torch.clamp(step, -clip_range_vf, clip_range_vf)
        inside = ((step >= -clip_range_vf) & (step <= clip_range_vf)).to(values.dtype)
    sq = (returns - vpred) ** 2
    value_loss = sq.mean()
    ent = 0.5 + HALF_LOG_2PI + log_std
    entropy_loss = -ent.sum()
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    return loss, dict(z=z, logp=logp, ratio=ratio, pmin=pmin, clipped=clipped, kl=kl, inside=inside, sq=sq, ent=ent, policy_loss=policy_loss,
                      value_loss=value_loss, entropy_loss=entropy_loss, approx_kl=kl.mean(), clip_fraction=clipped.mean())


def reference(d, clip_range=CLIP_RANGE, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5, reverse=False):
    """The float64 reference of one data set: {loss, stats [6], d_mean, d_log_std, d_value, log_probs} and, per reduction, the mean absolute
    term of its sum (stats_terms [6], d_log_std_terms [A]), plus the shares the coverage checks read.  reverse: the rows in the opposite
    order (and so every sum over rows), the per-row outputs turned back."""
    t = {k: torch.from_numpy(np.ascontiguousarray(v[::-1] if reverse and k != "log_std" else v).astype(np.float64)) for k, v in d.items()}
    mean, log_std, values = t["mean"].requires_grad_(), t["log_std"].requires_grad_(), t["values"].requires_grad_()
    loss, m = composition(mean, log_std, values, t["actions"], t["old_log_prob"], t["advantages"], t["returns"], t["old_values"], clip_range,
                          clip_range_vf, ent_coef, vf_coef, exact_exp=True)
    m["logp"].retain_grad()
    loss.backward()
    n = lambda x: x.detach().numpy()  # noqa: E731
    back = (lambda x: x[::-1].copy()) if reverse else (lambda x: x)
    # The statistics are the means of torch's float64 per-row terms taken with an exactly rounded sum (math.fsum): the reference's own
    # statistics then do not depend on the order of the rows at all, which is what lets it keep the 1e-5 of check_order_stability -- one
    # float64 ulp is already 2.4e-4 of a bound of 2^-40 |value|.  The gradients are autograd's, of torch's own loss.
    total = lambda x: math.fsum(n(x).tolist())  # noqa: E731
    rows = float(len(d["values"]))
    stat = {"policy_loss": -(total(m["pmin"]) / rows), "value_loss": total(m["sq"]) / rows, "entropy_loss": -total(m["ent"]),
            "approx_kl": total(m["kl"]) / rows, "clip_fraction": total(m["clipped"]) / rows}
    stat["loss"] = stat["policy_loss"] + ent_coef * stat["entropy_loss"] + vf_coef * stat["value_loss"]
    terms = {"policy_loss": total(m["pmin"].abs()) / rows, "value_loss": total(m["sq"].abs()) / rows,
             "entropy_loss": total(m["ent"].abs()) / act_cols(d), "approx_kl": total(m["kl"].abs()) / rows, "clip_fraction": stat["clip_fraction"]}
    terms["loss"] = terms["policy_loss"] + ent_coef * terms["entropy_loss"] + vf_coef * terms["value_loss"]
    dls_terms = (m["logp"].grad[:, None] * (m["z"].detach() ** 2 - 1.0)).abs().mean(0)
    return dict(loss=stat["loss"], torch_loss=loss.item(), stats=np.array([stat[k] for k in STATS]), d_mean=back(n(mean.grad)),
                d_log_std=n(log_std.grad), d_value=back(n(values.grad)), log_probs=back(n(m["logp"])),
                stats_terms=np.array([terms[k] for k in STATS]), d_log_std_terms=n(dls_terms),
                clip_share=stat["clip_fraction"], inside_share=float(m["inside"].mean()))


def act_cols(d):
    return float(len(d["log_std"]))


def closed_forms(d, clip_range=CLIP_RANGE, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5):
    """The hand-derived forms of include/dronenav.h in float64 NumPy: what the kernel evaluates, stated a second time."""
    f = {k: v.astype(np.float64) for k, v in d.items()}
    nb = float(len(f["values"]))
    inv = exp_correctly_rounded(-f["log_std"])
    logp, z = _logp64(d["mean"], d["log_std"], d["actions"])
    lr = logp - f["old_log_prob"]
    ratio = exp_correctly_rounded(lr)
    lo, hi, adv = 1.0 - clip_range, 1.0 + clip_range, f["advantages"]
    p1, p2 = adv * ratio, adv * np.clip(ratio, lo, hi)
    w = np.where(p1 < p2, 1.0, np.where(p1 > p2, 0.0, np.where((ratio >= lo) & (ratio <= hi), 1.0, 0.5)))
    g = -adv * w * ratio / nb
    if clip_range_vf is None:
        vpred, inside = f["values"], 1.0
    else:
        step = f["values"] - f["old_values"]
        vpred = f["old_values"] + np.clip(step, -clip_range_vf, clip_range_vf)
        inside = ((step >= -clip_range_vf) & (step <= clip_range_vf)).astype(np.float64)
    e = f["returns"] - vpred
    policy_loss, value_loss = -np.mean(np.minimum(p1, p2)), np.mean(e * e)
    entropy_loss = -np.sum(0.5 + HALF_LOG_2PI + f["log_std"])
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    return dict(loss=loss, stats=np.array([loss, policy_loss, value_loss, entropy_loss, np.mean((ratio - 1.0) - lr), np.mean(np.abs(ratio - 1.0) > clip_range)]),
                d_mean=g[:, None] * z * inv, d_log_std=(g[:, None] * (z * z - 1.0)).sum(0) - ent_coef,
                d_value=vf_coef * -2.0 * e * inside / nb, log_probs=logp)


# ---- tolerances, against reference() only ---------------------------------------------------------------------------------------------------
def tolerances(ref):
    """Per output of reference(): d_mean, d_value, log_probs one float32 ulp of the reference value or 2^-40 absolute, whichever is larger
    (the single rounding to float32, and near zero the last float64 bits of exp and 1 / B); d_log_std one float32 ulp or 2^-40 times the
    mean absolute term of its sum; stats 2^-40 times the mean absolute term of the sum or 2^-40 |value|, whichever is larger (a float64
    sum of B <= 2^11 terms in any order is within B 2^-53 <= 2^-42 of its mean absolute term, and exp is within a few 2^-53 of its
    value); loss one float32 ulp or the stats bound."""
    tol = {k: np.maximum(ulp32(ref[k]), EPS40) for k in ("d_mean", "d_value", "log_probs")}
    tol["d_log_std"] = np.maximum(ulp32(ref["d_log_std"]), EPS40 * ref["d_log_std_terms"])
    with np.errstate(invalid="ignore"):
        tol["stats"] = EPS40 * np.fmax(ref["stats_terms"], np.abs(ref["stats"]))
    tol["loss"] = np.fmax(ulp32(ref["loss"]), tol["stats"][0])
    return tol


def check_outputs(got, ref, tag):
    """got: {loss, stats [>= 6], d_mean, d_log_std, d_value, log_probs} as NumPy; every output within tolerances(ref).  Returns the largest
    distance, in units of the tolerance, per output."""
    tol, worst = tolerances(ref), {}
    for k in ("d_mean", "d_value", "log_probs", "d_log_std", "stats", "loss"):
        g = np.asarray(got[k], np.float64)
        dist, same = distance(g[:6] if k == "stats" else g, ref[k], tol[k])
        assert same, f"{tag}: {k}: the NaN cells differ from the reference's"
        assert dist <= 1.0, f"{tag}: {k} is {dist:.3f} of its tolerance from the float64 reference"
        worst[k] = dist
    return worst


def check_coverage(ref, spread, value_clip, tag):
    """The data set exercises both branches of every reduction it is used for: the reference's clip fraction lies strictly between 0.05 and
    0.95 for "near" and "far" (and is 0 in the first epoch), the share of rows inside the value clip strictly between 0.2 and 0.8."""
    if spread == "first":
        assert ref["clip_share"] == 0.0, f"{tag}: first epoch, but {ref['clip_share']} of the rows are clipped"
    else:
        assert 0.05 < ref["clip_share"] < 0.95, f"{tag}: clip fraction {ref['clip_share']} exercises one branch only"
    if value_clip:
        assert 0.2 < ref["inside_share"] < 0.8, f"{tag}: {ref['inside_share']} of the rows inside the value clip: one branch only"


def check_order_stability(batch, act_dim, spread, value_clip, coefs):
    """The reference summed forwards and backwards stays inside 1e-5 of its own tolerances.  Returns the largest distance seen."""
    kw = dict(clip_range_vf=CLIP_RANGE_VF if value_clip else None, ent_coef=coefs[0], vf_coef=coefs[1])
    d = data(batch, act_dim, spread)
    one, two = reference(d, **kw), reference(d, reverse=True, **kw)
    tol, worst = tolerances(one), 0.0
    for k in ("d_mean", "d_value", "log_probs", "d_log_std", "stats", "loss"):
        dist, same = distance(two[k], one[k], tol[k])
        assert same and dist <= 1e-5, f"B {batch}, A {act_dim}, {spread}: {k} moves by {dist:.3e} of its tolerance with the summation order"
        worst = max(worst, dist)
    return worst
