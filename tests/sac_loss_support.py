"""What the SAC loss tests share (pytest does not collect it; needs torch on the CPU only): the test data, the reference -- the arithmetic of
include/dronenav.h dn_sac_policy / dn_sac_critic_loss / dn_sac_actor_loss written as the plain torch composition in float64 on the CPU,
autograd producing every gradient -- the closed forms of the header restated in NumPy, the tolerances, and the checks the reference makes
on itself: coverage of every branch and stability under the order of the rows.

Tolerances (against the reference only, and nothing wider): a per-row float32 output is within one float32 ulp of the reference value or
2^-40 of the sum of the absolute terms of that output, whichever is larger (the single rounding to float32; near a cancellation the last
float64 bits of exp, tanh and log, which differ between libraries by a few 2^-53 of a term).  A float64 statistic is within 2^-40 of the
mean absolute term of its sum or of its value, whichever is larger (a float64 sum of B <= 2^11 terms in any order is within B 2^-53 <=
2^-42 of its mean absolute term).  A float32 loss is within one float32 ulp or the bound of its statistic.  The reference's own error, where it has
one, is added to the second bound (row_tolerance)."""
import decimal
import functools
import math

import numpy as np
import torch

from loss_support import ACT_DIMS, BATCHES, BLOCK_ROWS, COVERED_FROM, EPS40, HALF_LOG_2PI, distance, ulp32  # noqa: F401  (handed on to the tests)

CRITICS = (1, 2, 4)
GAMMAS = (0.0, 0.99)
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
LOG_EPS = 1e-6
FIXED_ENT_COEF = 0.2
TARGET_ENTROPY = -4.0


def exp_correctly_rounded(x):
    """exp of one float, rounded correctly (40 decimal digits, then one rounding): what csrc/dn_exp_cr.h gives for alpha."""
    with decimal.localcontext() as ctx:
        ctx.prec = 40
        return float(decimal.Decimal(float(x)).exp())


def _share(rng, n, frac):
    """A mask of n cells with exactly ceil(frac n) set, at drawn places: the shares the coverage checks ask for hold at every size."""
    m = np.zeros(n, bool)
    m[rng.permutation(n)[:math.ceil(frac * n)]] = True
    return m


def _frozen(d):
    for v in d.values():
        v.setflags(write=False)
    return d


# ---- data ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def policy_data(batch, act_dim):
    """mean, log_std (raw), noise, and the upstream gradients g_actions, g_log_prob, float32, made once and never written.  Of the
    elements 10 % have a raw log_std below -20, 10 % above 2, the rest in [-5, 1.5]; 10 % more have |mean| in [12, 16], with a raw log_std in [-5, -1], so that
    |pre| > 9 whatever the noise (std <= e^-1 there).  From 8 rows on: row 5 has noise 0 and mean 0 in column 0 (pre = 0 exactly), row 6 noise 0."""
    rng = np.random.default_rng(7000000 + 10 * batch + act_dim)
    n, f32 = batch * act_dim, np.float32
    low, high = _share(rng, n, 0.1), None
    rest = np.flatnonzero(~low)
    high = np.zeros(n, bool)
    high[rest[_share(rng, len(rest), 0.1 / 0.9)]] = True
    inside = ~low & ~high
    raw = np.where(low, -20.5 - 4.0 * rng.random(n), np.where(high, 2.25 + 1.5 * rng.random(n), -5.0 + 6.5 * rng.random(n)))
    far = np.zeros(n, bool)
    ins = np.flatnonzero(inside)
    far[ins[_share(rng, len(ins), 0.1 / 0.8)]] = True
    raw = np.where(far, -5.0 + 4.0 * rng.random(n), raw)
    mean = np.where(far, np.sign(rng.standard_normal(n)) * (12.0 + 4.0 * rng.random(n)), rng.standard_normal(n))
    noise = rng.standard_normal(n)
    d = dict(mean=mean.reshape(batch, act_dim).astype(f32), log_std=raw.reshape(batch, act_dim).astype(f32),
             noise=noise.reshape(batch, act_dim).astype(f32), g_actions=rng.standard_normal((batch, act_dim)).astype(f32),
             g_log_prob=rng.standard_normal(batch).astype(f32))
    if batch >= 8:
        d["noise"][5:7] = 0.0
        d["mean"][5, 0] = 0.0
    return _frozen(d)


def _with_picks(rng, batch, n_critics, scale):
    """n_critics columns of drawn values, the row's smallest placed at a critic chosen in turn (a drawn order): each critic is the min pick
    of 1 / n_critics of the rows at every size."""
    v = np.sort(scale * rng.standard_normal((batch, n_critics)), axis=1)
    pick = rng.permutation(batch) % n_critics
    out = v.copy()
    rows = np.arange(batch)
    out[rows, 0], out[rows, pick] = v[rows, pick], v[rows, 0]
    return [np.ascontiguousarray(out[:, c]).astype(np.float32) for c in range(n_critics)]


@functools.lru_cache(maxsize=None)
def loss_data(batch, n_critics):
    """The inputs of both losses, float32: q, next_q, q_pi (lists of n_critics arrays [batch]), next_log_prob, log_prob, rewards, dones (1 in
    30 % of the rows), log_ent_coef [1]."""
    rng = np.random.default_rng(9000000 + 10 * batch + n_critics)
    f32 = np.float32
    d = dict(next_log_prob=(-2.0 + 3.0 * rng.standard_normal(batch)).astype(f32), log_prob=(-2.0 + 3.0 * rng.standard_normal(batch)).astype(f32),
             rewards=rng.standard_normal(batch).astype(f32), dones=_share(rng, batch, 0.3).astype(f32),
             log_ent_coef=np.array([-1.2039728], f32))
    d["q"] = tuple((5.0 + 2.0 * rng.standard_normal(batch)).astype(f32) for _ in range(n_critics))
    d["next_q"] = tuple(_with_picks(rng, batch, n_critics, 3.0))
    d["q_pi"] = tuple(_with_picks(rng, batch, n_critics, 3.0))
    for v in d.values():
        for x in (v if isinstance(v, tuple) else (v,)):
            x.setflags(write=False)
    return d


# ---- the reference: the torch composition in float64, autograd for every gradient ---------------------------------------------------------
def squash_composition(mean, raw, eps, lo=LOG_STD_MIN, hi=LOG_STD_MAX):
    """The squashed head as include/dronenav.h states it, in the dtype and on the device of its tensors.  Returns actions, log_prob and a
    dict of what the tests read."""
    ls = torch.clamp(raw, lo, hi)
    std = torch.exp(ls)
    pre = mean + std * eps
    a = torch.tanh(pre)
    t = torch.exp(-2.0 * torch.abs(pre))
    J = 4.0 * t / ((1.0 + t) * (1.0 + t))
    terms = -0.5 * eps * eps - ls - HALF_LOG_2PI - torch.log(J + LOG_EPS)
    lp = terms[:, 0]
    for j in range(1, terms.shape[1]):                          # j ascending, as the header states it
        lp = lp + terms[:, j]
    return a, lp, dict(ls=ls, std=std, pre=pre, J=J, terms=terms)


def _t64(x, reverse=False):
    return torch.from_numpy(np.ascontiguousarray(x[::-1] if reverse else x).astype(np.float64))


def policy_reference(d, lo=LOG_STD_MIN, hi=LOG_STD_MAX, use_g_actions=True, use_g_log_prob=True, reverse=False):
    """{actions, log_prob, d_mean, d_log_std} in float64 and the absolute-term sums the tolerances read."""
    mean, raw = _t64(d["mean"], reverse).requires_grad_(), _t64(d["log_std"], reverse).requires_grad_()
    eps, g_a, g_lp = _t64(d["noise"], reverse), _t64(d["g_actions"], reverse), _t64(d["g_log_prob"], reverse)
    if not use_g_actions:
        g_a = torch.zeros_like(g_a)
    if not use_g_log_prob:
        g_lp = torch.zeros_like(g_lp)
    a, lp, m = squash_composition(mean, raw, eps, lo, hi)
    ((a * g_a).sum() + (lp * g_lp).sum()).backward()
    n = lambda x: x.detach().numpy()  # noqa: E731
    back = (lambda x: x[::-1].copy()) if reverse else (lambda x: x)
    J, std, e, aa = n(m["J"]), n(m["std"]), n(eps), n(a)
    K = 2.0 * aa * J / (J + LOG_EPS)
    ga, gl = n(g_a), n(g_lp)[:, None]
    dm_terms = np.abs(ga * J) + np.abs(gl * K)
    rawn = n(raw)
    return dict(actions=back(aa), log_prob=back(n(lp)), d_mean=back(n(mean.grad)), d_log_std=back(n(raw.grad)),
                actions_terms=back(np.abs(aa)),
                log_prob_terms=back((0.5 * e * e + np.abs(n(m["ls"])) + HALF_LOG_2PI + np.abs(np.log(J + LOG_EPS))).sum(1)),
                d_mean_terms=back(dm_terms), d_log_std_terms=back(dm_terms * np.abs(std * e) + np.abs(gl)),
                d_mean_own=back(2.0 ** -51 * np.abs(ga)), d_log_std_own=back(2.0 ** -51 * np.abs(ga) * np.abs(std * e)),
                pre=back(n(m["pre"])), J=back(J), terms=back(n(m["terms"])),
                low_share=float((rawn < lo).mean()), high_share=float((rawn > hi).mean()), inside_share=float(((rawn >= lo) & (rawn <= hi)).mean()),
                far_share=float((np.abs(n(m["pre"])) > 9.0).mean()))


def policy_closed_forms(d, lo=LOG_STD_MIN, hi=LOG_STD_MAX):
    """The hand-derived forms of include/dronenav.h in float64 NumPy: what the kernel evaluates, stated a second time."""
    f = {k: v.astype(np.float64) for k, v in d.items()}
    raw, eps = f["log_std"], f["noise"]
    ls = np.where(raw < lo, lo, np.where(raw > hi, hi, raw))
    std = np.exp(ls)
    pre = f["mean"] + std * eps
    a = np.tanh(pre)
    t = np.exp(-2.0 * np.abs(pre))
    J = 4.0 * t / ((1.0 + t) * (1.0 + t))
    terms = -0.5 * eps * eps - ls - HALF_LOG_2PI - np.log(J + LOG_EPS)
    lp = terms[:, 0].copy()
    for j in range(1, terms.shape[1]):
        lp = lp + terms[:, j]
    K = 2.0 * a * J / (J + LOG_EPS)
    d_pre = f["g_actions"] * J + f["g_log_prob"][:, None] * K
    d_ls = d_pre * std * eps - f["g_log_prob"][:, None]
    return dict(actions=a, log_prob=lp, d_mean=d_pre, d_log_std=np.where((raw >= lo) & (raw <= hi), d_ls, 0.0), J=J, terms=terms)


def _alpha(d, learned):
    return exp_correctly_rounded(float(d["log_ent_coef"][0])) if learned else FIXED_ENT_COEF


def _fsum(x):
    return math.fsum(np.asarray(x, np.float64).ravel().tolist())


def critic_reference(d, gamma, learned, reverse=False):
    """{loss, stats [3 + C], d_q [C, B], target_q} in float64, the mean absolute terms of the statistics, the absolute-term sums of the
    per-row outputs, and the shares the coverage checks read."""
    q = [_t64(x, reverse).requires_grad_() for x in d["q"]]
    nxt = torch.stack([_t64(x, reverse) for x in d["next_q"]])
    r, dn, nlp = _t64(d["rewards"], reverse), _t64(d["dones"], reverse), _t64(d["next_log_prob"], reverse)
    alpha, rows, C = _alpha(d, learned), float(len(d["rewards"])), len(q)
    nq = torch.min(nxt, dim=0).values
    y = r + (1.0 - dn) * gamma * (nq - alpha * nlp)
    loss = 0.5 * sum(((qc - y) ** 2).mean() for qc in q)
    loss.backward()
    n = lambda x: x.detach().numpy()  # noqa: E731
    back = (lambda x: x[..., ::-1].copy()) if reverse else (lambda x: x)
    sq = [_fsum(n((qc - y) ** 2)) / rows for qc in q]
    crit = sq[0]
    for c in range(1, C):
        crit = crit + sq[c]
    crit = 0.5 * crit
    y_terms = n(r.abs() + (1.0 - dn) * gamma * (nq.abs() + alpha * nlp.abs()))
    stats = np.array([crit, alpha, _fsum(n(y)) / rows] + [_fsum(n(qc)) / rows for qc in q])
    stats_terms = np.array([crit, alpha, _fsum(np.abs(n(y))) / rows] + [_fsum(np.abs(n(qc))) / rows for qc in q])
    picks = n(torch.min(nxt, dim=0).indices)
    return dict(loss=crit, torch_loss=loss.item(), stats=stats, stats_terms=stats_terms, d_q=back(np.stack([n(qc.grad) for qc in q])),
                target_q=back(n(y)), target_q_terms=back(y_terms), d_q_terms=back(np.stack([(np.abs(n(qc)) + y_terms) / rows for qc in q])),
                pick_shares=[float((picks == c).mean()) for c in range(C)], done_share=float(n(dn).mean()))


def critic_closed_forms(d, gamma, learned):
    f = lambda x: np.asarray(x, np.float64)  # noqa: E731
    alpha, rows = _alpha(d, learned), float(len(d["rewards"]))
    nq = f(d["next_q"][0]).copy()
    for x in d["next_q"][1:]:
        x = f(x)
        take = (x < nq) | (np.isnan(x) & ~np.isnan(nq))
        nq = np.where(take, x, nq)
    y = f(d["rewards"]) + (1.0 - f(d["dones"])) * gamma * (nq - alpha * f(d["next_log_prob"]))
    e = [f(qc) - y for qc in d["q"]]
    loss = np.mean(e[0] * e[0])
    for ec in e[1:]:
        loss = loss + np.mean(ec * ec)
    return dict(loss=0.5 * loss, d_q=np.stack([ec / rows for ec in e]), target_q=y,
                stats=np.array([0.5 * loss, alpha, np.mean(y)] + [np.mean(f(qc)) for qc in d["q"]]))


def actor_reference(d, learned, target_entropy=TARGET_ENTROPY, reverse=False):
    """{actor_loss, ent_coef_loss, stats [6], d_log_prob, d_q_pi [C, B], d_log_ent_coef} in float64 and the terms of the tolerances."""
    lp = _t64(d["log_prob"], reverse).requires_grad_()
    qpi = [_t64(x, reverse).requires_grad_() for x in d["q_pi"]]
    lec = torch.tensor(float(d["log_ent_coef"][0]), dtype=torch.float64, requires_grad=True)
    alpha, rows, C = _alpha(d, learned), float(len(d["log_prob"])), len(qpi)
    stacked = torch.stack(qpi)
    qmin = torch.min(stacked, dim=0)
    actor = (alpha * lp - qmin.values).mean()
    ent = -(lec * (lp + target_entropy).detach().mean()) if learned else torch.zeros((), dtype=torch.float64)
    (actor + ent).backward()
    n = lambda x: x.detach().numpy()  # noqa: E731
    back = (lambda x: x[..., ::-1].copy()) if reverse else (lambda x: x)
    lpn, qm = n(lp), n(qmin.values)
    actor_v = _fsum(alpha * lpn - qm) / rows
    m = _fsum(lpn + target_entropy) / rows
    ent_v, dlec = (-(float(lec.detach()) * m), -m) if learned else (0.0, 0.0)
    stats = np.array([actor_v, ent_v, alpha, _fsum(lpn) / rows, _fsum(qm) / rows, dlec])
    m_terms = _fsum(np.abs(lpn) + abs(target_entropy)) / rows
    stats_terms = np.array([_fsum(np.abs(alpha * lpn) + np.abs(qm)) / rows, abs(float(lec.detach())) * m_terms if learned else 0.0, alpha,
                            _fsum(np.abs(lpn)) / rows, _fsum(np.abs(qm)) / rows, m_terms if learned else 0.0])
    picks = n(qmin.indices)
    return dict(actor_loss=actor_v, ent_coef_loss=ent_v, torch_actor_loss=actor.item(), torch_ent_coef_loss=float(ent.detach()), stats=stats,
                stats_terms=stats_terms, d_log_prob=back(n(lp.grad)), d_q_pi=back(np.stack([n(x.grad) for x in qpi])),
                d_log_ent_coef=float(lec.grad) if learned else 0.0, pick_shares=[float((picks == c).mean()) for c in range(C)])


def actor_closed_forms(d, learned, target_entropy=TARGET_ENTROPY):
    """The NumPy statement, with the tie rule: the lowest c among equal values is the pick, the first NaN wins."""
    f = lambda x: np.asarray(x, np.float64)  # noqa: E731
    alpha, rows, lp = _alpha(d, learned), float(len(d["log_prob"])), f(d["log_prob"])
    qmin, pick = f(d["q_pi"][0]).copy(), np.zeros(len(lp), np.int64)
    for c, x in enumerate(d["q_pi"][1:], 1):
        x = f(x)
        take = (x < qmin) | (np.isnan(x) & ~np.isnan(qmin))
        qmin, pick = np.where(take, x, qmin), np.where(take, c, pick)
    m = np.mean(lp + target_entropy)
    lec = float(d["log_ent_coef"][0])
    actor = np.mean(alpha * lp - qmin)
    ent, dlec = (-(lec * m), -m) if learned else (0.0, 0.0)
    return dict(actor_loss=actor, ent_coef_loss=ent, d_log_prob=np.full(len(lp), alpha / rows),
                d_q_pi=np.stack([np.where(pick == c, -1.0 / rows, 0.0) for c in range(len(d["q_pi"]))]), d_log_ent_coef=dlec,
                stats=np.array([actor, ent, alpha, np.mean(lp), np.mean(qmin), dlec]))


# ---- tolerances, against the references only ------------------------------------------------------------------------------------------------
def row_tolerance(ref, key):
    """A per-row float32 output: one float32 ulp of the reference value or 2^-40 of the sum of its absolute terms, whichever is larger.
    The second bound also carries the reference's own error where it has one (`<key>_own`): torch's autograd takes d tanh / d pre as
    1 - a * a, which at a saturated element is wrong by up to 2^-51 absolutely, however small sech^2 is; times |g_actions| that is an
    error of the reference's d_mean, and times |std eps| more of its d_log_std (the kernel forms sech^2 without the cancellation)."""
    with np.errstate(invalid="ignore"):
        return np.fmax(ulp32(ref[key]), EPS40 * ref[key + "_terms"] + ref.get(key + "_own", 0.0))


def stats_tolerance(ref):
    with np.errstate(invalid="ignore"):
        return EPS40 * np.fmax(ref["stats_terms"], np.abs(ref["stats"]))


def loss_tolerance(ref, key, index):
    return float(np.fmax(ulp32(ref[key]), stats_tolerance(ref)[index]))


def _held(worst, tag, key, got, want, tol):
    dist, same = distance(got, want, tol)
    assert same, f"{tag}: {key}: the NaN cells differ from the reference's"
    assert dist <= 1.0, f"{tag}: {key} is {dist:.3f} of its tolerance from the float64 reference"
    worst[key] = dist


def check_policy(got, ref, tag, keys=("actions", "log_prob", "d_mean", "d_log_std")):
    """got: NumPy arrays under the reference's names.  Returns the largest distance per output, in units of the tolerance."""
    worst = {}
    for k in keys:
        _held(worst, tag, k, got[k], ref[k], row_tolerance(ref, k))
    return worst


def check_critic(got, ref, tag):
    """got: {loss, stats [8], d_q [C, B], target_q}."""
    worst, C = {}, len(ref["d_q"])
    _held(worst, tag, "d_q", got["d_q"], ref["d_q"], row_tolerance(ref, "d_q"))
    _held(worst, tag, "target_q", got["target_q"], ref["target_q"], row_tolerance(ref, "target_q"))
    _held(worst, tag, "stats", np.asarray(got["stats"])[:3 + C], ref["stats"], stats_tolerance(ref))
    assert (np.asarray(got["stats"])[3 + C:] == 0.0).all(), f"{tag}: the unused statistics must be 0"
    _held(worst, tag, "loss", got["loss"], ref["loss"], loss_tolerance(ref, "loss", 0))
    return worst


def check_actor(got, ref, tag, gradients=True):
    """got: {actor_loss, ent_coef_loss, stats [8], d_log_prob, d_q_pi [C, B], d_log_ent_coef}."""
    worst = {}
    if gradients:
        _held(worst, tag, "d_log_prob", got["d_log_prob"], ref["d_log_prob"], ulp32(ref["d_log_prob"]))
        _held(worst, tag, "d_q_pi", got["d_q_pi"], ref["d_q_pi"], ulp32(ref["d_q_pi"]))
    tol = stats_tolerance(ref)
    _held(worst, tag, "stats", np.asarray(got["stats"])[:6], ref["stats"], tol)
    assert (np.asarray(got["stats"])[6:] == 0.0).all(), f"{tag}: the unused statistics must be 0"
    _held(worst, tag, "actor_loss", got["actor_loss"], ref["actor_loss"], loss_tolerance(ref, "actor_loss", 0))
    _held(worst, tag, "ent_coef_loss", got["ent_coef_loss"], ref["ent_coef_loss"], loss_tolerance(ref, "ent_coef_loss", 1))
    _held(worst, tag, "d_log_ent_coef", got["d_log_ent_coef"], ref["d_log_ent_coef"], max(float(ulp32(ref["d_log_ent_coef"])), float(tol[5])))
    return worst


# ---- what the reference promises of its data ---------------------------------------------------------------------------------------------------
def check_policy_coverage(ref, tag):
    assert ref["low_share"] >= 0.05 and ref["high_share"] >= 0.05, f"{tag}: {ref['low_share']}, {ref['high_share']} of the elements clamped low, high"
    assert ref["inside_share"] >= 0.5, f"{tag}: {ref['inside_share']} of the elements inside the clamp"
    assert ref["far_share"] >= 0.05, f"{tag}: {ref['far_share']} of the elements have |pre| > 9"


def check_loss_coverage(ref, tag, dones=False):
    if len(ref["pick_shares"]) > 1:
        assert all(0.2 <= s <= 0.8 for s in ref["pick_shares"]), f"{tag}: the critics are the min pick in {ref['pick_shares']} of the rows"
    if dones:
        assert 0.1 <= ref["done_share"] <= 0.9, f"{tag}: dones is 1 in {ref['done_share']} of the rows"
