"""The SAC loss heads (include/dronenav.h dn_sac_policy, dn_sac_policy_backward, dn_sac_critic_loss, dn_sac_actor_loss; csrc/dn_sac_loss.hip,
sac.py) on the HIP path, against the float64 torch reference of tests/sac_loss_support.py within its tolerances and nothing wider.

 1. every output -- actions, log_prob, d_mean, d_log_std of the policy head; d_q, target_q, the float64 stats and the float32 loss of the
    critic loss; d_log_prob, d_q_pi, d_log_ent_coef, the stats and the two float32 losses of the actor loss -- with a learned and a fixed
    ent_coef and gamma in {0, 0.99}; each data set is first shown to meet the coverage conditions;
 2. edge values: one NaN mean element (NaN in that row only), one NaN reward (NaN in target_q and d_q of that row and in the loss),
    noise 0 and pre 0 exactly, a count below batch_size, sentinels either side of every output;
 3. the same call twice gives the same bits; eager equals graph replay bit for bit; the 16-byte path equals the 4-byte path (inputs and
    outputs moved by one word); the capture guard of the scratch;
 4. autograd: backward() into leaf inputs gives exactly the static buffers, a scaled loss scales them, backward after a later forward
    raises, actor_loss.backward() reaches mean and log_std through a torch stand-in critic;
 5. end to end: a ReplaySampler batch from a RingReplayBuffer the OffPolicyCollector filled, one full gradient step's parameter gradients
    of a small SacActor, SacCritic and log_ent_coef through the heads and through the float32 torch composition on the device, both against
    the same networks in float64 on the CPU under the reference losses.

Shapes: B in {1, 2, 63, 65, 1024, 1025, 2049} x A in {1, 3, 4, 8} for the policy head, the same B x C in {1, 2, 4} for the losses: 1025 and
2049 cross one and two boundaries of the 1024-row blocks, with a last block of one row; 63 and 65 are the wave edge; A = 4 and 8 take the
16-byte path.

Largest distances seen on an MI355X, in units of the tolerance (profiles/sac_loss_distances.txt): actions 0.5, log_prob 0.5, d_mean 0.583
(above one half where the reference's own 1 - a * a error counts, see sac_loss_support.row_tolerance), d_log_std 0.5; critic d_q 0.5,
target_q 0.5, stats 2.9e-4, loss 0.494; actor d_log_prob 0.485, d_q_pi 0.492, stats 2.5e-4, actor_loss 0.491, ent_coef_loss 0.492,
d_log_ent_coef 0.493 (the single rounding to float32).  End to end, parameter gradients against float64, of the largest gradient: 2.1e-8
through the heads and 5.3e-8 through the float32 composition."""
import copy
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import sac_loss_support as S  # noqa: E402
from gpu_support import DEV  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402

policy_shapes = pytest.mark.parametrize("batch,act_dim", [(b, a) for b in S.BATCHES for a in S.ACT_DIMS])
loss_shapes = pytest.mark.parametrize("batch,n_critics", [(b, c) for b in S.BATCHES for c in S.CRITICS])
SENTINEL = -7.0


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _np(x):
    return x.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _policy_device(batch, act_dim):
    return {k: _dev(v) for k, v in S.policy_data(batch, act_dim).items()}


@functools.lru_cache(maxsize=None)
def _loss_device(batch, n_critics):
    return {k: (tuple(_dev(x) for x in v) if isinstance(v, tuple) else _dev(v)) for k, v in S.loss_data(batch, n_critics).items()}


@functools.lru_cache(maxsize=None)
def _policy_reference(batch, act_dim, use_g_actions=True, use_g_log_prob=True):
    return S.policy_reference(S.policy_data(batch, act_dim), use_g_actions=use_g_actions, use_g_log_prob=use_g_log_prob)


@functools.lru_cache(maxsize=None)
def _critic_reference(batch, n_critics, gamma, learned):
    return S.critic_reference(S.loss_data(batch, n_critics), gamma, learned)


@functools.lru_cache(maxsize=None)
def _actor_reference(batch, n_critics, learned):
    return S.actor_reference(S.loss_data(batch, n_critics), learned)


def _guard(obj, names):
    """Replaces the static tensors `names` of obj by views with one row (or four words) of sentinels either side.  Returns the whole
    buffers; _intact checks them."""
    whole = {}
    for name in names:
        t = getattr(obj, name)
        pad = 4 if t.dim() == 1 else 1
        w = torch.full((t.shape[0] + 2 * pad,) + tuple(t.shape[1:]), SENTINEL, dtype=t.dtype, device=t.device)
        setattr(obj, name, w[pad:pad + t.shape[0]])
        assert getattr(obj, name).is_contiguous()
        whole[name] = (w, pad)
    return whole


def _intact(whole, tag):
    torch.cuda.synchronize()
    for name, (w, pad) in whole.items():
        assert bool((w[:pad] == SENTINEL).all()) and bool((w[-pad:] == SENTINEL).all()), (tag, name, "a sentinel beside the output was written")


POLICY_OUT = ("actions", "log_prob", "d_mean", "d_log_std")
CRITIC_OUT = ("d_q", "target_q", "loss", "stats")
ACTOR_OUT = ("d_log_prob", "d_q_pi", "d_log_ent_coef", "actor_loss", "ent_coef_loss", "stats")


def _run_policy(head, d, count=None, use_g_actions=True, use_g_log_prob=True):
    """Forward and backward on leaf inputs.  Returns the outputs as NumPy under the reference's names, and the leaves."""
    n = d["mean"].shape[0] if count is None else count
    mean, log_std = d["mean"][:n].clone().requires_grad_(), d["log_std"][:n].clone().requires_grad_()
    actions, log_prob = head(mean, log_std, d["noise"][:n])
    outs, grads = [], []
    if use_g_actions:
        outs.append(actions), grads.append(d["g_actions"][:n])
    if use_g_log_prob:
        outs.append(log_prob), grads.append(d["g_log_prob"][:n])
    torch.autograd.backward(outs, grads)
    torch.cuda.synchronize()
    got = dict(actions=_np(actions), log_prob=_np(log_prob), d_mean=_np(head.d_mean[:n]), d_log_std=_np(head.d_log_std[:n]))
    return got, (mean, log_std)


def _run_critic(crit, d, learned, count=None):
    n = d["rewards"].shape[0] if count is None else count
    q = [x[:n].clone().requires_grad_() for x in d["q"]]
    loss = crit(q, [x[:n] for x in d["next_q"]], d["next_log_prob"][:n], dict(rewards=d["rewards"][:n], dones=d["dones"][:n]),
                d["log_ent_coef"] if learned else None)
    loss.backward()
    torch.cuda.synchronize()
    return dict(loss=float(loss.detach()), stats=_np(crit.stats), d_q=_np(crit.d_q[:, :n]), target_q=_np(crit.target_q[:n])), q, loss


def _run_actor(act, d, learned, count=None):
    n = d["log_prob"].shape[0] if count is None else count
    lp = d["log_prob"][:n].clone().requires_grad_()
    q_pi = [x[:n].clone().requires_grad_() for x in d["q_pi"]]
    lec = d["log_ent_coef"].clone().requires_grad_() if learned else None
    actor_loss, ent_coef_loss = act(lp, q_pi, lec)
    (actor_loss + ent_coef_loss).backward()
    torch.cuda.synchronize()
    got = dict(actor_loss=float(actor_loss.detach()), ent_coef_loss=float(ent_coef_loss.detach()), stats=_np(act.stats), d_log_prob=_np(act.d_log_prob[:n]),
               d_q_pi=_np(act.d_q_pi[:, :n]), d_log_ent_coef=float(act.d_log_ent_coef) if learned else 0.0)
    return got, (lp, q_pi, lec)


def _critic(pkg, batch_size, n_critics, gamma, learned):
    return pkg.SacCriticLoss(batch_size, DEV, n_critics=n_critics, gamma=gamma, ent_coef=None if learned else S.FIXED_ENT_COEF)


def _actor(pkg, batch_size, n_critics, learned):
    return pkg.SacActorLoss(batch_size, DEV, n_critics=n_critics, target_entropy=S.TARGET_ENTROPY, ent_coef=None if learned else S.FIXED_ENT_COEF)


def _said(tag, worst):
    print(f"{tag}: largest distance from the float64 reference, in units of the tolerance: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---- 1. every output within tolerance -----------------------------------------------------------------------------------------------------
@policy_shapes
def test_policy_outputs_match_the_float64_reference(batch, act_dim):
    pkg = _pkg()
    d, ref = _policy_device(batch, act_dim), _policy_reference(batch, act_dim)
    if batch >= S.COVERED_FROM:
        S.check_policy_coverage(ref, (batch, act_dim))
    head = pkg.SacPolicyHead(batch, act_dim, DEV)
    whole = _guard(head, POLICY_OUT)
    got, (mean, log_std) = _run_policy(head, d)
    assert got["actions"].shape == (batch, act_dim) and got["log_prob"].shape == (batch,) and (np.abs(got["actions"]) <= 1.0).all()
    worst = S.check_policy(got, ref, (batch, act_dim))
    assert torch.equal(mean.grad, head.d_mean[:batch]) and torch.equal(log_std.grad, head.d_log_std[:batch])
    for flags in (dict(use_g_actions=False), dict(use_g_log_prob=False)):          # an output nobody used: a NULL gradient is zero
        got, _ = _run_policy(head, d, **flags)
        S.check_policy(got, _policy_reference(batch, act_dim, **flags), (batch, act_dim, flags))
    _intact(whole, (batch, act_dim))
    _said(f"policy B {batch}, A {act_dim}", worst)


@loss_shapes
def test_loss_outputs_match_the_float64_reference(batch, n_critics):
    pkg = _pkg()
    d = _loss_device(batch, n_critics)
    worst = {}
    for learned in (True, False):
        for gamma in S.GAMMAS:
            ref = _critic_reference(batch, n_critics, gamma, learned)
            if batch >= S.COVERED_FROM:
                S.check_loss_coverage(ref, (batch, n_critics, "critic"), dones=True)
            crit = _critic(pkg, batch, n_critics, gamma, learned)
            whole = _guard(crit, CRITIC_OUT)
            got, q, loss = _run_critic(crit, d, learned)
            assert loss.shape == () and loss.dtype == torch.float32
            for k, v in S.check_critic(got, ref, (batch, n_critics, gamma, learned)).items():
                worst["critic " + k] = max(worst.get("critic " + k, 0.0), v)
            names = crit.stats_dict()
            assert list(names) == ["critic_loss", "ent_coef", "target_q_mean"] + [f"q_mean_{c}" for c in range(n_critics)]
            assert list(names.values()) == got["stats"][:3 + n_critics].tolist()
            _intact(whole, (batch, n_critics, "critic"))
        ref = _actor_reference(batch, n_critics, learned)
        if batch >= S.COVERED_FROM:
            S.check_loss_coverage(ref, (batch, n_critics, "actor"))
        act = _actor(pkg, batch, n_critics, learned)
        whole = _guard(act, ACTOR_OUT)
        got, _ = _run_actor(act, d, learned)
        for k, v in S.check_actor(got, ref, (batch, n_critics, learned)).items():
            worst["actor " + k] = max(worst.get("actor " + k, 0.0), v)
        names = act.stats_dict()
        assert list(names) == ["actor_loss", "ent_coef_loss", "ent_coef", "log_prob_mean", "q_pi_min_mean"] and list(names.values()) == got["stats"][:5].tolist()
        if not learned:
            assert got["ent_coef_loss"] == 0.0 and got["stats"][1] == 0.0 and got["stats"][5] == 0.0 and float(act.d_log_ent_coef) == SENTINEL
        _intact(whole, (batch, n_critics, "actor"))
    _said(f"losses B {batch}, C {n_critics}", worst)


# ---- 2. edge values -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,act_dim", [(65, 3), (1025, 4), (2049, 8)])
def test_one_nan_mean_element_and_exact_zeros(batch, act_dim):
    pkg = _pkg()
    host = {k: v.copy() for k, v in S.policy_data(batch, act_dim).items()}
    head = pkg.SacPolicyHead(batch, act_dim, DEV)
    got, _ = _run_policy(head, _policy_device(batch, act_dim))
    assert got["actions"][5, 0] == 0.0 and np.isfinite(got["log_prob"][5:7]).all()           # pre = 0 exactly; noise 0 in rows 5 and 6
    want = np.tanh(host["mean"][6].astype(np.float64))          # noise 0: the action is tanh(mean)
    assert (np.abs(got["actions"][6] - want) <= S.ulp32(want)).all()
    for row in sorted({0, batch // 2, batch - 1}):
        host["mean"] = S.policy_data(batch, act_dim)["mean"].copy()
        host["mean"][row, act_dim - 1] = np.nan
        got, _ = _run_policy(head, {k: _dev(v) for k, v in host.items()})
        assert np.isnan(got["log_prob"][row]) and np.isfinite(np.delete(got["log_prob"], row)).all()
        bad = np.isnan(got["actions"])
        assert bad[row, act_dim - 1] and bad.sum() == 1
        assert np.isnan(got["d_mean"][row, act_dim - 1]) and np.isfinite(np.delete(got["d_mean"], row, axis=0)).all()
        assert np.isfinite(np.delete(got["d_log_std"], row, axis=0)).all()
        S.check_policy(got, S.policy_reference(host), (batch, act_dim, "NaN mean in row", row))


@pytest.mark.parametrize("batch,n_critics", [(65, 1), (1025, 2), (2049, 4)])
def test_one_nan_reward(batch, n_critics):
    pkg = _pkg()
    crit = _critic(pkg, batch, n_critics, 0.99, True)
    for row in sorted({0, batch // 2, batch - 1}):
        host = {k: (v if isinstance(v, tuple) else v.copy()) for k, v in S.loss_data(batch, n_critics).items()}
        host["rewards"][row] = np.nan
        got, _, _ = _run_critic(crit, dict(_loss_device(batch, n_critics), rewards=_dev(host["rewards"])), True)
        assert np.isnan(got["loss"]) and np.isnan(got["stats"][0]) and np.isnan(got["stats"][2]) and np.isfinite(got["stats"][3:]).all()
        assert np.isnan(got["target_q"][row]) and np.isfinite(np.delete(got["target_q"], row)).all()
        assert np.isnan(got["d_q"][:, row]).all() and np.isfinite(np.delete(got["d_q"], row, axis=1)).all()
        S.check_critic(got, S.critic_reference(host, 0.99, True), (batch, n_critics, "NaN reward in row", row))


def test_a_tie_of_q_pi_picks_the_lowest_critic():
    """Against the NumPy statement only: torch splits the gradient of a tie, the header gives it to the lowest c."""
    pkg = _pkg()
    host = {k: (tuple(x.copy() for x in v) if isinstance(v, tuple) else v.copy()) for k, v in S.loss_data(65, 4).items()}
    host["q_pi"][2][::2] = host["q_pi"][1][::2]                 # critics 1 and 2 tie in every other row
    host["q_pi"][3][:] = np.minimum(host["q_pi"][3], host["q_pi"][0])
    forms = S.actor_closed_forms(host, True)
    act = _actor(pkg, 65, 4, True)
    got, _ = _run_actor(act, dict(_loss_device(65, 4), q_pi=tuple(_dev(x) for x in host["q_pi"])), True)
    assert np.array_equal(got["d_q_pi"], forms["d_q_pi"].astype(np.float32))
    assert (forms["d_q_pi"] != 0.0).sum(0).tolist() == [1] * 65


@pytest.mark.parametrize("act_dim,n_critics", [(3, 1), (4, 2), (8, 4)])
def test_a_count_below_batch_size_leaves_later_rows_alone(act_dim, n_critics):
    pkg = _pkg()
    head, crit, act = pkg.SacPolicyHead(2049, act_dim, DEV), _critic(pkg, 2049, n_critics, 0.99, True), _actor(pkg, 2049, n_critics, True)
    for obj, names in ((head, POLICY_OUT), (crit, ("d_q", "target_q")), (act, ("d_log_prob", "d_q_pi"))):
        for name in names:
            getattr(obj, name).fill_(SENTINEL)
    for count in (1025, 65, 1):
        got, _ = _run_policy(head, _policy_device(count, act_dim))
        S.check_policy(got, _policy_reference(count, act_dim), (count, act_dim, "of 2049"))
        got, _, _ = _run_critic(crit, _loss_device(count, n_critics), True)
        S.check_critic(got, _critic_reference(count, n_critics, 0.99, True), (count, n_critics, "of 2049"))
        got, _ = _run_actor(act, _loss_device(count, n_critics), True)
        S.check_actor(got, _actor_reference(count, n_critics, True), (count, n_critics, "of 2049"))
    for t in (head.actions, head.log_prob, head.d_mean, head.d_log_std, crit.target_q, act.d_log_prob):
        assert bool((t[1025:] == SENTINEL).all())
    assert bool((crit.d_q[:, 1025:] == SENTINEL).all()) and bool((act.d_q_pi[:, 1025:] == SENTINEL).all())


# ---- 3. reproducible ------------------------------------------------------------------------------------------------------------------------
def _bits(obj, names):
    torch.cuda.synchronize()
    return [getattr(obj, n).clone().view(torch.int32 if getattr(obj, n).dtype == torch.float32 else torch.int64) for n in names]


def _poison(obj, names):
    for n in names:
        t = getattr(obj, n)
        t.view(torch.int32).fill_(0x7FC12345) if t.dtype == torch.float32 else t.fill_(float("nan"))
    if obj._scratch is not None:
        obj._scratch.fill_(float("nan"))


def _same_bits(a, b, names, tag):
    for name, x, y in zip(names, a, b):
        assert torch.equal(x, y), (tag, name)


@pytest.mark.parametrize("batch,act_dim,n_critics", [(2049, 4, 2), (1025, 3, 4), (65, 8, 1)])
def test_the_same_call_twice_gives_the_same_bits(batch, act_dim, n_critics):
    pkg = _pkg()
    head, crit, act = pkg.SacPolicyHead(batch, act_dim, DEV), _critic(pkg, batch, n_critics, 0.99, True), _actor(pkg, batch, n_critics, True)
    runs = ((head, POLICY_OUT, lambda: _run_policy(head, _policy_device(batch, act_dim))),
            (crit, CRITIC_OUT, lambda: _run_critic(crit, _loss_device(batch, n_critics), True)),
            (act, ACTOR_OUT, lambda: _run_actor(act, _loss_device(batch, n_critics), True)))
    for obj, names, run in runs:
        run()
        first = _bits(obj, names)
        _poison(obj, names)
        run()
        _same_bits(first, _bits(obj, names), names, (batch, type(obj).__name__))


def _captured(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # autograd's warm-up on the side stream, as torch asks before a capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph


@pytest.mark.parametrize("batch,act_dim,n_critics", [(2049, 4, 2), (1025, 3, 4)])
def test_eager_equals_graph_replay(batch, act_dim, n_critics):
    """Forward and backward of all three heads captured on one stream and replayed: the buffers, the losses and the leaf gradients are the
    eager call's bits."""
    pkg = _pkg()
    p, d = _policy_device(batch, act_dim), _loss_device(batch, n_critics)
    head, crit, act = pkg.SacPolicyHead(batch, act_dim, DEV), _critic(pkg, batch, n_critics, 0.99, True), _actor(pkg, batch, n_critics, True)
    mean, log_std, lp = p["mean"].clone().requires_grad_(), p["log_std"].clone().requires_grad_(), d["log_prob"].clone().requires_grad_()
    q, q_pi = [x.clone().requires_grad_() for x in d["q"]], [x.clone().requires_grad_() for x in d["q_pi"]]
    lec = d["log_ent_coef"].clone().requires_grad_()
    leaves = [mean, log_std, lp, lec] + q + q_pi
    objs = ((head, POLICY_OUT), (crit, CRITIC_OUT), (act, ACTOR_OUT))

    def step():
        for t in leaves:
            t.grad = None
        actions, log_prob = head(mean, log_std, p["noise"])
        torch.autograd.backward([actions, log_prob], [p["g_actions"], p["g_log_prob"]])
        crit(q, list(d["next_q"]), d["next_log_prob"], dict(rewards=d["rewards"], dones=d["dones"]), lec).backward()
        actor_loss, ent_coef_loss = act(lp, q_pi, lec)
        (actor_loss + ent_coef_loss).backward()

    step()                                                      # the scratch is made outside the capture
    torch.cuda.synchronize()
    eager = [_bits(o, names) for o, names in objs] + [[t.grad.clone() for t in leaves]]
    graph = _captured(step)
    grads = [t.grad for t in leaves]
    for o, names in objs:
        _poison(o, names)
    for g in grads:
        g.zero_()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for (o, names), want in zip(objs, eager):
            _same_bits(want, _bits(o, names), names, (batch, type(o).__name__, "replay"))
        for i, (x, y) in enumerate(zip(eager[-1], grads)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), ("leaf gradient", i)


def test_the_scratch_cannot_grow_inside_a_capture():
    pkg = _pkg()
    d = _loss_device(65, 2)
    for obj, run, ref_check in ((_critic(pkg, 65, 2, 0.99, True), _run_critic, lambda got: S.check_critic(got[0], _critic_reference(65, 2, 0.99, True), "after")),
                                (_actor(pkg, 65, 2, True), _run_actor, lambda got: S.check_actor(got[0], _actor_reference(65, 2, True), "after"))):
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match=type(obj).__name__ + ": the scratch would have to grow inside a graph capture"):
            with torch.cuda.graph(graph):
                run(obj, d, True)
        torch.cuda.synchronize()
        ref_check(run(obj, d, True))                            # and the object works afterwards


@pytest.mark.parametrize("batch,act_dim", [(1025, 4), (2049, 8), (63, 4)])
def test_the_16_byte_path_gives_the_bits_of_the_4_byte_path(batch, act_dim):
    """A = 4 and 8 on 16-byte-aligned tensors take 16-byte words; the same values behind any of the [batch, A] tensors moved by one 4-byte
    word take the 4-byte path."""
    pkg = _pkg()
    d = _policy_device(batch, act_dim)
    head = pkg.SacPolicyHead(batch, act_dim, DEV)
    assert all(d[k].data_ptr() % 16 == 0 for k in ("mean", "log_std", "noise", "g_actions"))
    assert all(getattr(head, k).data_ptr() % 16 == 0 for k in ("actions", "d_mean", "d_log_std"))
    _run_policy(head, d)
    aligned = _bits(head, POLICY_OUT)

    def moved(x):
        return torch.empty(x.numel() + 1, dtype=x.dtype, device=DEV)[1:].view(x.shape).copy_(x)
    for which in ("mean", "log_std", "noise", "g_actions", "actions", "d_mean", "d_log_std", "all"):
        dd = {k: (moved(v) if which in (k, "all") and v.dim() == 2 else v) for k, v in d.items()}
        h = pkg.SacPolicyHead(batch, act_dim, DEV)
        for k in ("actions", "d_mean", "d_log_std"):
            if which in (k, "all"):
                setattr(h, k, moved(getattr(h, k)))
                assert getattr(h, k).data_ptr() % 16 == 4 and getattr(h, k).is_contiguous()
        _run_policy(h, dd)
        _same_bits(aligned, _bits(h, POLICY_OUT), POLICY_OUT, (batch, act_dim, which, "moved by one word"))


# ---- 4. autograd ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,act_dim,n_critics", [(65, 3, 1), (1025, 4, 2)])
def test_backward_hands_on_the_static_buffers(batch, act_dim, n_critics):
    pkg = _pkg()
    p, d = _policy_device(batch, act_dim), _loss_device(batch, n_critics)
    head, crit, act = pkg.SacPolicyHead(2049, act_dim, DEV), _critic(pkg, 2049, n_critics, 0.99, True), _actor(pkg, 2049, n_critics, True)
    _, (mean, log_std) = _run_policy(head, p)
    assert torch.equal(mean.grad, head.d_mean[:batch]) and torch.equal(log_std.grad, head.d_log_std[:batch])
    assert mean.grad.data_ptr() != head.d_mean.data_ptr()      # a copy: the next call may overwrite the buffer, not the leaf's gradient
    for scale in (1.0, 3.0):
        q = [x.clone().requires_grad_() for x in d["q"]]
        q[0] = q[0].detach().view(batch, 1).requires_grad_()   # a critic's [count, 1] output is taken as it is
        loss = crit(q, list(d["next_q"]), d["next_log_prob"], d, d["log_ent_coef"])
        assert loss.requires_grad
        (loss * scale).backward()
        for c in range(n_critics):
            assert q[c].grad.shape == q[c].shape and torch.equal(q[c].grad.view(-1), crit.d_q[c, :batch] * scale), (c, scale)
        lp, q_pi, lec = d["log_prob"].clone().requires_grad_(), [x.clone().requires_grad_() for x in d["q_pi"]], d["log_ent_coef"].clone().requires_grad_()
        actor_loss, ent_coef_loss = act(lp, q_pi, lec)
        (scale * actor_loss + 2.0 * scale * ent_coef_loss).backward()
        assert torch.equal(lp.grad, act.d_log_prob[:batch] * scale) and torch.equal(lec.grad, act.d_log_ent_coef * (2.0 * scale))
        for c in range(n_critics):
            assert torch.equal(q_pi[c].grad, act.d_q_pi[c, :batch] * scale), (c, scale)
    # one of the two losses alone: the other's inputs get no gradient
    lp, lec = d["log_prob"].clone().requires_grad_(), d["log_ent_coef"].clone().requires_grad_()
    actor_loss, ent_coef_loss = act(lp, list(d["q_pi"]), lec)
    ent_coef_loss.backward()
    assert lp.grad is None and torch.equal(lec.grad, act.d_log_ent_coef)
    # no input asks for a gradient: plain tensors
    assert not crit(list(d["q"]), list(d["next_q"]), d["next_log_prob"], d, d["log_ent_coef"]).requires_grad
    assert not head(p["mean"], p["log_std"], p["noise"])[0].requires_grad
    fixed = _actor(pkg, batch, n_critics, False)
    lp = d["log_prob"].clone().requires_grad_()
    actor_loss, ent_coef_loss = fixed(lp, list(d["q_pi"]))
    assert actor_loss.requires_grad and not ent_coef_loss.requires_grad


def test_backward_after_a_later_forward_raises():
    pkg = _pkg()
    p, d = _policy_device(65, 4), _loss_device(65, 2)
    head, crit, act = pkg.SacPolicyHead(65, 4, DEV), _critic(pkg, 65, 2, 0.99, True), _actor(pkg, 65, 2, True)
    mean = p["mean"].clone().requires_grad_()
    first = head(mean, p["log_std"], p["noise"])[1].sum()
    second = head(mean, p["log_std"], p["noise"])[1].sum()
    with pytest.raises(RuntimeError, match="SacPolicyHead: backward of call 1 after call 2"):
        first.backward()
    second.backward()                                           # the later one is still good
    assert torch.equal(mean.grad, head.d_mean[:65])
    q = [x.clone().requires_grad_() for x in d["q"]]
    first = crit(q, list(d["next_q"]), d["next_log_prob"], d, d["log_ent_coef"])
    crit(q, list(d["next_q"]), d["next_log_prob"], d, d["log_ent_coef"])
    with pytest.raises(RuntimeError, match="SacCriticLoss: backward of call 1 after call 2"):
        first.backward()
    lp = d["log_prob"].clone().requires_grad_()
    first = act(lp, list(d["q_pi"]), d["log_ent_coef"])[0]
    act(lp, list(d["q_pi"]), d["log_ent_coef"])
    with pytest.raises(RuntimeError, match="SacActorLoss: backward of call 1 after call 2"):
        first.backward()


def test_the_pieces_chain_through_a_stand_in_critic():
    """actor_loss.backward() reaches mean and log_std: through log_prob directly, and through q_pi = a linear stand-in critic of the
    actions.  The same chain in float64 torch gives the reference."""
    pkg = _pkg()
    batch, A = 1025, 4
    p = _policy_device(batch, A)
    w = [torch.tensor(v, device=DEV) for v in ([0.5, -1.0, 2.0, 0.25], [-0.75, 1.5, 0.5, -2.0])]
    head, act = pkg.SacPolicyHead(batch, A, DEV), _actor(pkg, batch, 2, False)
    mean, log_std = p["mean"].clone().requires_grad_(), p["log_std"].clone().requires_grad_()
    actions, log_prob = head(mean, log_std, p["noise"])
    actor_loss, _ = act(log_prob, [actions @ w[0], actions @ w[1]])
    actor_loss.backward()
    host = S.policy_data(batch, A)
    m64, r64 = (torch.from_numpy(host[k].astype(np.float64)).requires_grad_() for k in ("mean", "log_std"))
    a64, lp64, _ = S.squash_composition(m64, r64, torch.from_numpy(host["noise"].astype(np.float64)))
    q64 = torch.stack([a64 @ x.double().cpu() for x in w])
    (S.FIXED_ENT_COEF * lp64 - q64.min(0).values).mean().backward()
    for name, got, want in (("mean", mean.grad, m64.grad), ("log_std", log_std.grad, r64.grad)):
        err = float((got.double().cpu() - want).abs().max()) / float(want.abs().max())
        # the upstream gradients and the outputs are float32: 2^-24 each for g_actions, g_log_prob and the output, of terms no larger than a
        # few times the largest gradient
        assert err <= 1e-6, (name, err)
    assert bool((log_std.grad[(p["log_std"] < S.LOG_STD_MIN) | (p["log_std"] > S.LOG_STD_MAX)] == 0.0).all())


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------------------
def _sb3_step(actor, critic, target, lec, batch, eps, eps_n, gamma, target_entropy, squash):
    """SB3's SAC.train body [from recall] in the precision of the networks: (critic_loss, actor_loss, ent_coef_loss)."""
    obs, next_obs = batch["obs"], batch["next_obs"]
    z = actor.latent_pi(obs)
    a_pi, lp = squash(actor.mu(z), actor.log_std(z), eps)
    ent_coef = torch.exp(lec.detach())
    ent_coef_loss = -(lec * (lp + target_entropy).detach()).mean()
    with torch.no_grad():
        zn = actor.latent_pi(next_obs)
        a_n, lp_n = squash(actor.mu(zn), actor.log_std(zn), eps_n)
        nq = torch.min(torch.stack(target(next_obs, a_n)), dim=0).values
        y = batch["rewards"] + (1.0 - batch["dones"]) * gamma * (nq - ent_coef * lp_n)
    critic_loss = 0.5 * sum(((q - y) ** 2).mean() for q in critic(obs, batch["actions"]))
    actor_loss = (ent_coef * lp - torch.min(torch.stack(critic(obs, a_pi)), dim=0).values).mean()
    return critic_loss, actor_loss, ent_coef_loss


def _literal_squash(mean, raw, eps):
    from drl_dronenavigation_amd.policy import LOG_STD_MAX, LOG_STD_MIN, SacActor
    return SacActor.squash(mean, torch.clamp(raw, LOG_STD_MIN, LOG_STD_MAX), eps)


def _reference_squash(mean, raw, eps):
    return S.squash_composition(mean, raw, eps)[:2]


def _gradients(losses, actor, critic, lec):
    critic_loss, actor_loss, ent_coef_loss = losses
    g = list(torch.autograd.grad(critic_loss, list(critic.parameters())))
    g += list(torch.autograd.grad(actor_loss + ent_coef_loss, list(actor.parameters()) + [lec]))
    return [x.detach().double().cpu().clone() for x in g]


def test_end_to_end_one_gradient_step():
    """A small SacActor (13-32-32) and SacCritic (32-32, C = 2) on a ReplaySampler batch from the ring an OffPolicyCollector filled: the
    parameter gradients of the critics, the actor and log_ent_coef (a) through the heads, (b) through the float32 torch composition on the
    device (SacActor.squash and SB3's expressions), (c) with the same networks in float64 on the CPU under the reference losses.  The
    distance of (a) from (c), over the largest gradient, is at most twice that of (b): both share the float32 networks' rounding, and the
    heads can only remove error."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    from drl_dronenavigation_amd.collector import OffPolicyCollector, RingReplayBuffer
    n, T, B, gamma, target_entropy = 256, 4, 256, 0.99, -4.0
    env = pkg.DroneVecEnv(tracks.reaching(), n, device=DEV, max_steps=3, normalize_obs=False, act_noise_sigma=0.002, obs_noise_sigma=0.01, seed=9)
    torch.manual_seed(0)
    col = OffPolicyCollector(env, pkg.FusedSacActor(pkg.SacActor().to(DEV), n, DEV, grade="fp32"), buffer_size=T, seed=2)
    buf = col.collect_cycle()
    assert isinstance(buf, RingReplayBuffer) and buf.full
    batch = {k: v.clone() for k, v in pkg.ReplaySampler(buf, B, seed=3).sample().items()}
    torch.cuda.synchronize()
    env.close()
    assert all(bool(torch.isfinite(batch[k]).all()) for k in ("obs", "next_obs", "actions", "rewards", "dones"))

    torch.manual_seed(7)
    actor, critic = pkg.SacActor(pi=(32, 32)).to(DEV), pkg.SacCritic(qf=(32, 32), n_critics=2).to(DEV)
    target = copy.deepcopy(critic)
    with torch.no_grad():
        for prm in target.parameters():
            prm.mul_(0.9)
    lec = torch.log(torch.full((1,), 0.3, device=DEV)).requires_grad_()
    eps, eps_n = torch.randn(B, 4, device=DEV), torch.randn(B, 4, device=DEV)

    head, head_n = pkg.SacPolicyHead(B, 4, DEV), pkg.SacPolicyHead(B, 4, DEV)
    crit = pkg.SacCriticLoss(B, DEV, n_critics=2, gamma=gamma)
    act = pkg.SacActorLoss(B, DEV, n_critics=2, target_entropy=target_entropy)
    obs, next_obs = batch["obs"], batch["next_obs"]
    z = actor.latent_pi(obs)
    a_pi, lp = head(actor.mu(z), actor.log_std(z), eps)
    with torch.no_grad():
        zn = actor.latent_pi(next_obs)
        a_n, lp_n = head_n(actor.mu(zn), actor.log_std(zn), eps_n)
        next_q = target(next_obs, a_n)
    critic_loss = crit(list(critic(obs, batch["actions"])), list(next_q), lp_n, batch, lec)
    actor_loss, ent_coef_loss = act(lp, list(critic(obs, a_pi)), lec)
    a = _gradients((critic_loss, actor_loss, ent_coef_loss), actor, critic, lec)
    b = _gradients(_sb3_step(actor, critic, target, lec, batch, eps, eps_n, gamma, target_entropy, _literal_squash), actor, critic, lec)
    cpu = lambda m: copy.deepcopy(m).double().cpu()  # noqa: E731
    actor64, critic64, target64 = cpu(actor), cpu(critic), cpu(target)
    lec64 = lec.detach().double().cpu().requires_grad_()
    batch64 = {k: v.double().cpu() for k, v in batch.items() if k != "indices"}
    c = _gradients(_sb3_step(actor64, critic64, target64, lec64, batch64, eps.double().cpu(), eps_n.double().cpu(), gamma, target_entropy,
                             _reference_squash), actor64, critic64, lec64)
    top = max(float(g.abs().max()) for g in c)
    err_a = max(float((x - z).abs().max()) for x, z in zip(a, c)) / top
    err_b = max(float((y - z).abs().max()) for y, z in zip(b, c)) / top
    print(f"SAC step: parameter gradients against float64: through the heads {err_a:.3e}, through the float32 composition {err_b:.3e} of the largest")
    assert top > 0.0 and all(bool(torch.isfinite(g).all()) for g in a + b + c)
    assert err_a <= 2.0 * err_b, (err_a, err_b)
    stats = dict(crit.stats_dict(), **act.stats_dict())
    assert all(np.isfinite(v) for v in stats.values()) and abs(stats["ent_coef"] - 0.3) < 1e-6, stats
