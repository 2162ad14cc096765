"""The PPO loss head (include/dronenav.h dn_ppo_loss, csrc/dn_ppo_loss.hip, ppo.py) on the HIP path, against the float64 torch reference
of tests/ppo_loss_support.py within its tolerances() and nothing wider.

 1. every output -- d_mean, d_value, log_probs, d_log_std, the float64 stats, the float32 loss -- for the three data sets (first epoch,
    near, far), the value clip off and on, ent_coef / vf_coef both zero and both nonzero; each data set is first shown to exercise both
    branches of its clamps;
 2. edge values: all advantages zero (policy gradients of value 0, a finite loss), one NaN advantage (NaN where the reference has NaN, that
    row only), B = 1, and a count below batch_size;
 3. the same call twice gives the same bits; eager equals graph replay bit for bit; the capture guard of the scratch; the 16-byte path
    equals the 4-byte path (inputs and d_mean moved by one word);
 4. autograd: loss.backward() into leaf mean, log_std and values gives exactly the static buffers, (3 loss).backward() three times them,
    backward after a second forward raises;
 5. end to end with the sampler and both collectors: parameter gradients of a small MlpActorCritic through PpoLoss and through the float32
    torch composition on the device, both against the same network in float64 on the CPU with the reference loss.

Shapes: B in {1, 2, 63, 65, 1024, 1025, 2049} x A in {1, 3, 4, 8}: 1025 and 2049 cross one and two boundaries of the 1024-row blocks, with
a last block of one row; 63 and 65 are the wave edge; A = 4 and 8 take the 16-byte path.

Largest distances seen on an MI355X, in units of the tolerance: d_mean 0.5, d_value 0.5, log_probs 0.5, d_log_std 0.499, loss 0.498 (the
single rounding to float32), stats 0.0057.  End to end, parameter gradients against float64, of the largest gradient: RolloutCollector
8.7e-8 through PpoLoss and 2.6e-7 through the float32 composition; FusedRolloutCollector 9.0e-8 and 2.7e-7."""
import copy
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import ppo_loss_support as P  # noqa: E402
from gpu_support import DEV  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402
from model_support import NOISE  # noqa: E402

shapes = pytest.mark.parametrize("batch,act_dim", [(b, a) for b in P.BATCHES for a in P.ACT_DIMS])
VARIANTS = [(vc, co) for vc in (False, True) for co in P.COEFS]
MB_KEYS = dict(actions="actions", log_probs="old_log_prob", advantages="advantages", returns="returns", values="old_values")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def _device_data(batch, act_dim, spread):
    """(mean, log_std, values, the minibatch dict) of one data set on the device, made once and never written."""
    d = P.data(batch, act_dim, spread)
    return _dev(d["mean"]), _dev(d["log_std"]), _dev(d["values"]), {k: _dev(d[v]) for k, v in MB_KEYS.items()}


@functools.lru_cache(maxsize=None)
def _reference(batch, act_dim, spread, value_clip, coefs):
    return P.reference(P.data(batch, act_dim, spread), clip_range_vf=P.CLIP_RANGE_VF if value_clip else None, ent_coef=coefs[0], vf_coef=coefs[1])


def _make(pkg, batch_size, act_dim, value_clip, coefs):
    return pkg.PpoLoss(batch_size, act_dim, DEV, clip_range=P.CLIP_RANGE, clip_range_vf=P.CLIP_RANGE_VF if value_clip else None,
                       ent_coef=coefs[0], vf_coef=coefs[1])


def _outputs(ppo, loss, count):
    """The outputs of the last call as NumPy, in the reference's names."""
    torch.cuda.synchronize()
    return dict(loss=float(loss.detach()), stats=ppo.stats.cpu().numpy(), d_mean=ppo.d_mean[:count].cpu().numpy(), d_log_std=ppo.d_log_std.cpu().numpy(),
                d_value=ppo.d_value[:count].cpu().numpy(), log_probs=ppo.log_probs[:count].cpu().numpy())


def _bits(ppo, count):
    torch.cuda.synchronize()
    return [t.clone().view(torch.int32 if t.dtype == torch.float32 else torch.int64)
            for t in (ppo.d_mean[:count], ppo.d_log_std, ppo.d_value[:count], ppo.log_probs[:count], ppo.loss, ppo.stats)]


def _same_bits(a, b, tag):
    for name, x, y in zip(("d_mean", "d_log_std", "d_value", "log_probs", "loss", "stats"), a, b):
        assert torch.equal(x, y), (tag, name)


# ---- 1. every output within tolerance -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", list(P.SPREADS))
@shapes
def test_outputs_match_the_float64_reference(batch, act_dim, spread):
    pkg = _pkg()
    mean, log_std, values, mb = _device_data(batch, act_dim, spread)
    worst = {}
    for value_clip, coefs in VARIANTS:
        ref = _reference(batch, act_dim, spread, value_clip, coefs)
        if batch >= P.COVERED_FROM:
            P.check_coverage(ref, spread, value_clip, (batch, act_dim, spread))
        ppo = _make(pkg, batch, act_dim, value_clip, coefs)
        loss = ppo(mean, log_std, values, mb)
        assert loss.shape == () and loss.dtype == torch.float32 and loss.device == ppo.device
        got = _outputs(ppo, loss, batch)
        assert (got["stats"][6:] == 0.0).all()
        names = ppo.stats_dict()
        assert list(names) == ["loss", "policy_gradient_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction"]
        assert list(names.values()) == got["stats"][:6].tolist()
        for k, v in P.check_outputs(got, ref, (batch, act_dim, spread, value_clip, coefs)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"B {batch}, A {act_dim}, {spread}: largest distance from the float64 reference, in units of the tolerance: "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---- 2. edge values -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,act_dim", [(1, 4), (65, 3), (1025, 4), (2049, 8)])
def test_zero_advantages_and_one_nan_advantage(batch, act_dim):
    pkg = _pkg()
    host = {k: v.copy() for k, v in P.data(batch, act_dim, "near").items()}
    mean, log_std, values, mb = _device_data(batch, act_dim, "near")
    ppo = _make(pkg, batch, act_dim, True, (0.0, 0.5))
    kw = dict(clip_range_vf=P.CLIP_RANGE_VF, ent_coef=0.0, vf_coef=0.5)

    host["advantages"][:] = 0.0
    loss = ppo(mean, log_std, values, dict(mb, advantages=_dev(host["advantages"])))
    got = _outputs(ppo, loss, batch)
    assert (got["d_mean"] == 0.0).all() and (got["d_log_std"] == 0.0).all() and np.isfinite(got["loss"]) and got["stats"][1] == 0.0
    P.check_outputs(got, P.reference(host, **kw), (batch, act_dim, "zero advantages"))

    for row in sorted({0, batch // 2, batch - 1}):              # the first lane, a middle one, the last row of the last block
        host["advantages"] = P.data(batch, act_dim, "near")["advantages"].copy()
        host["advantages"][row] = np.nan
        loss = ppo(mean, log_std, values, dict(mb, advantages=_dev(host["advantages"])))
        got = _outputs(ppo, loss, batch)
        assert np.isnan(got["loss"]) and np.isnan(got["stats"][:2]).all() and np.isfinite(got["stats"][2:]).all()
        assert np.isnan(got["d_log_std"]).all() and np.isfinite(got["d_value"]).all() and np.isfinite(got["log_probs"]).all()
        bad = np.isnan(got["d_mean"])
        assert bad[row].all() and not np.delete(bad, row, axis=0).any(), (batch, act_dim, row)
        P.check_outputs(got, P.reference(host, **kw), (batch, act_dim, "NaN advantage in row", row))


@pytest.mark.parametrize("act_dim", P.ACT_DIMS)
def test_a_short_last_minibatch(act_dim):
    """count < batch_size: the first `count` rows of the static tensors are the reference's, the rows beyond them are left alone."""
    pkg = _pkg()
    ppo = _make(pkg, 2049, act_dim, True, (0.01, 0.5))
    for t in (ppo.d_mean, ppo.d_value, ppo.log_probs):
        t.fill_(-7.0)
    for count in (1025, 65, 1):
        mean, log_std, values, mb = _device_data(count, act_dim, "far")
        loss = ppo(mean, log_std, values, mb)
        P.check_outputs(_outputs(ppo, loss, count), _reference(count, act_dim, "far", True, (0.01, 0.5)), (count, act_dim, "of 2049"))
    assert bool((ppo.d_mean[1025:] == -7.0).all()) and bool((ppo.d_value[1025:] == -7.0).all()) and bool((ppo.log_probs[1025:] == -7.0).all())


# ---- 3. reproducible ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,act_dim", [(2049, 4), (1025, 3), (65, 8)])
def test_the_same_call_twice_gives_the_same_bits(batch, act_dim):
    pkg = _pkg()
    mean, log_std, values, mb = _device_data(batch, act_dim, "near")
    ppo = _make(pkg, batch, act_dim, True, (0.01, 0.5))
    ppo(mean, log_std, values, mb)
    first = _bits(ppo, batch)
    for t in (ppo.d_mean, ppo.d_log_std, ppo.d_value, ppo.log_probs, ppo.loss):
        t.view(torch.int32).fill_(0x7FC12345)
    ppo.stats.fill_(float("nan"))
    ppo._scratch.fill_(float("nan"))
    ppo(mean, log_std, values, mb)
    _same_bits(first, _bits(ppo, batch), (batch, act_dim))


@pytest.mark.parametrize("batch,act_dim", [(2049, 4), (1025, 3)])
def test_eager_equals_graph_replay(batch, act_dim):
    """Forward and backward captured on one stream and replayed: the buffers, the loss and the leaf gradients are the eager call's bits."""
    pkg = _pkg()
    mean0, log_std0, values0, mb = _device_data(batch, act_dim, "far")
    mean, log_std, values = (t.clone().requires_grad_() for t in (mean0, log_std0, values0))
    ppo = _make(pkg, batch, act_dim, True, (0.01, 0.5))

    def step():
        for t in (mean, log_std, values):
            t.grad = None
        loss = ppo(mean, log_std, values, mb)
        loss.backward()
        return loss

    step()                                                      # the scratch is made outside the capture
    eager = _bits(ppo, batch) + [t.grad.clone() for t in (mean, log_std, values)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # autograd's warm-up on the side stream, as torch asks before a capture
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    grads = [mean.grad, log_std.grad, values.grad]
    for t in (ppo.d_mean, ppo.d_log_std, ppo.d_value, ppo.log_probs, ppo.loss):
        t.view(torch.int32).fill_(0x7FC12345)
    for g in grads:
        g.zero_()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replayed = _bits(ppo, batch) + [g.clone() for g in grads]
        _same_bits(eager[:6], replayed[:6], (batch, act_dim))
        for name, x, y in zip(("mean.grad", "log_std.grad", "values.grad"), eager[6:], replayed[6:]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name


def test_the_scratch_cannot_grow_inside_a_capture():
    pkg = _pkg()
    mean, log_std, values, mb = _device_data(65, 4, "near")
    ppo = _make(pkg, 65, 4, False, (0.0, 0.5))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="PpoLoss: the scratch would have to grow inside a graph capture"):
        with torch.cuda.graph(graph):
            ppo(mean, log_std, values, mb)
    torch.cuda.synchronize()
    loss = ppo(mean, log_std, values, mb)                       # and the object works afterwards
    P.check_outputs(_outputs(ppo, loss, 65), _reference(65, 4, "near", False, (0.0, 0.5)), "after the refused capture")


@pytest.mark.parametrize("batch,act_dim", [(1025, 4), (2049, 8), (63, 4)])
def test_the_16_byte_path_gives_the_bits_of_the_4_byte_path(batch, act_dim):
    """A = 4 and 8 on 16-byte-aligned tensors take 16-byte words; the same values behind mean, actions and d_mean moved by one 4-byte word
    take the 4-byte path."""
    pkg = _pkg()
    mean, log_std, values, mb = _device_data(batch, act_dim, "near")
    ppo = _make(pkg, batch, act_dim, True, (0.01, 0.5))
    assert mean.data_ptr() % 16 == 0 and mb["actions"].data_ptr() % 16 == 0 and ppo.d_mean.data_ptr() % 16 == 0
    ppo(mean, log_std, values, mb)
    aligned = _bits(ppo, batch)

    def moved(x):
        return torch.empty(x.numel() + 1, dtype=x.dtype, device=DEV)[1:].view(x.shape).copy_(x)
    for which in ("mean", "actions", "d_mean", "all"):
        m = moved(mean) if which in ("mean", "all") else mean
        a = moved(mb["actions"]) if which in ("actions", "all") else mb["actions"]
        ppo.d_mean = moved(ppo.d_mean) if which in ("d_mean", "all") else torch.zeros_like(mean)
        assert (m.data_ptr() % 16 == 4) == (which in ("mean", "all")) and (ppo.d_mean.data_ptr() % 16 == 4) == (which in ("d_mean", "all"))
        assert m.is_contiguous() and a.is_contiguous() and ppo.d_mean.is_contiguous()
        ppo(m, log_std, values, dict(mb, actions=a))
        _same_bits(aligned, _bits(ppo, batch), (batch, act_dim, which, "moved by one word"))


# ---- 4. autograd ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,act_dim", [(65, 3), (1025, 4)])
def test_backward_hands_on_the_static_buffers(batch, act_dim):
    pkg = _pkg()
    mean0, log_std0, values0, mb = _device_data(batch, act_dim, "near")
    ppo = _make(pkg, 2049, act_dim, True, (0.01, 0.5))
    for scale in (1.0, 3.0):
        mean, log_std, values = (t.clone().requires_grad_() for t in (mean0, log_std0, values0))
        loss = ppo(mean, log_std, values, mb)
        assert loss.requires_grad
        (loss if scale == 1.0 else scale * loss).backward()
        for name, leaf, buf in (("mean", mean, ppo.d_mean[:batch]), ("log_std", log_std, ppo.d_log_std), ("values", values, ppo.d_value[:batch])):
            assert leaf.grad.shape == leaf.shape and torch.equal(leaf.grad, buf * scale), (name, scale)
    # through a head: d (2 mean) / d mean = 2, so the leaf sees twice the buffer
    mean = mean0.clone().requires_grad_()
    ppo(mean * 2.0, log_std0, values0, dict(mb, actions=mb["actions"] * 2.0)).backward()
    assert torch.equal(mean.grad, ppo.d_mean[:batch] * 2.0)
    # no input asks for a gradient: a plain tensor
    assert not ppo(mean0, log_std0, values0, mb).requires_grad


def test_backward_after_a_second_forward_raises():
    pkg = _pkg()
    mean0, log_std0, values0, mb = _device_data(65, 4, "near")
    ppo = _make(pkg, 65, 4, False, (0.0, 0.5))
    mean = mean0.clone().requires_grad_()
    first = ppo(mean, log_std0, values0, mb)
    second = ppo(mean, log_std0, values0, mb)
    with pytest.raises(RuntimeError, match="PpoLoss: backward of call 1 after call 2"):
        first.backward()
    second.backward()                                           # the later one is still good
    assert torch.equal(mean.grad, ppo.d_mean[:65])


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------------------
def _float32_loss(net, mb, clip_range, clip_range_vf, ent_coef, vf_coef):
    """What a caller writes without PpoLoss: the torch composition in the network's own precision."""
    obs = mb["obs"].to(net.log_std.dtype)
    mean, _ = net._dist(obs)
    t = {k: mb[k].to(device=obs.device, dtype=obs.dtype) for k in MB_KEYS}
    return P.composition(mean, net.log_std, net.predict_values(obs), t["actions"], t["log_probs"], t["advantages"], t["returns"], t["values"],
                         clip_range, clip_range_vf, ent_coef, vf_coef)[0]


def _parameter_gradients(pkg, net, out, tag):
    """One minibatch of the rollout; the parameter gradients of `net` (a) through PpoLoss, (b) through the float32 composition on the
    device, (c) in float64 on the CPU through the reference's composition.  The largest error of (a) from (c) must not exceed twice that
    of (b), plus 1e-6 of the largest gradient: both share the float32 network backward, whose error neither controls."""
    kw = dict(clip_range=0.2, clip_range_vf=0.2, ent_coef=0.01, vf_coef=0.5)
    sampler = pkg.MinibatchSampler.for_rollout(out, 100, seed=5)
    mb = {k: v.clone() for k, v in sampler.gather(out, 0, 0).items()}
    ppo = pkg.PpoLoss(100, 4, DEV, **kw)

    def grads(model, loss):
        model.zero_grad(set_to_none=True)
        loss.backward()
        return [p.grad.detach().double().cpu().clone() for p in model.parameters()]

    mean, _ = net._dist(mb["obs"])
    a = grads(net, ppo(mean, net.log_std, net.predict_values(mb["obs"]), mb))
    b = grads(net, _float32_loss(net, mb, **kw))
    net64 = copy.deepcopy(net).double().cpu()
    c = grads(net64, _float32_loss(net64, {k: v.cpu() for k, v in mb.items()}, **kw))
    top = max(float(g.abs().max()) for g in c)
    err_a = max(float((x - z).abs().max()) for x, z in zip(a, c)) / top
    err_b = max(float((y - z).abs().max()) for y, z in zip(b, c)) / top
    print(f"{tag}: parameter gradients against float64: through PpoLoss {err_a:.3e}, through the float32 composition {err_b:.3e} of the largest")
    assert top > 0.0 and all(bool(torch.isfinite(g).all()) for g in a + b + c), tag
    assert err_a <= 2.0 * err_b + 1e-6, (tag, err_a, err_b)
    stats = ppo.stats_dict()
    assert all(np.isfinite(v) for v in stats.values()) and 0.0 <= stats["clip_fraction"] <= 1.0, stats


def _small_net(pkg):
    torch.manual_seed(7)
    return pkg.MlpActorCritic(pi=(32, 32), vf=(32, 32)).to(DEV)


def test_end_to_end_with_the_rollout_collector():
    """The small network collects its own rollout: the first epoch, ratio 1 but for the float32 rounding of the stored log-probabilities."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    from drl_dronenavigation_amd.collector import RolloutCollector
    n, T = 64, 4
    env = pkg.DroneVecEnv(tracks.circle(1, 4, 1), n, max_steps=3, seed=17, device=DEV, normalize_obs=True, **NOISE)
    net = _small_net(pkg)

    def policy(rows):
        with torch.no_grad():
            return net(torch.nan_to_num(rows).clamp(-5, 5))
    out = RolloutCollector(env, policy, T).collect()
    out = dict(out, obs=torch.nan_to_num(out["obs"]).clamp(-5, 5))
    torch.cuda.synchronize()
    _parameter_gradients(pkg, net, out, "RolloutCollector")
    env.close()


def test_end_to_end_with_the_fused_rollout_collector():
    """The rollout of another policy (the fused 512-512-256 network, log_std 0): a later epoch, with the ratio away from 1."""
    pkg = _pkg()
    from drl_dronenavigation_amd import tracks
    from drl_dronenavigation_amd.collector import FusedRolloutCollector
    n, T = 64, 4
    env = pkg.DroneVecEnv(tracks.circle(1, 4, 1), n, max_steps=3, seed=17, device=DEV, normalize_obs=True)
    torch.manual_seed(4)
    pol = pkg.FusedMlpPolicy(pkg.MlpActorCritic(log_std_init=0.0).to(DEV), n, DEV)
    out = FusedRolloutCollector(env, pol, T, use_graph=False, seed=1).collect()
    torch.cuda.synchronize()
    _parameter_gradients(pkg, _small_net(pkg), out, "FusedRolloutCollector")
    env.close()
