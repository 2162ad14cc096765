"""dn_mlp_forward on input rows of 17 .. 64 columns (csrc/dn_mlp_wide.hip: the wide forms of the four-wave kernel, grades bf16 / fp16, and
of the float32-grade kernel), on a real MI355X.

 5. every input column lands where its weights are: a network whose W1 has ONE non-zero column equals, bit for bit, the 13-column kernel
    fed that column (each layer-1 pre-activation is a single product plus exact zeros, whichever K-step adds them);
 6. zero padding is exact: a 13-input network embedded in 40 columns equals the 13-column kernel whatever the other 27 inputs hold;
 7. full-width accuracy against the bf16 emulation (bf16 grade) and the float64 evaluation (float32 / float16 grades);
 8. the masked forward and a single network on the wide path;
 9. RolloutCollector on cat(obs, goal) with FusedMlpPolicy (eager and graph-replayed) and on the privileged rows with FusedMlpValue.

The 13-column launches the wide ones are held against run dn_mlp.hip's kernels, which this feature does not touch."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mlp_support as S  # noqa: E402
from gpu_support import DEV  # noqa: E402
from gpu_support import pkg as _pkg  # noqa: E402

pytestmark = pytest.mark.gpu


def _pm():
    _pkg()
    from drl_dronenavigation_amd import policy_mfma as pm
    return pm


@pytest.mark.parametrize("obs_dim", [17, 32, 33, 64])
@pytest.mark.parametrize("grade", S.GRADES)
def test_every_column_lands_where_its_weights_are(grade, obs_dim):
    """The float32 grade's wide layer 1 forms its three partial products per K-step with the 16-column kernel's mfma3, in its order: all
    three grades are held to torch.equal."""
    pm = _pm()
    n = 33
    g = torch.Generator().manual_seed(1000 + obs_dim)
    layers = S.random_layers(obs_dim, 4, obs_dim)
    w1 = layers[0][0]
    zero_b1 = torch.zeros(512)
    wide = pm.pack_mlp([(torch.zeros_like(w1), zero_b1)] + layers[1:], DEV, grade)
    twin = pm.pack_mlp([(torch.zeros(512, 13), zero_b1)] + layers[1:], DEV, grade)
    x = (torch.rand((n, obs_dim), generator=g) * 2 - 1).to(DEV)
    x13 = torch.zeros((n, 13), device=DEV)
    out_w, out_t = torch.empty((n, 4), device=DEV), torch.empty((n, 4), device=DEV)
    seen = set()
    for j in range(obs_dim):
        wj = torch.zeros_like(w1)
        wj[:, j] = w1[:, j]
        wide["w1"].copy_(pm.pack_layer(wj, zero_b1, True, scale=pm.TANH_PRESCALE, grade=grade)[0])
        wt = torch.zeros(512, 13)
        wt[:, 0] = w1[:, j]
        twin["w1"].copy_(pm.pack_layer(wt, zero_b1, True, scale=pm.TANH_PRESCALE, grade=grade)[0])
        x13[:, 0] = x[:, j]
        pm.mlp_forward([wide], x, [out_w])
        pm.mlp_forward([twin], x13, [out_t])
        assert torch.equal(out_w, out_t), (j, float((out_w - out_t).abs().max()))
        seen.add(out_w.cpu().numpy().tobytes())
    assert len(seen) == obs_dim, "the outputs do not depend on the column: the check is vacuous"


@pytest.mark.parametrize("n", S.FLEETS)
@pytest.mark.parametrize("grade", S.GRADES)
def test_zero_padding_is_exact(grade, n):
    pm = _pm()
    g = torch.Generator().manual_seed(40 + n)
    nets13 = [S.random_layers(13, od, 7 + od) for od in (4, 1)]
    nets40 = []
    for layers in nets13:
        w = torch.zeros(512, 40)
        w[:, :13] = layers[0][0]
        nets40.append([(w, layers[0][1])] + layers[1:])
    x = torch.empty((n, 40))
    x[:, :13] = torch.rand((n, 13), generator=g) * 2 - 1
    x[:, 13:] = torch.randn((n, 27), generator=g) * 50.0                      # finite, far from unit size
    x = x.to(DEV)
    want = pm.mlp_forward([pm.pack_mlp(l, DEV, grade) for l in nets13], x[:, :13].contiguous())
    got = pm.mlp_forward([pm.pack_mlp(l, DEV, grade) for l in nets40], x)
    for a, b in zip(got, want):
        assert torch.equal(a, b), float((a - b).abs().max())


ABS_BARS = {"fp32": (1e-4, 1e-4), "fp16": (2.5e-3, 5e-3)}                        # the project's bars on (action mean, value)


@pytest.mark.parametrize("width", [17, 21, 52, 64])
def test_full_width_accuracy(width):
    """MlpActorCritic(obs_dim=W), actor and critic in one launch, N = 300.  bf16 grade: against the spelled-out bf16 emulation at the
    project's bars (max < 1e-2, mean < 3e-4: rounding flips in the 512-wide hidden layers, not the input width).  float32 / float16 grades:
    against the float64 evaluation of the float32 network, at 3 x the error of the 13-column network of the same grade and seed against
    ITS float64 evaluation, measured here (independent layer-1 rounding errors grow as sqrt(64 / 13) = 2.2, rounded up), and at the
    project's absolute bars (1e-4; 2.5e-3 / 5e-3).

    Measured on an MI355X, max |err| (pi, vf) wide | 13 columns: see profiles/time_mlp_wide.txt."""
    pkg, pm = _pkg(), _pm()
    n, dev = 300, torch.device(DEV)
    net, net13 = S.perturbed_net(pkg, width, 500 + width, dev), S.perturbed_net(pkg, 13, 500 + width, dev)
    torch.manual_seed(width)
    x = torch.rand((n, width), device=dev) * 2 - 1
    x13 = x[:, :13].contiguous()
    (pi, vf), (pi13, vf13) = S.layers_of(net), S.layers_of(net13)
    mean, value = pm.mlp_forward([pm.pack_mlp(pi, dev, "bf16"), pm.pack_mlp(vf, dev, "bf16")], x)
    fails = []
    for name, got, ref in (("pi", mean, S.mlp_reference(pi, x)), ("vf", value, S.mlp_reference(vf, x))):
        err = (got - ref).abs()
        print(f"W={width} bf16 {name}: max {float(err.max()):.3e} mean {float(err.mean()):.3e} vs the bf16 emulation")
        if not (float(err.max()) < 1e-2 and float(err.mean()) < 3e-4):
            fails.append(("bf16", name, float(err.max()), float(err.mean())))
    want, want13 = (S.f64(pi, x), S.f64(vf, x)), (S.f64(pi13, x13), S.f64(vf13, x13))
    for grade in ("fp32", "fp16"):
        got = pm.mlp_forward([pm.pack_mlp(pi, dev, grade), pm.pack_mlp(vf, dev, grade)], x)
        got13 = pm.mlp_forward([pm.pack_mlp(pi13, dev, grade), pm.pack_mlp(vf13, dev, grade)], x13)
        for k, name in enumerate(("pi", "vf")):
            e = float((got[k].double() - want[k]).abs().max())
            e13 = float((got13[k].double() - want13[k]).abs().max())
            print(f"W={width} {grade} {name}: max |err| vs float64 {e:.3e}; 13 columns {e13:.3e} (x 3 = {3 * e13:.3e}); absolute bar {ABS_BARS[grade][k]:.1e}")
            if not (e <= 3 * e13 and e <= ABS_BARS[grade][k]):
                fails.append((grade, name, e, e13))
    assert not fails, fails


@pytest.mark.parametrize("width", [21, 52])
@pytest.mark.parametrize("grade", S.GRADES)
def test_masked_forward_and_a_single_network(grade, width):
    pm = _pm()
    n = 300
    g = torch.Generator().manual_seed(width)
    pi, vf = pm.pack_mlp(S.random_layers(width, 4, 1), DEV, grade), pm.pack_mlp(S.random_layers(width, 1, 2), DEV, grade)
    x = (torch.rand((n, width), generator=g) * 2 - 1).to(DEV)
    mean, value = pm.mlp_forward([pi, vf], x)
    assert float(mean.abs().min()) > 0 and float(value.abs().min()) > 0
    (alone,) = pm.mlp_forward([vf], x)
    assert torch.equal(alone, value)
    (alone,) = pm.mlp_forward([pi], x)
    assert torch.equal(alone, mean)
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    mask[::97] = 1
    has = S.tiles_with_a_flag(mask)
    assert bool(has.any()) and bool((~has).any())
    for packs, full in (([vf], [value]), ([pi, vf], [mean, value])):
        outs = [torch.full_like(f, 7.0) for f in full]
        pm.mlp_forward(packs, x, outs, row_mask=mask)
        for o, f in zip(outs, full):
            assert torch.equal(o[has], f[has]) and float(o[~has].abs().sum()) == 0.0
    for other in (13, width - 1):                                             # another K-step count; the same one, another width
        with pytest.raises(ValueError, match="packed for"):
            pm.mlp_forward([vf], x[:, :other].contiguous())


def test_fused_collector_refuses_a_policy_packed_for_other_rows():
    """FusedRolloutCollector hands the packed networks to its step path by pointer, with the env's 13 columns as the width."""
    pkg, pm = _pkg(), _pm()
    from drl_dronenavigation_amd import tracks
    from drl_dronenavigation_amd.collector import FusedRolloutCollector
    env = pkg.DroneVecEnv(tracks.circle(1, 4, 1), 128, device=DEV)
    pol = pm.FusedMlpPolicy(pkg.MlpActorCritic(obs_dim=21), 128, DEV)
    with pytest.raises(ValueError, match="packed for 21"):
        FusedRolloutCollector(env, pol, 4)
    env.close()


def _goal_env(pkg):
    wp = np.array([[0.0, 1.0, 0.6], [-1.0, 0.0, 1.0], [0.0, -1.0, 0.6]])
    return pkg.DroneVecEnv(None, 256, target_points=wp, initial_xyzs=np.array([[1.0, 0.0, 0.5]]), aviary_dim=[-2.0, -2.0, 0.0, 2.0, 2.0, 2.0],
                           circle=False, cylinder=False, max_steps=40, seed=17, device=DEV, normalize_obs=False,
                           sensor=pkg.SensorModel(latency=(0, 8), bias=(0.01,) * 13), goal=pkg.GoalObservation(frame="body"))


def test_collector_runs_the_fused_policy_on_observation_and_goal():
    pkg, pm = _pkg(), _pm()
    from drl_dronenavigation_amd.collector import RolloutCollector
    n, T, dev = 256, 4, torch.device(DEV)
    torch.manual_seed(3)
    net = pkg.MlpActorCritic(obs_dim=21).to(dev)
    with torch.no_grad():
        net.action_net.bias.fill_(0.0922)                                       # hover: flights last
    env = _goal_env(pkg)
    pol = pm.FusedMlpPolicy(net, n, dev)
    buf = RolloutCollector(env, pol, T, policy_input="observation+goal").collect()
    assert tuple(buf["goal"].shape) == (T, n, 8)
    for t in range(T):
        seen = torch.cat((buf["obs"][t], buf["goal"][t]), dim=1)
        assert torch.equal(buf["values"][t], pm.mlp_forward([pol.pi, pol.vf], seen)[1].squeeze(-1)), t
    assert float(buf["values"].abs().sum()) > 0 and float(buf["goal"].abs().sum()) > 0
    env.close()
    # a replayed hipGraph of the rollout against an eager twin: deterministic actions, so that both fly the same flights
    runs = []
    for use_graph in (False, True):
        env = _goal_env(pkg)
        pol = pm.FusedMlpPolicy(net, n, dev)
        col = RolloutCollector(env, lambda x, pol=pol: pol(x, deterministic=True), T, policy_input="observation+goal", use_graph=use_graph)
        for _ in range(3):
            out = col.collect()
        torch.cuda.synchronize()
        assert (col._graph is not None) == use_graph
        runs.append({k: v.clone() for k, v in out.items()})
        env.close()
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    assert float(runs[0]["rewards"].abs().sum()) > 0


def test_collector_runs_the_fused_critic_on_the_privileged_rows():
    pkg, pm = _pkg(), _pm()
    from drl_dronenavigation_amd import tracks
    from drl_dronenavigation_amd.collector import RolloutCollector
    n, T, dev = 256, 4, torch.device(DEV)
    torch.manual_seed(4)
    env = pkg.DroneVecEnv(tracks.circle(1, 4, 1), n, max_steps=3, seed=17, device=DEV, normalize_obs=False,
                          privileged=pkg.PrivilegedObservation())
    module = pkg.MlpValue(52).to(dev)
    critic = pkg.FusedMlpValue(module, n, dev, grade="fp16")
    g = torch.Generator().manual_seed(3)
    w = (0.05 * torch.randn((13, 4), generator=g)).to(dev)

    def policy(obs):
        return 0.0922 + 0.01 * torch.tanh(obs @ w), obs[:, 0], -(obs * obs).sum(dim=1)

    col = RolloutCollector(env, policy, T, value_fn=critic, value_input="privileged")
    assert col._value_fn_takes_mask
    buf = col.collect()
    assert tuple(buf["privileged"].shape) == (T, n, 52)
    first = buf["values"].clone()
    for t in range(T):
        assert torch.equal(first[t], pm.mlp_forward([critic.vf], buf["privileged"][t].contiguous())[0].squeeze(-1)), t
    assert float(first.abs().sum()) > 0
    rows = buf["privileged"][0].clone()
    before = critic(rows).clone()
    addr = {k: v.data_ptr() for k, v in critic.vf.items() if torch.is_tensor(v)}
    with torch.no_grad():
        module.value_net.weight.mul_(-2.0)
        module.vf[0].weight.add_(0.01)
    assert torch.equal(critic(rows), before)                                    # the packed weights are a copy
    critic.refresh()
    assert not torch.equal(critic(rows), before)
    assert {k: v.data_ptr() for k, v in critic.vf.items() if torch.is_tensor(v)} == addr
    env.close()
