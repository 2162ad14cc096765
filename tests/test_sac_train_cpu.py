"""The training pass of the SAC networks and the Polyak update (include/dronenav.h dn_sac_train_*, dn_polyak_update, sac_train.py) without
a GPU: the four names are declared, exported and bound; the struct layout and every new constant hold against the compiled header; the
ABI version is unchanged; dn_sac_train_scratch_bytes follows its documented formula; every refusal returns DN_ERR_INVALID_ARGUMENT, names
its argument and comes before any device call (the pointers here are dummies); the constructor refusals of SacTrainer and PolyakUpdate
that need no device; the row selection of sac_train_support finds its rows for every case; and the scratch layout and the Polyak
expression, pinned by a stand-alone host program under the sanitizers."""
import ctypes as C

import pytest

import abi_support as abi
import host_program_support as hps
import sac_train_support as S

torch = pytest.importorskip("torch")

P = 4096                                 # a dummy non-NULL, 16-byte aligned address: every call here returns before it is used
BIG = 1 << 40                            # scratch_bytes that is never too small
A, B, F = S.BY_NAME["A"], S.BY_NAME["B"], S.BY_NAME["F"]


@pytest.fixture(scope="module")
def pkg():
    import drl_dronenavigation_amd as p
    p.build.build_library()
    return p


def test_the_four_names_are_declared_exported_and_bound(pkg):
    abi.check_names("dn_sac_train_scratch_bytes", "dn_sac_train_forward", "dn_sac_train_backward", "dn_polyak_update")
    arity = abi.header_arity()
    assert {k: v for k, v in arity.items() if k.startswith("dn_sac_train")} == {
        "dn_sac_train_scratch_bytes": 3, "dn_sac_train_forward": 10, "dn_sac_train_backward": 12}
    assert arity["dn_polyak_update"] == 7
    assert pkg.SacTrainer is pkg.sac_train.SacTrainer and pkg.PolyakUpdate is pkg.sac_train.PolyakUpdate
    assert "SacTrainer" in pkg.__all__ and "PolyakUpdate" in pkg.__all__


def test_struct_layout_and_constants_match_the_header(pkg):
    K = pkg._capi
    abi.check_layout(K.DnSacTrainConfig, 32, n_nets=0, n_layers=4, head_parts=8, activation=12, in0=16, in1=20, flags=24, reserved=28)
    got = abi.compiled().constants
    assert (got["DN_MLP_ACT_TANH"], got["DN_MLP_ACT_RELU"], got["DN_SAC_TRAIN_MAX_NETS"], got["DN_SAC_TRAIN_MAX_PARTS"]) == \
        (K.TRAIN_ACT_TANH, K.TRAIN_ACT_RELU, K.TRAIN_MAX_NETS, K.TRAIN_MAX_PARTS) == (S.TANH, S.RELU, 4, 2)
    assert got["DN_SAC_TRAIN_MAX_NETS"] == got["DN_SAC_MAX_CRITICS"] and got["DN_ADAM_MAX_TENSORS"] == K.ADAM_MAX_TENSORS == 32
    text = abi.header_text(comments=True)
    assert "n_nets at 0, n_layers at 4, head_parts at 8, activation at 12, in0 at 16, in1 at 20, flags at 24,\n *   reserved at 28; 32 bytes" in text
    assert "ReLU can follow without a new layout" not in text and "these three entry points take Tanh only" in text
    abi.check_version()                                # the ABI version stays


@pytest.mark.parametrize("g", S.GROUPS, ids=lambda g: g.name)
def test_scratch_bytes_follow_the_documented_formula(pkg, g):
    K, lib = pkg._capi, pkg._capi.load()
    cfg, table = S.tables(K, g)
    for batch in (1, S.R - 1, S.R, S.R + 1, 1 << 24):
        assert lib.dn_sac_train_scratch_bytes(C.byref(cfg), table, batch) == S.scratch_bytes(g, batch), batch
    if g is B:                                         # by hand at one chunk: 2 x 512 activations a row, 13 x 256 + 256 x 256 + 8 x 256 weights, 520 biases
        r = lambda b: (b + 255) // 256 * 256           # noqa: E731
        assert S.scratch_bytes(g, 1) == 2 * (1024 + 1024) + r(4 * 13 * 256) + 4 * 256 * 256 + 4 * 8 * 256 + 2048 + 2048 + 256
    if g is A:                                         # two networks: twice one network's
        assert S.scratch_bytes(g, 5) == 2 * S.T.scratch_bytes((17, 256, 256, 128, 1), 5)


def _calls(pkg, g=A, batch=5, flags=0, act=S.RELU, *, cfg=None, table=None, x0=P, x1="auto", out="auto", d_out="auto", d_x0=P + (1 << 20),
           d_x1="auto", scratch=P + (2 << 20), scratch_bytes=BIG):
    """The status of the three entry points for one set of arguments, and the message of each.  The defaults overlap nowhere: every weight
    and gradient entry and every output gets an address of its own."""
    K, lib = pkg._capi, pkg._capi.load()
    n = len(S.entry_dims(g))
    far = lambda k: (1 << 30) + (k << 22)              # noqa: E731  4 MiB apart: beyond any tensor of 5 rows
    ptrs = [[(far(4 * (c * n + l)), far(4 * (c * n + l) + 1), far(4 * (c * n + l) + 2), far(4 * (c * n + l) + 3)) for l in range(n)]
            for c in range(g.n_nets)]
    c, t = S.tables(K, g, act, ptrs, flags)
    c, t = (c if cfg is None else cfg), (t if table is None else table)
    cp, tp = (C.byref(c) if c else None), (t if t else None)
    heads = g.n_nets * len(g.parts)
    x1 = (P + (3 << 20) if g.in1 else None) if x1 == "auto" else x1
    d_x1 = (P + (4 << 20) if g.in1 else None) if d_x1 == "auto" else d_x1
    out = S.pointer_table([far(200 + i) for i in range(heads)]) if out == "auto" else out
    d_out = S.pointer_table([far(300 + i) for i in range(heads)]) if d_out == "auto" else d_out
    res = []
    for call in (lambda: lib.dn_sac_train_scratch_bytes(cp, tp, batch),
                 lambda: lib.dn_sac_train_forward(cp, tp, x0, x1, batch, out, scratch, scratch_bytes, 0, None),
                 lambda: lib.dn_sac_train_backward(cp, tp, x0, x1, d_out, batch, d_x0, d_x1, scratch, scratch_bytes, 0, None)):
        res.append((call(), lib.dn_last_error().decode()))
    return res


def _refused(results, word, which=(0, 1, 2)):
    for k in which:
        rc, text = results[k]
        assert rc == -1 and word in text, (k, rc, text, word)


def _short_scratch_is_next(pkg, **kw):
    """Nothing else is wrong with these arguments: the calls get as far as the short scratch."""
    g = kw.get("g", A)
    _refused(_calls(pkg, scratch_bytes=S.scratch_bytes(g, 5) - 1, **kw), "scratch_bytes", (1, 2))


def test_the_dummy_arguments_are_otherwise_fine(pkg):
    for g in S.GROUPS:
        assert _calls(pkg, g)[0][0] == S.scratch_bytes(g, 5)
        _short_scratch_is_next(pkg, g=g)


def test_shape_refusals_name_their_argument(pkg):
    K = pkg._capi
    _refused(_calls(pkg, cfg=False), "cfg")
    _refused(_calls(pkg, table=False), "layers")

    def with_cfg(**fields):
        cfg, _ = S.tables(K, A)
        for k, v in fields.items():
            setattr(cfg, k, v)
        return _calls(pkg, cfg=cfg)

    for n in (0, 5):
        _refused(with_cfg(n_nets=n), "n_nets")
    for n in (1, 5):
        _refused(with_cfg(n_layers=n), "n_layers")
    for n in (0, 3):
        _refused(with_cfg(head_parts=n), "head_parts")
    for a in (-1, 2):
        _refused(with_cfg(activation=a), "activation")
    for v in (0, 65):
        _refused(with_cfg(in0=v), "in0")
    _refused(with_cfg(in1=-1), "in1")
    _refused(with_cfg(in0=60, in1=5), "in1")
    _refused(with_cfg(in0=12), "layers[0][0].in_dim")   # in0 + in1 is not what layer 0 reads
    _refused(_calls(pkg, flags=4), "flags")
    _refused(with_cfg(reserved=1), "reserved")

    def with_table(c, l, field, value, g=A):
        _, table = S.tables(K, g)
        setattr(table[c * len(S.entry_dims(g)) + l], field, value)
        return _calls(pkg, g, table=table)

    for h in (0, 16, 48, 544):
        _refused(with_table(0, 1, "out_dim", h), "layers[0][1].out_dim")
    _refused(with_table(0, 2, "in_dim", 128), "layers[0][2].in_dim")                    # a broken chain
    _refused(with_table(1, 3, "in_dim", 256), "layers[1][3].in_dim")                    # ... in the second network's head
    for o in (0, 33):
        _refused(with_table(0, 3, "out_dim", o), "layers[0][3].out_dim")
    _refused(with_table(0, 2, "out_dim", 30, g=F), "layers[0][2].out_dim")              # 3 + 30 > 32 outputs together
    _refused(with_table(0, 2, "in_dim", 64, g=F), "layers[0][2].in_dim")                # the second part reads the last hidden layer too
    _refused(with_table(1, 3, "out_dim", 2), "layers[1][3].out_dim")                    # networks whose dimensions differ
    _, table = S.tables(K, A)
    table[4].out_dim, table[5].in_dim = 128, 128                                       # a chain of its own, but not network 0's shape
    _refused(_calls(pkg, table=table), "layers[1][0].out_dim")
    for batch in (0, -1, (1 << 24) + 1):
        _refused(_calls(pkg, batch=batch), "batch")
    assert _calls(pkg, batch=1 << 24)[0][0] > 0        # the largest batch is taken


def test_pointer_refusals_name_their_argument(pkg):
    K = pkg._capi
    _refused(_calls(pkg, x0=None), "x0", (1, 2))
    _refused(_calls(pkg, x1=None), "x1", (1, 2))                                        # in1 = 4 and no x1
    _refused(_calls(pkg, B, x1=P + (3 << 20)), "x1", (1, 2))                            # in1 = 0 and an x1
    _refused(_calls(pkg, B, d_x1=P + (4 << 20)), "d_x1", (2,))
    _refused(_calls(pkg, out=None), "out", (1,))
    _refused(_calls(pkg, d_out=None), "d_out", (2,))
    _refused(_calls(pkg, out=S.pointer_table([P + (8 << 20), 0])), "out[1]", (1,))
    _refused(_calls(pkg, d_out=S.pointer_table([0, P + (8 << 20)])), "d_out[0]", (2,))
    _refused(_calls(pkg, scratch=None), "scratch", (1, 2))
    _refused(_calls(pkg, scratch_bytes=S.scratch_bytes(A, 5) - 1), "scratch_bytes", (1, 2))
    _refused(_calls(pkg, scratch=P + (2 << 20) + 8), "scratch", (1, 2))
    _refused(_calls(pkg, x0=P + 2), "x0", (1, 2))
    _refused(_calls(pkg, x1=P + (3 << 20) + 1), "x1", (1, 2))
    _refused(_calls(pkg, d_x0=P + (1 << 20) + 2), "d_x0", (2,))
    n = len(S.entry_dims(A))
    for field in ("weight", "bias"):
        table = _table_like_calls(K, A)
        setattr(table[n + 1], field, None)
        _refused(_calls(pkg, table=table), f"layers[1][1].{field}", (1, 2))
    for field in ("d_weight", "d_bias"):
        table = _table_like_calls(K, A)
        setattr(table[n + 3], field, None)
        _refused(_calls(pkg, table=table), f"layers[1][3].{field}", (2,))
        # ... which the forward does not ask for, and the backward neither with DN_MLP_TRAIN_NO_PARAM_GRADS: both get as far as the
        # next refusal, the short scratch
        need = S.scratch_bytes(A, 5)
        _refused(_calls(pkg, table=table, scratch_bytes=need - 1), "scratch_bytes", (1,))
        _refused(_calls(pkg, table=table, scratch_bytes=need - 1, flags=K.TRAIN_NO_PARAM_GRADS), "scratch_bytes", (2,))
    table = _table_like_calls(K, A)
    table[2].weight = table[2].weight + 2
    _refused(_calls(pkg, table=table), "layers[0][2].weight", (1, 2))
    # nothing to do: no parameter gradients and neither input gradient; one of the two is enough
    _refused(_calls(pkg, flags=K.TRAIN_NO_PARAM_GRADS, d_x0=None, d_x1=None), "d_x0", (2,))
    _short_scratch_is_next(pkg, flags=K.TRAIN_NO_PARAM_GRADS, d_x0=None)
    _short_scratch_is_next(pkg, flags=K.TRAIN_NO_PARAM_GRADS, d_x1=None)
    _short_scratch_is_next(pkg, d_x0=None, d_x1=None)


def _table_like_calls(K, g):
    n = len(S.entry_dims(g))
    far = lambda k: (1 << 30) + (k << 22)              # noqa: E731
    ptrs = [[tuple(far(4 * (c * n + l) + k) for k in range(4)) for l in range(n)] for c in range(g.n_nets)]
    return S.tables(K, g, S.RELU, ptrs)[1]


def test_overlap_refusals_name_both_arguments(pkg):
    K = pkg._capi
    out0 = (1 << 30) + (200 << 22)                     # what _calls gives out[0]
    _refused(_calls(pkg, x0=out0), "out[0] overlaps x0", (1,))                          # an output on an input
    _refused(_calls(pkg, x1=out0 + 4), "out[0] overlaps x1", (1,))
    _refused(_calls(pkg, out=S.pointer_table([out0, out0])), "out[0] overlaps out[1]", (1,))     # two outputs on each other
    _refused(_calls(pkg, d_x0=P, x0=P), "d_x0 overlaps x0", (2,))
    _refused(_calls(pkg, d_x1=P + (1 << 20) + 8), "d_x0 overlaps d_x1", (2,))
    table = _table_like_calls(K, A)
    table[1].d_weight = table[0].weight                # a gradient on another layer's weight
    _refused(_calls(pkg, table=table), "layers[0][1].d_weight overlaps layers[0][0].weight", (2,))
    table = _table_like_calls(K, A)
    table[5].d_bias = table[0].d_bias                  # the two networks' gradients on each other
    _refused(_calls(pkg, table=table), "layers[0][0].d_bias overlaps layers[1][1].d_bias", (2,))
    scratch = P + (2 << 20)
    _refused(_calls(pkg, x0=scratch + 64), "scratch overlaps x0", (1, 2))
    d_out = S.pointer_table([(1 << 30) + (300 << 22), scratch + 1024])
    _refused(_calls(pkg, d_out=d_out), "scratch overlaps d_out[1]", (2,))


def _polyak(pkg, n=2, *, source="auto", target="auto", counts="auto", tau=0.005):
    lib = pkg._capi.load()
    far = lambda k: (1 << 30) + (k << 22)              # noqa: E731
    source = S.pointer_table([far(i) for i in range(max(n, 0))]) if source == "auto" else source
    target = S.pointer_table([far(100 + i) for i in range(max(n, 0))]) if target == "auto" else target
    counts = (C.c_int64 * max(n, 1))(*([1000] * max(n, 1))) if counts == "auto" else counts
    rc = lib.dn_polyak_update(n, source, target, counts, tau, 0, None)
    return rc, lib.dn_last_error().decode()


def test_polyak_refusals_name_their_argument(pkg):
    def refused(word, *a, **kw):
        rc, text = _polyak(pkg, *a, **kw)
        assert rc == -1 and word in text, (rc, text, word)

    for n in (0, -1, 33):
        refused("n_tensors", n)
    refused("source", source=None)
    refused("target", target=None)
    refused("counts", counts=None)
    for tau in (-0.1, 1.5, float("nan")):
        refused("tau", tau=tau)
    refused("counts[1]", counts=(C.c_int64 * 2)(5, 0))
    far = lambda k: (1 << 30) + (k << 22)              # noqa: E731
    refused("source[1]", source=S.pointer_table([far(0), 0]))
    refused("target[0]", target=S.pointer_table([0, far(101)]))
    refused("source[0]", source=S.pointer_table([far(0) + 2, far(1)]))
    refused("target[1]", target=S.pointer_table([far(100), far(101) + 1]))
    refused("target[0] overlaps source[0]", target=S.pointer_table([far(0), far(101)]))          # a source that is its target
    refused("target[1] overlaps source[0]", target=S.pointer_table([far(100), far(0) + 3996]))   # by its last element
    refused("target[0] overlaps target[1]", target=S.pointer_table([far(100), far(100) + 400]))
    if pkg._capi.load().dn_device_count() == 0:        # every argument in order: the call gets as far as the device
        assert _polyak(pkg, 32)[0] != -1 and _polyak(pkg, 1, tau=0.0)[0] != -1 and _polyak(pkg, 1, tau=1.0)[0] != -1


def test_trainer_refusals_that_need_no_device(pkg):
    nn = torch.nn
    M = pkg.SacTrainer
    lin = lambda *s: [nn.Linear(a, b) for a, b in zip(s[:-1], s[1:])]      # noqa: E731
    with pytest.raises(ValueError, match="activation must be"):
        M([lin(13, 64, 4)], 8, activation="gelu")
    with pytest.raises(ValueError, match="nets must hold 1..4"):
        M([], 8)
    with pytest.raises(ValueError, match="nets must hold 1..4"):
        M([lin(13, 64, 4) for _ in range(5)], 8)
    with pytest.raises(ValueError, match=r"nets\[0\] must hold 2..4 layers"):
        M([lin(13, 4)], 8)
    with pytest.raises(ValueError, match=r"nets\[1\] must hold 2..4 layers"):
        M([lin(13, 64, 4), lin(13, 64, 64, 64, 64, 4)], 8)
    with pytest.raises(ValueError, match="a tuple of two"):
        M([[nn.Linear(13, 64), (nn.Linear(64, 4), nn.Linear(64, 4), nn.Linear(64, 4))]], 8)
    with pytest.raises(ValueError, match=r"nets\[0\]\[1\] must be an nn.Linear"):
        M([[nn.Linear(13, 64), nn.ReLU(), nn.Linear(64, 4)]], 8)
    with pytest.raises(ValueError, match=r"nets\[0\]\[1\]\[1\] must be an nn.Linear"):
        M([[nn.Linear(13, 64), (nn.Linear(64, 4), nn.ReLU())]], 8)
    with pytest.raises(ValueError, match=r"nets\[0\]\[0\].weight must be torch.float32"):
        M([[nn.Linear(13, 64).double(), nn.Linear(64, 4)]], 8)
    with pytest.raises(ValueError, match=r"nets\[0\]\[1\] has no bias"):
        M([[nn.Linear(13, 64), nn.Linear(64, 4, bias=False)]], 8)
    strided = nn.Linear(13, 64)
    strided.weight = nn.Parameter(torch.zeros(13, 64).t())
    with pytest.raises(ValueError, match=r"nets\[0\]\[0\].weight must be dense"):
        M([[strided, nn.Linear(64, 4)]], 8)
    for bad in (0, (1 << 24) + 1, 2.0, True):
        with pytest.raises(ValueError, match="batch_size"):
            M([lin(13, 64, 4)], bad)
    with pytest.raises(ValueError, match="in_split must be"):
        M([lin(65, 64, 4)], 8)
    with pytest.raises(ValueError, match="in_split must be"):
        M([lin(17, 64, 4)], 8, in_split=(17, -1))
    with pytest.raises(ValueError, match=r"nets\[0\]\[0\].in_features must be in_split's 13 \+ 3 = 16"):
        M([lin(17, 64, 4)], 8, in_split=(13, 3))
    with pytest.raises(ValueError, match=r"nets\[0\]\[0\].out_features, a hidden width"):
        M([lin(13, 48, 4)], 8)
    with pytest.raises(ValueError, match=r"nets\[0\]\[1\].in_features must be nets\[0\]\[0\].out_features"):
        M([[nn.Linear(13, 64), nn.Linear(32, 32), nn.Linear(32, 4)]], 8)
    with pytest.raises(ValueError, match=r"nets\[0\]\[1\].out_features, a head part's"):
        M([lin(13, 64, 33)], 8)
    with pytest.raises(ValueError, match=r"nets\[0\]\[1\]\[1\].in_features must be"):
        M([[nn.Linear(13, 64), (nn.Linear(64, 4), nn.Linear(32, 4))]], 8)
    with pytest.raises(ValueError, match="at most 32 outputs together"):
        M([[nn.Linear(13, 64), (nn.Linear(64, 20), nn.Linear(64, 20))]], 8)
    with pytest.raises(ValueError, match="one shape"):
        M([lin(13, 64, 1), lin(13, 96, 1)], 8)
    with pytest.raises(ValueError, match=r"nets\[0\]\[0\].weight is on cpu"):
        M([lin(13, 64, 4)], 8)
    actor = pkg.SacActor()
    actor.latent_pi[1] = nn.Tanh()
    with pytest.raises(ValueError, match="actor.latent_pi must be Linear, ReLU pairs"):
        M.for_actor(actor, 8)
    critic = pkg.SacCritic()
    critic.q_networks[1][3] = nn.Tanh()
    with pytest.raises(ValueError, match=r"critic.q_networks\[1\]'s trunk must be Linear, ReLU pairs"):
        M.for_critics(critic, 8)
    with pytest.raises(ValueError, match="is on cpu"):             # the helpers pick latent_pi + (mu, log_std) and every q_network
        M.for_actor(pkg.SacActor(), 8)
    with pytest.raises(ValueError, match="is on cpu"):
        M.for_critics(pkg.SacCritic(), 8)
    with pytest.raises(ValueError, match="in_split"):              # 17 columns are not 10 + 4
        M.for_critics(pkg.SacCritic(), 8, in_split=(10, 4))


def test_polyak_update_refusals_that_need_no_device(pkg):
    U = pkg.PolyakUpdate
    t = lambda *s: torch.zeros(s)                      # noqa: E731
    with pytest.raises(ValueError, match="pair by pair"):
        U([t(3)], [t(3), t(3)])
    with pytest.raises(ValueError, match="1..32 tensors"):
        U([], [])
    with pytest.raises(ValueError, match="1..32 tensors"):
        U([t(2) for _ in range(33)], [t(2) for _ in range(33)])
    for tau in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="tau"):
            U([t(3)], [t(3)], tau)
    with pytest.raises(ValueError, match=r"target_params\[0\] must be torch.float32"):
        U([t(3)], [t(3).double()])
    with pytest.raises(ValueError, match=r"source_params\[1\] must be a tensor"):
        U([t(3), 1.0], [t(3), t(1)])
    with pytest.raises(ValueError, match=r"source_params\[0\] must be dense"):
        U([t(3, 4).t()], [t(4, 3)])
    with pytest.raises(ValueError, match="one shape"):
        U([t(3, 4)], [t(4, 3)])
    same = t(5)
    with pytest.raises(ValueError, match=r"source_params\[0\] is target_params\[0\]"):
        U([same], [same])
    with pytest.raises(ValueError, match=r"source_params\[0\] is target_params\[0\]"):
        U([same], [same.view(5)])
    with pytest.raises(ValueError, match="is on cpu"):
        U([t(3)], [t(3)])


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_the_row_selection_finds_its_rows(case):
    """Every case finds its `batch` rows among 8 batch candidates, at least one candidate in eight is kept, and the kept rows do keep
    every hidden pre-activation of the float64 reference off the kink by twice the forward bar."""
    g, act, batch = case
    sel = S.selection(g, batch)
    print(f"sac_train {S.case_id(case)}: {sel.kept_share:.3f} of the candidates kept")
    assert sel.found and sel.kept_share >= 1.0 / 8.0 and sel.x.shape == (batch, g.in0 + g.in1)
    # the rule restated here, apart from selection(): plain float64 products over the candidates, the bar from each layer's largest
    # |z| over all candidates, the first `batch` rows that clear it in every hidden layer of every network
    cand = S.candidates(g, batch).double()
    ok = torch.ones(len(cand), dtype=torch.bool)
    for net in S.layers_of(g):
        h = cand
        for w, b in net[:len(g.hidden)]:
            z = h @ w.double().t() + b.double()
            ok &= (z.abs() >= 2 * S.BOUND * z.abs().max()).all(dim=1)
            h = z.clamp(min=0.0)
    rows = torch.nonzero(ok).flatten()[:batch]
    assert len(rows) == batch and torch.equal(sel.x, cand[rows].float())
    assert abs(float(ok.double().mean()) - sel.kept_share) < 1e-12
    for net in S.layers_of(g):                         # ... and the kept rows alone clear the candidates' bar, layer by layer
        h_all, h = cand, sel.x.double()
        for w, b in net[:len(g.hidden)]:
            z_all, z = h_all @ w.double().t() + b.double(), h @ w.double().t() + b.double()
            assert float(z.abs().min()) >= 2 * S.BOUND * float(z_all.abs().max())
            h_all, h = z_all.clamp(min=0.0), z.clamp(min=0.0)


def test_the_scratch_layout_and_the_polyak_expression_on_the_host(tmp_path):
    """csrc/dn_internal.h's dn_sac_train_layout and csrc/dn_sac_math.h's dn_polyak in a program of their own, under the address and
    undefined-behaviour sanitizers."""
    exe = hps.build("check_sac_train_layout", tmp_path, sanitize=True, hip_headers=True, extra_flags=("-ffp-contract=off",))
    if exe is None:
        pytest.skip("the HIP headers are not installed")
    res = hps.run(exe, 3000000, timeout=300)
    assert res["failures"] == 0 and res["layouts"] > 10000 and res["polyak"] > 3000000
