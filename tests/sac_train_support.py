"""What the tests of the SAC networks' training pass share (tests/test_sac_train_cpu.py, tests/test_gpu_sac_train.py): the groups and
batches of the issue, the inputs with their row selection, the float64 reference through torch autograd on the CPU (computed once per
case), the scratch formula restated, and the ctypes tables of a call.  A plain module like tests/mlp_train_support.py -- pytest does not
collect it.

ReLU needs one condition the Tanh tests did not: no hidden pre-activation of the reference may sit at the kink, or a float32-grade
forward legitimately takes the other branch and a whole unit's gradient differs.  So the rows of a case are selected: 8 batch candidate
rows are drawn, every network of the group is evaluated in float64, and the first `batch` rows are kept in which every hidden
pre-activation has |z| >= 2 BOUND max |z|, the maximum over that layer and all candidates -- twice the forward bar, so a device inside
the bar cannot flip a sign.  A condition, not a tolerance: rows are replaced, never dropped, and no case is skipped."""
import collections
import ctypes as C
import functools

import torch

import mlp_train_support as T

R = T.R
BOUND = T.BOUND
TANH, RELU = 0, 1                        # DN_MLP_ACT_TANH, DN_MLP_ACT_RELU: test_sac_train_cpu.py holds them to the header

Group = collections.namedtuple("Group", "name n_nets in0 in1 hidden parts")
GROUPS = (Group("A", 2, 13, 4, (256, 256, 128), (1,)),       # the reference's critics
          Group("B", 1, 13, 0, (256, 256), (4, 4)),          # the reference's actor
          Group("C", 4, 12, 4, (32, 32), (1,)),              # 16 columns: the K-step edge, four networks
          Group("D", 3, 29, 4, (64, 32), (1,)),              # 33 columns
          Group("E", 1, 60, 4, (96,), (8, 8)),               # 64 columns, in0 a multiple of 4
          Group("F", 2, 15, 1, (32,), (3, 5)),               # a straddling load, odd parts
          Group("G", 1, 1, 0, (32,), (1,)),                  # the least of everything
          Group("H", 2, 1, 1, (32, 32, 32), (1, 1)),         # four layers
          Group("I", 1, 28, 4, (512,), (16, 16)),            # the widest hidden layer, a full 32-column head
          Group("J", 2, 14, 2, (160, 32), (2,)))
BY_NAME = {g.name: g for g in GROUPS}
EVERY_BATCH = (1, 33, 256, R + 1, 2 * R + 5)                 # on A and F; {33, R + 1} on the rest
CASES = tuple((g, RELU, b) for g in GROUPS for b in (EVERY_BATCH if g.name in "AF" else (33, R + 1))) + \
    ((BY_NAME["A"], TANH, R + 1), (BY_NAME["B"], TANH, R + 1))


def case_id(case):
    g, act, batch = case
    return f"{g.name}-{'relu' if act == RELU else 'tanh'}@{batch}"


def n_layers(g):
    return len(g.hidden) + 1


def entry_dims(g):
    """(in, out) of a network's table entries: the hidden layers, then the head's parts."""
    widths = (g.in0 + g.in1,) + g.hidden
    return list(zip(widths[:-1], widths[1:])) + [(g.hidden[-1], o) for o in g.parts]


def whole_sizes(g):
    """The network as mlp_train_support writes one: in, hidden widths, the head's parts together."""
    return (g.in0 + g.in1,) + g.hidden + (sum(g.parts),)


@functools.lru_cache(maxsize=None)
def layers_of(g):
    """[network][entry] = (W, b), float32 on the CPU, by mlp_train_support's rule, seeded per group."""
    gen = torch.Generator().manual_seed(2000 + GROUPS.index(g))
    return [[(torch.randn((o, i), generator=gen) * (1.4 / max(i, 16) ** 0.5), 0.1 * torch.randn((o,), generator=gen)) for i, o in entry_dims(g)]
            for _ in range(g.n_nets)]


def f64_forward(g, act, layers, x, hidden_out=None):
    """The outputs [network * parts + part] of x [rows, in0 + in1] in the tensors' own precision; hidden_out collects [network][layer] z."""
    outs = []
    for net in layers:
        h, zs = x, []
        for w, b in net[:len(g.hidden)]:
            z = h @ w.t() + b
            zs.append(z)
            h = torch.relu(z) if act == RELU else torch.tanh(z)
        outs += [h @ w.t() + b for w, b in net[len(g.hidden):]]
        if hidden_out is not None:
            hidden_out.append(zs)
    return outs


Selection = collections.namedtuple("Selection", "x kept_share found")


def candidates(g, batch):
    """The 8 batch candidate rows of a case, x ~ N(0, 1)."""
    gen = torch.Generator().manual_seed(3000 + 17 * GROUPS.index(g) + batch)
    return torch.randn((8 * batch, g.in0 + g.in1), generator=gen)


@functools.lru_cache(maxsize=None)
def selection(g, batch):
    """The rows of a case by the rule above, and what the CPU test asserts of it: the share of the candidates that pass, and whether
    `batch` of them were found."""
    cand = candidates(g, batch)
    zs = []
    with torch.no_grad():
        f64_forward(g, RELU, [[(w.double(), b.double()) for w, b in net] for net in layers_of(g)], cand.double(), zs)
    ok = torch.ones(8 * batch, dtype=torch.bool)
    for net in zs:
        for z in net:
            ok &= (z.abs() >= 2 * BOUND * float(z.abs().max())).all(dim=1)
    rows = torch.nonzero(ok).flatten()
    return Selection(cand[rows[:batch]].contiguous(), float(ok.double().mean()), len(rows) >= batch)


@functools.lru_cache(maxsize=None)
def inputs(g, batch):
    """x0, x1 (None with in1 = 0) and d_out [network * parts + part] ~ N(0, 1) / batch."""
    sel = selection(g, batch)
    assert sel.found, (g.name, batch)
    gen = torch.Generator().manual_seed(4000 + 17 * GROUPS.index(g) + batch)
    d_out = [(torch.randn((batch, o), generator=gen) / batch).contiguous() for _ in range(g.n_nets) for o in g.parts]
    return sel.x[:, :g.in0].contiguous(), (sel.x[:, g.in0:].contiguous() if g.in1 else None), d_out


Reference = collections.namedtuple("Reference", "outs grads d_x0 d_x1")


def reference_of(g, act, layers, x0, x1, d_out):
    """outs, the gradients in table order (weight, bias per entry, network by network), d_x0 and d_x1 of the float32 parameters and
    inputs evaluated in float64."""
    lay = [[(w.double().requires_grad_(), b.double().requires_grad_()) for w, b in net] for net in layers]
    x = (x0 if x1 is None else torch.cat((x0, x1), dim=1)).double().requires_grad_()
    outs = f64_forward(g, act, lay, x)
    torch.autograd.backward(outs, [d.double() for d in d_out])
    return Reference([o.detach() for o in outs], [t.grad for net in lay for pair in net for t in pair], x.grad[:, :g.in0].contiguous(),
                     x.grad[:, g.in0:].contiguous() if g.in1 else None)


@functools.lru_cache(maxsize=None)
def reference(g, act, batch):
    return reference_of(g, act, layers_of(g), *inputs(g, batch))


def scratch_bytes(g, batch):
    """The header's formula, restated: n_nets blocks, each the regions of one network with the head's parts taken together."""
    return g.n_nets * T.scratch_bytes(whole_sizes(g), batch)


def tables(K, g, act=RELU, ptrs=None, flags=0):
    """(cfg, layer table) for a group; ptrs: [network][entry] = (weight, bias, d_weight, d_bias) addresses, default a dummy non-NULL one."""
    dims = entry_dims(g)
    ptrs = ptrs or [[(4096, 4096, 4096, 4096)] * len(dims)] * g.n_nets
    table = (K.DnMlpTrainLayer * (g.n_nets * len(dims)))(*[K.DnMlpTrainLayer(*p, i, o) for net in ptrs for p, (i, o) in zip(net, dims)])
    return K.DnSacTrainConfig(g.n_nets, n_layers(g), len(g.parts), act, g.in0, g.in1, flags, 0), table


def pointer_table(addresses):
    return (C.c_void_p * len(addresses))(*addresses)
