#!/usr/bin/env python3
"""What do the entry points without a dn_env refuse, and in which order?  One digest per library, for a host-only change of the checks.

    python profiles/refusal_digest.py LIBRARY

Walks the 28 entry points of include/dronenav.h that take a device_id and no env.  Each starts from one valid call; then every argument
-- a config field and a field of a host table count as arguments -- takes each value of its FULL set alone, and every pair of arguments
takes each pair of values of their SHORT sets, so that a caller's two mistakes meet and the order of the checks shows.

    pointer   FULL: NULL, its own address, off by 1, 2 and 4 bytes, and for every other pointer q of the call q - 16, q - 4, q, q + 4, q + 16
              SHORT: NULL, off by 2, and q for every other pointer q
    integer   FULL: -1, 0, 1, the valid value and its two neighbours, 2^31 - 1, and 2^62 where the type holds it;  SHORT: 0 and the largest
    float     FULL: -inf, -1, -5e-324, 0, 0.5, the two neighbours of 1, 1, +inf, NaN;  SHORT: -1 and NaN
    a config, a host table: FULL and SHORT: NULL and the real one

That is the thinning of the full product: singles over everything, pairs over the SHORT sets, no triples.  Arguments the host reads are
real host memory (the configs, the field, tensor and network tables, counts, the out of dn_minibatch_permutation); device pointers are
numbers that are never followed: device_id is 2^20, so a call that passes validation ends at hipSetDevice with DN_ERR_HIP.  Needs no GPU.

Prints the number of calls per entry point and in all, and an FNV-1a 64 digest over every (entry point, case, status, message).  Run it
once per library, each in a process of its own, on the same machine: the HIP runtime's own error text is part of the messages.
"""
import ctypes as C
import itertools
import math
import sys


class T:
    """The host structs of include/dronenav.h that these entry points read, restated here so that no second library is loaded."""
    MINIBATCH_MAX_FIELDS, ADAM_MAX_TENSORS = 8, 32

    @staticmethod
    def make(name, fields):
        return type(name, (C.Structure,), {"_fields_": fields})


_VP, _I32, _I64, _U64, _F32, _F64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double
T.DnMlpNet = T.make("DnMlpNet", [(n, _VP) for n in ("w1", "w2", "w3", "wh", "b1", "b2", "b3", "bh", "out")]
                    + [(n, _I32) for n in ("out_dim", "grade", "arch", "reserved_")])
T.DnHistoryConfig = T.make("DnHistoryConfig", [(n, _I32) for n in ("frames", "actions", "extra_dim", "reserved")])
T.DnRownormConfig = T.make("DnRownormConfig", [("width", _I32), ("clip", _F32), ("epsilon", _F64)])
T.DnRetnormConfig = T.make("DnRetnormConfig", [("gamma", _F64), ("epsilon", _F64), ("clip", _F32), ("reserved", _I32)])
T.DnMinibatchField = T.make("DnMinibatchField", [("src", _VP), ("dst", _VP), ("width", _I32), ("normalize", _I32)])
T.DnMinibatchConfig = T.make("DnMinibatchConfig", [("seed", _U64), ("epoch", _U64), ("epsilon", _F64), ("num_fields", _I32), ("reserved", _I32)])
T.DnPpoLossConfig = T.make("DnPpoLossConfig", [(n, _F64) for n in ("clip_range", "clip_range_vf", "ent_coef", "vf_coef")]
                           + [("act_dim", _I32), ("reserved", _I32)])
T.DnAdamTensor = T.make("DnAdamTensor", [(n, _VP) for n in ("param", "grad", "exp_avg", "exp_avg_sq")] + [("count", _I64)])
T.DnSacConfig = T.make("DnSacConfig", [(n, _F64) for n in ("gamma", "target_entropy", "ent_coef", "log_std_min", "log_std_max")]
                       + [("act_dim", _I32), ("n_critics", _I32), ("reserved", _I64)])
T.DnSacPointer = T.make("DnSacPointer", [("p", _VP)])        # one entry of a host array of device pointers
T.DnAdamConfig = T.make("DnAdamConfig", [(n, _F64) for n in ("beta1", "beta2", "eps", "max_grad_norm")] + [("n_tensors", _I32), ("flags", _I32)])

DEVICE_ID = 1 << 20
FLOATS = [-math.inf, -1.0, -5e-324, 0.0, 0.5, math.nextafter(1.0, 0.0), 1.0, math.nextafter(1.0, 2.0), math.inf, math.nan]
FLOATS_SHORT = [-1.0, math.nan]
CTYPE = {"i32": C.c_int32, "i64": C.c_int64, "u64": C.c_uint64, "f64": C.c_double, "f32": C.c_float}


def p(name): return ("p", name)
def i32(name, valid): return ("i32", name, valid)
def i64(name, valid): return ("i64", name, valid)
def u64(name, valid): return ("u64", name, valid)
def f64(name, valid): return ("f64", name, valid)
def f32(name, valid): return ("f32", name, valid)
def struct(name, cls, fields, count=1, room=1): return ("s", name, cls, fields, count, room)
def host_i64(name, valid, room): return ("h", name, valid, room)


DEV, STREAM = ("dev",), ("stream",)
NET = [p("w1"), p("w2"), p("w3"), p("wh"), p("b1"), p("b2"), p("b3"), p("bh"), p("out"), i32("out_dim", [4, 1]), i32("grade", 0), i32("arch", 0)]
HISTORY = struct("cfg", T.DnHistoryConfig, [i32("frames", 2), i32("actions", 1), i32("extra_dim", 0), i32("reserved", 0)])
ROWNORM = struct("cfg", T.DnRownormConfig, [i32("width", 13), f32("clip", 10.0), f64("epsilon", 1e-8)])
RETNORM = struct("cfg", T.DnRetnormConfig, [f64("gamma", 0.99), f64("epsilon", 1e-8), f32("clip", 10.0), i32("reserved", 0)])
SAC = struct("cfg", T.DnSacConfig, [f64("gamma", 0.99), f64("target_entropy", -4.0), f64("ent_coef", 0.2), f64("log_std_min", -20.0),
                                    f64("log_std_max", 2.0), i32("act_dim", 4), i32("n_critics", 2), i64("reserved", 0)])
def sac_table(name): return struct(name, T.DnSacPointer, [p("p")], count=2, room=4)
SCRATCH = i64("scratch_bytes", None)         # None: what the entry point's dn_X_scratch_bytes gives for the valid call

# entry point -> (arguments in order, the call that sizes its scratch or None)
ENTRY_POINTS = {
    "dn_compact_done": ([p("done_mask"), i64("num_envs", 64), p("indices"), p("count"), DEV, STREAM], None),
    "dn_pack_done": ([p("done_mask"), i64("num_envs", 64), p("terminal_obs"), p("ep_return"), p("ep_length"), p("truncated"), p("found_targets"),
                      p("indices"), p("count"), p("packed"), DEV, STREAM], None),
    "dn_stream_copy": ([p("dst"), p("src"), i64("bytes", 64), DEV, STREAM], None),
    "dn_preprocess_action": ([p("actions"), i64("num_envs", 64), i32("normalize_actions", 1), p("rpm"), p("forces"), p("z_torque"), DEV, STREAM], None),
    "dn_add_bootstrap": ([p("reward"), p("terminal_value"), p("truncated"), f64("gamma", 0.99), i64("num_envs", 64), DEV, STREAM], None),
    "dn_mlp_forward": ([struct("nets", T.DnMlpNet, NET, count=2, room=2), i32("num_nets", 2), p("obs"), p("row_mask"), i64("num_envs", 64),
                        i32("obs_dim", 13), DEV, STREAM], None),
    "dn_gae": ([p("rewards"), p("values"), p("dones"), p("last_values"), p("last_dones"), i64("n_steps", 8), i64("n_envs", 64), f64("gamma", 0.99),
                f64("gae_lambda", 0.95), p("advantages"), p("returns"), DEV, STREAM], None),
    "dn_history_width": ([HISTORY], None),
    "dn_stack_history": ([HISTORY, i64("k", 2), i64("n", 64), p("prev"), p("obs"), p("actions"), p("done"), p("terminal_obs"), p("extra"),
                          p("terminal_extra"), p("rows"), p("terminal_rows"), DEV, STREAM], None),
    "dn_rownorm_state_doubles": ([i32("width", 13)], None),
    "dn_rownorm_scratch_bytes": ([i64("k", 2), i64("n", 64), i32("width", 13)], None),
    "dn_rownorm_init": ([ROWNORM, p("stats"), DEV, STREAM], None),
    "dn_rownorm": ([ROWNORM, p("stats"), i64("k", 2), i64("n", 64), p("rows"), p("out"), i32("update", 1), p("scratch"), SCRATCH, DEV, STREAM],
                   ("dn_rownorm_scratch_bytes", (_I64, _I64, _I32), (2, 64, 13))),
    "dn_retnorm_scratch_bytes": ([i64("k", 2), i64("n", 64)], None),
    "dn_retnorm_init": ([p("stats"), p("returns"), i64("n", 64), DEV, STREAM], None),
    "dn_retnorm": ([RETNORM, p("stats"), p("returns"), i64("k", 2), i64("n", 64), p("rewards"), p("done"), p("out"), i32("update", 1), p("scratch"),
                    SCRATCH, DEV, STREAM], ("dn_retnorm_scratch_bytes", (_I64, _I64), (2, 64))),
    "dn_minibatch_scratch_bytes": ([i64("batch", 64)], None),
    "dn_minibatch_permutation": ([u64("seed", 1), u64("epoch", 0), i64("m", 10), i64("start", 2), i64("count", 4), host_i64("out", [], 16)], None),
    "dn_minibatch": ([struct("cfg", T.DnMinibatchConfig, [u64("seed", 1), u64("epoch", 0), f64("epsilon", 1e-8), i32("num_fields", 2), i32("reserved", 0)]),
                      struct("fields", T.DnMinibatchField, [p("src"), p("dst"), i32("width", [4, 1]), i32("normalize", [0, 1])], count=2,
                             room=T.MINIBATCH_MAX_FIELDS),
                      i64("n_steps", 8), i64("n_envs", 16), i64("start", 0), i64("batch", 32), p("indices"), p("epoch_offset"), p("indices_out"),
                      p("scratch"), SCRATCH, DEV, STREAM], ("dn_minibatch_scratch_bytes", (_I64,), (32,))),
    "dn_ppo_loss_scratch_bytes": ([i64("batch", 8), i32("act_dim", 4)], None),
    "dn_ppo_loss": ([struct("cfg", T.DnPpoLossConfig, [f64("clip_range", 0.2), f64("clip_range_vf", 0.2), f64("ent_coef", 0.01), f64("vf_coef", 0.5),
                                                       i32("act_dim", 4), i32("reserved", 0)]),
                     i64("batch", 8)] + [p(n) for n in ("mean", "log_std", "value", "actions", "old_log_prob", "advantages", "returns", "old_values",
                                                        "d_mean", "d_log_std", "d_value", "log_prob_out", "loss", "stats", "scratch")]
                    + [SCRATCH, DEV, STREAM], ("dn_ppo_loss_scratch_bytes", (_I64, _I32), (8, 4))),
    "dn_adam_scratch_bytes": ([host_i64("counts", [100, 5000], T.ADAM_MAX_TENSORS), i32("n_tensors", 2)], None),
    "dn_adam_step": ([struct("cfg", T.DnAdamConfig, [f64("beta1", 0.9), f64("beta2", 0.999), f64("eps", 1e-8), f64("max_grad_norm", 0.5),
                                                     i32("n_tensors", 2), i32("flags", 0)]),
                      struct("tensors", T.DnAdamTensor, [p("param"), p("grad"), p("exp_avg"), p("exp_avg_sq"), i64("count", [100, 5000])], count=2,
                             room=T.ADAM_MAX_TENSORS),
                      p("lr"), p("state"), p("stats"), p("scratch"), SCRATCH, DEV, STREAM],
                     ("dn_adam_scratch_bytes", (lambda v: (_I64 * 2)(*v), _I32), ((100, 5000), 2))),
    "dn_sac_loss_scratch_bytes": ([i64("batch", 8), i32("n_critics", 2)], None),
    "dn_sac_policy": ([SAC, i64("batch", 8)] + [p(n) for n in ("mean", "log_std", "noise", "actions", "log_prob")] + [DEV, STREAM], None),
    "dn_sac_policy_backward": ([SAC, i64("batch", 8)] + [p(n) for n in ("mean", "log_std", "noise", "g_actions", "g_log_prob", "d_mean", "d_log_std")]
                               + [DEV, STREAM], None),
    "dn_sac_critic_loss": ([SAC, i64("batch", 8), sac_table("q"), sac_table("next_q")] + [p(n) for n in ("next_log_prob", "rewards", "dones", "log_ent_coef")]
                           + [sac_table("d_q")] + [p(n) for n in ("target_q", "loss", "stats", "scratch")] + [SCRATCH, DEV, STREAM],
                           ("dn_sac_loss_scratch_bytes", (_I64, _I32), (8, 2))),
    "dn_sac_actor_loss": ([SAC, i64("batch", 8), p("log_prob"), sac_table("q_pi"), p("log_ent_coef"), p("d_log_prob"), sac_table("d_q_pi")]
                          + [p(n) for n in ("d_log_ent_coef", "actor_loss", "ent_coef_loss", "stats", "scratch")] + [SCRATCH, DEV, STREAM],
                          ("dn_sac_loss_scratch_bytes", (_I64, _I32), (8, 2))),
}


def ints(kind, valid):
    big = [(1 << 31) - 1] + ([1 << 62] if kind == "i64" else [])
    if kind == "u64":
        return [0, 1, (1 << 64) - 1], [(1 << 64) - 1]
    return sorted({-1, 0, 1, valid - 1, valid, valid + 1, *big}), [0, big[-1]]


class Walk:
    """The dimensions of one entry point: key -> (valid value, FULL values, SHORT values); pointer values are (label, address)."""

    def __init__(self, lib, name):
        self.lib, self.name = lib, name
        self.args, sizer = ENTRY_POINTS[name]
        self.fn = getattr(lib, name)
        self.fn.restype = C.c_int64 if name.endswith(("_scratch_bytes", "_state_doubles")) else C.c_int32
        self.valid, self.pointers = {}, []
        self.dims = {}
        scratch = None
        if sizer:
            f = getattr(lib, sizer[0])
            f.restype = C.c_int64
            scratch = f(*[t(v) for t, v in zip(sizer[1], sizer[2])])
        for a in self.args:
            self.declare(a, "", 0, scratch)
        for key in self.pointers:
            base = self.valid[key][1]
            full = [("null", 0), ("own", base), ("+1", base + 1), ("+2", base + 2), ("+4", base + 4)]
            short = [("null", 0), ("+2", base + 2)]
            for q in self.pointers:
                if q != key:
                    qb = self.valid[q][1]
                    full += [("%s%+d" % (q, d), qb + d) for d in (-16, -4, 0, 4, 16)]
                    short.append(("%s+0" % q, qb))
            self.dims[key] = (full, short)

    def declare(self, a, prefix, index, scratch):
        kind = a[0]
        if kind in ("dev", "stream"):
            return
        key = prefix + a[1]
        if kind == "p":
            self.valid[key] = ("own", 0x10000000 + 0x1000000 * len(self.pointers))
            self.pointers.append(key)
        elif kind in ("i32", "i64", "u64"):
            v = a[2][index] if isinstance(a[2], list) else scratch if a[2] is None else a[2]
            self.valid[key] = v
            self.dims[key] = ints(kind, v)
        elif kind in ("f32", "f64"):
            self.valid[key] = a[2]
            self.dims[key] = (FLOATS, FLOATS_SHORT)
        elif kind == "s":
            self.valid[key] = "real"
            self.dims[key] = (["null", "real"], ["null", "real"])
            for k in range(a[4]):
                for f in a[3]:
                    self.declare(f, "%s[%d]." % (key, k) if a[5] > 1 else key + ".", k, scratch)
        elif kind == "h":
            self.valid[key] = "real"
            self.dims[key] = (["null", "real"], ["null", "real"])
            for k, v in enumerate(a[2]):
                self.valid["%s[%d]" % (key, k)] = v
                self.dims["%s[%d]" % (key, k)] = ints("i64", v)

    def call(self, values):
        keep, argv = [], []
        for a in self.args:
            kind = a[0]
            if kind == "dev":
                argv.append(C.c_int32(DEVICE_ID))
            elif kind == "stream":
                argv.append(C.c_void_p(0))
            elif kind == "p":
                argv.append(C.c_void_p(values[a[1]][1]))
            elif kind == "s":
                table = (a[2] * a[5])()
                for k in range(a[4]):
                    for f in a[3]:
                        v = values[("%s[%d]." % (a[1], k) if a[5] > 1 else a[1] + ".") + f[1]]
                        setattr(table[k], f[1], v[1] if f[0] == "p" else v)
                keep.append(table)
                argv.append(C.cast(table, C.c_void_p) if values[a[1]] == "real" else C.c_void_p(0))
            elif kind == "h":
                table = (C.c_int64 * a[3])(*[values["%s[%d]" % (a[1], k)] for k in range(len(a[2]))])
                keep.append(table)
                argv.append(C.cast(table, C.c_void_p) if values[a[1]] == "real" else C.c_void_p(0))
            else:
                argv.append(CTYPE[kind](values[a[1]]))
        status = self.fn(*argv)
        return status, (self.lib.dn_last_error().decode() if status < 0 else "")

    def cases(self):
        yield {}
        for key, (full, _) in self.dims.items():
            for v in full:
                yield {key: v}
        for (ka, (_, sa)), (kb, (_, sb)) in itertools.combinations(self.dims.items(), 2):
            for va, vb in itertools.product(sa, sb):
                yield {ka: va, kb: vb}


def label(v):
    return v[0] if isinstance(v, tuple) else repr(v)


def main(path):
    lib = C.CDLL(path)
    lib.dn_last_error.restype = C.c_char_p
    digest, total = 0xcbf29ce484222325, 0
    for name in ENTRY_POINTS:
        walk, calls = Walk(lib, name), 0
        for case in walk.cases():
            status, message = walk.call(dict(walk.valid, **case))
            line = "%s|%s|%d|%s\n" % (name, ",".join("%s=%s" % (k, label(v)) for k, v in case.items()), status, message)
            for byte in line.encode():
                digest = ((digest ^ byte) * 0x100000001b3) & 0xffffffffffffffff
            calls += 1
        print("%-28s %7d calls" % (name, calls))
        total += calls
    print("%d calls, digest %016x" % (total, digest))


if __name__ == "__main__":
    main(sys.argv[1])
