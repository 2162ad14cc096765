"""What tests/test_gpu_role_sweep.py shares with the child process it starts: the sweep build of the five-wave fused step (csrc/dn_kernels.hip
under -DDN_5W_ROLE_SWEEP) takes its role table, its fallback orders and its priorities from a device buffer, so one library runs every
wave-to-role assignment, and every one must give the bits of the one-wave kernel.  The variant lists, the flight both processes make
(fly), and the child itself: `python tests/role_sweep_support.py JOB.json` with DN_LIB_PATH naming the sweep library.  A plain module:
pytest does not collect it and does not rewrite its asserts, so every assert here carries its own message."""
import ctypes as C
import itertools
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drl-dronenavigation_amd", "csrc")
DEV = "cuda:0"

N1 = 132                                    # two tiles and a ragged one of four rows, all first tiles
CHAINS = {"N1": (2, 3, 7, 20), "N2": (2, 7)}    # launches chained from one reset: state, statistics and the skewed pipeline carry over
NOISES = ({}, {"obs_noise_sigma": 0.01, "act_noise_sigma": 0.001})      # the NOISE = false and NOISE = true instantiations
DASHES = ["-----"] * 4
PERMS = ["".join(p) for p in itertools.permutations("LAQXN")]


def n2(num_cus):
    """One full and one ragged second tile beside a full set of first tiles."""
    return 64 * (num_cus + 1) + 4


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def shipped():
    """(the eight rows of DN_ROLE_TABLE, the two orders of DN_ROLE_ORDER, DN_5W_PRIO), read from the sources the library is built from."""
    head = _source("dn_role_place.h")
    rows = re.findall(r'"([LAQXN-]{5})"', re.search(r"DnRoleTable DN_ROLE_TABLE = (.*);", head).group(1))
    orders = re.findall(r'"([LAQXN]{5})"', re.search(r"DN_ROLE_ORDER\[2\]\[6\] = (.*);", head).group(1))
    prio = re.search(r'#define DN_5W_PRIO "([0-3]{5})"', _source("dn_kernels.hip")).group(1)
    assert len(rows) == 8 and len(orders) == 2, (rows, orders)
    return rows, orders, prio


def rot2(pi):
    return pi[2:] + pi[:2]


def value(rows, orders, prio):
    """The eleven-word value of DN_5W_ROLE_SWEEP: eight table rows, two fallback orders, the priorities of L A Q X N."""
    return ",".join(list(rows) + list(orders) + [prio])


def family(name):
    """[(label, value of DN_5W_ROLE_SWEEP)] of a variant family."""
    rows, orders, prio = shipped()
    if name == "forced":        # the table names nothing: wave w runs pi[w] (second tile: rotated pi[w]) through the device's fallback branch
        return [(f"forced {pi}|{rot2(pi)}", value(DASHES * 2, (pi, rot2(pi)), prio)) for pi in PERMS]
    if name == "ranked":        # every named placement gives the wave of rank r the role pi[r]: dn_place_rank on the device
        return [(f"ranked {pi}|{rot2(pi)}", value([pi] * 4 + [rot2(pi)] * 4, orders, prio)) for pi in PERMS]
    if name == "priorities":    # priorities move the roles' relative timing; the mail slots are double-buffered on barriers alone
        mirror = "".join(str(3 - int(ch)) for ch in prio)
        assert (prio, mirror) == ("22311", "11022"), (prio, mirror)
        return [(f"{what} prio {pr}", value(r, orders, pr)) for pr in ("00000", "33333", prio, mirror)
                for what, r in (("shipped table", rows), ("forced shipped orders", DASHES * 2))]
    raise ValueError(name)


def parser_cases():
    """(accepted values, refused values) of dn_debug_role_sweep."""
    rows, orders, prio = shipped()
    nine = ",".join(rows + [prio])                                      # what profiles/sweep_5w_roles.py sends
    good = [("nine words", nine), ("eleven words", value(rows, orders, prio)), ("eleven words, forced", value(DASHES * 2, ("XNAQL", "QLXNA"), "01230"))]
    bad = [("ten words", ",".join(rows + [orders[0], prio])),
           ("an order with a repeated letter", value(rows, ("LQANN", orders[1]), prio)),
           ("an order with a dash", value(rows, (orders[0], "ANLQ-"), prio)),
           ("an order of dashes", value(rows, ("-----", orders[1]), prio)),
           ("a row that is no permutation", value(["XNQLL"] + rows[1:], orders, prio)),
           ("a row that is no permutation, nine words", ",".join(["XNQLL"] + rows[1:] + [prio])),
           ("a priority of 4", value(rows, orders, "22411")),
           ("twelve words", value(rows, orders, prio) + "," + prio),
           ("an empty value", "")]
    return good, bad


def actions(torch, n, steps):
    """Seeded U(-1, 1), the same in every process."""
    gen = torch.Generator().manual_seed(1000 + n)
    return (torch.rand((steps, n, 4), generator=gen) * 2 - 1).to(DEV)


def fly(pkg, torch, n, chain, noise, acts, want=None, tag=""):
    """A fresh environment of seed 7 (normaliser on, max_steps = 3: episodes end inside launches and on their edges), its reset, and the
    launches of `chain` one after the other on successive actions.  Returns {"launch<j>.<tensor>": device tensor of everything
    rollout_tensor(want_terminal=True) returns, "state.<field>": bytes of every field of get_state(), "stats": repr, "waves", "num_cus"}.
    With `want` (such a dict) every entry is compared as it arrives, on the device, and the first that differs raises with `tag`."""
    from drl_dronenavigation_amd import tracks
    env = pkg.DroneVecEnv(tracks.reaching(), n, normalize_obs=True, max_steps=3, seed=7, device=DEV, **noise)
    got = {}

    def keep(name, x):
        if want is not None:
            assert name in want, f"{tag}: {name} is not in the reference"
            same = torch.equal(x, want[name]) if torch.is_tensor(x) else x == want[name]
            assert same, f"MISMATCH {tag}: fleet {n}, {name} differs from the one-wave reference"
        got[name] = x

    try:
        env.reset()
        got["waves"], got["num_cus"] = env.kernel_waves(fused=True), env.num_cus
        t = 0
        for j, k in enumerate(chain):
            out = env.rollout_tensor(acts[t:t + k].contiguous(), want_terminal=True)
            t += k
            for name, x in out.items():
                keep(f"launch{j}(K={k}).{name}", x)
        torch.cuda.synchronize()
        state = env.get_state()              # every field of dn_env_state (the normaliser's rms_* with rms_m2); the struct's padding bytes are nobody's
        import numpy as np
        for name in state.dtype.names:
            keep(f"state.{name}", np.ascontiguousarray(state[name]).tobytes())
        keep("stats", repr(sorted(env.stats().items())))
    finally:
        env.close()
    if want is not None:
        missing = set(want) - set(got)
        assert not missing, f"{tag}: {sorted(missing)} of the reference were not produced"
    return got


def check_reference(ref, chain):
    names = {n.split(".", 1)[1] for n in ref if n.startswith("launch0")}
    assert names >= {"obs", "reward", "done", "truncated", "found_targets", "terminal_obs", "ep_return", "ep_length", "done_mask"}, names
    assert {"state.rms_mean", "state.rms_var", "state.rms_count", "state.rms_m2", "stats"} <= set(ref), sorted(ref)
    assert any(bool(ref[f"launch{j}(K={k}).done"].any()) for j, k in enumerate(chain)), "max_steps = 3: some episode must end in the chain"


def to_host(res):
    """The numpy form of what fly returns, for an .npz file: tensors as arrays, bytes and strings as uint8 arrays."""
    import numpy as np
    out = {}
    for name, v in res.items():
        if hasattr(v, "cpu"):
            out[name] = v.cpu().numpy()
        elif isinstance(v, (str, bytes)):
            out[name] = np.frombuffer(v.encode() if isinstance(v, str) else v, np.uint8)
        else:
            out[name] = np.asarray(v)
    return out


LETTERS = "LAQXN"                           # the role numbers of dn_role_place.h
SEEN_TILES = 1024                           # DN_SWEEP_TILES of the sweep build


def check_roles_seen(seen, v, n, num_cus, tag):
    """`seen`: what dn_debug_role_seen gives after a five-wave launch under the value `v` -- [tile][wave] role numbers.  Every tile's five
    waves ran a permutation of the roles; where the table names nothing for a tile (rows "-----") wave w ran order[tile kind][w], i.e. the
    forced assignment is the one that flew.  Returns (the number of tiles held to a forced order, the number of tiles with named rows whose
    waves ran something else than the fallback order: the table's branch, for certain)."""
    words = v.split(",") if v is not None else []
    rows = words[:8] if words else DASHES * 2
    orders = words[8:10] if len(words) == 11 else shipped()[1]
    forced = named = 0
    for tile in range(min((n + 63) // 64, SEEN_TILES)):
        second = (tile // num_cus) & 1
        assert all(int(r) < 5 for r in seen[tile][:5]), f"{tag}: tile {tile} ran the role numbers {list(seen[tile][:5])}"
        ran = "".join(LETTERS[int(r)] for r in seen[tile][:5])
        assert sorted(ran) == sorted(LETTERS), f"{tag}: the waves of tile {tile} ran {ran}, no permutation of the roles"
        if all(r == "-----" for r in rows[4 * second:4 * second + 4]):
            assert ran == orders[second], f"{tag}: the waves of tile {tile} ({'second' if second else 'first'}) ran {ran}, forced was {orders[second]}"
            forced += 1
        elif ran != orders[second]:
            named += 1
    return forced, named


def main(job_path):
    """The child: DN_LIB_PATH names the sweep library.  Job: {"fleet": "N1" | "N2", "n", "family": "forced" | "ranked" | "priorities" |
    "parser" | "reference", "report": path of the JSON result, "npz": path (family "reference")}.  Exit status 1 with one MISMATCH line on
    the first variant, launch and tensor that differs from the same library's one-wave kernels."""
    with open(job_path) as f:
        job = json.load(f)
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import drl_dronenavigation_amd as pkg
    path = pkg._capi.library_path()
    assert path == os.environ.get("DN_LIB_PATH") and os.path.basename(path) == "libdronenav_role_sweep.so", path
    raw = C.CDLL(path)
    n, chain, fam = job["n"], CHAINS[job["fleet"]], job["family"]
    acts = actions(torch, n, sum(chain))
    rows, orders, prio = shipped()
    report = {"fleet": job["fleet"], "n": n, "family": fam, "library": path, "variants": 0, "flights": 0, "refused": 0, "forced_tiles": 0,
              "named_tiles": 0, "seconds": {}}
    seen = np.zeros((SEEN_TILES, 8), np.uint8)

    def set_variant(v):
        os.environ["DN_5W_ROLE_SWEEP"] = v
        return raw.dn_debug_role_sweep()

    for noise in NOISES:
        label = "noise" if noise else "plain"
        t0 = time.perf_counter()
        os.environ["DN_WAVES"] = "1"
        ref = fly(pkg, torch, n, chain, noise, acts)
        assert ref["waves"] == 1, ref["waves"]
        assert job["fleet"] == "N1" and n == N1 or job["fleet"] == "N2" and n == n2(ref["num_cus"]), (job["fleet"], n, ref["num_cus"])
        check_reference(ref, chain)
        os.environ["DN_WAVES"] = "5"

        def variant(name, v):
            assert set_variant(v) == 0, f"{name}: dn_debug_role_sweep refused {v!r}"
            return flight(f"variant {name} ({v}), {label}", v)

        def flight(tag, v):
            """One flight under the value `v` (None: no value) against the reference, then the roles its last launch's waves ran."""
            report["flights"] += 1
            got = fly(pkg, torch, n, chain, noise, acts, want=ref, tag=tag)
            assert got["waves"] == 5, f"{tag}: kernel_waves(fused=True) is {got['waves']}"
            seen[:] = 255
            assert raw.dn_debug_role_seen(seen.ctypes.data_as(C.c_void_p)) == 0, f"{tag}: dn_debug_role_seen"
            forced, named = check_roles_seen(seen, v, n, got["num_cus"], tag)
            report["forced_tiles"] += forced
            report["named_tiles"] += named
            return got

        if fam == "reference":          # for the parent, which flies the shipped library: the one-wave reference and the shipped table's five waves
            five = variant("shipped table", value(rows, orders, prio))
            np.savez(job["npz"] + f".{label}.w1.npz", **to_host(ref))
            np.savez(job["npz"] + f".{label}.w5.npz", **to_host(five))
            report["variants"] += 1
        elif fam == "parser":
            good, bad = parser_cases()
            for name, v in good:
                variant(name, v)
                report["variants"] += 1
                for bad_name, b in bad:     # each refusal leaves the accepted variant in force: the next launches still match
                    assert set_variant(b) == 1, f"{bad_name}: dn_debug_role_sweep took {b!r}"
                    report["refused"] += 1
                flight(f"variant {name} ({v}) after {len(bad)} refusals, {label}", v)
            del os.environ["DN_5W_ROLE_SWEEP"]      # no value: the fallback orders in every placement, the shipped priorities
            assert raw.dn_debug_role_sweep() == 0, "dn_debug_role_sweep without a value"
            flight(f"no value, {label}", None)
        else:
            for name, v in family(fam):
                variant(name, v)
                report["variants"] += 1
        torch.cuda.synchronize()
        report["seconds"][label] = round(time.perf_counter() - t0, 3)
    with open(job["report"], "w") as f:
        json.dump(report, f)


if __name__ == "__main__":
    try:
        main(sys.argv[1])
    except AssertionError as e:
        print(e, file=sys.stderr, flush=True)
        sys.exit(1)
