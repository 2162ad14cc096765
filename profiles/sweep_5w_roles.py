# Role orders and static priorities of the five-wave fused step, swept on one library (sweep build: -DDN_5W_ROLE_SWEEP on
# dn_kernels_mw.hip, selected with DN_LIB_PATH): the kernel takes its role table and priorities from a device buffer that
# dn_debug_role_sweep fills from the environment variable DN_5W_ROLE_SWEEP, so every variant replays the SAME hipGraph of 20 launches
# of 64 steps (as profiles/time_fused.py does).  One process, one time limit outside; the first failure ends it.
#   DN_LIB_PATH=<sweep lib> python profiles/sweep_5w_roles.py [n_drones] [uniform|hover] [stages, e.g. 123]
#
# The census (profiles/placement_census.py, profiles/role_placement.md) says a tile's waves go to the SIMDs in the cyclic order
# 0 2 1 3 from a start that varies by CU, and the second tile of a CU starts one place further on: which waves share a SIMD follows from
# the wave index and the tile alone.  So a variant is a pair of wave-index orders (first tile | second tile); order_rows() states it
# in the table's terms, one row per doubled SIMD, ranks by (SIMD id, wave index).
import os, sys, itertools, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import drl_dronenavigation_amd as pkg
from drl_dronenavigation_amd import tracks

n = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
dist = sys.argv[2] if len(sys.argv) > 2 else "uniform"
stages = sys.argv[3] if len(sys.argv) > 3 else "123"
K, LAUNCHES = 64, 20
CYCLE = (0, 2, 1, 3)
BASE = ("LQANX", "ANLQX", "22311")


def order_rows(order):
    rows = [None] * 4
    for k in range(4):
        simd = [CYCLE[(k + w) % 4] for w in range(5)]
        ranked = sorted(range(5), key=lambda w: (simd[w], w))
        rows[CYCLE[k]] = "".join(order[w] for w in ranked)
    return rows


dev = torch.device("cuda:0")
raw = C.CDLL(pkg._capi.library_path())
env = pkg.DroneVecEnv(tracks.REGISTRY["reaching"](), n, max_steps=4096, normalize_obs=True, seed=1, device=dev)
env.reset_tensor()
assert env.kernel_waves(fused=True) == 5
torch.manual_seed(0)
acts = (torch.rand((K, n, 4), device=dev) * 2 - 1) if dist == "uniform" else (0.0922 + 0.003 * torch.randn((K, n, 4), device=dev))
s = torch.cuda.Stream(dev)
with torch.cuda.stream(s):
    out = env.rollout_tensor(acts)
    for _ in range(25): env.rollout_tensor(acts, out=out)       # into the steady state of episode ends
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(LAUNCHES): env.rollout_tensor(acts, out=out)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def set_variant(v):
    a, b, prio = v
    os.environ["DN_5W_ROLE_SWEEP"] = ",".join(order_rows(a) + order_rows(b) + [prio])
    assert raw.dn_debug_role_sweep() == 0, v


def replay_us():
    e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / LAUNCHES / K


def measure(variants, reps, label):
    """us per step of each variant: the best of `reps` replays, the variants taken in turn within each repetition."""
    best = {v: 1e9 for v in variants}
    for rep in range(reps):
        for k, v in enumerate(variants):
            set_variant(v)
            best[v] = min(best[v], replay_us())
            if k % 2000 == 1999: print(f"  .. {label} rep {rep}: {k + 1} of {len(variants)}", flush=True)
    return best


def show(title, best, top):
    print(f"## {title}")
    ranked = sorted(best.items(), key=lambda kv: kv[1])
    for v, us in ranked[:top]:
        print(f"  {v[0]} | {v[1]} | {v[2]}: {us:.4f}" + ("   <- shipped before this sweep" if v == BASE else ""))
    if BASE in best:
        print(f"  {BASE[0]} | {BASE[1]} | {BASE[2]}: {best[BASE]:.4f} is rank {[v for v, _ in ranked].index(BASE) + 1} of {len(ranked)}; worst {ranked[-1][1]:.4f}")
    return [v for v, _ in ranked]


print(f"# {n} drones, {dist} actions, graph of {LAUNCHES} launches of {K} steps; us per vector step", flush=True)
set_variant(BASE)
print("baseline, ten replays:", " ".join(f"{replay_us():.4f}" for _ in range(10)), flush=True)
orders = ["".join(p) for p in itertools.permutations("LAQXN")]
keep = [BASE]
if "1" in stages:       # the whole grid of order pairs at the shipped priorities, one replay each, then the best 200 again
    grid = [(a, b, BASE[2]) for a in orders for b in orders]
    best = measure(grid, 1, "grid")
    ranked = show("stage 1: all 14 400 order pairs, one replay each", best, 20)
    cand = ranked[:200] + ([BASE] if BASE not in ranked[:200] else [])
    best = measure(cand, 5, "best 200")
    keep = show("stage 2: the best 200 (and the baseline), best of five replays in turn", best, 30)[:4]
    if BASE not in keep: keep.append(BASE)
if "3" in stages:       # priorities 1..3 per role around each kept order pair
    prios = ["".join(p) for p in itertools.product("123", repeat=5) if "3" in p or p == tuple("22211")]
    grid = [(a, b, pr) for (a, b, _) in keep for pr in prios]
    best = measure(grid, 3, "priorities")
    ranked = show("stage 3: priorities of L A Q X N in 1..3 on the kept order pairs, best of three", best, 30)
    final = ranked[:12] + [v for v in keep if v not in ranked[:12]]
    best = measure(final, 10, "final")
    show("final: the best twelve and the kept pairs, best of ten replays in turn", best, 20)
    # spread of the winner and of the baseline: ten replays each, alternating
    win = sorted(best.items(), key=lambda kv: kv[1])[0][0]
    rows = {win: [], BASE: []}
    for _ in range(10):
        for v in rows:
            set_variant(v); rows[v].append(replay_us())
    for v, r in rows.items():
        print(f"  {v}: " + " ".join(f"{x:.4f}" for x in r))
set_variant(BASE)
env.close()
print("sweep done")
