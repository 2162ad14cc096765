# Where the hardware puts the waves of the five-wave fused step (census build: -DDN_PLACE_CENSUS on dn_kernels_mw.hip, selected with
# DN_LIB_PATH): every wave of every workgroup of a launch leaves its HW_ID and XCC_ID; this prints, per launch, the SIMD of each wave of
# each CU's tiles, whether tiles b and b + num_cus share a CU, and the distribution of placement patterns over the launches.
#   DN_LIB_PATH=<census lib> python profiles/placement_census.py [n_drones] [launches] [K]
import os, sys, ctypes as C
from collections import Counter, defaultdict
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import drl_dronenavigation_amd as pkg
from drl_dronenavigation_amd import tracks

n = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 24
K = int(sys.argv[3]) if len(sys.argv) > 3 else 64
TILES, WAVES = 1024, 5
dev = torch.device("cuda:0")
num_cus = torch.cuda.get_device_properties(0).multi_processor_count
raw = C.CDLL(pkg._capi.library_path())
buf = (C.c_uint * (TILES * 8 * 2))()
env = pkg.DroneVecEnv(tracks.REGISTRY["reaching"](), n, max_steps=4096, normalize_obs=True, seed=1, device=dev)
env.reset_tensor()
tiles = (n + 63) // 64
assert tiles <= TILES and env.kernel_waves(fused=True) == 5, (tiles, env.kernel_waves(fused=True))
acts = torch.rand((K, n, 4), device=dev) * 2 - 1
print(f"# {n} drones = {tiles} tiles on {num_cus} CUs, {launches} launches of {K} steps, five waves per tile")

pair_patterns, own_patterns, doubled, shared, tiles_on_cu = Counter(), Counter(), Counter(), Counter(), Counter()
first = None
for launch in range(launches):
    env.rollout_tensor(acts)
    assert raw.dn_debug_place(buf) == 0
    v = np.ctypeslib.as_array(buf).reshape(TILES, 8, 2)[:tiles, :WAVES].astype(np.int64)
    hw, xcc = v[..., 0], v[..., 1] & 15
    # HW_REG_HW_ID (gfx9): wave_id [3:0], simd_id [5:4], pipe_id [7:6], cu_id [11:8], sh_id [12], se_id [15:13]
    simd, slot = (hw >> 4) & 3, hw & 15
    cu_key = (xcc << 8) | (((hw >> 13) & 7) << 5) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 15)
    assert (cu_key == cu_key[:, :1]).all(), "a workgroup's waves sit on one CU"
    cu_of = cu_key[:, 0]
    by_cu = defaultdict(list)
    for b in range(tiles):
        by_cu[int(cu_of[b])].append(b)
        s = tuple(int(x) for x in simd[b])
        own_patterns[s] += 1
        c = Counter(s)
        doubled[tuple(sorted(c.values(), reverse=True))] += 1
    for b in range(tiles - num_cus):
        shared[bool(cu_of[b] == cu_of[b + num_cus])] += 1
    for cu, ts in by_cu.items():
        tiles_on_cu[len(ts)] += 1
        if len(ts) == 2:
            a, b = sorted(ts)
            pair_patterns[(tuple(int(x) for x in simd[a]), tuple(int(x) for x in simd[b]), b - a == num_cus)] += 1
    if launch == 0:
        first = (by_cu, simd.copy(), slot.copy(), cu_of.copy(), xcc.copy())

by_cu, simd, slot, cu_of, xcc = first
print(f"## launch 0, per CU (xcc.se.sh.cu): tile: SIMD of waves 0..4 (wave slot of waves 0..4)")
for cu in sorted(by_cu):
    parts = [f"tile {b:4d}: simd {' '.join(str(int(x)) for x in simd[b])} (slots {' '.join(str(int(x)) for x in slot[b])})" for b in sorted(by_cu[cu])]
    print(f"  cu {cu >> 8}.{(cu >> 5) & 7}.{(cu >> 4) & 1}.{cu & 15:2d}  " + "   ".join(parts))
print(f"## xcc of tiles 0..15 in launch 0: {[int(x) for x in xcc[:16, 0]]}")
print(f"## over {launches} launches")
print(f"tiles per occupied CU (CU-launches): {dict(sorted(tiles_on_cu.items()))}")
print(f"tiles b and b + num_cus on the same CU: {dict(shared)}")
print(f"waves per SIMD inside one workgroup, sorted (workgroup-launches): {dict(doubled)}")
print("SIMD of waves 0..4 of one workgroup, the commonest 16:")
for s, k in own_patterns.most_common(16):
    print(f"  {' '.join(map(str, s))}: {k}")
print(f"  ... {len(own_patterns)} distinct")
print("CUs with two tiles: SIMDs of the lower tile | of the higher tile | higher = lower + num_cus, the commonest 24:")
for (a, b, sh), k in pair_patterns.most_common(24):
    print(f"  {' '.join(map(str, a))} | {' '.join(map(str, b))} | {sh}: {k}")
print(f"  ... {len(pair_patterns)} distinct")
# what a workgroup can see of itself against what it shares the CU with: the doubled SIMD of each tile of a pair
dd = Counter()
for (a, b, sh), k in pair_patterns.items():
    da = [s for s, c in Counter(a).items() if c > 1]
    db = [s for s, c in Counter(b).items() if c > 1]
    dd[(tuple(da), tuple(db))] += k
print(f"doubled SIMD of the lower tile, of the higher tile (CU-launches): {dict(dd.most_common(20))}")
env.close()
