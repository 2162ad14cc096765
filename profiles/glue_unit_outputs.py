#!/usr/bin/env python3
"""The outputs of the rollout-glue kernels whose text the glue unit changed, bit for bit, from two builds of the library:
    python3 profiles/glue_unit_outputs.py PARENT_LIBRARY [DIRECTORY]   both builds, each in a fresh child process, then the comparison;
                                                                      exit status 0 when every array has the same bytes
    python3 profiles/glue_unit_outputs.py write OUT.npz                one build (DN_LIB_PATH picks it; unset = the in-tree library)
    python3 profiles/glue_unit_outputs.py compare A.npz B.npz
What is kept, as the integer view of its bytes, with the shapes and inputs of tests/rollout_glue_support.py:
  dn_policy_sample  at every fleet of FLEETS and every row of LOG_STD_ROWS, sampled and deterministic: actions, clipped, log_prob
  dn_pack_done      at every size of PACK_SIZES and every density of PACK_DENSITIES: count, indices[:count], packed[:count]
  dn_compact_done   on the same masks: count, indices[:count]
tests/test_gpu_rollout_glue.py holds the same calls to their references; the sampled actions it bounds (one ulp of expf) and does not
pin, which is what this comparison adds."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
SEED = 20240917


def write(target):
    import torch

    import drl_dronenavigation_amd as pkg
    import rollout_glue_support as R
    from drl_dronenavigation_amd import _capi, tracks

    dev = torch.device("cuda:0")
    lib = _capi.load()
    to = lambda a: torch.from_numpy(np.array(a, order="C")).to(dev)  # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731
    out = {}

    def keep(tag, t):
        out[tag] = t.detach().cpu().contiguous().view(torch.int32).numpy()

    for n in R.FLEETS:
        env = pkg.DroneVecEnv(tracks.reaching(), n, device=dev, env_id_offset=12345)
        env.reset_tensor()
        mean = to(R.means(n))
        for ls in R.LOG_STD_ROWS:
            for det in (0, 1):
                a, c, lp = torch.empty((n, 4), device=dev), torch.empty((n, 4), device=dev), torch.empty(n, device=dev)
                _capi.check(lib.dn_policy_sample(env._handle, mean.data_ptr(), (C.c_float * 4)(*ls), SEED, det, a.data_ptr(), c.data_ptr(),
                                                 lp.data_ptr(), stream()))
                torch.cuda.synchronize(dev)
                for name, t in (("actions", a), ("clipped", c), ("log_prob", lp)):
                    keep(f"policy_sample/{n}/{ls}/{det}/{name}", t)
        env.close()
    for n in R.PACK_SIZES:
        tobs, ep_ret, ep_len, trunc, found = (to(x) for x in R.pack_inputs(n))
        for density in R.PACK_DENSITIES:
            mask = to(R.mask_words(R.done_bits(n, density), n))
            idx, cnt = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
            idx2, cnt2, packed = torch.zeros_like(idx), torch.zeros_like(cnt), torch.zeros((n, 16), device=dev)
            _capi.check(lib.dn_pack_done(mask.data_ptr(), n, tobs.data_ptr(), ep_ret.data_ptr(), ep_len.data_ptr(), trunc.data_ptr(),
                                         found.data_ptr(), idx.data_ptr(), cnt.data_ptr(), packed.data_ptr(), 0, stream()))
            _capi.check(lib.dn_compact_done(mask.data_ptr(), n, idx2.data_ptr(), cnt2.data_ptr(), 0, stream()))
            torch.cuda.synchronize(dev)
            k, k2 = int(cnt.item()), int(cnt2.item())
            for name, t in (("pack/count", cnt), ("pack/indices", idx[:k]), ("pack/packed", packed[:k]), ("compact/count", cnt2),
                            ("compact/indices", idx2[:k2])):
                keep(f"{name}/{n}/{density}", t)
    os.makedirs(os.path.dirname(os.path.abspath(target)), exist_ok=True)
    np.savez(target, **out)
    print(f"{len(out)} arrays, {sum(a.nbytes for a in out.values())} bytes -> {target} (library: {os.environ.get('DN_LIB_PATH', 'in-tree')})")


def compare(first, second):
    a, b = np.load(first), np.load(second)
    names = sorted(set(a.files) | set(b.files))
    differ = [n for n in names if n not in a.files or n not in b.files or not np.array_equal(a[n], b[n])]
    for n in differ:
        print("differs:", n)
    print(f"{len(names)} arrays, {len(differ)} differ")
    return 1 if differ or not names else 0


def both(parent_library, directory):
    files = []
    for tag, env in (("parent", dict(os.environ, DN_LIB_PATH=os.path.abspath(parent_library))),
                     ("this_build", {k: v for k, v in os.environ.items() if k != "DN_LIB_PATH"})):
        files.append(os.path.join(directory, f"glue_unit_outputs_{tag}.npz"))
        subprocess.run([sys.executable, os.path.abspath(__file__), "write", files[-1]], env=env, check=True, timeout=300)
    return compare(*files)


if __name__ == "__main__":
    if sys.argv[1] == "write":
        sys.exit(write(sys.argv[2]))
    if sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(both(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else tempfile.gettempdir()))
