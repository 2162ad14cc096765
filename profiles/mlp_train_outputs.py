#!/usr/bin/env python3
"""Every output of dn_mlp_train_forward / dn_mlp_train_backward, bit for bit, for comparing two builds of the library:
    python3 profiles/mlp_train_outputs.py write LIBRARY OUT.npz     one build, in a fresh process each
    python3 profiles/mlp_train_outputs.py compare A.npz B.npz       exit status 0 when every array has the same bytes
The library is loaded by path and only the three dn_mlp_train_* names are bound, so a build from before the SAC family serves as well as
this one.  The cases are the networks of tests/mlp_train_support.EVERY_BATCH at every batch of BATCHES, with that module's parameters and
inputs; kept are out, every d_weight and d_bias and d_x as the integer view of their bytes."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def write(library, target):
    import torch

    import mlp_train_support as T
    from drl_dronenavigation_amd import _capi as K

    lib = C.CDLL(library)
    for name in ("dn_mlp_train_scratch_bytes", "dn_mlp_train_forward", "dn_mlp_train_backward"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = K.PROTOTYPES[name]
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = {}
    for sizes in T.EVERY_BATCH:
        layers = [(w.to(dev), b.to(dev)) for w, b in T.layers_of(sizes)]
        for batch in T.BATCHES:
            x, d = (t.to(dev) for t in T.inputs(sizes, batch))
            grads = [torch.full_like(t, float("nan")) for pair in layers for t in pair]
            res, d_x = torch.full((batch, sizes[-1]), float("nan"), device=dev), torch.full((batch, sizes[0]), float("nan"), device=dev)
            cfg, table = T.tables(K, sizes, [(w.data_ptr(), b.data_ptr(), grads[2 * i].data_ptr(), grads[2 * i + 1].data_ptr())
                                             for i, (w, b) in enumerate(layers)])
            need = lib.dn_mlp_train_scratch_bytes(C.byref(cfg), table, batch)
            scratch = torch.empty(need // 8, dtype=torch.float64, device=dev)
            assert lib.dn_mlp_train_forward(C.byref(cfg), table, x.data_ptr(), batch, res.data_ptr(), scratch.data_ptr(), need, 0, stream) == 0
            assert lib.dn_mlp_train_backward(C.byref(cfg), table, x.data_ptr(), d.data_ptr(), batch, d_x.data_ptr(), scratch.data_ptr(), need, 0,
                                             stream) == 0
            torch.cuda.synchronize(dev)
            tag = T.case_id((sizes, batch))
            for name, t in [("out", res), ("d_x", d_x)] + [(f"grad{j}", g) for j, g in enumerate(grads)]:
                out[f"{tag}/{name}"] = np.ascontiguousarray(t.cpu().numpy()).view(np.int32)
    np.savez(target, **out)
    print(f"{library}: {len(out)} arrays, {sum(a.size for a in out.values())} words -> {target}")


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    differ = [k for k in a.files if k not in b.files or not np.array_equal(a[k], b[k])] + [k for k in b.files if k not in a.files]
    words = sum(a[k].size for k in a.files)
    print(f"{len(a.files)} | {len(b.files)} arrays, {words} words: {len(differ)} differ" + "".join(f"\n    differs: {k}" for k in differ))
    print("outputs identical" if not differ else f"{len(differ)} differences")
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "write":
        write(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
