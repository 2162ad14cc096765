#!/usr/bin/env python3
"""The bits of both fleet-wide normalisers (csrc/dn_rownorm.hip, csrc/dn_retnorm.hip) as one SHA-256 per case:
    python3 profiles/fleet_norm_digest.py [output file]
For a change that must not move a bit, run it on both builds (DN_LIB_PATH selects a library of the same ABI) and compare the listings line
for line.  Per case, three update_normalize calls of K steps on N rows from seeded data, starting at the prior; hashed after every call:
the output, the statistics and (return normaliser) the returns.  Cases (K, N): (3, 2 blocks + 1), (9, 8 blocks), (17, 8 blocks + 1),
(9, 16 blocks + 1) of DN_ROWNORM_BLOCK_ROWS = 1024 rows -- up to three blocks, exactly one batch of 8 blocks, a second pass of the merge's
block loop whose prefetch had one block in range, and a full and a partial prefetch; K = 9 and 17 pass the 8 steps the row normaliser's
merge takes side by side and the 8 updates it loads ahead.  The row normaliser runs at W = 1, 13, 52 and 64."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import drl_dronenavigation_amd as pkg  # noqa: E402

BLOCK_ROWS = 1024
CASES = ((3, 2 * BLOCK_ROWS + 1), (9, 8 * BLOCK_ROWS), (17, 8 * BLOCK_ROWS + 1), (9, 16 * BLOCK_ROWS + 1))
WIDTHS = (1, 13, 52, 64)
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def feed(h, *tensors):
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())


for W in WIDTHS:
    for K, N in CASES:
        g = torch.Generator(device="cpu").manual_seed(1000 * W + 10 * N + K)
        scales = 10.0 ** ((torch.arange(W) % 7) - 3.0)
        norm, h = pkg.RowNormalizer(W, dev, clip=2.5), hashlib.sha256()
        for call in range(3):
            x = torch.randn((K, N, W), generator=g) * scales + 5.0 * scales
            x[..., 0] = 14468.0 + torch.randn((K, N), generator=g)          # a rotor-speed column
            feed(h, norm.update_normalize(x.to(dev)), norm.stats)
        say(f"rownorm W={W} K={K} N={N} {h.hexdigest()}")
for K, N in CASES:
    g = torch.Generator(device="cpu").manual_seed(100 * N + K)
    norm, h = pkg.ReturnNormalizer(N, dev, clip=2.5), hashlib.sha256()
    for call in range(3):
        r = 3.0 * torch.randn((K, N), generator=g) - 0.5
        d = (torch.rand((K, N), generator=g) < 0.05).to(torch.uint8)
        feed(h, norm.update_normalize(r.to(dev), d.to(dev)), norm.stats, norm.returns)
    say(f"retnorm K={K} N={N} {h.hexdigest()}")
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
