#!/usr/bin/env python3
"""Widenings and narrowings by role of the five-wave fused kernel (no GPU needed): the companion of role_isa.sh for one question --
how many float32 <-> float64 conversions does each role's K-step loop of dn_step_many_5w_kernel<double, false> hold?

    python profiles/role_cvt.py [--asm FILE.s] [extra hipcc flags]  ->  stdout

Compiles dn_kernels_mw.hip to assembly with -DDN_ROLE_MARK (or reads an assembly file made that way) and counts, from each role's mark
to the backward branch that closes its loop: v_cvt_f64_f32 (up), v_cvt_f32_f64 (down), float64 arithmetic (v_*_f64 less conversions,
compares and transcendentals) and every other vector instruction.  Like role_isa.sh it is the code's size by role -- rarely taken
blocks are inside the count -- not the dynamic mix.  It also prints the kernel's register, spill and LDS figures where the compiler's
resource remarks are available (when it compiles itself).
"""
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = "_ZN12_GLOBAL__N_122dn_step_many_5w_kernelIdLb0EEEv8DnParams8DnStepIOi"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "-fno-fast-math", "--cuda-device-only", "-S", "-DDN_ROLE_MARK", "-Rpass-analysis=kernel-resource-usage"]
TRANS = ("v_rsq", "v_rcp", "v_sqrt", "v_exp", "v_log", "v_sin", "v_cos")


def role_loops(path):
    body, on = [], False
    for l in open(path):
        if l.startswith(KERN + ":"):
            on = True
            continue
        if on:
            if l.startswith(".Lfunc_end"):
                break
            body.append(l.rstrip("\n"))
    labels, ins, marks = {}, [], {}
    for l in body:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        t = l.strip()
        m = re.match(r"; DN_ROLE_LOOP (\w)", t)
        if m:
            marks[m.group(1)] = len(ins)
            continue
        if l.startswith("\t") and t and not t.startswith((".", ";")):
            ins.append(t)
    loops = {}
    for name in "LAQNX":
        start = marks[name]
        # as in role_isa.sh: the header is the last label at or before the mark, the end the LAST backward branch to a label <= start
        hdr = max(v for v in labels.values() if v <= start)
        end = None
        for i in range(start, len(ins)):
            m = re.match(r"s_cbranch\w*\s+(\.LBB\d+_\d+)|s_branch\s+(\.LBB\d+_\d+)", ins[i])
            if m:
                tgt = labels.get(m.group(1) or m.group(2))
                if tgt is not None and tgt <= start and tgt >= hdr - 400:
                    end = i
            if i > start and any(i == v for k, v in marks.items() if k != name):
                break
        loops[name] = ins[hdr:end + 1]
    return loops


def table(loops):
    print(f"{'role':4} {'cvt up':>7} {'cvt down':>9} {'f64 arith':>10} {'other VALU':>11} {'VALU':>6}")
    tot = Counter()
    for name in "LAQNX":
        c = Counter(x.split()[0] for x in loops[name])
        valu = sum(v for k, v in c.items() if k.startswith("v_"))
        up = sum(v for k, v in c.items() if k.startswith("v_cvt_f64_f32"))
        down = sum(v for k, v in c.items() if k.startswith("v_cvt_f32_f64"))
        f64 = sum(v for k, v in c.items() if k.startswith("v_") and "f64" in k and not k.startswith(("v_cvt", "v_cmp") + TRANS))
        row = dict(up=up, down=down, f64=f64, other=valu - up - down - f64, valu=valu)
        tot.update(row)
        print(f"{name:4} {up:7d} {down:9d} {f64:10d} {row['other']:11d} {valu:6d}")
    print(f"{'sum':4} {tot['up']:7d} {tot['down']:9d} {tot['f64']:10d} {tot['other']:11d} {tot['valu']:6d}")


def resources(remarks):
    keys = ("VGPRs:", "ScratchSize", "Occupancy", "SGPRs Spill", "VGPRs Spill", "LDS Size")
    on = False
    for l in remarks.splitlines():
        if "Function Name:" in l:
            on = KERN in l
        elif on and "remark:" in l and any(k in l for k in keys):
            print("   ", l.split("remark:")[1].replace("[-Rpass-analysis=kernel-resource-usage]", "").strip())


def main(argv):
    if "--asm" in argv:
        i = argv.index("--asm")
        table(role_loops(argv[i + 1]))
        return
    with tempfile.TemporaryDirectory() as t:
        out = os.path.join(t, "mw.s")
        r = subprocess.run(["hipcc"] + FLAGS + argv + [os.path.join(ROOT, "drl-dronenavigation_amd", "csrc", "dn_kernels_mw.hip"), "-o", out],
                           stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.exit(r.stderr)
        table(role_loops(out))
        print("dn_step_many_5w_kernel<double, false>:")
        resources(r.stderr)


if __name__ == "__main__":
    main(sys.argv[1:])
