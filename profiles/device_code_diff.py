#!/usr/bin/env python3
"""Is the device code of two builds the same?  For a host-only change (launchers, the C ABI) the answer must be yes.

    python profiles/device_code_diff.py OLD/csrc NEW/csrc [--new-template-arg]

For every object with a gfx950 code object in both directories: extracts the code object (llvm-objdump --offloading), lists its FUNC
symbols (llvm-readelf -s --wide), disassembles it (llvm-objdump -d), splits the text by symbol and strips the address and encoding
columns.  Prints the symbol count per object and every symbol that exists on one side only or whose instruction text differs; the
exit status is 0 when there is none.  Needs no GPU.

--new-template-arg: for a change that gives a kernel template one more trailing bool argument (default false) and adds code objects.
A kernel that exists on the new side only is compared with the old kernel of the same name less that trailing `false` (its last Lb0E,
and the last XT<n>_E of a dependent argument type such as StepArg<...>::type), where the old side has one.  Two things that move with the
code object's layout and the symbol's name, not with the kernel, are masked on both sides: the immediates of the s_add_u32 / s_addc_u32
pair after an s_getpc_b64 (pc-relative data offsets) and the symbol names inside <...> branch-target annotations.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJECTS = ["dn_kernels.o", "dn_kernels.exact.o", "dn_kernels_mw.o", "dn_kernels_mw.exact.o", "dn_fused.o", "dn_fused.exact.o", "dn_mlp.o"]


def tool(name):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm") + "/llvm/bin", os.environ.get("ROCM_PATH", "/opt/rocm") + "/lib/llvm/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return shutil.which(name) or name


def functions(obj, work):
    """{symbol: instruction text} of the gfx950 code object inside obj."""
    shutil.copy(obj, os.path.join(work, "in.o"))
    subprocess.check_call([tool("llvm-objdump"), "--offloading", "in.o"], cwd=work, stdout=subprocess.DEVNULL)
    cos = [f for f in os.listdir(work) if f.startswith("in.o") and "gfx950" in f]
    assert len(cos) == 1, cos
    co = os.path.join(work, cos[0])
    syms, listed = set(), 0
    for line in subprocess.check_output([tool("llvm-readelf"), "-s", "--wide", co], text=True).splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[6] != "UND":
            syms.add(f[7])
            listed += 1                                             # .dynsym and .symtab both list a kernel
    text, cur = {}, None
    for line in subprocess.check_output([tool("llvm-objdump"), "-d", co], text=True).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1) if m.group(1) in syms else None
            if cur:
                text[cur] = []
        elif cur and line.strip():
            text[cur].append(re.sub(r"\s*//.*$", "", line).strip())     # "\tinsn operands   // ADDR: ENCODING"
    for f in os.listdir(work):
        os.remove(os.path.join(work, f))
    assert set(text) == syms, (len(text), len(syms))
    return {s: "\n".join(t) for s, t in text.items()}, listed


def less_trailing_false(sym):
    """sym with the last Lb0E of its first run of bool template arguments dropped (and the last XT<n>_E of a dependent list), or None."""
    m = re.match(r"^(.*?I[df]?)((?:Lb[01]E)+)(E.*)$", sym)
    if not m or not m.group(2).endswith("Lb0E"):
        return None
    rest = re.sub(r"XT\d+_E(E4typeE)", r"\1", m.group(3), count=1)
    return m.group(1) + m.group(2)[:-4] + rest


def masked(text):
    out, pc = [], 0
    for line in text.split("\n"):
        line = re.sub(r"<[^>]*>", "<L>", line)
        if "s_getpc_b64" in line:
            pc = 3
        elif pc:
            pc -= 1
            if line.startswith(("s_add_u32", "s_addc_u32")):
                line = re.sub(r"0x[0-9a-f]+|\b\d+$", "IMM", line)
        out.append(line)
    return "\n".join(out)


def main(old, new, new_template_arg=False):
    bad = 0
    for name in OBJECTS:
        with tempfile.TemporaryDirectory() as work:
            (a, na), (b, nb) = functions(os.path.join(old, name), work), functions(os.path.join(new, name), work)
        if new_template_arg:
            a = {s: masked(t) for s, t in a.items()}
            renamed = {}
            for s, t in b.items():
                was = less_trailing_false(s) if s not in a else None
                renamed[was if was in a and was not in b else s] = masked(t)
            b = renamed
        only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        differ = sorted(s for s in set(a) & set(b) if a[s] != b[s])
        print(f"{name}: {len(a)} | {len(b)} functions ({na} | {nb} FUNC entries), {len(only_a)} only old, {len(only_b)} only new, {len(differ)} with different text")
        for tag, group in (("only old", only_a), ("only new", only_b), ("differs", differ)):
            for s in group:
                print(f"    {tag}: {s}")
        bad += len(only_a) + len(only_b) + len(differ)
    print("device code identical" if not bad else f"{bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if x != "--new-template-arg"]
    sys.exit(main(args[0], args[1], "--new-template-arg" in sys.argv[1:]))
