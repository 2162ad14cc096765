#!/usr/bin/env python3
"""Is the device code of two builds the same?  For a host-only change (launchers, the C ABI) the answer must be yes.

    python profiles/device_code_diff.py OLD/csrc NEW/csrc [--new-template-arg | --model-level | --by-library]

For every object with a gfx950 code object in both directories: extracts the code object (llvm-objdump --offloading), lists its FUNC
symbols (llvm-readelf -s --wide), disassembles it (llvm-objdump -d), splits the text by symbol and strips the address and encoding
columns.  Prints the symbol count per object and every symbol that exists on one side only or whose instruction text differs; the
exit status is 0 when there is none.  Needs no GPU.

--new-template-arg: for a change that gives a kernel template one more trailing bool argument (default false) and adds code objects.
A kernel that exists on the new side only is compared with the old kernel of the same name less that trailing `false` (its last Lb0E,
and the last XT<n>_E of a dependent argument type such as StepArg<...>::type), where the old side has one.  Two things that move with the
code object's layout and the symbol's name, not with the kernel, are masked on both sides: the immediates of the s_add_u32 / s_addc_u32
pair after an s_getpc_b64 (pc-relative data offsets) and the symbol names inside <...> branch-target annotations.

--model-level: for the change that names dn_step_many_1w_kernel's model family by one level.  An old kernel <R, NORM, NOISE, ONE, XOPT,
SAMPLE, DYN, WIND, ACT, SENS, PRIV, GOAL> is compared with the new kernel <R, NORM, NOISE, ONE, XOPT, SAMPLE, M>, M = the number of
`true`s in DYN ... GOAL; it is an error if they are not a prefix of that run.  The StepArg<...>::type inside the name maps likewise.
Every other function pairs by identical name; both sides are masked as above.

--by-library: for a change that moves functions between objects.  Functions pair by name over all objects of a library as build.py links
it (the default library: every .o; the exact library: the .exact.o where there is one and the .o otherwise; an object that one side does
not have is skipped on that side).  A function pairs with the one of the same object where both sides have it there, else with the first
object in link order that holds it on the old side.  A further copy of a function that is paired (the old build emitted it in more
objects, or the new one does) is listed as dropped or added and is not a difference; a NAME on one side only is.  Both sides are masked
as under --new-template-arg: an object that lost or gained functions has another layout.  The per-object function counts are printed as
before, then one summary per library, every moved function, and for every function whose text differs the number of differing lines.

In every mode the padding lines at a function's very end are dropped (trailing s_nop / s_code_end lines and the disassembler's `...`):
they fill up to the next function's alignment or the section's end, so they depend on the function's neighbour, not on the function.
Nothing else is dropped: code that the compiler placed behind the last s_endpgm is compared like the rest.

With any pairing, and without one, the entries of the code object's metadata note are compared for every paired kernel as well: VGPR,
AGPR and SGPR counts, both spill counts, LDS size, private segment size and kernarg segment size.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile


def objects():
    """Every object of the build with a device code object: one per .hip source, and the .exact.o of each step source (build.py)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "drl-dronenavigation_amd"))
    import build
    out = []
    for src in build.SOURCES:
        stem, ext = os.path.splitext(src)
        if ext == ".hip":                                           # the .cpp units are host code only
            out += [stem + ".o"] + ([stem + ".exact.o"] if src in build.STEP_SOURCES else [])
    return out


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
    meta = metadata(subprocess.check_output([tool("llvm-readelf"), "--notes", co], text=True))
    for f in os.listdir(work):
        os.remove(os.path.join(work, f))
    assert set(text) == syms, (len(text), len(syms))
    for t in text.values():                                         # the padding at a function's end depends on what follows it
        while t and (t[-1].startswith(("s_nop", "s_code_end")) or t[-1] == "..."):
            t.pop()
    return {s: "\n".join(t) for s, t in text.items()}, listed, meta


META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
             ".private_segment_fixed_size", ".kernarg_segment_size")


def metadata(notes):
    """{kernel name: {key: value}} for META_KEYS, from the amdhsa.kernels list of the AMDGPU metadata note as llvm-readelf prints it."""
    out, cur, at = {}, None, None
    for line in notes.splitlines():
        indent = len(line) - len(line.lstrip())
        if at is None:
            if line.strip() == "amdhsa.kernels:":
                at = -1
            continue
        if at < 0:
            at = indent                                             # the column of the list's dashes
        if indent < at or (indent == at and not line.lstrip().startswith("- ")):
            break                                                   # the next key of the note
        m = re.match(r"^\s{%d}(?:- | {2})(\.\w+):\s*(\S*)$" % at, line)       # the kernel's own keys, not those of its .args
        if not m:
            continue
        if line[at] == "-":
            cur = {}
        if m.group(1) == ".name":
            out[m.group(2)] = cur
        elif m.group(1) in META_KEYS:
            cur[m.group(1)] = m.group(2)
    assert all(len(v) == len(META_KEYS) for v in out.values()), "metadata note: a kernel lacks one of %s" % (META_KEYS,)
    return out


def less_trailing_false(sym):
    """sym with the last Lb0E of its first run of bool template arguments dropped (and the last XT<n>_E of a dependent list), or None."""
    m = re.match(r"^(.*?I[df]?)((?:Lb[01]E)+)(E.*)$", sym)
    if not m or not m.group(2).endswith("Lb0E"):
        return None
    rest = re.sub(r"XT\d+_E(E4typeE)", r"\1", m.group(3), count=1)
    return m.group(1) + m.group(2)[:-4] + rest


def model_level_name(sym):
    """The new name of an old dn_step_many_1w_kernel instantiation (any other symbol: unchanged); ValueError off the chain."""
    m = re.match(r"^(.*22dn_step_many_1w_kernelI[df](?:Lb[01]E){5})((?:Lb[01]E){6})(E.*7StepArgI)(?:XT\d+_E){6}(E4typeE.*)$", sym)
    if not m:
        if "22dn_step_many_1w_kernelI" in sym and not re.search(r"22dn_step_many_1w_kernelI[df](?:Lb[01]E){5}Li\d+EE", sym):
            raise ValueError("dn_step_many_1w_kernel with an unexpected argument list: " + sym)
        return sym
    flags = re.findall(r"Lb([01])E", m.group(2))
    level = flags.count("1")
    if flags != ["1"] * level + ["0"] * (6 - level):
        raise ValueError("the model flags %s are not a prefix of DYN ... GOAL: %s" % ("".join(flags), sym))
    return "%sLi%dE%sXT5_E%s" % (m.group(1), level, m.group(3), m.group(4))


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


def library_objects(exact):
    """The objects with device code that build.py links into the default (exact: the exact) library, in link order."""
    objs = objects()
    if not exact:
        return [o for o in objs if not o.endswith(".exact.o")]
    return [o for o in objs if o.endswith(".exact.o") or o[:-2] + ".exact.o" not in objs]       # the .exact.o where there is one


def by_library(old, new):
    """--by-library: pairs by name over all objects of a library, so that a function that moved between objects is compared."""
    bad, cache = 0, {}

    def load(d, name):
        if (d, name) not in cache:
            path = os.path.join(d, name)
            with tempfile.TemporaryDirectory() as work:
                cache[d, name] = functions(path, work) if os.path.exists(path) else None
        return cache[d, name]

    for lib, exact in (("libdronenav.so", False), ("libdronenav_exact.so", True)):
        print(f"{lib}:")
        a, b, ma, mb = {}, {}, {}, {}                               # {(object, symbol): text}, {(object, kernel): metadata}
        for name in library_objects(exact):
            sides = [load(old, name), load(new, name)]
            for got, text, meta in zip(sides, (a, b), (ma, mb)):
                if got:
                    text.update({(name, s): masked(t) for s, t in got[0].items()})      # an object that lost functions has another layout
                    meta.update({(name, s): v for s, v in got[2].items()})
            print(f"    {name}: " + " | ".join("absent" if not g else f"{len(g[0])} functions ({g[1]} FUNC entries)" for g in sides))
        pairs = [(k, k) for k in a if k in b]                       # same object first ...
        left_a, left_b = [k for k in a if k not in b], [k for k in b if k not in a]
        moved = []
        for kb in left_b:                                           # ... then by name: the first holder in link order
            ka = next((k for k in left_a if k[1] == kb[1]), None)
            if ka:
                moved.append((ka, kb))
                left_a.remove(ka)
        names_a, names_b = {k[1] for k in a}, {k[1] for k in b}
        dropped = [k for k in left_a if k[1] in names_b]            # further old copies of a function that the new build emits in fewer objects
        extra = [k for k in left_b if k[1] in names_a and k not in {kb for _, kb in moved}]      # ... and in more
        only_a, only_b = [k for k in left_a if k[1] not in names_b], [k for k in left_b if k[1] not in names_a]
        differ = [(ka, kb) for ka, kb in pairs + moved if a[ka] != b[kb]]
        kernels = [(ka, kb) for ka, kb in pairs + moved if ka in ma and kb in mb]
        meta_differ = [(ka, kb) for ka, kb in kernels if ma[ka] != mb[kb]]
        print(f"    {len(a)} | {len(b)} functions, {len(pairs)} paired in the same object, {len(moved)} moved, {len(dropped)} | {len(extra)} further "
              f"copies of functions that are paired, {len(only_a)} only old, {len(only_b)} only new, {len(differ)} with different text; "
              f"{len(kernels)} paired kernels ({len(ma)} | {len(mb)}), {len(meta_differ)} with different metadata")
        for tag, group in (("old copy dropped", dropped), ("new copy added", extra)):
            for obj, s in group:
                print(f"    {tag}: {obj}: {s}")
        for ka, kb in moved:
            print(f"    moved: {kb[1]}: {ka[0]} -> {kb[0]}")
        for tag, group in (("only old", only_a), ("only new", only_b)):
            for obj, s in group:
                print(f"    {tag}: {obj}: {s}")
        for ka, kb in differ:
            la, lb = a[ka].split("\n"), b[kb].split("\n")
            n = sum(x != y for x, y in zip(la, lb)) + abs(len(la) - len(lb))
            print(f"    differs: {kb[0]}: {kb[1]}: {n} lines of {len(la)} | {len(lb)}")
            if len(la) == len(lb) and n <= 40:                      # few enough to read: the lines themselves
                for i, (x, y) in enumerate(zip(la, lb)):
                    if x != y:
                        print(f"        {i}: {x}  |  {y}")
        for ka, kb in meta_differ:
            print(f"    metadata: {kb[0]}: {kb[1]}: " + ", ".join(f"{k} {ma[ka][k]} | {mb[kb][k]}" for k in META_KEYS if ma[ka][k] != mb[kb][k]))
        bad += len(only_a) + len(only_b) + len(differ) + len(meta_differ)
    print("device code identical" if not bad else f"{bad} differences")
    return 1 if bad else 0


def main(old, new, new_template_arg=False, model_level=False):
    bad = 0
    for name in objects():
        with tempfile.TemporaryDirectory() as work:
            (a, na, ma), (b, nb, mb) = functions(os.path.join(old, name), work), functions(os.path.join(new, name), work)
        if new_template_arg:
            a = {s: masked(t) for s, t in a.items()}
            renamed, meta = {}, {}
            for s, t in b.items():
                was = less_trailing_false(s) if s not in a else None
                renamed[was if was in a and was not in b else s] = masked(t)
                if s in mb:
                    meta[was if was in a and was not in b else s] = mb[s]
            b, mb = renamed, meta
        elif model_level:
            a, ma = {model_level_name(s): masked(t) for s, t in a.items()}, {model_level_name(s): v for s, v in ma.items()}
            b = {s: masked(t) for s, t in b.items()}
        only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        differ = sorted(s for s in set(a) & set(b) if a[s] != b[s])
        kernels = sorted(set(ma) & set(mb) & set(a) & set(b))
        meta_differ = [s for s in kernels if ma[s] != mb[s]]
        print(f"{name}: {len(a)} | {len(b)} functions ({na} | {nb} FUNC entries), {len(only_a)} only old, {len(only_b)} only new, {len(differ)} with different text; "
              f"{len(kernels)} paired kernels ({len(ma)} | {len(mb)}), {len(meta_differ)} with different metadata")
        for tag, group in (("only old", only_a), ("only new", only_b), ("differs", differ)):
            for s in group:
                print(f"    {tag}: {s}")
        for s in meta_differ:
            print(f"    metadata: {s}: " + ", ".join(f"{k} {ma[s][k]} | {mb[s][k]}" for k in META_KEYS if ma[s][k] != mb[s][k]))
        bad += len(only_a) + len(only_b) + len(differ) + len(meta_differ) + abs(len(ma) - len(kernels)) + abs(len(mb) - len(kernels))
    print("device code identical" if not bad else f"{bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if not x.startswith("--")]
    if "--by-library" in sys.argv[1:]:
        sys.exit(by_library(args[0], args[1]))
    sys.exit(main(args[0], args[1], "--new-template-arg" in sys.argv[1:], "--model-level" in sys.argv[1:]))
