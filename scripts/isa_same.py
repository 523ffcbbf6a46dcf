#!/usr/bin/env python3
"""Are the kernels of two builds the same, instruction for instruction?

    python scripts/isa_same.py DIR_A DIR_B [--allow-operand-order SUBSTRING ...] [--pair REGEX ...]

Each directory holds hipcc `-S` gfx950 assembly files with the same names, one
per translation unit of the stencil kernels, made with the flags CMakeLists.txt
gives those files:

    for t in stencil stencil_pipe_f32 stencil_pipe_f64 stencil_pipe_chunks stencil_held stencil_levels \\
             stencil_pipe_levels_f32 stencil_pipe_levels_f64 stencil_pipe_levels_src_f32 stencil_pipe_levels_src_f64; do
      hipcc --offload-arch=gfx950 --cuda-device-only -S -O3 -munsafe-fp-atomics -fno-slp-vectorize \\
            -std=c++17 -Icsrc/include -Wno-unused-result csrc/kernels/$t.hip -o DIR/$t.s &
    done; wait

(bench/stencil_tune.hip and bench/stencil_tune64.hip compile the same way.)
Files are matched by name and split into kernels by symbol (the parser of
scripts/isa_mix.py). Comments, the per-build __hip_cuid_* lines and the
function index in local labels are dropped; every kernel is then

    identical      the remaining text is equal;
    operand-order  same opcode sequence, same .amdhsa_next_free_vgpr / _sgpr and
                   private / group segment sizes, and every differing line is a
                   plain commutative VALU operation (kCommutative) with its two
                   source operands exchanged: bitwise harmless;
    different      anything else, a symbol on one side only included.

A build that renames kernels (other template arguments, another namespace)
pairs them with --pair REGEX, repeatable: a kernel whose demangled name (its
symbol, if no demangler is found) matches REGEX is keyed by the tuple of the
regex's groups instead of by its symbol, and its own symbol is replaced by a
placeholder inside its body. Two kernels of one file and side under one key are
an error (exit status 2), never a pair.

One summary line per file, one line per kernel that is not identical (both
VGPR counts, the first opcode-count differences). Exit status 0 only if every
kernel is identical, or is operand-order and its (demangled) name contains one
of the --allow-operand-order substrings. A kernel pull request that claims its
parent's kernels unchanged shows this tool's output (docs/PERF.md).
"""
import collections
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_mix import kernel_spans, ops  # noqa: E402

kCommutative = ("v_add_f32", "v_add_f64", "v_mul_f32", "v_mul_f64", "v_pk_add_f32", "v_pk_mul_f32")
kFigures = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_private_segment_fixed_size",
            ".amdhsa_group_segment_fixed_size")


def normalised(lines):
    out = []
    for l in lines:
        t = l.split(";")[0].strip()
        if not t or t.startswith("//") or "__hip_cuid_" in t:
            continue
        out.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def kernels(path):
    lines = open(path).read().splitlines()
    return {sym: normalised(lines[a:b + 1]) for sym, a, b in kernel_spans(lines)}


def figures(body):
    f = {}
    for t in body:
        p = t.split()
        if p[0] in kFigures:
            f[p[0]] = p[1]
    return f


def swapped(a, b):
    """Both lines are one commutative VALU operation, sources exchanged."""
    pa, pb = a.split(None, 1), b.split(None, 1)
    if len(pa) != 2 or len(pb) != 2 or pa[0] != pb[0]:
        return False
    if re.sub(r"_e(32|64)$", "", pa[0]) not in kCommutative:
        return False
    oa, ob = [x.strip() for x in pa[1].split(",")], [x.strip() for x in pb[1].split(",")]
    if len(oa) != 3 or len(ob) != 3 or any(" " in x for x in oa + ob):  # no modifiers (DPP, op_sel, ...)
        return False
    return oa[0] == ob[0] and oa[1] == ob[2] and oa[2] == ob[1]


def classify(a, b):
    if a == b:
        return "identical"
    if ops(a) != ops(b) or figures(a) != figures(b) or len(a) != len(b):
        return "different"
    return "operand-order" if all(x == y or swapped(x, y) for x, y in zip(a, b)) else "different"


def demangled(symbols):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if tool and symbols:
        r = subprocess.run([tool], input="\n".join(symbols), capture_output=True, text=True)
        names = r.stdout.splitlines()
        if r.returncode == 0 and len(names) == len(symbols):
            return dict(zip(symbols, names))
    return {s: s for s in symbols}


class Ambiguous(Exception):
    pass


def keyed(side, kern, names, pairs):
    """{key: (symbol, body)}: the key is the symbol, or for a kernel that a
    --pair regex matches the tuple of its groups (its body then names itself by
    a placeholder)."""
    out = {}
    for sym, body in kern.items():
        m = next(filter(None, (p.search(names[sym]) for p in pairs)), None)
        key = m.groups() if m else sym
        if m:
            body = [t.replace(sym, "<kernel>") for t in body]
        if key in out:
            raise Ambiguous(f"{side}: --pair gives {names[out[key][0]]} and {names[sym]} the same key {key}")
        out[key] = (sym, body)
    return out


def compare_file(name, path_a, path_b, allow, pairs=()):
    """Prints the file's lines; returns the number of kernels that fail."""
    ka, kb = kernels(path_a), kernels(path_b)
    names = demangled(sorted(set(ka) | set(kb)))
    ka, kb = keyed(path_a, ka, names, pairs), keyed(path_b, kb, names, pairs)
    count, bad, notes = collections.Counter(), 0, []
    for key in sorted(set(ka) | set(kb), key=str):
        sym = (ka.get(key) or kb[key])[0]
        if key not in ka or key not in kb:
            count["only in A" if key in ka else "only in B"] += 1
            bad += 1
            notes.append(f"  {'only in A' if key in ka else 'only in B'}: {names[sym]}")
            continue
        a, b = ka[key][1], kb[key][1]
        kind = classify(a, b)
        count[kind] += 1
        if kind == "identical":
            continue
        ok = kind == "operand-order" and any(s in names[sym] or s in sym for s in allow)
        bad += not ok
        ca, cb = collections.Counter(ops(a)), collections.Counter(ops(b))
        delta = [f"{k} {ca[k]} -> {cb[k]}" for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k]][:4]
        if kind == "operand-order":
            delta = [f"{sum(x != y for x, y in zip(a, b))} lines swap their sources" + (" (allowed)" if ok else "")]
        va, vb = figures(a).get(kFigures[0], "?"), figures(b).get(kFigures[0], "?")
        notes.append(f"  {kind}: {names[sym]}: vgpr {va} -> {vb}; " + (", ".join(delta) or "same opcode counts"))
    print(f"{name}: {len(set(ka) | set(kb))} kernels: {count['identical']} identical, "
          f"{count['operand-order']} operand-order, {count['different']} different, "
          f"{count['only in A']} only in A, {count['only in B']} only in B")
    for n in notes:
        print(n)
    return bad


def main(argv):
    allow, pairs, dirs, i = [], [], [], 0
    while i < len(argv):
        if argv[i] == "--allow-operand-order" and i + 1 < len(argv):
            allow.append(argv[i + 1])
            i += 2
        elif argv[i] == "--pair" and i + 1 < len(argv):
            pairs.append(re.compile(argv[i + 1]))
            i += 2
        else:
            dirs.append(argv[i])
            i += 1
    if len(dirs) != 2:
        print(__doc__)
        return 2
    fa = {f for f in os.listdir(dirs[0]) if f.endswith(".s")}
    fb = {f for f in os.listdir(dirs[1]) if f.endswith(".s")}
    bad = 0
    for f in sorted(fa | fb):
        if f not in fa or f not in fb:
            print(f"{f}: only in {dirs[0] if f in fa else dirs[1]}")
            bad += 1
            continue
        try:
            bad += compare_file(f, os.path.join(dirs[0], f), os.path.join(dirs[1], f), allow, pairs)
        except Ambiguous as e:
            print(e)
            return 2
    if not fa | fb:
        print("no .s files")
        bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
