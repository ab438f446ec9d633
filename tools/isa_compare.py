"""Compare the kernels of two sets of `hipcc -S` listings, kernel by kernel: the check of a refactor that must not change what a launch computes.

usage: python tools/isa_compare.py --before DIR --after DIR [--rename REGEX=REPL ...] [--new REGEX]
Each DIR holds NAME.s (hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S) and NAME.remarks (the stderr of the same command with
-Rpass-analysis=kernel-resource-usage).  Kernels are matched by name and template arguments, whichever file they are in; --rename rewrites a
name of the `after` side first (a kernel that gained a template argument or lost a suffix), --new marks kernels of the after side that have no
counterpart by design.  Verdicts:
  identical       the same instruction stream (labels renumbered)
  same-arithmetic the same ORDERED list of floating-point and conversion instructions (v_*f32*, v_pk_*, v_rsq*, v_cvt*; operands reduced to
                  their kind, modifiers such as neg / abs / op_sel / literals kept), scratch 0 and the same occupancy: the differences are
                  register numbers and the order of the other instructions
  DIFFERENT       neither: a finding
  new / gone      no counterpart
Prints one row per kernel: verdict, instructions before -> after, occupancy before -> after, scratch after.
"""
import argparse
import collections
import glob
import os
import re

TYPES = {"DF16b": "bf16", "f": "float", "d": "double", "i": "int", "l": "long", "b": "bool"}


def kernel_name(sym):
    """name<template arguments> of a mangled kernel symbol (integers and the plain types above; anything else stays mangled)"""
    m = re.match(r"_ZN?(?:12_GLOBAL__N_1)?(\d+)", sym)
    if not m:
        return sym
    n = int(m.group(1))
    name, rest = sym[m.end():m.end() + n], sym[m.end() + n:]
    if not rest.startswith("I"):
        return name
    args, rest = [], rest[1:]
    while rest and not rest.startswith("E"):
        m = re.match(r"L[a-z](n?)(\d+)E", rest)
        if m:
            args.append(("-" if m.group(1) else "") + m.group(2))
        else:
            m = re.match("|".join(sorted(TYPES, key=len, reverse=True)), rest)
            if not m:
                return sym
            args.append(TYPES[m.group(0)])
        rest = rest[m.end():]
    return f"{name}<{','.join(args)}>"


def kernels_of(path):
    """{symbol: [instruction, ...]} of one listing"""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if line.startswith("\t.section") or line.startswith(".Lfunc_end"):
            cur = None
        s = line.split(";")[0].strip()
        if cur is None or not s or s.startswith(".") or s.endswith(":"):
            continue
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(s.split())))
    return out


def resources_of(path):
    """{symbol: (occupancy, scratch bytes per lane)} of one remarks file"""
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = [None, None]
        m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
        if m and cur:
            out[cur][0] = int(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            out[cur][1] = int(m.group(1))
    return out


def arithmetic(ins):
    """the ordered floating-point / conversion instructions, register numbers dropped"""
    keep = []
    for s in ins:
        op = s.split()[0]
        if re.match(r"v_(\w*f32|pk_|rsq|cvt)", op):
            s = re.sub(r"\b([vsa])\[\d+:\d+\]", r"\1", s)
            keep.append(re.sub(r"\b([vsa])\d+\b", r"\1", s))
    return keep


def load(d, renames):
    ks = collections.OrderedDict()
    for s in sorted(glob.glob(os.path.join(d, "*.s"))):
        res = resources_of(s[:-2] + ".remarks")
        for sym, ins in kernels_of(s).items():
            name = kernel_name(sym)
            for pat, repl in renames:
                name = re.sub(pat, repl, name)
            ks.setdefault(name, []).append((os.path.basename(s)[:-2], ins, res.get(sym, [None, None])))
    return ks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", required=True)
    ap.add_argument("--after", required=True)
    ap.add_argument("--rename", action="append", default=[])
    ap.add_argument("--new", default=None)
    a = ap.parse_args()
    before = load(a.before, [])
    after = load(a.after, [r.split("=", 1) for r in a.rename])
    print(f"{'kernel':44s} {'before':10s} {'after':10s} {'verdict':16s} {'instr':>12s} {'occupancy':>9s} {'scratch':>7s}")
    bad = 0
    for name in list(before) + [n for n in after if n not in before]:
        for bf, bi, (bocc, _) in before.get(name, [(None, None, (None, None))]):
            for af, ai, (aocc, ascr) in after.get(name, [(None, None, (None, None))]):
                if ai is None:
                    verdict = "gone"
                elif bi is None:
                    verdict = "new" if a.new and re.search(a.new, name) else "new (unexpected)"
                elif bi == ai:
                    verdict = "identical"
                elif arithmetic(bi) == arithmetic(ai) and ascr == 0 and aocc == bocc:
                    verdict = "same-arithmetic"
                else:
                    verdict = "DIFFERENT"
                bad += verdict in ("DIFFERENT", "new (unexpected)")
                n = f"{len(bi) if bi is not None else '-'} -> {len(ai) if ai is not None else '-'}"
                occ = f"{bocc or '-'} -> {aocc or '-'}"
                print(f"{name:44s} {bf or '-':10s} {af or '-':10s} {verdict:16s} {n:>12s} {occ:>9s} {'-' if ascr is None else ascr:>7}")
    print(f"{bad} finding(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main())
