#!/usr/bin/env python3
"""Compare the kernels of two builds by their assembly text (make asm: build/*.s).

For every __global__ symbol of the baseline file and of the new files (their union: a kernel may
have moved to another translation unit) one line:
  same             instruction stream and kernel descriptor identical
  descriptor-same  descriptor identical, stream differs: + the per-mnemonic count delta
  DESCRIPTOR-DIFF  + the descriptor fields that differ (and the mnemonic delta)
  missing / new    only in the baseline / only in the new files
Comments are stripped and local labels (.LBB<n>_<m>, .Ltmp<n>, ...) renumbered in order of first
appearance inside the kernel, so moving a kernel inside or between files does not count.  Exit
status 1 on DESCRIPTOR-DIFF or missing, unless the symbol was given with --removed NAME (the
mangled symbol or the plain function name).  --renamed OLD=NEW (mangled symbols; a changed template
parameter list changes the name) compares the baseline's OLD against the new files' NEW as one
kernel, listed under NEW; both must exist, otherwise `missing` and exit status 1.  Pure text
comparison: no GPU, no table of mnemonics.

Usage: tools/kernel_diff.py BASE.s NEW.s [NEW2.s ...] [--removed NAME ...] [--renamed OLD=NEW ...]"""
import argparse
import re
import sys
from collections import Counter

_LOCAL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def source_names(sym):
    """Plain identifiers of an Itanium-mangled symbol's (nested) name: _ZN3m3d9nn_kernelE… →
    ['m3d', 'nn_kernel']."""
    m = re.match(r"_ZN?", sym)
    names, i = [], m.end() if m else len(sym)
    while i < len(sym) and sym[i].isdigit():
        j = i
        while sym[j].isdigit():
            j += 1
        n = int(sym[i:j])
        names.append(sym[j:j + n])
        i = j + n
    return names


def parse(text):
    """{symbol: (stream, descriptor)}: stream = the kernel's labels and instructions, normalised;
    descriptor = {field: value} of its .amdhsa_kernel block."""
    lines = [ln.split(";", 1)[0].rstrip() for ln in text.splitlines()]
    kernels = {}
    for k, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        desc = {}
        for d in lines[k + 1:]:
            if d.strip() == ".end_amdhsa_kernel":
                break
            f = d.split()
            if f:
                desc[f[0].replace(".amdhsa_", "")] = " ".join(f[1:])
        kernels[m.group(1)] = ([], desc)
    for k, ln in enumerate(lines):
        sym = ln[:-1] if ln.endswith(":") else None
        if sym not in kernels:
            continue
        stream, ids = kernels[sym][0], {}
        for b in lines[k + 1:]:
            s = b.strip()
            if s.startswith(".amdhsa_kernel") or s.startswith(".Lfunc_end"):
                break
            if not s or (s.startswith(".") and not s.endswith(":")):
                continue  # blank, or an assembler directive (.p2align, .section)
            stream.append(_LOCAL.sub(lambda l: ids.setdefault(l.group(0), f".L{len(ids)}"), " ".join(s.split())))
    return kernels


def mnemonics(stream):
    return Counter(s.split()[0] for s in stream if not s.endswith(":"))


def delta(a, b):
    ca, cb = mnemonics(a), mnemonics(b)
    d = {m: cb[m] - ca[m] for m in sorted(set(ca) | set(cb)) if cb[m] != ca[m]}
    total = sum(cb.values()) - sum(ca.values())
    return f"instructions {sum(ca.values())} -> {sum(cb.values())} ({total:+d}): " + (
        ", ".join(f"{m} {v:+d}" for m, v in d.items()) or "same counts, other order or operands")


def compare(base_text, new_texts, removed=(), renamed=()):
    """(report lines, exit status); renamed = (OLD, NEW) symbol pairs"""
    base, new = parse(base_text), {}
    for t in new_texts:
        new.update(parse(t))
    out, bad = [], 0
    for old, sym in renamed:
        if old in base and sym in new and sym not in base:
            stream, desc = base.pop(old)
            base[sym] = ([ln.replace(old, sym) for ln in stream], desc)
        else:
            out.append(f"missing  {sym}\n    --renamed {old}={sym}: " +
                       ("no such baseline symbol" if old not in base else
                        "no such new symbol" if sym not in new else "the baseline has both"))
            bad = 1
    for sym in sorted(set(base) | set(new)):
        gone_ok = sym in removed or any(n in removed for n in source_names(sym))
        if sym not in new:
            out.append(f"{'removed' if gone_ok else 'missing'}  {sym}")
            bad |= not gone_ok
        elif sym not in base:
            out.append(f"new  {sym}")
        else:
            (sa, da), (sb, db) = base[sym], new[sym]
            if da != db:
                fields = ", ".join(f"{f} {da.get(f)} -> {db.get(f)}" for f in sorted(set(da) | set(db))
                                   if da.get(f) != db.get(f))
                out.append(f"DESCRIPTOR-DIFF  {sym}\n    {fields}\n    {delta(sa, sb)}")
                bad = 1
            elif sa != sb:
                out.append(f"descriptor-same  {sym}\n    {delta(sa, sb)}")
            else:
                out.append(f"same  {sym}")
    return out, int(bad)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("base")
    ap.add_argument("new", nargs="+")
    ap.add_argument("--removed", action="append", default=[], metavar="NAME")
    ap.add_argument("--renamed", action="append", default=[], metavar="OLD=NEW")
    a = ap.parse_args(argv)
    if any(r.count("=") != 1 for r in a.renamed):
        ap.error("--renamed takes OLD=NEW")
    read = lambda p: open(p, encoding="utf-8", errors="replace").read()
    out, rc = compare(read(a.base), [read(p) for p in a.new], a.removed, [r.split("=") for r in a.renamed])
    print("\n".join(out))
    return rc


if __name__ == "__main__":
    sys.exit(main())
