#!/usr/bin/env python3
"""Compare two gfx950 assembly listings of one translation unit, kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --offload-device-only -S sat_conv_glds.hip -o new.s
    python tools/isa_diff.py old.s new.s

A kernel is "the same" when its instruction lines (comments, directives and blank lines stripped) and its resource
metadata (.vgpr_count, .sgpr_count, .group_segment_fixed_size, .private_segment_fixed_size, .vgpr_spill_count) are equal.
Prints the kernels that differ, with instruction-count and metadata deltas, and exits non-zero if there are any.
"""
import re
import sys

META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count")
_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")


def _strip(line):
    line = line.split(";", 1)[0]              # (no string literal with a ';' occurs on an instruction line)
    line = re.sub(r"//.*", "", line)
    return " ".join(line.split())


def parse(path):
    """-> ({kernel symbol: [instruction lines]}, {kernel symbol: {metadata key: value}})"""
    text = open(path, errors="replace").read().splitlines()
    kernels = {m.group(1) for line in text for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)] if m}
    body, cur = {}, None
    for line in text:
        m = _LABEL.match(line)
        if m and m.group(1) in kernels:
            cur = body.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        s = _strip(line)
        if s.startswith(".Lfunc_end") or s.startswith(".section") or s.startswith(".amdhsa_kernel"):
            cur = None
            continue
        if not s or s.startswith("."):          # directives and local labels (.LBB...) carry no instruction
            if s.startswith(".LBB") or s.startswith(".Ltmp"):
                cur.append(re.sub(r"\d+", "#", s))      # keep the block structure, not its numbering
            continue
        cur.append(re.sub(r"\.LBB\d+_\d+", ".LBB#", s))
    # amdhsa.kernels: one YAML list entry per kernel, its keys in alphabetical order (so .name comes after some of them)
    items = [(len(m.group(1)), m.group(2) == "-", m.group(3), m.group(4))
             for line in text for m in [re.match(r"^(\s*)(-?)\s*(\.[a-z_]+):\s*(\S*)", line)] if m]
    top = min((ind for ind, dash, _, _ in items if dash), default=0)
    meta, entry = {}, {}
    for ind, dash, key, val in items + [(top, True, "", "")]:
        if dash and ind == top:
            if entry.get(".name") in kernels:
                meta[entry[".name"]] = {k: entry.get(k) for k in META}
            entry = {}
        if ind <= top + 2:                      # the entry's own keys, not those of its .args
            entry[key] = val
    return body, meta


def n_insn(lines):
    return sum(1 for s in lines if not s.startswith("."))


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    (b0, m0), (b1, m1) = parse(argv[1]), parse(argv[2])
    bad = []
    for k in sorted(set(b0) | set(b1)):
        if k not in b0 or k not in b1:
            bad.append(f"{k}: only in {'the second' if k not in b0 else 'the first'} listing")
            continue
        why = []
        if b0[k] != b1[k]:
            at = next((i for i, (x, y) in enumerate(zip(b0[k], b1[k])) if x != y), min(len(b0[k]), len(b1[k])))
            first = " | ".join(v[at] if at < len(v) else "<end>" for v in (b0[k], b1[k]))
            why.append(f"instructions {n_insn(b0[k])} -> {n_insn(b1[k])} (first difference at line {at}: {first})")
        for key in META:
            v0, v1 = m0.get(k, {}).get(key), m1.get(k, {}).get(key)
            if v0 != v1:
                why.append(f"{key} {v0} -> {v1}")
        if why:
            bad.append(f"{k}: " + ", ".join(why))
    print(f"{len(b0)} / {len(b1)} kernels, {len(bad)} differ")
    for line in bad:
        print("  " + line)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
