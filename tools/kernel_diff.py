#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds, unit by unit: the check a refactor of kernel code
rests on (the method of profiles/r11_kernel_disasm_pipe_split.txt).

Per unit: llvm-objdump -d of the unbundled code object, split per kernel symbol, with addresses
and the padding after each function stripped, compared as text; and each kernel's metadata note
(VGPR / SGPR / AGPR counts, spill counts, scratch, static LDS, workgroup size).  A pc-relative
data address (an instruction's 32-bit literal that, added to the instruction's own end, lands on
a data symbol) is compared as that symbol's section, size and offset, so a kernel does not differ
because a constant moved or was renamed.  Exits non-zero on any difference.

usage: python3 tools/kernel_diff.py <build dir A> <build dir B> [--rename OLD=NEW ...] [unit ...]
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile

from kernel_regs import B, code_object

META = ("vgpr_count", "sgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count",
        "private_segment_fixed_size", "group_segment_fixed_size", "max_flat_workgroup_size")


def run(*cmd):
    return subprocess.check_output(cmd, text=True)


def load(obj):
    """{kernel symbol: (instruction lines, metadata tuple)} of one object file."""
    with tempfile.TemporaryDirectory() as t:
        co = code_object(obj, t)
        meta = {}
        for blk in re.split(r"\n\s+- \.", run(f"{B}/llvm-readelf", "--notes", co)):
            m = re.search(r"\.name:\s+(\S+)", blk)
            if m:
                meta[m.group(1)] = tuple(int((re.search(r"\." + k + r":\s+(\d+)", blk) or [0, "0"])[1]) for k in META)
        secs = {int(m[1]): m[2] for m in re.finditer(r"^\s*\[\s*(\d+)\] (\S+)", run(f"{B}/llvm-readelf", "-S", co), re.M)}
        size, data = {}, []  # function sizes; (address, size, section) of the data symbols
        for m in re.finditer(r"^\s*\d+: ([0-9a-f]+)\s+(\d+)\s+(\w+)\s+\w+\s+\w+\s+(\d+) (\S+)",
                             run(f"{B}/llvm-readelf", "-sW", co), re.M):
            if m[3] == "FUNC":
                size[m[5]] = int(m[2])
            elif m[3] == "OBJECT" and not m[5].endswith(".kd"):
                data.append((int(m[1], 16), int(m[2]), secs.get(int(m[4]), m[4])))
        out, name, end = {}, None, 0
        for ln in run(f"{B}/llvm-objdump", "-d", "--no-show-raw-insn", co).splitlines():
            h = re.match(r"([0-9a-f]+) <(\S+)>:$", ln)
            if h:
                name = h[2] if h[2] in meta else None
                end = int(h[1], 16) + size.get(h[2], 0)
                if name:
                    out[name] = ([], meta[name])
                continue
            m = re.match(r"\t(.*?)\s*// ([0-9A-F]+): ((?:[0-9A-F]{8} ?)+)", ln)
            if not (name and m) or int(m[2], 16) >= end:  # (past the symbol's size: padding)
                continue
            text, words = m[1], m[3].split()
            if len(words) == 2:  # a literal: pc-relative to a data symbol?
                tgt = (int(m[2], 16) + int(words[1], 16)) & 0xFFFFFFFF  # (after s_getpc: its result is this address)
                for a, sz, sec in data:
                    if a <= tgt < a + max(sz, 1):
                        text = re.sub(r"0x[0-9a-f]+$", f"<{sec} object of {sz} bytes + {tgt - a}>", text)
            out[name][0].append(text)
        return out


def main():
    args, ren = [], {}
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--rename":
            old, new = next(it).split("=")
            ren[old] = new
        else:
            args.append(a)
    da, db = args[0], args[1]
    units = args[2:] or sorted({f[:-2] for d in (da, db) for f in os.listdir(d) if f.endswith(".o")})
    print(f"{'unit':24s} {'kernel symbols (A / B)':30s} {'same set':10s} {'identical streams':18s} identical registers+LDS+scratch")
    ndiff, detail = 0, []
    for u in units:
        oa, ob = (os.path.join(d, u + ".o") for d in (da, db))
        if not all(os.path.exists(o) and b".hip_fatbin" in open(o, "rb").read() for o in (oa, ob)):
            if os.path.exists(oa) != os.path.exists(ob):
                ndiff += 1
                print(f"{u:24s} in one build only")
            continue  # (a host-only unit)
        ka = {ren.get(k, k): v for k, v in load(oa).items()}
        kb = load(ob)
        both = sorted(set(ka) & set(kb))
        only = [f"    only in A: {k}" for k in sorted(set(ka) - set(kb))] + [f"    only in B: {k}" for k in sorted(set(kb) - set(ka))]
        st = [k for k in both if ka[k][0] == kb[k][0]]
        mt = [k for k in both if ka[k][1] == kb[k][1]]
        print(f"{u:24s} {f'{len(ka)} / {len(kb)}':30s} {'no' if only else 'yes':10s} "
              f"{f'{len(st)} of {len(both)}':18s} {len(mt)} of {len(both)}")
        print("\n".join(only), end="\n" if only else "")
        ndiff += len(only)
        for k in both:
            if k in st and k in mt:
                continue
            ndiff += 1
            detail.append(f"--- {u}: {k}")
            if k not in mt:
                detail.append("    " + ", ".join(f"{n} {x} -> {y}" for n, x, y in zip(META, ka[k][1], kb[k][1]) if x != y))
            if k not in st:
                d = list(difflib.unified_diff(ka[k][0], kb[k][0], "A", "B", lineterm="", n=2))
                detail += ["    " + x for x in d[:60]] + ([f"    ... {len(d) - 60} more diff lines"] if len(d) > 60 else [])
    print(f"differences among kernels present in both builds, or kernels in one build only: {ndiff}")
    print("\n".join(detail), end="\n" if detail else "")
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main())
