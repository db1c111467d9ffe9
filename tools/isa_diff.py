#!/usr/bin/env python3
"""Compare the kernels of two gfx950 assembly files (the *-hip-amdgcn-amd-amdhsa-gfx950.s that -save-temps=obj leaves):

    tools/isa_diff.py OLD.s NEW.s

Per kernel symbol `same` -- every instruction (comments dropped, branch labels kept) and the four resource lines of the kernel
descriptor agree -- or the instruction counts, those four values and the mnemonics whose counts changed.  A text comparison for
refactors that must not move the code; run by hand, not part of the build."""
import collections
import re
import subprocess
import sys

RES = ("next_free_vgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    """{symbol: (instruction and label lines, {resource: value})} of every kernel of the file"""
    code, res, cur, desc = {}, {}, None, None
    for raw in open(path):
        line = re.sub(r"\s*;.*", "", raw).strip()
        m = re.match(r"\.(type|amdhsa_kernel|amdhsa_(\w+))\s+([^,\s]+)(,@function)?", line)
        if not line:
            continue
        if m and m.group(1) == "amdhsa_kernel":
            desc = res.setdefault(m.group(3), {})
        elif line == ".end_amdhsa_kernel":
            desc = None
        elif desc is not None:
            if m and m.group(2) in RES:
                desc[m.group(2)] = m.group(3)
        elif m and m.group(4):
            cur = code.setdefault(m.group(3), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and (not line.startswith(".") or re.match(r"\.LBB\w+:", line)):
            cur.append(line)
    return {k: (code[k][1:], res[k]) for k in res if k in code}      # [1:]: the symbol's own label


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    syms = sorted(set(old) | set(new))
    names = dict(zip(syms, subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")))
    differ = 0
    for k in sorted(syms, key=names.get):
        if k in old and k in new and old[k] == new[k]:
            print(f"same      {names[k]}")
            continue
        differ += 1
        if k not in old or k not in new:
            print(f"{'only old' if k in old else 'only new'}  {names[k]}")
            continue
        (co, ro), (cn, rn) = old[k], new[k]
        mo, mn = (collections.Counter(l.split()[0] for l in c if not l.endswith(":")) for c in (co, cn))
        print(f"DIFFERS   {names[k]}\n    instructions {sum(mo.values())} -> {sum(mn.values())}")
        print("    " + ", ".join(f"{r} {ro.get(r)}" + ("" if ro.get(r) == rn.get(r) else f" -> {rn.get(r)}") for r in RES))
        print("    " + ", ".join(f"{m} {mo[m]} -> {mn[m]}" for m in sorted(set(mo) | set(mn)) if mo[m] != mn[m]))
    print(f"{len(syms) - differ} same, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
