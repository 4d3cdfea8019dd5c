"""Static instruction counts of one kernel in a gfx950 assembly listing, whole and
per loop (a loop = the labels from a backward branch's target to the branch;
inner loops are listed on their own and are included in their outer loop).
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --save-temps=obj \
        -c minimap2_rs_amd/csrc/mm2g_kernels.hip -o /tmp/k.o
    python tools/isa_loops.py /tmp/mm2g_kernels-hip-amdgcn-amd-amdhsa-gfx950.s _Z11k_sort_readILb0ELi1024EEvN4mm2g8SortArgsE
Each loop line: first and last label, VALU / SALU / LDS / VMEM counts, and the
LDS / VMEM mnemonics in it (to tell the loops apart)."""
import re
import sys
from collections import Counter


def kind(m):
    if m.startswith("ds_"):
        return "LDS"
    if m.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "VMEM"
    if m.startswith("v_"):
        return "VALU"
    if m.startswith("s_"):
        return "SALU"
    return "other"


def main():
    path, kern = sys.argv[1], sys.argv[2]
    body, on = [], False
    for ln in open(path):
        if ln.startswith(kern + ":"):
            on = True
            continue
        if on:
            if ln.startswith(".Lfunc_end"):
                break
            body.append(ln.rstrip())
    labels, ins = {}, []          # label -> index of its first instruction; (mnemonic, operands)
    for ln in body:
        t = ln.split(";")[0].strip()
        if not t or t.startswith("."):
            m = re.match(r"^(\.LBB\d+_\d+):", t)
            if m:
                labels[m.group(1)] = len(ins)
            continue
        parts = t.split(None, 1)
        ins.append((parts[0], parts[1] if len(parts) > 1 else ""))
    tot = Counter(kind(m) for m, _ in ins)
    print(f"{kern}: {len(ins)} instructions", dict(tot))
    loops = set()
    for i, (m, ops) in enumerate(ins):
        if m.startswith("s_cbranch") or m == "s_branch":
            tgt = ops.strip()
            if tgt in labels and labels[tgt] <= i:
                loops.add((labels[tgt], i, tgt))
    for a, b, tgt in sorted(loops):
        c = Counter(kind(m) for m, _ in ins[a:b + 1])
        mem = Counter(m for m, _ in ins[a:b + 1] if kind(m) in ("LDS", "VMEM"))
        print(f"  {tgt:>12} [{a:5d},{b:5d}] VALU {c['VALU']:5d} SALU {c['SALU']:5d} LDS {c['LDS']:4d} VMEM {c['VMEM']:4d}  "
              + " ".join(f"{k}x{v}" for k, v in sorted(mem.items())))


if __name__ == "__main__":
    main()
