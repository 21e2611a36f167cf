#!/usr/bin/env python3
"""
Scan a gfx950 assembly listing for the wait states the compiler cannot count around MFMAs and wide stores that sit in `asm`
statements (csrc/gemm_dense.h, gemm_dense128.h, gemm_i8_inplace.h, gemm_fused4.h issue them that way: DESIGN.md 5.3b).

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off --cuda-device-only -S csrc/gemm_dense.hip -o gemm_dense.s
    python tools/mfma_asm_hazards.py gemm_dense.s

Reported, with the first few places of each kind, and the exit status is 1 if A or C is found:
  A  a VALU instruction writes a register that an MFMA reads less than two wait states later (the allocator's v_accvgpr_mov in
     front of an MFMA of the tail: the asm statement has to begin with `s_nop 1`);
  C  a VALU instruction writes a data register of a buffer / global store of more than 8 bytes less than two wait states behind
     it (the statement has to end with `s_nop 1`);
  B  a vector instruction touches the destination of an MFMA that is fewer than three MFMAs and twelve instructions old -- listed
     for reading only: behind a k-loop a barrier and a wait usually lie in between.
"""
import re
import sys


def regs(tok):
    out = set()
    for m in re.finditer(r"\b([av])\[(\d+):(\d+)\]|\b([av])(\d+)\b", tok):
        if m.group(1):
            out |= {(m.group(1), i) for i in range(int(m.group(2)), int(m.group(3)) + 1)}
        else:
            out.add((m.group(4), int(m.group(5))))
    return out


def instructions(path):
    ins = []
    for line in open(path):
        if not line.startswith("\t"):
            continue
        text = line.split(";")[0].strip()
        if not text or text.startswith("."):
            continue
        op, _, rest = text.partition(" ")
        ins.append((op, [o.strip() for o in rest.split(",")], text))
    return ins


def scan(ins, show=5):
    found = {"A": [], "B": [], "C": []}
    for i, (op, ops, text) in enumerate(ins):
        if op.startswith("v_mfma"):
            dst = regs(ops[0])
            src = set().union(*[regs(o) for o in ops[1:]])
            states = 0
            for k in range(1, 4):                       # A: back over at most two wait states
                if i - k < 0:
                    break
                pop, pops, ptext = ins[i - k]
                if pop == "s_nop":
                    states += int(pops[0]) + 1
                    continue
                if pop.startswith("v_mfma") or states >= 2:
                    break
                if pop.startswith("v_") and regs(pops[0]) & src:
                    found["A"].append(f"{ptext}  ->  {text}")
                states += 1
            mfmas = 0
            for k in range(1, 13):                      # B: ahead
                if i + k >= len(ins):
                    break
                nop_, nops, ntext = ins[i + k]
                if nop_.startswith("v_mfma"):
                    mfmas += 1
                    if mfmas >= 3:
                        break
                    continue
                if nop_.startswith(("v_", "ds_", "buffer_", "global_")) and set().union(*[regs(o) for o in nops]) & dst:
                    found["B"].append(f"{text}  ->  {ntext}  (+{k} instructions, {mfmas} MFMAs between)")
        elif op.startswith(("buffer_store_dwordx", "global_store_dwordx")) and op[-1] in "34":
            data = regs(ops[0]) if op.startswith("buffer") else regs(ops[1])
            states = 0
            for k in (1, 2):                            # C
                if i + k >= len(ins) or states >= 2:
                    break
                nop_, nops, ntext = ins[i + k]
                if nop_ == "s_nop":
                    states += int(nops[0]) + 1
                    continue
                if nop_.startswith("v_") and not nop_.startswith("v_mfma") and regs(nops[0]) & data:
                    found["C"].append(f"{text}  ->  {ntext}")
                states += 1
    for kind in "ACB":
        print(f"{kind}: {len(found[kind])}")
        for line in found[kind][:show]:
            print("   ", line)
    return found


if __name__ == "__main__":
    f = scan(instructions(sys.argv[1]))
    sys.exit(1 if f["A"] or f["C"] else 0)
