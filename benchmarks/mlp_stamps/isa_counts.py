"""Instruction counts per basic block of one mlp_fused_kernel instantiation, from the compiler's assembly.

usage: isa_counts.py FILE.s [--kernel SUBSTRING] [--min N] [--out FILE.json --label NAME]
  FILE.s: mlp.hip compiled with the product flags plus  -DMLP_FAST_BUILD --cuda-device-only -S
  SUBSTRING of the mangled kernel name; default: the headline <8, false, true, false, false, false>.
Prints one line per basic block that holds MFMAs or at least N (default 16) vector instructions -- the chunk bodies are
the blocks with 128 (16 slots) or 8 x slots MFMAs, the two ReLU blocks hold 128 maxima (or compare / select pairs) and at
most the MFMAs of the slot they were scheduled into -- and the kernel's register and scratch sizes.
"""
import argparse
import json
import os
import re

ap = argparse.ArgumentParser()
ap.add_argument("asm")
ap.add_argument("--kernel", default="mlp_fused_kernelILi8ELb0ELb1ELb0ELb0ELb0E")
ap.add_argument("--min", type=int, default=16)
ap.add_argument("--out")
ap.add_argument("--label", default="build")
args = ap.parse_args()

lines = open(args.asm).read().split("\n")
begin = next(i for i, l in enumerate(lines) if re.match(r"^_ZN\S*" + re.escape(args.kernel) + r"\S*:", l))
end = next(i for i in range(begin, len(lines)) if lines[i].lstrip().startswith(".end_amdhsa_kernel"))

KEYS = ("mfma", "valu", "s_nop", "v_accvgpr", "v_cmp", "v_cndmask", "v_maximum3", "v_log", "lds", "vmem", "scratch")


def kind(op):
    if op.startswith("v_mfma"):
        return ["mfma"]
    if op.startswith("v_accvgpr"):
        return ["v_accvgpr"]
    if op.startswith("v_"):
        k = ["valu"]
        for name in ("v_cmp", "v_cndmask", "v_maximum3", "v_log"):
            if op.startswith(name):
                k.append(name)
        return k
    if op == "s_nop":
        return ["s_nop"]
    if op.startswith("ds_"):
        return ["lds"]
    if op.startswith("scratch_"):
        return ["scratch", "vmem"]
    if op.startswith(("global_", "buffer_", "flat_")):
        return ["vmem"]
    return []


blocks, cur = [], {"label": "entry", "line": begin}
for i in range(begin + 1, end):
    l = lines[i]
    m = re.match(r"^(\.LBB\S+):", l)
    if m:
        blocks.append(cur)
        cur = {"label": m.group(1), "line": i}
        continue
    t = l.strip()
    if not t or t[0] in ".;" or t.endswith(":"):
        continue
    for k in kind(t.split()[0]):
        cur[k] = cur.get(k, 0) + 1
blocks.append(cur)

total = {k: sum(b.get(k, 0) for b in blocks) for k in KEYS}
meta = {}
for l in lines[end:end + 400]:
    m = re.match(r"^; (ScratchSize|NumVgprs|NumAgprs|TotalNumVgprs|codeLenInByte|LDSByteSize): (\d+)", l)
    if m and m.group(1) not in meta:
        meta[m.group(1)] = int(m.group(2))
shown = [b for b in blocks if b.get("mfma", 0) or b.get("valu", 0) >= args.min]
for b in shown:
    print(b["label"], " ".join(f"{k}={b[k]}" for k in KEYS if b.get(k)))
print("total", " ".join(f"{k}={total[k]}" for k in KEYS))
print("meta", meta)
if args.out:
    table = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            table = json.load(f)
    table[args.label] = {"kernel": args.kernel, "meta": meta, "total": total,
                         "blocks": [{k: b[k] for k in ("label",) + KEYS if b.get(k)} for b in shown]}
    with open(args.out, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
