"""Static instruction count of a kernel in a hipcc -S listing, split by VALU / scalar / LDS / memory, up to the first
write-through observation store (`buffer_store_dwordx4 ... sc1`) and in all.

    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> --cuda-device-only -S -o overcooked.s csrc/overcooked.hip
    python tools/front_count.py overcooked.s 'mrl_overcooked_step_fixedILi20ELi8ELi5ELi1ELi6ELb0ELb0ELb1E'

Lines are counted in listing order from the kernel's entry, so blocks that hipcc lays out in front of the first store
but that a full group never executes (none in the shipped kernels: the rare paths sit behind s_endpgm) would be counted
too; --skip LABEL[,LABEL...] leaves out the blocks that start at these labels (up to the next label)."""
import argparse
import re
import sys


def classify(op):
    if op.startswith(("ds_",)):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "mem"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "scalar"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("kernel", help="substring of the mangled kernel name")
    ap.add_argument("--skip", default="")
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    lines = open(args.listing).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and args.kernel in l and ":" in l)  # the entry label
    front, total = {}, {}
    seen_store = False
    skipping = False
    detail = {"branch": 0, "wait": 0, "v_cmp": 0, "v_cndmask": 0, "saveexec": 0, "exec_restore": 0, "mask_op": 0}
    for l in lines[start + 1:]:
        s = l.strip()
        if s.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            skipping = m.group(1) in skip
            continue
        if not s or s.startswith((";", ".")):
            continue
        op = s.split()[0]
        c = classify(op)
        if c is None:
            continue
        total[c] = total.get(c, 0) + 1
        if seen_store or skipping:
            continue
        if op == "buffer_store_dwordx4" and "sc1" in s:
            seen_store = True
            continue
        front[c] = front.get(c, 0) + 1
        if op.startswith(("s_cbranch", "s_branch")):
            detail["branch"] += 1
        elif op.startswith(("s_waitcnt", "s_nop")):
            detail["wait"] += 1
        elif op.startswith("v_cmp"):
            detail["v_cmp"] += 1
        elif op.startswith("v_cndmask"):
            detail["v_cndmask"] += 1
        elif "saveexec" in op:
            detail["saveexec"] += 1
        elif re.match(r"s_(or|and|andn2|mov)_b64$", op) and re.search(r"\bexec\b", s.split(None, 1)[1].split(",")[0]):
            detail["exec_restore"] += 1
        elif re.match(r"s_(and|or|xor|andn2|orn2|nor|nand)_b64$", op):
            detail["mask_op"] += 1
    order = ("valu", "scalar", "lds", "mem")
    print("in front of the first sc1 store:", "  ".join(f"{k} {front.get(k, 0)}" for k in order), " all", sum(front.values()))
    print("   of these:", "  ".join(f"{k} {v}" for k, v in detail.items()))
    print("whole kernel:                   ", "  ".join(f"{k} {total.get(k, 0)}" for k in order), " all", sum(total.values()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
