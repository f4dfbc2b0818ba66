#!/usr/bin/env python3
"""Static instruction counts of the search kernel per region of a wave's fixed part (profiles/search_fixed_isa_counts.txt).

Compiles a prune.hip with the Makefile's flags and -DREART_PRUNE_MARKS to gfx950 assembly, cuts the text of one kernel at the
PR_MARK comment lines and counts, per piece, VALU / SALU / SMEM / LDS / VMEM instructions (s_waitcnt and s_nop apart).
    python tools/isa_regions.py [path/to/prune.hip] [--kernel knn_group_kernelILb0] [--include DIR ...]
A piece runs from its mark to the next mark IN THE TEXT: the block layout follows the source closely but not exactly, and the
scheduler moves arithmetic across a mark (it is a comment, not a barrier), so a piece is good to a few instructions.  Both
instantiations of knn_pruned_wave are inlined: every mark of it appears twice (`#1`, `#2`; the one with nine loads in `seeds`
is K = 3).  Needs hipcc, no GPU."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("VALU", "SALU", "SMEM", "LDS", "VMEM", "waitcnt", "nop")


def classify(op):
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op == "s_nop":
        return "nop"
    if op.startswith(("s_load", "s_buffer_load")):
        return "SMEM"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source", nargs="?", default=os.path.join(ROOT, "reart_amd", "csrc", "prune.hip"))
    ap.add_argument("--kernel", default="knn_group_kernelILb0")
    ap.add_argument("--include", action="append", default=[])
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "prune.s")
        cmd = [args.hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
               "-DREART_PRUNE_MARKS", args.source, "-o", out] + [f"-I{d}" for d in args.include]
        subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
        text = open(out).read().splitlines()
    start = next((k for k, l in enumerate(text) if re.match(r"^_Z\w*" + re.escape(args.kernel) + r"\w*:", l)), None)
    if start is None:
        sys.exit(f"no kernel matching {args.kernel}")
    name = text[start].split(":")[0]
    regions, seen = [["entry", collections.Counter()]], collections.Counter()
    for l in text[start + 1:]:
        t = l.strip()
        if t.startswith(".Lfunc_end"):
            break
        m = re.match(r";\s*PRMARK (\w+)", t)
        if m:
            seen[m.group(1)] += 1
            regions.append([f"{m.group(1)}#{seen[m.group(1)]}", collections.Counter()])
            continue
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        c = classify(t.split()[0])
        if c:
            regions[-1][1][c] += 1
    print(f"# {name}")
    print("# region        " + "".join(f"{c:>9}" for c in CLASSES) + "   VALU+SALU")
    tot = collections.Counter()
    for rname, cnt in regions:
        tot.update(cnt)
        print(f"{rname:<16}" + "".join(f"{cnt[c]:>9}" for c in CLASSES) + f"{cnt['VALU'] + cnt['SALU']:>12}")
    print(f"{'whole kernel':<16}" + "".join(f"{tot[c]:>9}" for c in CLASSES) + f"{tot['VALU'] + tot['SALU']:>12}")


if __name__ == "__main__":
    main()
