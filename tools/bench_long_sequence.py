#!/usr/bin/env python3
"""Times the fused relaxation iteration over the sequence length: the headline recipe of bench.py (synthetic sequence,
N = 4096, P = 20, Chamfer + flow, graph replay, no host sync) at pose_len B = T - 1 in {19, 58, 59, 116, 232, 464}, and
B in {19, 58} again with tune_long = 1 (the long-sequence kernels of csrc/model_long.hip on shapes that fit in LDS: the
only same-shape A/B of the two paths).

    python tools/bench_long_sequence.py [--parent-root DIR] [--out profiles/long_sequence_bench.json]
        every shape in a child process of its own under a time limit (a failing child ends the run); with --parent-root
        (a built checkout of the commit to compare with) B = 19 and 58 are also run on that tree, alternated with this
        one.  A whole tree, not REART_LIB alone: the bindings refuse a library that lacks an entry point they declare.
    python tools/bench_long_sequence.py --shape B[,long]
        one shape: warm-up, five timed windows of at least 0.5 s, one JSON line (median, min, max iterations/s)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_long_sequence.py --shape B[,long] --trace-steps 200
        kernel times come from a separate run like this one (never together with --pmc), summarised by
    python tools/bench_long_sequence.py --kernel-stats DIR
        mean time per call of the model's kernels, from the *kernel_stats.csv under DIR
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.environ.get("REART_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(19, 0), (58, 0), (59, 0), (116, 0), (232, 0), (464, 0), (19, 1), (58, 1)]
N, P = 4096, 20


def build(B, long_):
    import numpy as np
    import torch

    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine, tuning_from_env
    from reart_amd.synthetic import make_sequence, split_canonical

    dev = torch.device("cuda:0")
    seq = make_sequence(T=B + 1, n_parts=8, pts_per_part=N // 8, seed=2, n_ref=3000, with_flow=True)
    ci = (B + 1) // 2
    cano, pcs = split_canonical(seq["complete"], ci)
    torch.manual_seed(2)
    model = BaseModel(num_parts=P, pose_len=B).to(dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tuning = tuning_from_env()
    if long_:
        tuning["tune_long"] = 1       # (a tree without the field fails here: the long kernels are not in it)
    return RelaxEngine(t(cano), t(pcs), model, ci, [t(r) for r in seq["ref_loc"]], [t(f) for f in seq["ref_flow"]],
                       n_iter=15000, seed=2, tuning=tuning)


def run_shape(B, long_, trace_steps, window_s=0.5, repeats=5):
    import torch

    eng = build(B, long_)
    eng.capture(steps_per_graph=10)
    if trace_steps:
        eng.step(trace_steps)
        torch.cuda.synchronize()
        return dict(B=B, tune_long=long_, traced_steps=trace_steps)
    eng.step(50)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.step(50)
    torch.cuda.synchronize()
    per = max((time.perf_counter() - t0) / 50, 1e-6)
    n = max(50, int(window_s * 1.2 / per) // 10 * 10)
    rates = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.step(n)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        rates.append(n / el)
    it, log = eng.loss_log()
    import numpy as np

    assert np.isfinite(log.cpu().numpy()).all()
    return dict(B=B, tune_long=long_, N=N, P=P, steps_per_window=n, window_s=round(n / statistics.median(rates), 3),
                it_s_median=round(statistics.median(rates), 1), it_s_min=round(min(rates), 1), it_s_max=round(max(rates), 1),
                us_per_iter=round(1e6 / statistics.median(rates), 2))


def kernel_stats(d):
    """{kernel family: mean microseconds per call} of the model's kernels from rocprofv3's kernel_stats.csv under d."""
    out = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            for fam in ("base_fwd_long_kernel", "base_fwd_kernel", "base_bwd_long_kernel", "base_bwd_block_kernel",
                        "base_bwd_finalize_kernel", "pose_table_kernel", "search", "post_kernel"):
                if fam in name:
                    calls, total = int(row["Calls"]), float(row["TotalDurationNs"])
                    c0, t0 = out.get(fam, (0, 0.0))
                    out[fam] = (c0 + calls, t0 + total)
                    break
    return {k: dict(calls=c, us_per_call=round(t / c / 1e3, 2)) for k, (c, t) in out.items()}


def child(shape, root=None, timeout=240):
    env = dict(os.environ)
    if root:
        env["REART_BENCH_ROOT"] = os.path.abspath(root)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", "%d,%d" % shape], env=env, timeout=timeout,
                       capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"shape {shape} (tree {root or 'this one'}) ended with status {r.returncode}: nothing more is started")
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape")
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--parent-root")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_stats(a.kernel_stats)))
        return
    if a.shape:
        v = [int(x) for x in a.shape.split(",")]
        print(json.dumps(run_shape(v[0], v[1] if len(v) > 1 else 0, a.trace_steps)))
        return
    results = dict(recipe=f"synthetic, N={N}, P={P}, Chamfer + flow, graph replay (10 iterations per graph)", shapes=[], parent_ab=[])
    if a.parent_root:
        for B in (19, 58):
            for rep in range(2):            # alternated: parent, branch, parent, branch
                for tag, lib in (("parent", a.parent_root), ("branch", None)):
                    results["parent_ab"].append(dict(child((B, 0), lib), which=tag, round=rep))
    for shape in SHAPES:
        results["shapes"].append(child(shape))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
