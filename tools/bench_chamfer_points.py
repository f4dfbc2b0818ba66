#!/usr/bin/env python3
"""The per-point Chamfer distances as one warm operator (utils.chamfer.ChamferPoints: reart_chamfer_points and
reart_chamfer_points_backward) against what it replaces, on the headline shape (synthetic T = 20 frames x N = 4096 points):
value and gradient of  (w * d_xy).sum() + (v * d_yx).sum()  with random per-point weights, x drifting a little every call (a
fixed cycle of perturbed copies) against a fixed y.

  operator      ChamferPoints: one warm forward, one backward launch
  composition   the same expression through ChamferDistance: two cold knn_points searches and their backward

Timing: device events around --iters calls after --warmup, --reps repeats, the two sides alternating in one process; median
(min - max) milliseconds per call into --out (default profiles/chamfer_points_bench.json), printed as one JSON line.

Kernel times and launches per call come from traces taken in runs of their own (tracing slows the host):
`--count K --side operator|composition` runs warm-up + K calls of ONE side untimed, e.g. under
`rocprofv3 --kernel-trace --stats -f csv -d DIR --`.  `--kernel-stats LABEL=DIR ... --k K` reads such directories, writes
profiles/chamfer_points_kernel_stats.csv (per kernel: calls and average / minimum / maximum nanoseconds) and adds, per label,
launches per call and the kernel time per call (summed over the kernels that run in every call) to --out.
Without a GPU it fails."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(v, nd=4):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], nd), min=round(v[0], nd), max=round(v[-1], nd))


def merge(path, **items):
    out = json.load(open(path)) if os.path.exists(path) else {}
    out.update(items)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(items))


def window(fn, n):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n          # ms per call


def sides(dev, T, N, which):
    import numpy as np
    import torch

    from reart_amd.synthetic import make_sequence
    from reart_amd.utils.chamfer import ChamferDistance, ChamferPoints

    frames = make_sequence(T=T + 1, n_parts=8, pts_per_part=N // 8, seed=2, with_flow=False)["complete"].astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x0, y = t(frames[:-1]), t(frames[1:])
    gen = torch.Generator(device=dev).manual_seed(3)
    clouds = [(x0 + 1e-3 * torch.randn(x0.shape, device=dev, generator=gen)).requires_grad_(True) for _ in range(8)]
    w = torch.rand(x0.shape[:2], device=dev, generator=gen)
    v = torch.rand(y.shape[:2], device=dev, generator=gen)
    state = {"i": 0}
    fns = {}
    if "operator" in which:
        points = ChamferPoints()

        def operator():
            x = clouds[state["i"] % len(clouds)]
            state["i"] += 1
            d_xy, d_yx = points(x, y)
            return torch.autograd.grad((w * d_xy).sum() + (v * d_yx).sum(), x)
        fns["operator"] = operator
    if "composition" in which:
        cd = ChamferDistance()

        def composition():
            x = clouds[state["i"] % len(clouds)]
            state["i"] += 1
            return torch.autograd.grad((w * cd(x, y)).sum() + (v * cd(y, x)).sum(), x)
        fns["composition"] = composition
    return fns


def kernel_stats(args):
    rows, summary = [], {}
    for item in args.kernel_stats:
        label, d = item.split("=", 1)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit(f"no kernel stats under {d}")
        launches, every = 0, [0.0, 0.0, 0.0]
        for r in csv.DictReader(open(files[0])):
            calls = int(r["Calls"])
            name = r["Name"] if len(r["Name"]) <= 160 else r["Name"][:157] + "..."      # ATen's template names run to kilobytes
            rows.append([label, name, calls, r["AverageNs"], r["MinNs"], r["MaxNs"]])
            launches += calls
            if calls >= args.k:                 # runs in every call of the trace (its warm-up calls are traced too)
                for j, col in enumerate(("AverageNs", "MinNs", "MaxNs")):
                    every[j] += calls / args.k * float(r[col]) / 1e3
        summary[label] = {"launches_per_call": round(launches / args.k, 2), "traced_calls": args.k,
                          "kernels_us_per_call": dict(zip(("sum_of_averages", "sum_of_minima", "sum_of_maxima"), (round(v, 1) for v in every)))}
    with open(args.stats_out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Run", "Name", "Calls", "AverageNs", "MinNs", "MaxNs"])
        w.writerows(rows)
    merge(args.out, kernels=summary)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--count", type=int, default=None, help="untimed: warm-up + this many calls of --side (for a trace)")
    ap.add_argument("--side", choices=["operator", "composition"], default="operator")
    ap.add_argument("--kernel-stats", nargs="+", metavar="LABEL=DIR")
    ap.add_argument("--k", type=int, default=100, help="calls of the traced runs (their --warmup + --count)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chamfer_points_bench.json"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "chamfer_points_kernel_stats.csv"))
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args)
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_chamfer_points.py needs an MI355X")
    dev = torch.device("cuda:0")
    fns = sides(dev, args.frames, args.points, ("operator", "composition") if args.count is None else (args.side,))
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    if args.count is not None:
        for _ in range(args.count):
            fns[args.side]()
        torch.cuda.synchronize()
        print(json.dumps({"side": args.side, "counted_calls": args.count}))
        return
    ms = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            ms[k].append(window(fn, args.iters))
    a = {k: dict(stats(v), unit="ms per value + gradient") for k, v in ms.items()}
    a["ranges_apart"] = bool(a["operator"]["max"] < a["composition"]["min"] or a["composition"]["max"] < a["operator"]["min"])
    a["composition_over_operator_median"] = round(a["composition"]["median"] / a["operator"]["median"], 3)
    merge(args.out, workload=f"synthetic T={args.frames} x N={args.points}, weighted per-point Chamfer, x drifting against fixed y",
          device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, reps=args.reps, weighted_sum=a)


if __name__ == "__main__":
    main()
