#!/usr/bin/env python3
"""Throughput of the import-only path: the reference's loop body over the HIP operators with PyTorch autograd and
torch.optim.Adam (run_robot.OperatorLoop), base model, on the headline workload (synthetic T = 20 frames x N = 4096 points,
20 parts, Chamfer + flow), without `--fused_losses` (two knn_points searches + the sorted backward per iteration, one
blend_anchor_motion per frame pair) and with it (ChamferLoss + blend_anchor_motion_batch).

Timing: device events around `--iters` iterations after `--warmup`, `--reps` repeats, the two paths alternating in one process;
median, minimum and maximum in iterations per second.  `--mode baseline` builds and times the flag-off loop alone and uses
nothing newer than OperatorLoop itself, so with `--tree DIR` (import reart_amd from a checkout in DIR) the same script measures
an older commit.  Writes --out (default profiles/operator_loop_bench.json) and prints it as one JSON line.

Launches per iteration come from kernel traces taken in runs of their own (tracing slows the host): `--count K` runs warm-up +
K iterations of ONE mode untimed; two such runs with different K under `rocprofv3 --kernel-trace -f csv -d DIR` differ by the
launches of the extra iterations.  `--launches OFF_A OFF_B ON_A ON_B --k K_A K_B` reads the four trace directories and adds
`launches_per_iteration` to --out.  `--merge-baseline PATH` adds the flag-off figures of a `--mode baseline --out PATH` run (of
another checkout, taken in the same session) to --out as `parent_commit_flag_off`.
Without a GPU it fails.
Usage: python tools/bench_operator_loop.py [--mode both|baseline|fused] [--iters 200] [--warmup 50] [--reps 5] [--tree DIR] [--out PATH]"""
import argparse
import csv
import functools
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_loop(rr, dev, fused, T, N, parts):
    import numpy as np
    import torch

    from reart_amd.networks.model import BaseModel
    from reart_amd.synthetic import make_sequence, split_canonical
    from reart_amd.utils.model_utils import tau_cosine

    seq = make_sequence(T=T, n_parts=8, pts_per_part=N // 8, seed=2, n_ref=3000, with_flow=True)
    cano, pcs = split_canonical(seq["complete"], 2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(dev)
    argv = ["--model", "base", "--use_flow_loss", "--cano_idx", "2", "--num_parts", str(parts)] + (["--fused_losses"] if fused else [])
    a = rr.build_parser().parse_args(argv)
    torch.manual_seed(2)
    model = BaseModel(num_parts=parts, pose_len=T - 1).to(dev)
    tau = functools.partial(tau_cosine, max_iter=a.n_iter, end_temp=a.end_tau, start_temp=a.start_tau)
    return rr.OperatorLoop(a, model, t(cano), t(pcs), [t(r) for r in seq["ref_loc"]], [t(f) for f in seq["ref_flow"]], tau)


class Runner:
    def __init__(self, loop):
        self.loop, self.i, self.last = loop, 0, None

    def run(self, n):
        for _ in range(n):
            self.last = self.loop.iteration(self.i)
            self.i += 1

    def window(self, n):
        import torch

        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        self.run(n)
        e1.record()
        torch.cuda.synchronize()
        return n / (1e-3 * e0.elapsed_time(e1))


def stats(v):
    v = sorted(v)
    return dict(median_it_s=round(v[len(v) // 2], 1), min_it_s=round(v[0], 1), max_it_s=round(v[-1], 1))


def trace_rows(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {d}")
    return sum(1 for f in files for _ in csv.DictReader(open(f)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="both", choices=["both", "baseline", "fused"])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--parts", type=int, default=20)
    ap.add_argument("--count", type=int, default=None, help="untimed: warm-up + this many iterations of --mode baseline|fused (for a trace)")
    ap.add_argument("--launches", nargs=4, metavar="DIR", help="trace directories: flag off K_A, off K_B, flag on K_A, on K_B")
    ap.add_argument("--k", nargs=2, type=int, default=[10, 30], metavar="K", help="the --count of the A and the B traces")
    ap.add_argument("--merge-baseline", metavar="PATH", help="add the flag_off figures of this baseline run's JSON to --out")
    ap.add_argument("--tree", default=ROOT, help="import reart_amd from this checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "operator_loop_bench.json"))
    args = ap.parse_args()

    if args.merge_baseline:
        out, base = json.load(open(args.out)), json.load(open(args.merge_baseline))
        out["parent_commit_flag_off"] = {k: base["flag_off"][k] for k in ("median_it_s", "min_it_s", "max_it_s")}
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
        return
    if args.launches:
        out = json.load(open(args.out))
        n = [trace_rows(d) for d in args.launches]
        per = args.k[1] - args.k[0]
        out["launches_per_iteration"] = {"flag_off": round((n[1] - n[0]) / per, 2), "fused_losses": round((n[3] - n[2]) / per, 2),
                                         "method": f"kernel-trace rows of {args.k[1]} minus {args.k[0]} iterations, one traced run each"}
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
        return

    sys.path.insert(0, os.path.abspath(args.tree))
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_operator_loop.py needs an MI355X")
    from reart_amd import run_robot as rr

    dev = torch.device("cuda:0")
    modes = {"both": ("flag_off", "fused_losses"), "baseline": ("flag_off",), "fused": ("fused_losses",)}[args.mode]
    runners = {m: Runner(build_loop(rr, dev, m == "fused_losses", args.frames, args.points, args.parts)) for m in modes}
    for r in runners.values():
        r.run(args.warmup)
    if args.count is not None:
        for r in runners.values():
            r.run(args.count)
        torch.cuda.synchronize()
        print(json.dumps({"mode": args.mode, "counted_iterations": args.count}))
        return
    rates = {m: [] for m in modes}
    for _ in range(args.reps):                       # the paths alternate
        for m in modes:
            rates[m].append(runners[m].window(args.iters))
    out = {"workload": f"OperatorLoop, base model, synthetic T={args.frames} x N={args.points}, {args.parts} parts, Chamfer + flow",
           "iters": args.iters, "warmup": args.warmup, "reps": args.reps, "tree": os.path.abspath(args.tree) == ROOT and "this commit" or "other checkout",
           "device": torch.cuda.get_device_name(0),
           "note": "the modes alternate in one process and draw their Gumbel noise from one generator in turn, so their trajectories "
                   "(last_losses) differ"}
    for m in modes:
        out[m] = stats(rates[m])
        out[m]["last_losses"] = {k: float(v.detach()) for k, v in runners[m].last.items()}
    if len(modes) == 2:
        off, on = out["flag_off"], out["fused_losses"]
        out["fused_over_off_median"] = round(on["median_it_s"] / off["median_it_s"], 3)
        out["ranges_apart"] = bool(on["min_it_s"] > off["max_it_s"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
