#!/usr/bin/env python3
"""Forward + backward of the connection term on pc_trans_list: networks.loss.ConnectionTerm (reart_connection_select +
reart_connection_term) against the composition networks.loss.compute_connection_loss with utils.chamfer.ChamferDistance(), the
reference's loop over the edges, on the same GPU.  T = 19 frames, N = 4096 points, P = 20 parts (slabs of the cloud along x, 204
or 205 points each, so every part has at least k points), k = 10:

  chain       E = 19, the edges BaseModel.joint_connection holds
  all_pairs   E = 380, all ordered pairs of different parts
Three sides: `operator_select` selects anew in every call (labels that change every iteration), `operator_kept` calls
select() once and then forward(pc_trans_list) (labels that never change), `composition`.  Timing: device events around --iters
calls after --warmup, --reps repeats, the sides alternating in one process; median (min - max), milliseconds per forward +
backward.  Merges its figures into --out (default profiles/connection_term_bench.json) and prints them as one JSON line.

`--only SIDE --calls N --shape NAME` runs N calls of one side and nothing else: the process a kernel trace counts launches of.
`--launches STATS.csv --only SIDE --shape NAME --calls N` reads the kernel statistics of such a trace (rocprofv3 --kernel-trace
--stats) and merges the launches per call into --out: kernels dispatched at least N times, divided by N.
Without a GPU it fails."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_flow_term import merge, stats, window  # noqa: E402

SIDES = ("operator_select", "operator_kept", "composition")


def make_inputs(dev, T, N, P, seed=5):
    import numpy as np
    import torch

    rng = np.random.default_rng(seed)
    cano = rng.uniform(-0.5, 0.5, (N, 3)).astype(np.float32)
    seg = np.empty(N, np.int64)
    seg[np.argsort(cano[:, 0], kind="stable")] = np.arange(N) * P // N
    pc = (cano[None] + rng.normal(0, 0.02, (T, N, 3))).astype(np.float32)
    to = lambda a: torch.from_numpy(a).to(dev)
    return to(cano), to(seg), to(pc).requires_grad_(True)


def sides(dev, T, N, P, k, shape, only=None):
    import torch

    from reart_amd.networks.loss import ConnectionTerm, compute_connection_loss
    from reart_amd.utils.chamfer import ChamferDistance

    if shape == "chain":
        edges = [(p, p + 1) for p in range(P - 1)]
    else:
        edges = [(a, b) for a in range(P) for b in range(P) if a != b]
    cano, seg, pc = make_inputs(dev, T, N, P)
    conn = torch.tensor(edges, dtype=torch.int64, device=dev)
    fresh, kept, cd = ConnectionTerm(edges, k=k), ConnectionTerm(edges, k=k), ChamferDistance()
    if only in (None, "operator_kept"):      # a trace of another side sees no launch of this selection
        kept.select(cano, seg)
    return {"operator_select": lambda: torch.autograd.grad(fresh(cano, seg, pc), pc),
            "operator_kept": lambda: torch.autograd.grad(kept(pc), pc),
            "composition": lambda: torch.autograd.grad(compute_connection_loss(cano, seg, conn, pc, cd, k=k), pc)}, len(edges)


def apart(a, b):
    return bool(a["max"] < b["min"] or b["max"] < a["min"])


def measure(fns, args):
    import torch

    g = {k: fn()[0] for k, fn in fns.items()}
    worst = float((g["operator_select"] - g["composition"]).abs().max() / g["composition"].abs().max())
    assert torch.equal(g["operator_select"], g["operator_kept"])
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    ms = {k: [] for k in fns}
    for rep in range(args.reps):
        for k, fn in fns.items():
            ms[k].append(window(fn, args.iters))
        print(f"repeat {rep + 1} of {args.reps}: " + "  ".join(f"{k} {v[-1]:.4f}" for k, v in ms.items()), file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    out = {k: dict(stats(v), unit="ms per forward + backward") for k, v in ms.items()}
    for k in ("operator_select", "operator_kept"):
        out[f"ranges_apart_{k}_composition"] = apart(out[k], out["composition"])
        out[f"composition_over_{k}_median"] = round(out["composition"]["median"] / out[k]["median"], 3)
    out["largest_gradient_difference_of_max"] = float(f"{worst:.2e}")
    return out


def launches(path, calls):
    rows = [r for r in csv.DictReader(open(path)) if int(r["Calls"]) >= calls]
    return round(sum(int(r["Calls"]) for r in rows) / calls, 1), sorted(r["Name"][:80] for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=19)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--parts", type=int, default=20)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--only", choices=SIDES, help="run --calls calls of one side and nothing else")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--shape", choices=("chain", "all_pairs"), default="chain")
    ap.add_argument("--launches", help="kernel statistics (csv) of a trace of --only SIDE --shape NAME --calls N: merge its launches per call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "connection_term_bench.json"))
    args = ap.parse_args()
    if args.launches:
        n, names = launches(args.launches, args.calls)
        out = json.load(open(args.out)) if os.path.exists(args.out) else {}
        kt = out.setdefault("kernel_trace", dict(
            method="rocprofv3 --kernel-trace --stats, one process per side and shape (--only SIDE --shape NAME --calls N); "
                   "kernels dispatched at least N times, divided by N", launches_per_forward_backward={}, kernels={}))
        kt["launches_per_forward_backward"][f"{args.only}_{args.shape}"] = n
        if args.only != "composition":
            kt["kernels"][f"{args.only}_{args.shape}"] = names
        merge(args.out, kernel_trace=kt)
        return
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_connection_term.py needs an MI355X")
    dev = torch.device("cuda:0")
    T, N, P, k = args.frames, args.points, args.parts, args.k
    if args.only:
        fn = sides(dev, T, N, P, k, args.shape, args.only)[0][args.only]
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return
    res = {}
    for shape in ("chain", "all_pairs"):
        fns, E = sides(dev, T, N, P, k, shape)
        res[shape] = dict(measure(fns, args), workload=f"T={T} frames, N={N} points, P={P} parts, E={E} edges, k={k}")
    merge(args.out, device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, reps=args.reps, **res)


if __name__ == "__main__":
    main()
