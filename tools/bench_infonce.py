#!/usr/bin/env python3
"""Forward + backward to both descriptor sets of the contrastive descriptor loss: networks.loss.DescriptorInfoNCE
(reart_infonce_forward + reart_infonce_backward) against the composition torch.bmm + F.cross_entropy on the same GPU, at the
project's workload, C = 64-D descriptors of N1 = N2 = 4096 points, tau = 0.07, a tenth of the rows unused:

  pairs19   B = 19 frame pairs
  pair1     B = 1
Timing: device events around --iters calls after --warmup, --reps repeats, the sides alternating in one process; median
(min - max), milliseconds per forward + backward.  Peak memory: torch.cuda.max_memory_allocated of one call of each side after
a reset, with the bytes the operands themselves hold beside it.  Accuracy: the worst error / bound per output over the case
table of tests/infonce_ref.py, through the class.  Merges its figures into --out (default profiles/infonce_bench.json) and
prints them as one JSON line.

`--only SIDE --calls N --shape NAME` runs N calls of one side and nothing else: the process a kernel trace is taken of.
`--launches STATS.csv --only SIDE --shape NAME --calls N` reads the kernel statistics of such a trace (rocprofv3 --kernel-trace
--stats) and merges launches per call and the average time per launch of every kernel dispatched at least N times into --out.
Without a GPU it fails."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_flow_term import merge, stats, window  # noqa: E402

SIDES = ("operator", "composition")
SHAPES = {"pairs19": 19, "pair1": 1}


def sides(dev, B, N, C, tau, seed=3):
    import numpy as np
    import torch
    import torch.nn.functional as F

    from reart_amd.networks.loss import DescriptorInfoNCE

    rng = np.random.default_rng(seed)
    unit = lambda a: (a / np.linalg.norm(a, axis=2, keepdims=True)).astype(np.float32)
    f1 = torch.from_numpy(unit(rng.standard_normal((B, N, C)))).to(dev).requires_grad_(True)
    f2 = torch.from_numpy(unit(rng.standard_normal((B, N, C)))).to(dev).requires_grad_(True)
    p = rng.integers(0, N, (B, N))
    p[rng.random((B, N)) < 0.1] = -1
    pos = torch.from_numpy(p.astype(np.int64)).to(dev)
    op = DescriptorInfoNCE(tau=tau)

    def composition():
        logits = torch.bmm(f1, f2.transpose(1, 2)) / tau
        return F.cross_entropy(logits.reshape(-1, N), pos.reshape(-1), ignore_index=-1)

    return {"operator": lambda: torch.autograd.grad(op(f1, f2, pos), (f1, f2)),
            "composition": lambda: torch.autograd.grad(composition(), (f1, f2))}


def apart(a, b):
    return bool(a["max"] < b["min"] or b["max"] < a["min"])


def peak(fn):
    import torch

    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    held = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return dict(max_memory_allocated=int(torch.cuda.max_memory_allocated()), held_before_the_call=int(held))


def measure(fns, args):
    import torch

    g = {k: fn() for k, fn in fns.items()}
    worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(g["operator"], g["composition"]))
    del g
    mem = {k: peak(fn) for k, fn in fns.items()}
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    ms = {k: [] for k in fns}
    for rep in range(args.reps):
        for k, fn in fns.items():
            ms[k].append(window(fn, args.iters))
        print(f"repeat {rep + 1} of {args.reps}: " + "  ".join(f"{k} {v[-1]:.4f}" for k, v in ms.items()), file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    out = {k: dict(stats(v), unit="ms per forward + backward", **mem[k]) for k, v in ms.items()}
    out["ranges_apart"] = apart(out["operator"], out["composition"])
    out["composition_over_operator_median"] = round(out["composition"]["median"] / out["operator"]["median"], 3)
    out["largest_gradient_difference_of_max"] = float(f"{worst:.2e}")
    return out


def accuracy(dev):
    """Worst error / bound per output over the tests' case table."""
    import torch

    sys.path.insert(0, ROOT)
    from reart_amd.networks.loss import DescriptorInfoNCE
    from tests import infonce_ref as nr

    worst = {}
    for c in nr.CASES:
        r = nr.restate(c)
        b = nr.bounds(c, r)
        to = lambda a: torch.from_numpy(a).to(dev)
        f1, f2 = to(c["f1"]).requires_grad_(True), to(c["f2"]).requires_grad_(True)
        op = DescriptorInfoNCE(tau=c["tau"])
        loss = op(f1, f2, to(c["pos"]), None if c["mask"] is None else to(c["mask"]))
        loss.backward()
        out = dict(loss=loss.item(), row_loss=op.last[0].cpu().numpy(), dF1=f1.grad.cpu().numpy(), dF2=f2.grad.cpu().numpy(),
                   top=op.last[1].cpu().numpy(), count=int(op.last[2]))
        for k, v in nr.worst(out, r, b).items():
            worst[k] = max(worst.get(k, 0), v)
    return {k: (v if isinstance(v, int) else float(f"{v:.3g}")) for k, v in worst.items()}


def launches(path, calls):
    rows = [r for r in csv.DictReader(open(path)) if int(r["Calls"]) >= calls]
    per = {r["Name"][:80]: dict(launches_per_call=round(int(r["Calls"]) / calls, 2), average_us=round(float(r["AverageNs"]) / 1e3, 2)) for r in rows}
    return round(sum(int(r["Calls"]) for r in rows) / calls, 1), per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--tau", type=float, default=0.07)
    ap.add_argument("--only", choices=SIDES, help="run --calls calls of one side and nothing else")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--shape", choices=tuple(SHAPES), default="pairs19")
    ap.add_argument("--launches", help="kernel statistics (csv) of a trace of --only SIDE --shape NAME --calls N")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infonce_bench.json"))
    args = ap.parse_args()
    if args.launches:
        n, per = launches(args.launches, args.calls)
        out = json.load(open(args.out)) if os.path.exists(args.out) else {}
        kt = out.setdefault("kernel_trace", dict(
            method="rocprofv3 --kernel-trace --stats, one process per side and shape (--only SIDE --shape NAME --calls N); "
                   "kernels dispatched at least N times", launches_per_forward_backward={}, kernels={}))
        kt["launches_per_forward_backward"][f"{args.only}_{args.shape}"] = n
        if args.only == "operator":
            kt["kernels"][f"{args.only}_{args.shape}"] = per
        merge(args.out, kernel_trace=kt)
        return
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_infonce.py needs an MI355X")
    dev = torch.device("cuda:0")
    N, C = args.points, args.channels
    if args.only:
        fn = sides(dev, SHAPES[args.shape], N, C, args.tau)[args.only]
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return
    res = {"worst_error_over_bound": accuracy(dev)}
    for shape, B in SHAPES.items():
        res[shape] = dict(measure(sides(dev, B, N, C, args.tau), args), workload=f"B={B}, N1=N2={N}, C={C}, tau={args.tau}, 10 % of the rows unused")
        torch.cuda.empty_cache()
    merge(args.out, device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, reps=args.reps, **res)


if __name__ == "__main__":
    main()
