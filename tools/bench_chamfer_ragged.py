#!/usr/bin/env python3
"""The warm Chamfer loss on clouds of differing lengths in one batch (utils.chamfer.ChamferLoss with x_lengths / y_lengths:
reart_chamfer_loss_ragged) against what a caller had before, on N = 19 elements padded to P1 = P2 = 4096 points: value and
gradient for x, x drifting a little every call (a fixed cycle of perturbed copies) against a fixed y.

  (a) ragged_lengths   lengths drawn once, uniform in [1024, 4096] (seeded), for x and for y:
        ragged         ChamferLoss(x, y, x_lengths, y_lengths): one warm call
        composition    two knn_points with lengths, the sums, autograd (the cold path)
        trimmed        19 dense ChamferLoss calls on the trimmed clouds, a module each
  (b) full_lengths     all lengths 4096: the ragged entry against the dense entry (the price of the staging launch)
  (c) dense_vs_parent  the dense entry of this tree against another tree's (--parent DIR, a built checkout of the parent
                       commit): a process per tree and window, the trees alternating

Timing: device events around --iters calls after --warmup, --reps repeats, the sides alternating; median (min - max)
milliseconds per call into --out (default profiles/chamfer_ragged_bench.json), printed as JSON lines.  Launches per call are
counted from the entries' sources (include/reart_hip.h), not traced.  Without a GPU it fails."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N, P = 19, 4096


def stats(v, nd=4):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], nd), min=round(v[0], nd), max=round(v[-1], nd))


def apart(a, b):
    return bool(a["max"] < b["min"] or b["max"] < a["min"])


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


def clouds(dev):
    """(8 perturbed copies of x [N,P,3], y [N,P,3]) of the synthetic sequence the other operator benchmarks use."""
    import numpy as np
    import torch

    from reart_amd.synthetic import make_sequence

    frames = make_sequence(T=N + 1, n_parts=8, pts_per_part=P // 8, seed=2, with_flow=False)["complete"].astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x0, y = t(frames[:-1]), t(frames[1:])
    gen = torch.Generator(device=dev).manual_seed(3)
    return [x0 + 1e-3 * torch.randn(x0.shape, device=dev, generator=gen) for _ in range(8)], y


def dense_side(dev):
    import torch

    from reart_amd.utils.chamfer import ChamferLoss

    xs, y = clouds(dev)
    xs = [x.requires_grad_(True) for x in xs]
    mod, state = ChamferLoss(), {"i": 0}

    def dense():
        x = xs[state["i"] % len(xs)]
        state["i"] += 1
        return torch.autograd.grad(mod(x, y), x)
    return dense


def sides(dev, lx, ly, which):
    import torch

    from reart_amd.utils.chamfer import ChamferLoss, knn_points

    xs, y = clouds(dev)
    state = {"i": 0}
    fns = {}
    leaves = [x.clone().requires_grad_(True) for x in xs]
    tlx, tly = torch.tensor(lx, device=dev), torch.tensor(ly, device=dev)

    def pick(seq):
        v = seq[state["i"] % len(seq)]
        state["i"] += 1
        return v

    if "ragged" in which:
        ragged_mod = ChamferLoss()

        def ragged():
            x = pick(leaves)
            return torch.autograd.grad(ragged_mod(x, y, x_lengths=tlx, y_lengths=tly), x)
        fns["ragged"] = ragged
    if "dense" in which:
        dense_mod = ChamferLoss()

        def dense():
            x = pick(leaves)
            return torch.autograd.grad(dense_mod(x, y), x)
        fns["dense"] = dense
    if "composition" in which:
        def composition():
            x = pick(leaves)
            loss = knn_points(x, y, tlx, tly, K=1).dists.sum() + knn_points(y, x, tly, tlx, K=1).dists.sum()
            return torch.autograd.grad(loss, x)
        fns["composition"] = composition
    if "trimmed" in which:
        mods = [ChamferLoss() for _ in range(N)]
        cut = [[x[n:n + 1, :lx[n]].clone().requires_grad_(True) for n in range(N)] for x in xs]
        ycut = [y[n:n + 1, :ly[n]].clone() for n in range(N)]

        def trimmed():
            parts = pick(cut)
            return [torch.autograd.grad(mods[n](parts[n], ycut[n]), parts[n]) for n in range(N)]
        fns["trimmed"] = trimmed
    return fns


def measure(fns, args):
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    ms = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            ms[k].append(window(fn, args.iters))
    return {k: dict(stats(v), unit="ms per value + gradient") for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="(c) only: a built checkout of the parent commit")
    ap.add_argument("--root", default=None, help="child of (c): the tree to import reart_amd from; prints one window's ms")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chamfer_ragged_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else ROOT)
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_chamfer_ragged.py needs an MI355X")
    dev = torch.device("cuda:0")
    if args.root:                                # one window of the dense entry of that tree
        fn = dense_side(dev)
        for _ in range(args.warmup):
            fn()
        print(json.dumps({"ms": window(fn, args.iters)}))
        return
    common = dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, reps=args.reps,
                  workload=f"synthetic N={N} x P1=P2={P}, bidirectional Chamfer sum, value + gradient for x, x drifting against fixed y")
    if args.parent:
        ms = {"this_tree": [], "parent": []}
        for _ in range(args.reps):
            for k, root in (("this_tree", ROOT), ("parent", args.parent)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--iters", str(args.iters),
                                      "--warmup", str(args.warmup)], check=True, capture_output=True, text=True).stdout
                ms[k].append(json.loads(out.strip().splitlines()[-1])["ms"])
        c = {k: dict(stats(v), unit="ms per value + gradient") for k, v in ms.items()}
        c["ranges_apart"] = apart(c["this_tree"], c["parent"])
        c["this_over_parent_median"] = round(c["this_tree"]["median"] / c["parent"]["median"], 3)
        c["regression"] = bool(c["ranges_apart"] and c["this_tree"]["median"] > c["parent"]["median"])
        return merge(args.out, dense_vs_parent=c, **common)
    rng = np.random.default_rng(7)
    lx, ly = [int(v) for v in rng.integers(1024, P + 1, N)], [int(v) for v in rng.integers(1024, P + 1, N)]
    a = measure(sides(dev, lx, ly, ("ragged", "composition", "trimmed")), args)
    a["x_lengths"], a["y_lengths"] = lx, ly
    for other in ("composition", "trimmed"):
        a[f"ranges_apart_ragged_{other}"] = apart(a["ragged"], a[other])
        a[f"{other}_over_ragged_median"] = round(a[other]["median"] / a["ragged"]["median"], 3)
    # counted from the sources, not traced: the ragged entry is the dense entry's launches (x's image, x's boxes, the search,
    # the consumer when y is unchanged, + one 4-byte memset) and ONE staging launch in front; `trimmed` is N dense calls
    a["native_launches_per_call"] = {"ragged": "dense + 1 (5 with y unchanged)", "dense": 4, "trimmed": 4 * N}
    b = measure(sides(dev, [P] * N, [P] * N, ("ragged", "dense")), args)
    b["ranges_apart"] = apart(b["ragged"], b["dense"])
    b["ragged_over_dense_median"] = round(b["ragged"]["median"] / b["dense"]["median"], 3)
    merge(args.out, ragged_lengths=a, full_lengths=b, **common)


if __name__ == "__main__":
    main()
