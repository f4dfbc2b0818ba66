#!/usr/bin/env python3
"""The flow term as one operator (utils.flow_utils.FlowTerm, reart_flow_term) against what it replaces, on the headline shape
(synthetic T = 20 frames x N = 4096 points, 3000 reference points per frame pair).

  --part a   the operator alone against the composition (cat, blend_anchor_motion_batch, cat, subtraction, flow_loss, multiply,
             and autograd back to pc_trans): value and gradient of one iteration, milliseconds.  The clouds move a little every
             iteration (a fixed cycle of perturbed copies), as in a run.
  --part b   OperatorLoop --fused_losses --fused_flow (base model, 20 parts, Chamfer + flow) with FlowTerm against the same loop with the
             composition in its place, iterations per second.
  --part c   KinematicEngine.iteration with warm_flow on and off on the workload of `bench.py --config kinematic` (a relaxation
             result projected with --use_assign_loss --assign_iter 0 --downsample 2 --assign_gap 1), iterations per second.
Timing: device events around --iters iterations after --warmup, --reps repeats, the two sides alternating in one process;
median (min - max).  Each part merges its figures into --out (default profiles/flow_term_bench.json) and prints them as one JSON
line.  Part (b), the flagged loop against the parent commit's, is tools/bench_operator_loop.py --mode fused on both trees
(--tree), a process each; `--merge-loop THIS.json PARENT.json [...]` copies the results into --out, `--loop-launches` the
launches per iteration of both loops from kernel traces of `bench_operator_loop.py --mode fused --count K` with two different K.

Kernel times and launches per iteration come from traces taken in runs of their own (tracing slows the host):
`--count K --side operator|composition` runs warm-up + K iterations of ONE side of part (a) untimed, e.g. under
`rocprofv3 --kernel-trace --stats -f csv -d DIR --`; with `--tree DIR` the composition is the one of the checkout in DIR.
`--kernel-stats LABEL=DIR ... --k K` reads such directories, writes profiles/flow_term_kernel_stats.csv (per kernel: calls and
average / minimum / maximum nanoseconds) and adds, per label, launches per iteration and the kernel time per iteration, summed
over the kernels that run in every iteration (the library's own, and all of them with ATen's), to --out.
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


# ---------------------------------------------------------------------------------------------------------------- part a
def operator_sides(dev, T, N, cano_idx, sides):
    import numpy as np
    import torch

    from reart_amd.knn_cuda import KNN
    from reart_amd.networks.loss import flow_loss
    from reart_amd.synthetic import make_sequence, split_canonical
    from reart_amd.utils import flow_utils as fu

    seq = make_sequence(T=T, n_parts=8, pts_per_part=N // 8, seed=2, n_ref=3000, with_flow=True)
    cano, pcs = split_canonical(seq["complete"], cano_idx)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(dev)
    cano, pcs = t(cano), t(pcs)
    refs, flows = [t(r) for r in seq["ref_loc"]], [t(f) for f in seq["ref_flow"]]
    gen = torch.Generator(device=dev).manual_seed(3)
    clouds = [(pcs + 1e-3 * torch.randn(pcs.shape, device=dev, generator=gen)).requires_grad_(True) for _ in range(8)]
    state = {"i": 0}
    fns = {}
    if "operator" in sides:
        term = fu.FlowTerm(refs, flows, cano_idx)

        def operator():
            x = clouds[state["i"] % len(clouds)]
            state["i"] += 1
            return torch.autograd.grad(term(x, cano), x)
        fns["operator"] = operator
    if "composition" in sides:
        ref_batch, knn, c = fu.pad_reference_sets(refs, flows), KNN(k=3, transpose_mode=True), cano_idx

        def composition():
            x = clouds[state["i"] % len(clouds)]
            state["i"] += 1
            with torch.no_grad():
                comp = torch.cat((x[:c], cano[None], x[c:]), dim=0)
                gt, mask = fu.blend_anchor_motion_batch(comp[:-1], *ref_batch, knn, return_mask=True)
            comp = torch.cat((x[:c], cano[None], x[c:]), dim=0)
            return torch.autograd.grad(1.0 * flow_loss(gt, comp[1:] - comp[:-1], flow_mask_list=mask), x)
        fns["composition"] = composition
    return fns


def part_a(args, dev):
    import torch

    fns = operator_sides(dev, args.frames, args.points, 2, ("operator", "composition") if args.count is None else (args.side,))
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    if args.count is not None:
        for _ in range(args.count):
            fns[args.side]()
        torch.cuda.synchronize()
        print(json.dumps({"side": args.side, "counted_iterations": args.count}))
        return
    ms = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            ms[k].append(window(fn, args.iters))
    a = {k: dict(stats(v), unit="ms per value + gradient") for k, v in ms.items()}
    a["ranges_apart"] = bool(a["operator"]["max"] < a["composition"]["min"])
    a["composition_over_operator_median"] = round(a["composition"]["median"] / a["operator"]["median"], 3)
    merge(args.out, workload=f"synthetic T={args.frames} x N={args.points}, 3000 reference points per pair", device=torch.cuda.get_device_name(0),
          iters=args.iters, warmup=args.warmup, reps=args.reps, a_operator_alone=a)


# ---------------------------------------------------------------------------------------------------------------- part b
def part_b(args, dev):
    """The flagged loop with FlowTerm against the same loop with the composition in its place (``flow_term = None``: the
    launches of the parent commit's flagged loop), alternating in one process."""
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_operator_loop as bol
    from reart_amd import run_robot as rr
    from reart_amd.utils.flow_utils import FlowTerm

    runners = {}
    for name in ("composition", "flow_term"):
        loop = bol.build_loop(rr, dev, True, args.frames, args.points, 20)       # --fused_losses; --fused_flow is set here
        loop.flow_term = None if name == "composition" else FlowTerm(loop.pc_ref_list, loop.flow_ref_list, loop.args.cano_idx,
                                                                      weight=loop.args.lambda_flow, robust=loop.args.use_robust_loss)
        runners[name] = bol.Runner(loop)
    for r in runners.values():
        r.run(args.warmup)
    rate = {k: [] for k in runners}
    for _ in range(args.reps):
        for k, r in runners.items():
            rate[k].append(r.window(args.iters))
    b = {k: dict(stats(v, 1), unit="iterations/s") for k, v in rate.items()}
    b["ranges_apart"] = bool(b["flow_term"]["min"] > b["composition"]["max"])
    b["flow_term_over_composition_median"] = round(b["flow_term"]["median"] / b["composition"]["median"], 3)
    merge(args.out, b_operator_loop_one_process=b)


# ---------------------------------------------------------------------------------------------------------------- part c
def part_c(args, dev):
    import contextlib
    import copy

    import numpy as np
    import torch

    import bench
    from reart_amd import run_robot as rr
    from reart_amd import tail
    from reart_amd.kinematic_engine import KinematicEngine

    T, N = args.frames, args.points
    cano_idx = T // 2
    eng, seq, model = bench.build_instance(dev, T, N, cano_idx, seed=2, use_flow=True)
    eng.capture(steps_per_graph=50)
    eng.step(args.base_iters)
    torch.cuda.synchronize()
    cano, pcs = eng.caller_clouds()
    with torch.no_grad():
        _, seg0, trans0 = model(cano)
    seg_s, trans_s, conn_s = tail.extract_structure(seg0, trans0, cano)
    result = {"pred_cano_part": seg_s.cpu().numpy(), "pred_pose_list": trans_s.cpu().numpy(),
              "joint_connection": conn_s.cpu().numpy().tolist(), "cano_idx": cano_idx}
    a = rr.build_parser().parse_args(["--model", "kinematic", "--use_flow_loss", "--use_assign_loss", "--assign_iter", "0", "--downsample", "2",
                                      "--assign_gap", "1", "--cano_idx", str(cano_idx), "--n_iter", "15000"])
    with contextlib.redirect_stdout(sys.stderr):
        kin = rr.build_kinematic_from_base(result, cano, pcs, a).to(dev)
    t_ = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    refs, flows = [t_(r) for r in seq["ref_loc"]], [t_(f) for f in seq["ref_flow"]]
    loops, its = {}, {}
    for name, warm in (("warm_flow_off", False), ("warm_flow_on", True)):
        loops[name] = KinematicEngine(copy.deepcopy(kin), cano, pcs, a.cano_idx, refs, flows, trans_lr=a.trans_lr, weight_decay=a.weight_decay,
                                      assign_iter=a.assign_iter, assign_gap=a.assign_gap, downsample=a.downsample,
                                      lambda_assign=a.lambda_assign, lambda_flow=a.lambda_flow, use_robust_loss=a.use_robust_loss,
                                      use_assign_loss=a.use_assign_loss, warm_flow=warm)
        its[name] = 0

    def step(name):
        loops[name].iteration(its[name])
        its[name] += 1
    for name in loops:
        for _ in range(args.warmup):
            step(name)
    rate = {k: [] for k in loops}
    for _ in range(args.reps):
        for name in loops:
            rate[name].append(1e3 / window(lambda: step(name), args.iters))
    c = {k: dict(stats(v, 1), unit="iterations/s") for k, v in rate.items()}
    c["ranges_apart"] = bool(c["warm_flow_on"]["min"] > c["warm_flow_off"]["max"])
    c["on_over_off_median"] = round(c["warm_flow_on"]["median"] / c["warm_flow_off"]["median"], 3)
    c["last_losses"] = {k: {n: float(v) for n, v in loops[k].losses.items()} for k in loops}
    c["lap_fallbacks"] = {k: int(loops[k].lap_fallbacks) for k in loops}
    merge(args.out, c_kinematic_engine=c)


# ---------------------------------------------------------------------------------------------------------------- traces
def kernel_stats(args):
    rows, summary = [], {}
    for item in args.kernel_stats:
        label, d = item.split("=", 1)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit(f"no kernel stats under {d}")
        launches, own, every = 0, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        for r in csv.DictReader(open(files[0])):
            calls = int(r["Calls"])
            rows.append([label, r["Name"], calls, r["AverageNs"], r["MinNs"], r["MaxNs"]])
            launches += calls
            if calls >= args.k:                 # runs in every iteration of the trace (its warm-up iterations are traced too)
                for acc in (every,) + ((own,) if "at::" not in r["Name"] else ()):      # own: the library's kernels, not ATen's
                    for j, col in enumerate(("AverageNs", "MinNs", "MaxNs")):
                        acc[j] += calls / args.k * float(r[col]) / 1e3
        summary[label] = {"launches_per_iteration": round(launches / args.k, 2), "traced_iterations": args.k,
                          "library_kernels_us_per_iteration": dict(zip(("sum_of_averages", "sum_of_minima", "sum_of_maxima"), (round(v, 1) for v in own))),
                          "all_kernels_us_per_iteration": dict(zip(("sum_of_averages", "sum_of_minima", "sum_of_maxima"), (round(v, 1) for v in every)))}
    with open(args.stats_out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Run", "Name", "Calls", "AverageNs", "MinNs", "MaxNs"])
        w.writerows(rows)
    merge(args.out, kernels=summary)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b", "c"], default="a")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--base-iters", type=int, default=2000, help="part c: iterations of the relaxation the projection starts from")
    ap.add_argument("--count", type=int, default=None, help="untimed: warm-up + this many iterations of --side (for a trace)")
    ap.add_argument("--side", choices=["operator", "composition"], default="operator")
    ap.add_argument("--tree", default=ROOT, help="import reart_amd from this checkout")
    ap.add_argument("--kernel-stats", nargs="+", metavar="LABEL=DIR")
    ap.add_argument("--k", type=int, default=100, help="iterations of the traced runs (their --warmup + --count)")
    ap.add_argument("--merge-loop", nargs="+", metavar="JSON",
                    help="bench_operator_loop.py --mode fused results, one process each: this tree, the parent's[, this tree, the parent's ...]")
    ap.add_argument("--loop-launches", nargs=4, metavar="DIR",
                    help="kernel-trace directories of bench_operator_loop.py --mode fused --count K: this tree K_A, K_B, the parent's K_A, K_B")
    ap.add_argument("--lk", nargs=2, type=int, default=[10, 30], metavar="K", help="the --count of the A and the B loop traces")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_term_bench.json"))
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "flow_term_kernel_stats.csv"))
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args)
    if args.merge_loop:
        keys = ("median_it_s", "min_it_s", "max_it_s")
        runs = [{k: json.load(open(p))["fused_losses"][k] for k in keys} for p in args.merge_loop]
        this, parent = runs[0::2], runs[1::2]        # processes in the order they ran: this tree, the parent's, this tree, ...
        b = {"this_commit": this, "parent_commit": parent,
             "ranges_apart": bool(min(r["min_it_s"] for r in this) > max(r["max_it_s"] for r in parent)),
             "this_over_parent_median": [round(a["median_it_s"] / b_["median_it_s"], 3) for a, b_ in zip(this, parent)]}
        if os.path.exists(args.out) and "b_operator_loop_fused" in json.load(open(args.out)):
            b["launches_per_iteration"] = json.load(open(args.out))["b_operator_loop_fused"].get("launches_per_iteration")
        return merge(args.out, b_operator_loop_fused=b)
    if args.loop_launches:
        n = []
        for d in args.loop_launches:
            files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
            if not files:
                raise SystemExit(f"no kernel trace under {d}")
            n.append(sum(1 for f in files for _ in csv.DictReader(open(f))))
        per = args.lk[1] - args.lk[0]
        out = json.load(open(args.out)) if os.path.exists(args.out) else {}
        b = out.get("b_operator_loop_fused", {})
        b["launches_per_iteration"] = {"this_commit": round((n[1] - n[0]) / per, 2), "parent_commit": round((n[3] - n[2]) / per, 2),
                                       "method": f"kernel-trace rows of {args.lk[1]} minus {args.lk[0]} iterations, one traced run each"}
        return merge(args.out, b_operator_loop_fused=b)
    sys.path.insert(0, os.path.abspath(args.tree))
    sys.path.insert(1, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_flow_term.py needs an MI355X")
    dev = torch.device("cuda:0")
    {"a": part_a, "b": part_b, "c": part_c}[args.part](args, dev)


if __name__ == "__main__":
    main()
