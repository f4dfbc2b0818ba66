#!/usr/bin/env python3
"""reart_amd.optim.Adam (every parameter of every group in one launch) against torch.optim.Adam, in the places it is offered.

  --part step   the step alone: host wall time per `step()` over --steps steps that end in a synchronise, after --step-warmup,
                for torch.optim.Adam(foreach=True), torch.optim.Adam(foreach=False) and reart_amd.optim.Adam, alternating in one
                process; microseconds, median (min - max) over --reps.  Three sets of tensors: the base model's five in their two
                groups (T = 20, P = 20, H = 128), a kinematic model's three (9 joints, T = 20), ik_single's one (amsgrad).
                The gradients are fixed tensors: a step costs the same whatever they hold.
  --part loop   run_robot.OperatorLoop on the headline workload (base model, synthetic T = 20 x N = 4096, 20 parts, Chamfer +
                flow) with --fused_losses --fused_flow, --adam torch and --adam fused alternating in one process
                (--adam both), iterations per second from device events around --iters iterations after --warmup.
                `--adam torch --tree DIR` times the loop of another checkout (the parent commit) in a process of its own;
                `--merge-parent PATH` adds its figures to --out.
  --part ik     ik_single per novel pose with and without fused_adam, on the model and targets of tools/bench_ik.py (M = 3).
Launches per iteration come from kernel traces taken in runs of their own: `--part loop --adam torch|fused --count K` runs
warm-up + K iterations untimed, e.g. under `rocprofv3 --kernel-trace -f csv -d DIR --`; `--launches TORCH_A TORCH_B FUSED_A
FUSED_B --k K_A K_B` reads four such directories.  Every part merges its figures into --out (default
profiles/fused_adam_bench.json) and prints them as one JSON line.  Without a GPU it fails."""
import argparse
import csv
import functools
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(v, nd):
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


# ------------------------------------------------------------------------------------------------------------------ step
def tensor_sets(dev):
    """name -> (param groups as the loops build them, options)"""
    import torch

    from reart_amd.networks.model import BaseModel

    new = lambda *shape: (0.1 * torch.randn(*shape, device=dev)).requires_grad_(True)
    model = BaseModel(num_parts=20, pose_len=19).to(dev)
    seg = [p for p in model.seg_head.parameters() if p.requires_grad]
    return {"base_model_5_tensors_2_groups": ([{"params": [model.proposal_6d, model.proposal_t], "lr": 1e-2}, {"params": seg, "lr": 1e-3}],
                                              dict(lr=1e-3, weight_decay=0)),
            "kinematic_model_3_tensors": ([{"params": [new(9, 3), new(9, 3), new(19, 9)]}], dict(lr=1e-2, weight_decay=0)),
            "ik_single_1_tensor_amsgrad": ([{"params": [new(1, 9)]}], dict(lr=1e-1, amsgrad=True))}


def part_step(args, dev):
    import torch

    from reart_amd.optim import Adam

    sides = {"torch_foreach": lambda g, o: torch.optim.Adam(g, foreach=True, **o),
             "torch_single_tensor": lambda g, o: torch.optim.Adam(g, foreach=False, **o), "fused": lambda g, o: Adam(g, **o)}
    out = {}
    for name, (groups, options) in tensor_sets(dev).items():
        params = [p for g in groups for p in g["params"]]
        start = [p.detach().clone() for p in params]
        for p in params:
            p.grad = torch.randn_like(p)
        opts = {}
        for side, make in sides.items():          # one optimiser per side on the same tensors: a step costs the same wherever they are
            opts[side] = make([dict(g) for g in groups], options)

        def window(opt, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                opt.step()
            torch.cuda.synchronize()
            return 1e6 * (time.perf_counter() - t0) / n

        for opt in opts.values():
            window(opt, args.step_warmup)
        us = {side: [] for side in opts}
        for _ in range(args.reps):
            for side, opt in opts.items():
                us[side].append(window(opt, args.steps))
        row = {side: dict(stats(v, 2), unit="microseconds of host wall time per step") for side, v in us.items()}
        assert opts["fused"].last_path == "native" and opts["fused"].last_launches == 1
        row["sizes"] = [p.numel() for p in params]
        for other in ("torch_foreach", "torch_single_tensor"):
            row[f"{other}_over_fused_median"] = round(row[other]["median"] / row["fused"]["median"], 2)
            row[f"ranges_apart_from_{other}"] = bool(row["fused"]["max"] < row[other]["min"])
        out[name] = row
        with torch.no_grad():
            for p, s in zip(params, start):
                p.copy_(s)
    merge(args.out, device=torch.cuda.get_device_name(0),
          step_alone=dict(out, steps=args.steps, warmup=args.step_warmup, reps=args.reps,
                          method="host clock around the steps and the synchronise that ends them; the sides alternate in one process"))


# ------------------------------------------------------------------------------------------------------------------ loop
def build_loop(rr, dev, fused_adam, T, N, parts):
    import numpy as np
    import torch

    from reart_amd.networks.model import BaseModel
    from reart_amd.synthetic import make_sequence, split_canonical
    from reart_amd.utils.model_utils import tau_cosine

    seq = make_sequence(T=T, n_parts=8, pts_per_part=N // 8, seed=2, n_ref=3000, with_flow=True)
    cano, pcs = split_canonical(seq["complete"], 2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(dev)
    argv = ["--model", "base", "--use_flow_loss", "--cano_idx", "2", "--num_parts", str(parts), "--fused_losses", "--fused_flow"]
    a = rr.build_parser().parse_args(argv + (["--fused_adam"] if fused_adam else []))
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


def part_loop(args, dev):
    import torch

    from reart_amd import run_robot as rr

    sides = ("torch", "fused") if args.adam == "both" else (args.adam,)
    runners = {s: Runner(build_loop(rr, dev, s == "fused", args.frames, args.points, 20)) for s in sides}
    for r in runners.values():
        r.run(args.warmup)
    if args.count is not None:
        for r in runners.values():
            r.run(args.count)
        torch.cuda.synchronize()
        print(json.dumps({"adam": args.adam, "counted_iterations": args.count}))
        return
    rate = {s: [] for s in sides}
    for _ in range(args.reps):
        for s in sides:
            rate[s].append(runners[s].window(args.iters))
    b = {s: dict(stats(v, 1), unit="iterations/s", last_losses={k: float(x.detach()) for k, x in runners[s].last.items()})
         for s, v in rate.items()}
    if "fused" in runners:
        opt = runners["fused"].loop.optimizer
        b["fused"].update(last_path=opt.last_path, last_launches=opt.last_launches)
    if len(sides) == 2:
        b["ranges_apart"] = bool(b["fused"]["min"] > b["torch"]["max"])
        b["fused_over_torch_median"] = round(b["fused"]["median"] / b["torch"]["median"], 3)
    b.update(workload=f"OperatorLoop --fused_losses --fused_flow, base model, synthetic T={args.frames} x N={args.points}, 20 parts, Chamfer + flow",
             iters=args.iters, warmup=args.warmup, reps=args.reps, tree="this commit" if os.path.abspath(args.tree) == ROOT else "other checkout",
             note="the sides alternate in one process and draw their Gumbel noise from one generator in turn, so their trajectories differ")
    merge(args.out, **{"operator_loop" if len(sides) == 2 else f"operator_loop_{args.adam}_alone": b})


# -------------------------------------------------------------------------------------------------------------------- ik
def part_ik(args, dev):
    import numpy as np
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_ik

    from reart_amd.utils.kinematic_utils import ik_single

    model, cano_pc = bench_ik.demo_model(dev)
    samples = bench_ik.make_samples(model, cano_pc, 3, dev)
    res = {}

    def run(fused):
        res[fused] = np.array([ik_single(model, cano_pc, s, dev, fused_adam=fused)[0] for s in samples])

    for fused in (False, True):
        run(fused)
    ms = {False: [], True: []}
    for _ in range(args.reps):
        for fused in (False, True):
            ms[fused].append(bench_ik.window(lambda: run(fused)) / len(samples))
    c = {"torch": dict(stats(ms[False], 3), unit="ms per pose", mean_err=float(res[False].mean())),
         "fused_adam": dict(stats(ms[True], 3), unit="ms per pose", mean_err=float(res[True].mean()))}
    c["ranges_apart"] = bool(c["fused_adam"]["max"] < c["torch"]["min"])
    c["torch_over_fused_median"] = round(c["torch"]["median"] / c["fused_adam"]["median"], 3)
    c["setting"] = "tools/bench_ik.py: demo model, 14 sparse points, 200 steps, M = 3 poses, device events around work that ends in a copy to the host"
    merge(args.out, ik_single=c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["step", "loop", "ik"], default="step")
    ap.add_argument("--adam", choices=["torch", "fused", "both"], default="both")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--step-warmup", type=int, default=200)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--count", type=int, default=None, help="--part loop, untimed: warm-up + this many iterations of --adam torch|fused (for a trace)")
    ap.add_argument("--launches", nargs=4, metavar="DIR", help="kernel-trace directories: --adam torch K_A, K_B, --adam fused K_A, K_B")
    ap.add_argument("--k", nargs=2, type=int, default=[10, 30], metavar="K", help="the --count of the A and the B traces")
    ap.add_argument("--merge-parent", metavar="PATH", help="add the figures of a `--part loop --adam torch --tree DIR --out PATH` run to --out")
    ap.add_argument("--tree", default=ROOT, help="import reart_amd from this checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_adam_bench.json"))
    args = ap.parse_args()
    if args.merge_parent:
        return merge(args.out, operator_loop_parent_commit=json.load(open(args.merge_parent))["operator_loop_torch_alone"])
    if args.launches:
        n = []
        for d in args.launches:
            files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
            if not files:
                raise SystemExit(f"no kernel trace under {d}")
            n.append(sum(1 for f in files for _ in csv.DictReader(open(f))))
        per = args.k[1] - args.k[0]
        return merge(args.out, launches_per_iteration={"torch": round((n[1] - n[0]) / per, 2), "fused": round((n[3] - n[2]) / per, 2),
                                                       "method": f"kernel-trace rows of {args.k[1]} minus {args.k[0]} iterations, one traced run each"})
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_adam.py needs an MI355X")
    {"step": part_step, "loop": part_loop, "ik": part_ik}[args.part](args, torch.device("cuda:0"))


if __name__ == "__main__":
    main()
