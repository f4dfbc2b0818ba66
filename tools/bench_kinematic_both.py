#!/usr/bin/env python3
"""The kinematic projection with the Chamfer loss in every iteration (`--recon_with_assign`): KinematicEngine's
recon_with_assign mode (`--fused_recon`) against the operator loop that computes the same objective.

Workload: that of `bench.py --config kinematic`, built the same way (bench.build_instance, --base-iters relaxation iterations,
tail.extract_structure, run_robot.build_kinematic_from_base): synthetic T = 20 x N = 4096, flow on, --assign_iter 0; at
`--downsample 2 --assign_gap 1` (README.md:125) and at `--downsample 4 --assign_gap 5`.
Sides, alternating in one process, each on its own copy of the kinematic model:
  a  the engine in the new mode                      (--model kinematic --recon_with_assign --fused_recon)
  b  OperatorLoop                                    (--model kinematic --recon_with_assign)
  c  the same loop with --fused_losses --fused_flow --fused_adam
  d  the engine without the Chamfer term, for scale  (--model kinematic)
Method: --reps windows of --iters iterations after --warmup, device events around every window; median (min - max) in
iterations per second, the ratios a/b and a/c at the medians and whether the ranges are apart.
Kernel times (eager, between events, --kernel-calls calls each): reart_kin_post_recon and reart_kin_post without their flow
branch (the consumer launch + the loss launch), and the Chamfer term (reart_gather_points + reart_chamfer_loss, warm).
Launches per iteration: `--count K --side a|b` runs warm-up + K iterations of one side untimed, for a kernel trace taken in a run
of its own; `--launches A_K0 A_K1 B_K0 B_K1 --k K0 K1` reads four trace directories and adds the figures to --out.
Writes --out (default profiles/kinematic_both_bench.json) and prints it as one JSON line.  Without a GPU it fails."""
import argparse
import contextlib
import copy
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDES = {"a": ["--recon_with_assign", "--fused_recon"], "b": ["--recon_with_assign"],
         "c": ["--recon_with_assign", "--fused_losses", "--fused_flow", "--fused_adam"], "d": []}
NAMES = {"a": "engine_recon_with_assign", "b": "operator_loop", "c": "operator_loop_fused_losses_flow_adam", "d": "engine_default_mode"}


def workload(dev, T, N, base_iters):
    import numpy as np
    import torch

    import bench
    from reart_amd import tail

    cano_idx = T // 2
    eng, seq, model = bench.build_instance(dev, T, N, cano_idx, seed=2, use_flow=True)
    eng.capture(steps_per_graph=50)
    eng.step(base_iters)
    torch.cuda.synchronize()
    cano, pcs = eng.caller_clouds()
    with torch.no_grad():
        _, seg0, trans0 = model(cano)
    seg_s, trans_s, conn_s = tail.extract_structure(seg0, trans0, cano)
    result = {"pred_cano_part": seg_s.cpu().numpy(), "pred_pose_list": trans_s.cpu().numpy(),
              "joint_connection": conn_s.cpu().numpy().tolist(), "cano_idx": cano_idx}
    t_ = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return cano_idx, cano, pcs, result, [t_(r) for r in seq["ref_loc"]], [t_(f) for f in seq["ref_flow"]]


def make_side(rr, dev, side, wl, downsample, gap):
    cano_idx, cano, pcs, result, refs, flows = wl
    a = rr.build_parser().parse_args(["--model", "kinematic", "--use_flow_loss", "--use_assign_loss", "--assign_iter", "0", "--downsample",
                                      str(downsample), "--assign_gap", str(gap), "--cano_idx", str(cano_idx), "--n_iter", "15000"] + SIDES[side])
    with contextlib.redirect_stdout(sys.stderr):
        kin = rr.build_kinematic_from_base(copy.deepcopy(result), cano, pcs, a).to(dev)
    return rr.make_projection_loop(a, kin, cano, pcs, refs, flows)


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


def apart(x, y):
    return bool(x["min_it_s"] > y["max_it_s"] or x["max_it_s"] < y["min_it_s"])


def timed_us(fn, calls):
    import torch

    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(1e3 * e0.elapsed_time(e1) / calls, 2)


def kernel_times(eng, calls):
    """On the buffers of a recon_with_assign engine that has run: the two entries without references (two launches each)."""
    from reart_amd import _lib

    L, p = _lib.lib(), _lib.ptr
    n = int(eng.src_idx.numel())
    head = (p(eng.pc_trans), p(eng.cano), eng.B, eng.N, eng.cano_idx, p(eng._pc_src), p(eng.tgt_pts), p(eng.lap_state["cols"]), p(eng._slot), n,
            eng.lambda_assign, None, None, None, 0, 3, eng.euclid, eng.lambda_flow, int(eng.robust), eng.smooth)
    tail = (p(eng.G), p(eng._matched_buf), p(eng._loss4), p(eng._post_ws), eng._post_ws.numel())

    def recon():
        _lib.check(L.reart_kin_post_recon(*head, p(eng._g_recon), p(eng._inv_x), p(eng._loss_recon), *tail, _lib.stream()), "reart_kin_post_recon")

    def plain():
        _lib.check(L.reart_kin_post(*head, *tail, _lib.stream()), "reart_kin_post")

    return {"consumer_with_chamfer_input_us": timed_us(recon, calls), "consumer_without_chamfer_input_us": timed_us(plain, calls),
            "chamfer_term_gather_plus_call_us": timed_us(eng._recon_term, calls),
            "method": f"{calls} eager calls between two device events, host launch time included; the consumer entries without their "
                      "flow branch: kin_grad + kin_loss launch"}


def trace_rows(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {d}")
    return sum(1 for f in files for _ in csv.DictReader(open(f)))


def write(out, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--base-iters", type=int, default=2000)
    ap.add_argument("--kernel-calls", type=int, default=200)
    ap.add_argument("--configs", default="2:1,4:5", help="downsample:assign_gap pairs")
    ap.add_argument("--count", type=int, default=None, help="untimed: warm-up + this many iterations of --side (for a trace)")
    ap.add_argument("--side", default="a", choices=sorted(SIDES))
    ap.add_argument("--launches", nargs=4, metavar="DIR", help="trace directories: side a K0, a K1, side b K0, b K1")
    ap.add_argument("--k", nargs=2, type=int, default=[10, 30], metavar="K")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kinematic_both_bench.json"))
    args = ap.parse_args()

    if args.launches:
        out = json.load(open(args.out))
        n = [trace_rows(d) for d in args.launches]
        per = args.k[1] - args.k[0]
        out["launches_per_iteration"] = {NAMES["a"]: round((n[1] - n[0]) / per, 2), NAMES["b"]: round((n[3] - n[2]) / per, 2),
                                         "method": f"kernel-trace rows of {args.k[1]} minus {args.k[0]} iterations, one traced run each, "
                                                   "downsample 2, assign_gap 1 (a graph replay counts its kernels)"}
        return write(out, args.out)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_kinematic_both.py needs an MI355X")
    from reart_amd import run_robot as rr

    dev = torch.device("cuda:0")
    wl = workload(dev, args.frames, args.points, args.base_iters)
    configs = [tuple(int(v) for v in c.split(":")) for c in args.configs.split(",")]
    if args.count is not None:
        r = Runner(make_side(rr, dev, args.side, wl, *configs[0]))
        r.run(args.warmup + args.count)
        torch.cuda.synchronize()
        print(json.dumps({"side": args.side, "counted_iterations": args.count}))
        return
    out = {"workload": f"kinematic projection, synthetic T={args.frames} x N={args.points}, flow on, --assign_iter 0, "
                       f"{args.base_iters} relaxation iterations before it (bench.py --config kinematic's construction)",
           "iters": args.iters, "warmup": args.warmup, "reps": args.reps, "device": torch.cuda.get_device_name(0), "sides": NAMES,
           "note": "the sides alternate in one process, each on its own copy of the model: their trajectories differ by rounding"}
    for ds, gap in configs:
        runners = {s: Runner(make_side(rr, dev, s, wl, ds, gap)) for s in SIDES}
        for r in runners.values():
            r.run(args.warmup)
        rates = {s: [] for s in SIDES}
        for _ in range(args.reps):
            for s in SIDES:
                rates[s].append(runners[s].window(args.iters))
        res = {NAMES[s]: stats(rates[s]) for s in SIDES}
        for s in SIDES:
            res[NAMES[s]]["last_losses"] = {k: float(v.detach()) for k, v in runners[s].last.items()}
            res[NAMES[s]]["lap_solves"] = int(runners[s].loop.lap_solves)
            res[NAMES[s]]["lap_fallbacks"] = int(runners[s].loop.lap_fallbacks)
        a, b, c = res[NAMES["a"]], res[NAMES["b"]], res[NAMES["c"]]
        res["a_over_b_median"] = round(a["median_it_s"] / b["median_it_s"], 3)
        res["a_over_c_median"] = round(a["median_it_s"] / c["median_it_s"], 3)
        res["a_b_ranges_apart"], res["a_c_ranges_apart"] = apart(a, b), apart(a, c)
        res["kernel_times"] = kernel_times(runners["a"].loop, args.kernel_calls)
        out[f"downsample_{ds}_assign_gap_{gap}"] = res
        del runners
    write(out, args.out)


if __name__ == "__main__":
    main()
