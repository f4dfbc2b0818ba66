#!/usr/bin/env python3
"""GPU timing of the exact assignment above 4096 points per frame (reart_lap_auction_large behind
linear_sum_assignment_batch) against the path those sizes took before it: scipy.optimize.linear_sum_assignment on the host,
one matrix after the other.

Workload: B = 19 matrices (the T - 1 frame pairs of a 20-frame sequence) of n in {4097, 6144, 8192} columns:
cost = cdist(frame t, frame t + 1) of reart_amd.synthetic.make_sequence (8 parts, n points drawn per frame from
8 x ceil(n / 8) by a seeded permutation), passed with their points as compute_ass_err passes them.  n = 4096 through the
path below the limit (race=True, as compute_ass_err calls it) is timed next to it, so that the step at the limit is on record.
Every GPU figure is a device-event time around linear_sum_assignment_batch (which ends with its copy to the host) after a
warm-up of the shape; `--reps` repeats; median, minimum and maximum.  `stats` are the solver's own per-matrix counts of the
last repeat: phases, auction rounds, bids, certificate rounds (minimum and maximum over the batch).
Host reference: wall time of the serial scipy loop on this machine's CPU, once per size, over `--host_b` matrices of the
batch (default 19; 3 at n = 8192, scaled to 19 -- `host_scaled_from` says so), and whether scipy's permutation equals the GPU's.
Writes --out (default profiles/lap_large_bench.json) after every size and prints it as one JSON line at the end.
Usage: python tools/bench_lap_large.py [--reps 5] [--sizes 4097,6144,8192] [--no_host] [--out PATH]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

B = 19


def problems(n, dev, seed=2):
    from reart_amd.synthetic import make_sequence
    from reart_amd.utils.lap import cdist

    per = -(-n // 8)
    seq = make_sequence(T=B + 1, n_parts=8, pts_per_part=per, seed=seed, with_flow=False)
    rng = np.random.default_rng(n)
    frames = np.stack([f[rng.permutation(8 * per)[:n]] for f in seq["complete"]]).astype(np.float32)
    src = torch.from_numpy(frames[:-1]).to(dev).contiguous()
    tgt = torch.from_numpy(frames[1:]).to(dev).contiguous()
    return src, tgt, cdist(src, tgt)


def window(fn):
    """One device-event time (ms) of fn(), which ends in a synchronise."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def spread(ms):
    ms = sorted(ms)
    return dict(median_ms=round(ms[len(ms) // 2], 2), min_ms=round(ms[0], 2), max_ms=round(ms[-1], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="4097,6144,8192")
    ap.add_argument("--host_b", default="4097:19,6144:19,8192:3", help="matrices of the batch the host reference solves, per size")
    ap.add_argument("--no_host", action="store_true", help="GPU figures only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lap_large_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lap_large.py needs an MI355X")

    from scipy.optimize import linear_sum_assignment

    from reart_amd.utils.lap import linear_sum_assignment_batch

    dev = torch.device("cuda:0")
    host_b = {int(k): int(v) for k, v in (kv.split(":") for kv in args.host_b.split(","))}
    out = {"B": B, "reps": args.reps, "device": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)),
           "required_speedup": 5.0, "rows": []}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for n in [4096] + [int(v) for v in args.sizes.split(",")]:
        src, tgt, cost = problems(n, dev)
        res = {}

        def solve():
            res["out"], res["fallbacks"], res["stats"] = linear_sum_assignment_batch(cost, return_stats="full", points=(src, tgt),
                                                                                      race=True)

        solve()                                                   # warm-up of the shape
        ms = [window(solve) for _ in range(args.reps)]
        st = np.asarray(res["stats"])
        st[:, 0] &= 0xffff                                        # (a race reports its winner in the upper half)
        row = dict(n=n, path="reart_lap_auction_race" if n <= 4096 else "reart_lap_auction_large", gpu=spread(ms),
                   fallbacks=int(res["fallbacks"]),
                   stats={k: [int(st[:, i].min()), int(st[:, i].max())] for i, k in enumerate(("phases", "rounds", "bids", "cert_rounds"))})
        print(f"n = {n}: {row['gpu']} fallbacks {row['fallbacks']} {row['stats']}", file=sys.stderr, flush=True)
        if n > 4096 and not args.no_host:
            hb = min(host_b.get(n, B), B)
            same = True
            t0 = time.perf_counter()
            for b in range(hb):
                same &= bool(np.array_equal(linear_sum_assignment(cost[b].cpu().numpy())[1], res["out"][b][1]))
                print(f"  host matrix {b}: {time.perf_counter() - t0:.1f} s so far", file=sys.stderr, flush=True)
            host_s = time.perf_counter() - t0                     # (includes the copy of each matrix from the device, as the parent's path did)
            row["host_scipy_serial_s"] = round(host_s * B / hb, 2)
            row["host_scaled_from"] = hb
            row["host_permutations_equal_gpu"] = same
            row["speedup"] = round(row["host_scipy_serial_s"] * 1e3 / row["gpu"]["median_ms"], 1)
            row["meets_required_speedup"] = bool(row["speedup"] >= out["required_speedup"])
        out["rows"].append(row)
        write()
        del src, tgt, cost, res
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
