#!/usr/bin/env python3
"""GPU timing of the warm assignment re-solve above 4096 points per frame (reart_lap_resolve_large behind
linear_sum_assignment_points) against the path those sizes took before it: a cold reart_lap_auction_large at every refresh.

Workload: the B = 19 problems of tools/bench_lap_large.py (`problems()`) at n in {4097, 6144, 8192} as step 0, solved cold into a
state; then, for sigma in {1e-4, 1e-3, 1e-2}, a sequence of `--steps` (8) re-solves in which every source point moves by
N(0, sigma) per step (1e-3 is the order one Adam step moves the kinematic projection's costs), and one JUMP: the source frames
replaced by unrelated ones (the batch rolled by seven frames, the points of every frame permuted).
Timing: per step a device-event time around linear_sum_assignment_points (cdist, the solve and the copy of its flags and
columns to the host) after a warm-up of the shape; in the same process and alternating with it, the cold solve of the same
points (cdist + linear_sum_assignment_batch without a state: the parent's path).  `--reps` (5) repeats of every sequence, each
from a copy of the state step 0 left; median, minimum and maximum over all steps of all repeats.  Also recorded per sigma:
the re-solve's own per-matrix counts (released rows, rows left for the searches, search steps, certificate rounds, row-reduction
steps; minimum and maximum over batch, steps and repeats), matrices solved cold after a warm attempt, host fallbacks, and
whether every permutation equals the cold solve's (where one differs: whether the two exact totals of the fp32 entries differ
too -- equal totals are a tie between optima, unequal ones would be an error).
Step limit: before anything is timed, every size's jump is run through the C entry alone with `--probe_steps_per_n` x n steps
allowed (every matrix is given up there, most of its steps are search steps, as in a real jump); its device time over the
steps taken is the time of one sequential step, and the median of `--reps` cold solves of step 0 over that is the number of
steps that cost one cold solve (`max_steps.multiple_of_n`).  The smallest multiple over the sizes, rounded down, is what
LAP_LARGE_STEPS_PER_N (csrc/lap.hip) is set from, and the timed runs below use exactly that limit (`max_steps_in_effect`,
set through reart_amd.utils.lap.RESOLVE_LARGE_MAX_STEPS), whatever the library was built with.
Routing: `routed_warm` of a size is true when the sigma = 1e-3 median is below the cold median and their minimum-maximum
ranges do not overlap.
Writes --out (default profiles/lap_resolve_large_bench.json) after every size and prints it as one JSON line at the end.
Usage: python tools/bench_lap_resolve_large.py [--reps 5] [--steps 8] [--sizes 4097,6144,8192] [--out PATH]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.bench_lap_large import B, problems, spread, window  # noqa: E402

SIGMAS = (1e-4, 1e-3, 1e-2)
STAT_NAMES = ("released", "left_for_searches", "search_steps", "cert_rounds", "reduction_steps")


def split_stats(st):
    """[B,4] words of reart_lap_resolve's layout -> [B,5] (bit 30 of word 0 dropped, word 3 split)."""
    st = np.asarray(st, dtype=np.int64)
    return np.stack((st[:, 0] & 0xffff, st[:, 1], st[:, 2], st[:, 3] & 0xff, st[:, 3] >> 8), axis=1)


def minmax(rows):
    a = np.concatenate(rows, axis=0)
    return {k: [int(a[:, i].min()), int(a[:, i].max())] for i, k in enumerate(STAT_NAMES)}


def totals_differ(cost, ours, cold):
    """Matrices whose two permutations differ -> (how many, how many of those have different exact totals: not a tie)."""
    import math

    differ = not_tied = 0
    for b, (a, c) in enumerate(zip(ours, cold)):
        if np.array_equal(a[1], c[1]):
            continue
        differ += 1
        cb = cost[b]
        rows = torch.arange(cb.shape[0], device=cb.device)
        ta = math.fsum(cb[rows, torch.from_numpy(a[1]).to(cb.device)].double().cpu().tolist())
        tc = math.fsum(cb[rows, torch.from_numpy(c[1]).to(cb.device)].double().cpu().tolist())
        not_tied += int(ta != tc)
    return differ, not_tied


def jump_of(src0, n):
    """Unrelated frames: the batch rolled by seven, the points of every frame permuted."""
    perm = torch.from_numpy(np.random.default_rng(n).permutation(n)).to(src0.device)
    return src0.roll(7, 0)[:, perm].contiguous()


def probe_step_time(cost, state, max_steps):
    """The C entry alone on `cost` from a copy of `state` with `max_steps` allowed -> (device ms, [B,5] counts, given up)."""
    from reart_amd import _lib

    L = _lib.lib()
    nb, n, _ = cost.shape
    col, prices = state["cols"].clone().int().contiguous(), state["prices"].clone()
    cert = torch.zeros((nb,), dtype=torch.int32, device=cost.device)
    ws = torch.zeros((L.reart_lap_resolve_large_workspace_bytes(nb, n),), dtype=torch.uint8, device=cost.device)

    def run():
        col.copy_(state["cols"])
        prices.copy_(state["prices"])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(L.reart_lap_resolve_large(_lib.ptr(cost), nb, n, max_steps, _lib.ptr(col), _lib.ptr(cert), _lib.ptr(prices),
                                             _lib.ptr(prices), _lib.ptr(ws), ws.numel(), _lib.stream()), "reart_lap_resolve_large")
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    run()                                                         # warm-up
    ms = run()
    off = ((8 * nb * n + 255) // 256) * 256
    raw = ws[off:off + 16 * nb].view(torch.int32).reshape(nb, 4).cpu().numpy()
    return ms, split_stats(raw), int(((raw[:, 0] >> 30) & 1).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--sizes", default="4097,6144,8192")
    ap.add_argument("--probe_steps_per_n", type=int, default=32, help="steps allowed per matrix, as a multiple of n, when the jump is timed per step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lap_resolve_large_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lap_resolve_large.py needs an MI355X")

    from reart_amd.utils import lap

    dev = torch.device("cuda:0")
    out = {"B": B, "reps": args.reps, "steps": args.steps, "device": torch.cuda.get_device_name(0), "rows": []}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    sizes = [int(v) for v in args.sizes.split(",")]
    derive = {}
    for n in sizes:                                               # the step limit first: the timed runs below use it
        src0, tgt, _ = problems(n, dev)
        del _
        base = {}
        lap.linear_sum_assignment_points(src0, tgt, base)
        cold = lambda: lap.linear_sum_assignment_batch(lap.cdist(src0, tgt), points=(src0, tgt))
        cold()
        c_ms = spread([window(cold) for _ in range(args.reps)])
        allowed = args.probe_steps_per_n * n
        p_ms, p_st, p_gave_up = probe_step_time(lap.cdist(jump_of(src0, n), tgt), base, allowed)
        taken = int((p_st[:, 2] + p_st[:, 4]).max())
        us = 1e3 * p_ms / max(taken, 1)
        derive[n] = dict(probe_allowed=allowed, probe_ms=round(p_ms, 2), probe_steps_taken_max=taken, probe_given_up=p_gave_up,
                         us_per_step=round(us, 3), cold_step0=c_ms, steps_of_one_cold_solve=int(1e3 * c_ms["median_ms"] / us),
                         multiple_of_n=round(1e3 * c_ms["median_ms"] / us / n, 2))
        print(f"n = {n}: {derive[n]}", file=sys.stderr, flush=True)
        del src0, tgt, base
        torch.cuda.empty_cache()
    out["max_steps_multiple_of_n"] = int(min(d["multiple_of_n"] for d in derive.values()))
    for n in sizes:
        lap.RESOLVE_LARGE_MAX_STEPS = out["max_steps_multiple_of_n"] * n + 64
        src0, tgt, _ = problems(n, dev)
        base = {}
        _, fb0 = lap.linear_sum_assignment_points(src0, tgt, base, return_stats=True)          # step 0: cold, into the state
        res = {}

        def warm_solve(src, state):
            res["out"], res["fb"], res["st"] = lap.linear_sum_assignment_points(src, tgt, state, return_stats="full")

        def cold_solve(src):
            res["cold"], res["cold_fb"] = lap.linear_sum_assignment_batch(lap.cdist(src, tgt), return_stats=True, points=(src, tgt))

        copy = lambda: {"prices": base["prices"].clone(), "cols": base["cols"].clone()}
        warm_solve(src0, copy())                                  # warm-up of both shapes
        cold_solve(src0)
        row = dict(n=n, step0_fallbacks=int(fb0), sigmas=[])
        cold_ms = []
        for sigma in SIGMAS:
            ms, stats, forms = [], [], set()
            n_cold = fbs = differ = not_tied = 0
            for rep in range(args.reps):
                gen = torch.Generator(device=dev).manual_seed(1000 * rep + int(round(-np.log10(sigma))))
                state, src = copy(), src0
                for _ in range(args.steps):
                    src = (src + sigma * torch.randn(src.shape, generator=gen, device=dev)).contiguous()
                    ms.append(window(lambda: warm_solve(src, state)))
                    cold_ms.append(window(lambda: cold_solve(src)))
                    stats.append(split_stats(res["st"]))
                    forms.add(state.get("resolve_form"))
                    n_cold += int(state.get("resolve_cold", 0))
                    fbs += int(res["fb"]) + int(res["cold_fb"])
                    d_, t_ = totals_differ(lap.cdist(src, tgt), res["out"], res["cold"])
                    differ, not_tied = differ + d_, not_tied + t_
            row["sigmas"].append(dict(sigma=sigma, warm=spread(ms), forms=sorted(str(f) for f in forms), stats=minmax(stats),
                                      resolve_cold=n_cold, fallbacks=fbs, permutations_equal_cold=differ == 0,
                                      permutations_differ=differ, of_those_with_unequal_exact_totals=not_tied))
            print(f"n = {n} sigma = {sigma}: {row['sigmas'][-1]}", file=sys.stderr, flush=True)
        # the jump: unrelated frames
        jump = jump_of(src0, n)
        ms, stats, jcold = [], [], []
        n_cold = fbs = differ = not_tied = 0
        for rep in range(args.reps):
            state = copy()
            ms.append(window(lambda: warm_solve(jump, state)))
            jcold.append(window(lambda: cold_solve(jump)))
            stats.append(split_stats(res["st"]))
            n_cold += int(state.get("resolve_cold", 0))
            fbs += int(res["fb"]) + int(res["cold_fb"])
            d_, t_ = totals_differ(lap.cdist(jump, tgt), res["out"], res["cold"])
            differ, not_tied = differ + d_, not_tied + t_
        row["jump"] = dict(warm=spread(ms), cold=spread(jcold), stats=minmax(stats), resolve_cold=n_cold, fallbacks=fbs,
                           permutations_equal_cold=differ == 0, permutations_differ=differ, of_those_with_unequal_exact_totals=not_tied)
        row["cold"] = spread(cold_ms)
        w3 = row["sigmas"][SIGMAS.index(1e-3)]["warm"]
        row["routed_warm"] = bool(w3["median_ms"] < row["cold"]["median_ms"] and w3["max_ms"] < row["cold"]["min_ms"])
        row["max_steps"] = derive[n]
        row["max_steps_in_effect"] = int(lap.RESOLVE_LARGE_MAX_STEPS)
        print(f"n = {n}: cold {row['cold']} jump {row['jump']} routed_warm {row['routed_warm']} {row['max_steps']}", file=sys.stderr, flush=True)
        out["rows"].append(row)
        write()
        del src0, tgt, base, res, jump
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
