#!/usr/bin/env python3
"""GPU timing of the float64 K-nearest search (csrc/knn_anyd.hip, float64); prints one JSON line.

  knn_points     N in {1, 8}, P1 = P2 = 4096, D in {3, 16, 64, 256}, K in {1, 8, 64, 1024}

each row times the float64 search, the float32 search on the same clouds cast to float32 (knn.hip / knn_list.hip at
D = 3, knn_anyd.hip otherwise) and float64 torch.cdist(...).topk(K, largest=False) on the same GPU (speed only: its
rounding differs from the search's contract).  Times are device-event means over `--reps` calls after `--warmup`
calls, in milliseconds.
Usage: python tools/bench_knn_f64.py [--reps 5] [--warmup 2]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / reps, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn_f64.py needs an MI355X")

    from reart_amd.utils.chamfer import knn_points

    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    out = {"knn_points": []}
    w, r = args.warmup, args.reps

    for N in (1, 8):
        for D in (3, 16, 64, 256):
            p1 = (torch.rand((N, 4096, D), generator=g, dtype=torch.float64) * 0.7 - 0.35).to(dev)
            p2 = (torch.rand((N, 4096, D), generator=g, dtype=torch.float64) * 0.7 - 0.35).to(dev)
            q1, q2 = p1.float(), p2.float()
            for K in (1, 8, 64, 1024):
                ms = timed(lambda: knn_points(p1, p2, K=K), w, r)
                ms32 = timed(lambda: knn_points(q1, q2, K=K), w, r)
                ref = timed(lambda: torch.cdist(p1, p2).topk(K, dim=-1, largest=False), w, r)
                out["knn_points"].append(dict(N=N, P1=4096, P2=4096, D=D, K=K, f64_ms=ms, f32_ms=ms32,
                                              cdist_topk_f64_ms=ref, f64_over_f32=round(ms / ms32, 3),
                                              speedup_vs_cdist_topk_f64=round(ref / ms, 3)))

    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
