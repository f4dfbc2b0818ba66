#!/usr/bin/env python3
"""GPU timing of the large-K search (16 < K <= 1024) and of FPS on clouds above 12 288 points; prints one JSON line.

  knn_points   N in {1, 8}, P1 = P2 = 4096, K in {32, 64, 200, 1024}, next to the same GPU's
               torch.cdist(...).topk(K, largest=False) (speed only: its rounding differs from the search's contract)
  KNN(k=64)    B = 19, 4096 x 4096 (transpose_mode=True)
  FPS          N in {16 384, 65 536, 262 144, 2^21}, M in {512, 2048}, B in {1, 8}, CUDA rules

Times are device-event means over `--reps` calls after `--warmup` calls, in milliseconds.
Usage: python tools/bench_large_knn_fps.py [--reps 5] [--warmup 2] [--quick]"""
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
    ap.add_argument("--quick", action="store_true", help="FPS: 1 warm-up and 1 timed call per shape")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_large_knn_fps.py needs an MI355X")

    from reart_amd.knn_cuda import KNN
    from reart_amd.networks.pointnet2_utils import farthest_point_sample
    from reart_amd.utils.chamfer import knn_points

    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    out = {"knn_points": [], "knn_cuda": [], "fps": []}

    for N in (1, 8):
        p1 = (torch.rand((N, 4096, 3), generator=g) * 0.7 - 0.35).to(dev)
        p2 = (torch.rand((N, 4096, 3), generator=g) * 0.7 - 0.35).to(dev)
        for K in (32, 64, 200, 1024):
            ms = timed(lambda: knn_points(p1, p2, K=K), args.warmup, args.reps)
            ref = timed(lambda: torch.cdist(p1, p2).topk(K, dim=-1, largest=False), args.warmup, args.reps)
            out["knn_points"].append({"N": N, "P1": 4096, "P2": 4096, "K": K, "ms": ms, "cdist_topk_ms": ref,
                                      "speedup_vs_cdist_topk": round(ref / ms, 3)})

    ref_pts = (torch.rand((19, 4096, 3), generator=g) * 0.7 - 0.35).to(dev)
    qry_pts = (torch.rand((19, 4096, 3), generator=g) * 0.7 - 0.35).to(dev)
    knn = KNN(k=64, transpose_mode=True)
    ms = timed(lambda: knn(ref_pts, qry_pts), args.warmup, args.reps)
    ref = timed(lambda: torch.cdist(qry_pts, ref_pts).topk(64, dim=-1, largest=False), args.warmup, args.reps)
    out["knn_cuda"].append({"B": 19, "nr": 4096, "nq": 4096, "k": 64, "ms": ms, "cdist_topk_ms": ref,
                            "speedup_vs_cdist_topk": round(ref / ms, 3)})

    fw, fr = (1, 1) if args.quick else (1, max(1, args.reps // 2))
    for N in (16384, 65536, 262144, 1 << 21):
        for B in (1, 8):
            xyz = (torch.rand((B, N, 3), generator=g) * 2 - 1).to(dev)
            for M in (512, 2048):
                ms = timed(lambda: farthest_point_sample(xyz, M, cuda_mode=True), fw, fr)
                out["fps"].append({"B": B, "N": N, "M": M, "ms": ms, "us_per_round": round(ms * 1e3 / M, 3)})
            del xyz

    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
