#!/usr/bin/env python3
"""GPU timing of the K-nearest search for points of any dimension D != 3 (csrc/knn_anyd.hip); prints one JSON line.

  knn_points     N in {1, 8}, P1 = P2 = 4096, D in {2, 6, 16, 64, 128, 256}, K in {1, 8, 64, 1024}
  KNN(k=1)       19 pairs of 4096 x 64-D descriptors (transpose_mode=False, [19, 64, 4096]: the matching="mnn" shape)
  backward       knn_points_backward at N = 1, 4096 x 4096, D = 64, K = 8

each next to the same GPU's torch.cdist(...).topk(K, largest=False) (speed only: its rounding differs from the search's
contract).  Times are device-event means over `--reps` calls after `--warmup` calls, in milliseconds.
Usage: python tools/bench_knn_dim.py [--reps 5] [--warmup 2]"""
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


def row(ms, ref, **kw):
    return dict(kw, ms=ms, cdist_topk_ms=ref, speedup_vs_cdist_topk=round(ref / ms, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn_dim.py needs an MI355X")

    from reart_amd import chamferdist_C
    from reart_amd.knn_cuda import KNN
    from reart_amd.utils.chamfer import knn_points

    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    out = {"knn_points": [], "knn_cuda": [], "backward": []}
    w, r = args.warmup, args.reps

    for N in (1, 8):
        for D in (2, 6, 16, 64, 128, 256):
            p1 = (torch.rand((N, 4096, D), generator=g) * 0.7 - 0.35).to(dev)
            p2 = (torch.rand((N, 4096, D), generator=g) * 0.7 - 0.35).to(dev)
            for K in (1, 8, 64, 1024):
                ms = timed(lambda: knn_points(p1, p2, K=K), w, r)
                ref = timed(lambda: torch.cdist(p1, p2).topk(K, dim=-1, largest=False), w, r)
                out["knn_points"].append(row(ms, ref, N=N, P1=4096, P2=4096, D=D, K=K))

    f1 = torch.randn((19, 64, 4096), generator=g).to(dev)
    f2 = torch.randn((19, 64, 4096), generator=g).to(dev)
    knn = KNN(k=1, transpose_mode=False)
    ms = timed(lambda: knn(f2, f1), w, r)
    ref = timed(lambda: torch.cdist(f1.transpose(1, 2), f2.transpose(1, 2)).topk(1, dim=-1, largest=False), w, r)
    out["knn_cuda"].append(row(ms, ref, B=19, nr=4096, nq=4096, D=64, k=1))

    p1 = (torch.rand((1, 4096, 64), generator=g) * 0.7 - 0.35).to(dev)
    p2 = (torch.rand((1, 4096, 64), generator=g) * 0.7 - 0.35).to(dev)
    idx, _ = chamferdist_C.knn_points_idx(p1, p2, None, None, 8)
    gd = torch.randn((1, 4096, 8), generator=g).to(dev)
    ms = timed(lambda: chamferdist_C.knn_points_backward(p1, p2, None, None, idx, gd), w, r)

    def torch_bwd():   # the same gradient by autograd through gather + squared distance, speed only
        a, b = p1.detach().requires_grad_(True), p2.detach().requires_grad_(True)
        nn = b[0][idx[0]]                                          # [4096, 8, 64]
        ((a[0][:, None] - nn) ** 2).sum(-1).mul(gd[0]).sum().backward()

    ref = timed(torch_bwd, w, r)
    out["backward"].append(dict(N=1, P1=4096, P2=4096, D=64, K=8, ms=ms, torch_autograd_ms=ref,
                                speedup_vs_torch_autograd=round(ref / ms, 3)))

    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
