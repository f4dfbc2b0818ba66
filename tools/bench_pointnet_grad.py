#!/usr/bin/env python3
"""Forward + backward of the correspondence extractor to its parameters, (descriptors * U).sum(), through the HIP path
(PointNet2Msg2.forward(grad=True): reart_mlp_layer / reart_three_interpolate forward, reart_mlp_layer_backward /
reart_three_interpolate_backward behind two autograd functions) against the same layers written with PyTorch tensor operations
on the same GPU, the way the reference writes them (networks/pointnet2_utils.py:194-348: index, subtract the centre, cat,
1x1 conv + eval BatchNorm as one folded matrix product, ReLU, max over the group; three-neighbour interpolation as gather and
weighted sum).  Both sides take their sampling (FPS, ball query) from the same HIP kernels, outside the graph.

  extractor   PointNet2Msg2(64), seeded weights, B = 2 clouds of N = 4096 points on a bumpy sphere

Timing: device events around --iters calls after --warmup, --reps repeats, the two sides alternating in one process; median
(min - max), milliseconds per forward + backward.  Merges its figures into --out (default profiles/pointnet_grad_bench.json)
and prints them as one JSON line.  `--calls N --side operator|composition` runs N calls of one side and nothing else: the run
to put under a kernel trace for the launches per call.  Without a GPU it fails."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_flow_term import merge, stats, window  # noqa: E402


def torch_extractor(net, pts):
    """PointNet2Msg2.forward as tensor operations with autograd: pts [B,N,3] -> [B,N,64]."""
    import torch

    from reart_amd.networks import pointnet2_utils as pn2
    from reart_amd.networks.feature_extractor import _fold_grad

    def stack(x, convs, bns):
        for conv, bn in zip(convs, bns):
            Wt, b = _fold_grad(conv, bn)
            x = torch.relu(x @ Wt + b)
        return x

    def msg(sa, xyz, feats):
        with torch.no_grad():
            new_xyz, idx_list = sa.sample(xyz)
        outs = []
        for i, idx in enumerate(idx_list):
            x = torch.cat([pn2.index_points(feats, idx), pn2.index_points(xyz, idx) - new_xyz[:, :, None, :]], dim=-1)
            outs.append(stack(x, sa.conv_blocks[i], sa.bn_blocks[i]).max(dim=2)[0])
        return new_xyz, torch.cat(outs, dim=-1)

    def fp(m, xyz1, xyz2, points1, points2):
        B, N, _ = xyz1.shape
        if xyz2.shape[1] == 1:
            interp = points2.expand(B, N, -1)
        else:
            with torch.no_grad():
                d, idx = pn2.square_distance(xyz1, xyz2).sort(dim=-1)
                d, idx = d[:, :, :3], idx[:, :, :3]
                w = 1.0 / (d + 1e-8)
                w = w / w.sum(dim=2, keepdim=True)
            interp = (pn2.index_points(points2, idx) * w[..., None]).sum(dim=2)
        x = interp if points1 is None else torch.cat([points1, interp], dim=-1)
        return stack(x, m.mlp_convs, m.mlp_bns)

    l1_xyz, l1 = msg(net.sa1, pts, pts)
    l2_xyz, l2 = msg(net.sa2, l1_xyz, l1)
    l3 = stack(torch.cat([l2_xyz, l2], dim=-1), net.sa3.mlp_convs, net.sa3.mlp_bns).max(dim=1, keepdim=True)[0]
    l2n = fp(net.fp3, l2_xyz, l2_xyz[:, :1], l2, l3)
    l1n = fp(net.fp2, l1_xyz, l2_xyz, l1, l2n)
    l0n = fp(net.fp1, pts, l1_xyz, torch.cat([pts, pts], dim=-1), l1n)
    return stack(l0n, [net.conv1], [net.bn1])


def sides(dev, B, N):
    import numpy as np
    import torch

    from reart_amd.networks.feature_extractor import PointNet2Msg2
    from reart_amd.synthetic import extractor_state

    net = PointNet2Msg2(64)
    net.load_state_dict(extractor_state(net))
    net = net.to(dev).eval()
    rng = np.random.default_rng(3)
    v = rng.normal(size=(B, N, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    pts = torch.from_numpy((v * (0.5 + 0.05 * rng.normal(size=(B, N, 1)))).astype(np.float32)).to(dev)
    xyz = pts.permute(0, 2, 1).contiguous()
    U = torch.from_numpy(rng.normal(size=(B, N, 64)).astype(np.float32)).to(dev)
    params = list(net.parameters())

    def run(forward):
        for p in params:
            p.grad = None
        (forward() * U).sum().backward()
        return [p.grad for p in params]

    return {"operator": lambda: run(lambda: net(xyz, grad=True).permute(0, 2, 1)), "composition": lambda: run(lambda: torch_extractor(net, pts))}


def measure(fns, args):
    import torch

    a, b = fns["operator"](), fns["composition"]()
    worst = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b))
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    ms = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            ms[k].append(window(fn, args.iters))
    torch.cuda.synchronize()
    out = {k: dict(stats(v), unit="ms per forward + backward") for k, v in ms.items()}
    out["ranges_apart"] = bool(out["operator"]["max"] < out["composition"]["min"] or out["composition"]["max"] < out["operator"]["min"])
    out["composition_over_operator_median"] = round(out["composition"]["median"] / out["operator"]["median"], 3)
    out["largest_gradient_difference_of_max"] = float(f"{worst:.2e}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clouds", type=int, default=2)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=0, help="run this many calls of --side and nothing else (for a kernel trace)")
    ap.add_argument("--side", choices=("operator", "composition"), default="operator")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointnet_grad_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_pointnet_grad.py needs an MI355X")
    dev = torch.device("cuda:0")
    fns = sides(dev, args.clouds, args.points)
    if args.calls:
        for _ in range(args.calls):
            fns[args.side]()
        torch.cuda.synchronize()
        return
    merge(args.out, device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, reps=args.reps,
          extractor=dict(measure(fns, args), workload=f"PointNet2Msg2(64) forward + backward to its parameters, B={args.clouds} x N={args.points}"))


if __name__ == "__main__":
    main()
