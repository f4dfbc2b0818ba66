#!/usr/bin/env python3
"""Forward + backward of a loss on the transforms, (A * pc_trans).sum() + (W * trans_list).sum(), through the HIP operators
(BaseModel.forward / KinematicModel.forward with their autograd functions, reart_pose_trans_backward and
reart_fk_backward_trans behind them) against the same expression written with PyTorch tensor operations on the same GPU, the
way the reference writes its models (networks/model.py:39-70, :151-165; utils/kinematic_utils.py:151-198):

  base        BaseModel, T = 20 frames (19 poses), N = 4096 points, 20 parts, injected Gumbel noise, tau = 1
  kinematic   KinematicModel over a random tree of 10 parts (9 revolute joints), 19 poses, N = 4096 points (labels given: the
              1-NN label transfer is the same launch on both sides and is left out of both)
Gradients w.r.t. the models' parameters.  Timing: device events around --iters calls after --warmup, --reps repeats, the two
sides alternating in one process; median (min - max), milliseconds per forward + backward.  Merges its figures into --out
(default profiles/transform_grad_bench.json) and prints them as one JSON line.

`--merge-loop THIS.json PARENT.json [...]` copies the results of tools/bench_operator_loop.py runs (one process each, this
tree and the parent commit's with --tree, alternating) into --out: what the removed host synchronisation of the base model's
backward does to the import-only loop.  Without a GPU it fails."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_flow_term import merge, stats, window  # noqa: E402


def r6d_torch(d6):
    import torch
    import torch.nn.functional as F

    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = F.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


def with_bottom_row(top):
    import torch

    bottom = top.new_tensor([0.0, 0.0, 0.0, 1.0]).expand(top.shape[:-2] + (1, 4))
    return torch.cat([top, bottom], -2)


# ------------------------------------------------------------------------------------------------------------------ base
def base_sides(dev, T, N, P):
    import torch
    import torch.nn.functional as F

    from reart_amd.networks.model import BaseModel, sample_gumbel

    B = T - 1
    gen = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda *s: torch.randn(s, device=dev, generator=gen)
    torch.manual_seed(5)
    model = BaseModel(num_parts=P, pose_len=B).to(dev)
    with torch.no_grad():
        model.proposal_6d += 0.05 * rnd(B, P, 6)
        model.proposal_t += 0.01 * rnd(B, P, 3)
    cano, A, W = 0.3 * rnd(N, 3), rnd(B, N, 3), rnd(B, P, 4, 4)
    noise = sample_gumbel((N, P), dev)
    params = list(model._weights()) + [model.proposal_6d, model.proposal_t]

    def loss_grads(out, trans):
        return torch.autograd.grad((out * A).sum() + (trans * W).sum(), params)

    def operator():
        out, _, trans = model(cano, tau=1.0, gumbel=noise)
        return loss_grads(out, trans)

    def composition():
        W1, b1, W2, p6d, pt = params
        h = torch.relu(cano @ W1[:, :, 0].T + b1)
        s = h @ W2[:, :, 0].T
        y = ((s + noise) / 1.0).softmax(-1)
        weight = F.one_hot(y.argmax(-1), P).to(y.dtype) - y.detach() + y
        R = r6d_torch(p6d)
        pc = torch.einsum("bpij,nj->bpni", R, cano) + pt[:, :, None, :]
        out = torch.einsum("np,bpni->bni", weight, pc)
        return loss_grads(out, with_bottom_row(torch.cat([R, pt[..., None]], -1)))

    return {"operator": operator, "composition": composition}


# ------------------------------------------------------------------------------------------------------------- kinematic
def hat(w):
    import torch

    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], z, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def screw_torch(l, m, theta, d):
    """Screw parameters -> SE(3) [B,E,4,4] (screw_se3/screw_utils.py:6-30, geo_utils.py:90-222): the strict no-rotation test at
    1e-6 and the clamp of the squared rotation norm at 1e-4 as selects."""
    import torch

    no_rot = (theta.abs() < 1e-6) | ((theta - math.pi).abs() < 1e-6)
    q = torch.cross(l, m, dim=-1)
    v_rot = torch.cross(q, l, dim=-1) + (d / torch.where(no_rot, torch.ones_like(theta), theta))[..., None] * l
    w = torch.where(no_rot[..., None], torch.zeros_like(l), l)
    v = torch.where(no_rot[..., None], l, v_rot)
    om, u = w * theta[..., None], v * theta[..., None]
    n2 = (om * om).sum(-1).clamp(min=1e-4)
    ph = n2.sqrt()
    K = hat(om)
    K2 = K @ K
    eye = torch.eye(3, device=l.device).expand(K.shape)
    f = lambda x: x[..., None, None]
    R = eye + f(ph.sin() / ph) * K + f((1.0 - ph.cos()) / n2) * K2
    V = eye + f((1.0 - ph.cos()) / n2) * K + f((ph - ph.sin()) / (ph * n2)) * K2
    return with_bottom_row(torch.cat([R, V @ u[..., None]], -1))


def kinematic_sides(dev, T, N, P):
    import numpy as np
    import torch

    from reart_amd.utils.kinematic_utils import _FK

    B, E = T - 1, P - 1
    rng = np.random.default_rng(5)
    parent = np.array([-1] + [int(rng.integers(0, c)) for c in range(1, P)], np.int32)
    edge_of = np.array([-1] + list(range(E)), np.int32)
    order = np.arange(P, dtype=np.int32)
    t = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    axis = rng.normal(size=(E, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    params = [t(axis).requires_grad_(True), t(rng.normal(0, 0.3, (E, 3))).requires_grad_(True),
              t(rng.uniform(0.05, 1.5, (B, E))).requires_grad_(True)]
    x, part = t(rng.uniform(-0.3, 0.3, (N, 3))), t(rng.integers(0, P, N), np.int64)
    A, W = t(rng.normal(size=(B, N, 3))), t(rng.normal(size=(B, P, 4, 4)))
    tree = tuple(t(a, np.int32) for a in (parent, edge_of, order))

    def loss_grads(out, trans):
        return torch.autograd.grad((out * A).sum() + (trans * W).sum(), params)

    def operator():
        out, trans = _FK.apply(x, part, params[0], params[1], params[2], None, *tree, True)
        return loss_grads(out, trans)

    def composition():
        l, m, theta = params
        T_rel = screw_torch(l[None].expand(B, E, 3), m[None].expand(B, E, 3), theta, torch.full_like(theta, 1e-6))
        F = [None] * P
        for c in order:                                           # parts root to leaf, one product each
            F[c] = torch.eye(4, device=dev).expand(B, 4, 4) if parent[c] < 0 else F[parent[c]] @ T_rel[:, edge_of[c]]
        trans = torch.stack(F, 1)
        Tn = trans[:, part]
        out = (Tn[..., :3, :3] @ x[None, :, :, None])[..., 0] + Tn[..., :3, 3]
        return loss_grads(out, trans)

    return {"operator": operator, "composition": composition}


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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--merge-loop", nargs="+", metavar="JSON",
                    help="bench_operator_loop.py results, one process each: this tree, the parent's[, this tree, the parent's ...]")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transform_grad_bench.json"))
    args = ap.parse_args()
    if args.merge_loop:
        runs = [json.load(open(p)) for p in args.merge_loop]
        keys = ("median_it_s", "min_it_s", "max_it_s")
        loop = {}
        for mode in ("flag_off", "fused_losses"):
            this, parent = [{k: r[mode][k] for k in keys} for r in runs[0::2]], [{k: r[mode][k] for k in keys} for r in runs[1::2]]
            loop[mode] = {"this_commit": this, "parent_commit": parent,
                          "ranges_apart": bool(min(r["min_it_s"] for r in this) > max(r["max_it_s"] for r in parent)
                                               or max(r["max_it_s"] for r in this) < min(r["min_it_s"] for r in parent)),
                          "this_over_parent_median": [round(a["median_it_s"] / b["median_it_s"], 3) for a, b in zip(this, parent)]}
        return merge(args.out, operator_loop=dict(loop, workload=runs[0]["workload"], iters=runs[0]["iters"], warmup=runs[0]["warmup"],
                                                  reps=runs[0]["reps"], method="processes in the order they ran: this tree, the parent "
                                                  "commit's, this tree, ...; inside a process the two modes alternate"))
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_transform_grad.py needs an MI355X")
    dev = torch.device("cuda:0")
    T, N = args.frames, args.points
    merge(args.out, device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, reps=args.reps,
          base_model=dict(measure(base_sides(dev, T, N, 20), args), workload=f"BaseModel T={T} x N={N}, 20 parts, tau 1, injected noise"),
          kinematic_model=dict(measure(kinematic_sides(dev, T, N, 10), args),
                               workload=f"fk + rigid apply, random tree of 10 parts (9 joints), T={T} x N={N}"))


if __name__ == "__main__":
    main()
