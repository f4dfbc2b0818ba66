#!/usr/bin/env python3
"""Forward + backward of the screw-consistency term on trans_list: networks.loss.StructureTerm (reart_structure_term, two
launches) against the same expression written with PyTorch tensor operations on the same GPU, the way the reference writes it
(networks/loss.py:32-57 over utils/graph_utils.py compute_relative_trans / compute_mean_screw_param and screw_se3's
transform_to_dq / dq_to_screw / se3_exp_map), restricted to the E edges and with selects in place of masked writes:

  tree        T = 19 frames, P = 20 parts, E = 19 edges (a random tree)
  all_pairs   T = 19 frames, P = 20 parts, E = 400 (all ordered pairs, the diagonal included)
Gradient w.r.t. trans_list.  Timing: device events around --iters calls after --warmup, --reps repeats, the two sides
alternating in one process; median (min - max), milliseconds per forward + backward.  Merges its figures into --out (default
profiles/structure_term_bench.json) and prints them as one JSON line.

`--only SIDE --calls N --shape NAME` runs N calls of one side and nothing else: the process a kernel trace counts launches of.
Without a GPU it fails."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_flow_term import merge, stats, window  # noqa: E402
from bench_transform_grad import screw_torch  # noqa: E402


def q_mul(q1, q2):
    import torch

    w = q2[..., 0] * q1[..., 0] - q2[..., 1] * q1[..., 1] - q2[..., 2] * q1[..., 2] - q2[..., 3] * q1[..., 3]
    x = q2[..., 0] * q1[..., 1] + q2[..., 1] * q1[..., 0] - q2[..., 2] * q1[..., 3] + q2[..., 3] * q1[..., 2]
    y = q2[..., 0] * q1[..., 2] + q2[..., 1] * q1[..., 3] + q2[..., 2] * q1[..., 0] - q2[..., 3] * q1[..., 1]
    z = q2[..., 0] * q1[..., 3] - q2[..., 1] * q1[..., 2] + q2[..., 2] * q1[..., 1] + q2[..., 3] * q1[..., 0]
    return torch.stack([w, x, y, z], -1)


def screw_of(R, t):
    """Rigid motions (R [...,3,3], t [...,3]) -> axis, moment, theta, distance (transform_to_dq + dq_to_screw)."""
    import torch

    m = lambda i, j: R[..., i, j]
    a = torch.stack([1 + m(0, 0) + m(1, 1) + m(2, 2), 1 + m(0, 0) - m(1, 1) - m(2, 2), 1 - m(0, 0) + m(1, 1) - m(2, 2),
                     1 - m(0, 0) - m(1, 1) + m(2, 2)], -1)
    qa = a.clamp(min=0).sqrt()
    cand = torch.stack([
        torch.stack([qa[..., 0] ** 2, m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1)], -1),
        torch.stack([m(2, 1) - m(1, 2), qa[..., 1] ** 2, m(1, 0) + m(0, 1), m(0, 2) + m(2, 0)], -1),
        torch.stack([m(0, 2) - m(2, 0), m(1, 0) + m(0, 1), qa[..., 2] ** 2, m(1, 2) + m(2, 1)], -1),
        torch.stack([m(1, 0) - m(0, 1), m(2, 0) + m(0, 2), m(2, 1) + m(1, 2), qa[..., 3] ** 2], -1)], -2)
    cand = cand / (2.0 * qa[..., None].clamp(min=0.1))
    best = qa.argmax(-1)
    qr = torch.gather(cand, -2, best[..., None, None].expand(best.shape + (1, 4)))[..., 0, :]
    qd = 0.5 * q_mul(torch.cat([torch.zeros_like(t[..., :1]), t], -1), qr)
    qn = qr / qr.norm(dim=-1, keepdim=True)
    theta = 2.0 * torch.atan2(qn[..., 1:].norm(dim=-1), qn[..., 0])
    no_rot = (theta.abs() < 1e-6) | ((theta - math.pi).abs() < 1e-6)
    tt = q_mul(2.0 * qd, qr * qr.new_tensor([1.0, -1.0, -1.0, -1.0]))[..., 1:]
    d0 = tt.norm(dim=-1)
    l = torch.where(no_rot[..., None], tt / (d0 + 1e-10)[..., None],
                    qr[..., 1:] / torch.where(no_rot, torch.ones_like(theta), torch.sin(theta / 2))[..., None])
    up = l.sum(-1) >= 0
    theta, l = torch.where(up, theta, -theta), torch.where(up[..., None], l, -l)
    d = torch.where(no_rot, torch.where(up, d0, -d0), (tt * l).sum(-1))
    one = (no_rot & (d.abs() <= 1e-8))[..., None] & l.new_tensor([1.0, 0.0, 0.0]).bool()
    l = torch.where(one, torch.ones_like(l), l)
    theta = torch.where(no_rot, torch.full_like(theta, 1e-6), theta)
    tl = torch.cross(tt, l, dim=-1)
    return l, 0.5 * (tl + torch.cross(l, tl / torch.tan(theta / 2)[..., None], dim=-1)), theta, d


def structure_term_torch(tl, e0, e1, weight=1.0):
    import torch

    A, B = tl[:, e0], tl[:, e1]
    RaT = A[..., :3, :3].transpose(-1, -2)
    R, t = RaT @ B[..., :3, :3], (RaT @ (B[..., :3, 3] - A[..., :3, 3])[..., None])[..., 0]
    E = R.shape[1]
    with torch.no_grad():
        l, m, theta, d = screw_of(R, t)
        unit = ((theta.abs() <= 1e-5) | ((theta - math.pi).abs() <= 1e-5)) & (d <= 1e-5)
        keep = (~unit).to(R.dtype)
        n = keep.sum(0)
        w = torch.where(((n == 0) | (E <= 1))[None], torch.ones_like(keep), keep)
        ml, mm = (l * w[..., None]).sum(0) / w.sum(0)[:, None], (m * w[..., None]).sum(0) / w.sum(0)[:, None]
        pris = (d.abs().mean(0) > theta.abs().mean(0))[None]
        G = screw_torch(ml[None].expand_as(l), mm[None].expand_as(m), torch.where(pris, torch.full_like(theta, 1e-6), theta),
                        torch.where(pris, d, torch.full_like(d, 1e-6)))
    MR = R @ G[..., :3, :3].transpose(-1, -2)
    eR = MR - torch.eye(3, device=tl.device)
    et = t - (MR @ G[..., :3, 3:])[..., 0]
    return weight * ((eR * eR).sum() + (et * et).sum())


def make_motion(dev, T, P, seed=5):
    """Part motions: a revolute screw per part (every third part slides instead) plus small noise -> trans_list [T,P,4,4]."""
    import numpy as np
    import torch

    rng = np.random.default_rng(seed)
    tr = np.tile(np.eye(4), (T, P, 1, 1))
    s = np.linspace(0.6, 1.0, T)
    for p in range(1, P):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        if p % 3 == 0:
            tr[:, p, :3, 3] = rng.uniform(-0.3, 0.3, 3) + (0.4 * s)[:, None] * axis
        else:
            K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
            point, ang = rng.uniform(-0.3, 0.3, 3), rng.uniform(0.4, 1.4)
            for t in range(T):
                R = np.eye(3) + math.sin(ang * s[t]) * K + (1 - math.cos(ang * s[t])) * (K @ K)
                tr[t, p, :3, :3], tr[t, p, :3, 3] = R, point - R @ point
        tr[:, p, :3, 3] += rng.normal(0, 1e-3, (T, 3))
    return torch.from_numpy(tr.astype(np.float32)).to(dev)


def sides(dev, T, P, shape):
    import numpy as np
    import torch

    from reart_amd.networks.loss import StructureTerm

    rng = np.random.default_rng(7)
    if shape == "tree":
        edges = np.array([(int(rng.integers(0, c)), c) for c in range(1, P)], np.int64)
    else:
        edges = np.array([(a, b) for a in range(P) for b in range(P)], np.int64)
    tl = make_motion(dev, T, P).requires_grad_(True)
    term = StructureTerm(edges)
    e0, e1 = (torch.from_numpy(edges[:, k].copy()).to(dev) for k in (0, 1))
    return {"operator": lambda: torch.autograd.grad(term(tl), tl),
            "composition": lambda: torch.autograd.grad(structure_term_torch(tl, e0, e1), tl)}, len(edges)


def measure(fns, args):
    import torch

    a, b = fns["operator"]()[0], fns["composition"]()[0]
    worst = float((a - b).abs().max() / b.abs().max())
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
    ap.add_argument("--frames", type=int, default=19)
    ap.add_argument("--parts", type=int, default=20)
    ap.add_argument("--only", choices=("operator", "composition"), help="run --calls calls of one side and nothing else")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--shape", choices=("tree", "all_pairs"), default="tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_term_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_structure_term.py needs an MI355X")
    dev = torch.device("cuda:0")
    T, P = args.frames, args.parts
    if args.only:
        fn = sides(dev, T, P, args.shape)[0][args.only]
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return
    res = {}
    for shape in ("tree", "all_pairs"):
        fns, E = sides(dev, T, P, shape)
        res[shape] = dict(measure(fns, args), workload=f"T={T} frames, P={P} parts, E={E} edges")
    merge(args.out, device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, reps=args.reps, **res)


if __name__ == "__main__":
    main()
