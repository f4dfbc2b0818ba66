#!/usr/bin/env python3
"""GPU timing of retargeting on the demo model (tests/golden/kinematic.npz: P = 10, E = 9; the 14 sparse points of
tests/golden/ik_nao.npz): the parent path, one Adam loop of separate launches per novel pose (ik_single), against the fused
path, all poses in one launch (ik_batch = ik_fit + one forward of all poses + one copy to the host).

Targets: the sparse points and the canonical cloud carried by seeded ground-truth angles (|theta| in [0.2, 0.8]), M in
{3, 64, 1024} novel poses.  The parent path is serial in M and is timed at M = 3 only.  Every figure is a device-event time
around work that ends in a synchronise (both paths end with their copy to the host), after a warm-up of the shape; `--reps`
repeats, the two paths alternating in one process; median, minimum and maximum are reported, per call and per pose.
`ik_fit_ms` is the kernel call alone (reart_ik_fit, 200 steps) inside the same window discipline.
Writes --out (default profiles/ik_fused_bench.json) and prints it as one JSON line.  Without a GPU it fails.
Usage: python tools/bench_ik.py [--reps 5] [--sizes 3,64,1024] [--fused_only] [--out PATH]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def demo_model(dev):
    from reart_amd.knn_cuda import KNN
    from reart_amd.networks.model import KinematicModel
    from reart_amd.utils.kinematic_utils import JointTree

    K = np.load(os.path.join(GOLDEN, "kinematic.npz"))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    parent, edge_of = K["parent"], K["edge_of_part"]
    edges = sorted(((int(edge_of[c]), c, int(parent[c])) for c in range(len(parent)) if parent[c] >= 0))
    tree = JointTree([[c, p] for _, c, p in edges], int(K["order"][0]))
    model = KinematicModel(pose_len=9, seg_part=t(K["seg_part"]), cano_pc=t(K["cano_pc"]), knn=KNN(k=1, transpose_mode=True),
                           edge_index={f"{c}_{p}": e for e, c, p in edges}, paths_to_base=tree.paths_to_base,
                           reverse_topo=K["order"].tolist(), axis_list=t(K["axis"]), moment_list=t(K["moment"]),
                           theta_list=t(K["theta"])).to(dev)
    return model, t(K["cano_pc"]).float()


def make_samples(model, cano_pc, M, dev, seed=0):
    rng = np.random.default_rng(seed)
    E = model.axis_list.shape[0]
    star = torch.from_numpy((rng.uniform(0.2, 0.8, (M, E)) * rng.choice([-1.0, 1.0], (M, E))).astype(np.float32)).to(dev)
    src = torch.from_numpy(np.load(os.path.join(GOLDEN, "ik_nao.npz"))["sparse_cano_0"]).float().to(dev)
    with torch.no_grad():
        tgt = model(src, theta_list=star)[0].cpu().numpy()
        novel = model(cano_pc, theta_list=star)[0].cpu().numpy()
    src = src.cpu().numpy()
    return [dict(sparse_cano_pc=src, sparse_novel_pc=tgt[m], novel_pc=novel[m]) for m in range(M)]


def window(fn):
    """One device-event time (ms) of fn(), which ends in a synchronise."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ms, M):
    ms = sorted(ms)
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4),
                median_ms_per_pose=round(ms[len(ms) // 2] / M, 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="3,64,1024")
    ap.add_argument("--fused_only", action="store_true", help="skip the parent path (a profiler run of the fused kernel)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik_fused_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ik.py needs an MI355X")

    from reart_amd.utils.kinematic_utils import ik_batch, ik_fit, ik_single

    dev = torch.device("cuda:0")
    model, cano_pc = demo_model(dev)
    out = {"model": "tests/golden/kinematic.npz", "P": 10, "E": int(model.axis_list.shape[0]), "n": 14, "n_iter": 200,
           "reps": args.reps, "rows": []}
    for M in (int(v) for v in args.sizes.split(",")):
        samples = make_samples(model, cano_pc, M, dev)
        src = torch.from_numpy(samples[0]["sparse_cano_pc"]).float().to(dev)
        tgt = torch.from_numpy(np.stack([s["sparse_novel_pc"] for s in samples])).float().to(dev)
        part = model.seg_forward(src)
        res = {}

        def fused():
            res["fused"] = ik_batch(model, cano_pc, samples, dev)[0]

        def fit():
            ik_fit(model, src, tgt, part=part)
            torch.cuda.synchronize()

        def parent():
            res["parent"] = np.array([ik_single(model, cano_pc, s, dev)[0] for s in samples])

        with_parent = M <= 3 and not args.fused_only
        fused(), fit()                                            # warm-up of the shape
        if with_parent:
            parent()
        t = {"fused": [], "fit": [], "parent": []}
        for _ in range(args.reps):                                # the paths alternate
            if with_parent:
                t["parent"].append(window(parent))
            t["fused"].append(window(fused))
            t["fit"].append(window(fit))
        row = dict(M=M, ik_batch=stats(t["fused"], M), ik_fit=stats(t["fit"], M), fused_mean_err=float(res["fused"].mean()))
        if with_parent:
            row["ik_single_loop"] = stats(t["parent"], M)
            row["parent_mean_err"] = float(res["parent"].mean())
            row["max_rel_err_difference"] = float(np.abs(res["fused"] - res["parent"]).max() / np.abs(res["parent"]).max())
            row["parent_over_ik_batch"] = round(row["ik_single_loop"]["median_ms"] / row["ik_batch"]["median_ms"], 2)
        out["rows"].append(row)
    out["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
