#!/usr/bin/env python3
"""Forward times of the public PointNet++ layer classes on one MI355X -> profiles/pointnet_layers_bench.json.

Per configuration (A: the extractor with normals, B: a single-scale trunk, C: multi-scale grouping without features -- the
configurations of tests/golden/make_golden_pointnet_layers.py at a working size) the forward with the fused chain and with
one launch per layer (``feature_extractor.FUSE_CHAIN = False``) on this tree, alternated.

With ``--parent DIR`` (a checkout of the parent commit with its library built) the shapes the parent can already run layer
by layer -- multi-scale levels with six feature columns, K in {32, 64, 128} -- are timed in that checkout and in this tree,
one fresh process each, alternated; and ``bench.py --config extractor`` (normal_channel=False, which must not move) likewise.

Method: device events around ``--steps`` forwards after ``--warmup`` untimed ones, ``--repeats`` alternated rounds, every
round's figure kept (spread = min .. max of the rounds).

    python tools/bench_pointnet_layers.py [--parent DIR] [--out profiles/pointnet_layers_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# shapes the parent commit runs today (its _SAMsg, one launch per layer): (npoint, radii, nsamples, in_channel, mlps)
PARENT_SHAPES = {
    "A_level1_normals": (512, [0.05, 0.1, 0.2], [32, 64, 128], 6, [[32, 32, 64], [64, 64, 128], [64, 96, 128]]),
    "msg_K32_64-64-128": (512, [0.1], [32], 6, [[64, 64, 128]]),
    "msg_K64_64-96-128": (512, [0.2], [64], 6, [[64, 96, 128]]),
    "msg_K128_128-128-256": (512, [0.4], [128], 6, [[128, 128, 256]]),
}


def clouds(B, N, dev, normals):
    import numpy as np
    import torch

    from reart_amd.synthetic import make_sequence

    seq = make_sequence(T=B, n_parts=8, pts_per_part=N // 8, seed=2, with_flow=False)
    pts = torch.from_numpy(seq["complete"]).float()
    pts = pts - pts.mean(dim=1, keepdim=True)
    pts = pts / pts.norm(dim=-1).max()
    if normals:
        n = np.random.default_rng(5).normal(size=tuple(pts.shape)).astype(np.float32)
        pts = torch.cat([pts, torch.from_numpy(n / np.linalg.norm(n, axis=-1, keepdims=True))], dim=2)
    return pts.to(dev).contiguous()                     # [B,N,3 or 6]


def timed(fn, steps, warmup):
    import torch

    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def seeded(module, seed, dev):
    from reart_amd.synthetic import extractor_state

    module.load_state_dict(extractor_state(module, seed=seed))
    return module.to(dev).eval()


def stats(ms):
    s = sorted(ms)
    return {"ms": [round(x, 4) for x in ms], "median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4)}


def worker(args):
    """One process, one tree (``--root``): the PARENT_SHAPES through ``_SAMsg.run`` (the name both trees have)."""
    sys.path.insert(0, args.root)
    import torch

    from reart_amd.networks import feature_extractor as fe

    assert os.path.realpath(os.path.dirname(os.path.dirname(os.path.dirname(fe.__file__)))) == os.path.realpath(args.root), fe.__file__
    dev = torch.device("cuda:0")
    pts6 = clouds(args.clouds, args.points, dev, True)
    xyz = pts6[:, :, :3].contiguous()
    out = {}
    for name, shape in PARENT_SHAPES.items():
        layer = seeded(fe._SAMsg(*shape), 31, dev)
        out[name] = timed(lambda: layer.run(xyz, pts6, cuda_mode=True), args.steps, args.warmup)
    print("WORKER " + json.dumps(out))


def run_worker(root, args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--clouds", str(args.clouds), "--points",
                        str(args.points), "--steps", str(args.steps), "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"worker in {root} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("WORKER ")][-1][7:])


def run_bench_extractor(root):
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--config", "extractor", "--steps", "20", "--warmup", "3",
                        "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, cwd=root)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {root} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])["ms_per_step"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with reart_amd/csrc/libreart_hip.so built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointnet_layers_bench.json"))
    ap.add_argument("--clouds", type=int, default=16)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    sys.path.insert(0, ROOT)
    import torch

    from reart_amd.networks import feature_extractor as fe
    from reart_amd.networks import pointnet2_utils as pu

    if not torch.cuda.is_available():
        raise SystemExit("bench_pointnet_layers needs an MI355X: nothing is measured without one")
    dev = torch.device("cuda:0")
    pts6 = clouds(args.clouds, args.points, dev, True)
    xyz6 = pts6.permute(0, 2, 1).contiguous()
    xyz = xyz6[:, :3].contiguous()
    ext = seeded(fe.PointNet2Msg2(64, normal_channel=True), 31, dev)
    sa1 = seeded(pu.PointNetSetAbstraction(512, 0.2, 24, 3, [64, 64, 128], False), 32, dev)
    sa2 = seeded(pu.PointNetSetAbstraction(128, 0.4, 64, 128 + 3, [128, 128, 256], False), 33, dev)
    sa3 = seeded(pu.PointNetSetAbstraction(None, None, None, 256 + 3, [256, 512, 1024], True), 34, dev)
    msg = seeded(pu.PointNetSetAbstractionMsg(512, [0.1, 0.2, 0.4], [16, 32, 128], 0, [[32, 32, 64], [64, 64, 128], [64, 96, 128]]), 35, dev)

    def trunk():
        l1_xyz, l1 = sa1(xyz, None)
        l2_xyz, l2 = sa2(l1_xyz, l1)
        return sa3(l2_xyz, l2)

    configs = {"A_extractor_normals": lambda: ext(xyz6), "B_single_scale_trunk": trunk, "C_msg_no_features": lambda: msg(xyz, None)}
    result = {"device": torch.cuda.get_device_name(0), "clouds": args.clouds, "points": args.points, "steps": args.steps, "warmup": args.warmup,
              "repeats": args.repeats, "sampling_rules": "CUDA", "method": "device events, alternated rounds, every round kept",
              "fused_vs_per_layer": {}}
    for name, fn in configs.items():
        ms = {"fused": [], "per_layer": []}
        for _ in range(args.repeats):
            for mode in ("fused", "per_layer"):
                fe.FUSE_CHAIN = mode == "fused"
                try:
                    ms[mode].append(timed(fn, args.steps, args.warmup))
                finally:
                    fe.FUSE_CHAIN = True
        result["fused_vs_per_layer"][name] = {k: stats(v) for k, v in ms.items()}
        print(name, json.dumps(result["fused_vs_per_layer"][name]), flush=True)
    if args.parent:
        parent = os.path.abspath(args.parent)
        rounds = {"parent": [], "tree": []}
        ext_ms = {"parent": [], "tree": []}
        for _ in range(min(args.repeats, 3)):
            for who, root in (("parent", parent), ("tree", ROOT)):
                rounds[who].append(run_worker(root, args))
                ext_ms[who].append(run_bench_extractor(root))
                print(who, json.dumps(rounds[who][-1]), ext_ms[who][-1], flush=True)
        result["against_parent"] = {}
        for name in PARENT_SHAPES:
            p, c = stats([r[name] for r in rounds["parent"]]), stats([r[name] for r in rounds["tree"]])
            # adopted: the tree's slowest round beats the parent's fastest, i.e. by more than the spread of both
            result["against_parent"][name] = {"parent_per_layer": p, "tree_fused": c, "adopted": c["max_ms"] < p["min_ms"]}
        result["extractor_normal_channel_false"] = {"what": "bench.py --config extractor --steps 20 --warmup 3, ms per step",
                                                    "parent": stats(ext_ms["parent"]), "tree": stats(ext_ms["tree"])}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
