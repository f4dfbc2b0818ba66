#!/usr/bin/env python3
"""Golden GRADIENTS of the PointNet++ layer classes and the correspondence extractor: the REFERENCE's own autograd modules
(networks/pointnet2_utils.py, networks/feature_extractor.py) in eval() on this container's CPU (CPU-fallback rules for FPS /
ball query), differentiated through the scalar (output * U).sum().  The weights are NOT stored: generator and tests make them
from the same seeds with `reart_amd.synthetic.extractor_state`; inputs and U come from recorded seeds too.  The FPS start
indices the reference draws from torch's generator are recorded by re-seeding.  Data only: seeds, starts, gradient tensors.

    python tests/golden/make_golden_pointnet_grad.py

Configurations (CONFIGS below; the tests build the same ones through ``build_ours``), all on B = 2:
  msg                       PointNetSetAbstractionMsg(16, [0.2, 0.4], [16, 24], 5, [[8, 8, 16], [16, 12, 20]]) on N = 200
  sa / sa_nopoints          PointNetSetAbstraction(16, 0.3, 16, 3 (+ 5), [8, 16], group_all=False), points given / None
  sa_all / sa_all_nopoints  the same with group_all=True
  fp_s1 / fp_s1_nop1        PointNetFeaturePropagation([16, 12]) with ONE coarse point, points1 given / None
  fp_s16 / fp_s16_nop1      the same with 16 coarse points (the three-neighbour interpolation)
  extractor                 PointNet2Msg2(64) on N = 1024; gradients of EXTRACTOR_GRADS.  Its cloud's seed is rejected where the
                            reference's float32 gradients are not within EXTRACTOR_MARGIN of the float64 restatement's

A seed of a small-layer case is rejected (the next one is tried) where the float32 forward of
tests/pointnet_grad_ref.Restatement has a pooled top-two gap between distinct values, or a selected pre-activation, below
MARGIN of its layer's largest activation: the reference's float32 decisions are then the restatement's and ours.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REART_REFERENCE", "/root/reference")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from reart_amd.synthetic import extractor_state  # noqa: E402

TORCH_SEED = 91
MARGIN = 1e-4
EXTRACTOR_MARGIN = 2e-5
B = 2
MSG = dict(npoint=16, radius_list=[0.2, 0.4], nsample_list=[16, 24], in_channel=5, mlp_list=[[8, 8, 16], [16, 12, 20]])
# name -> kind, points per cloud, feature widths (points / points1, points2), first data seed
CONFIGS = {
    "msg": dict(kind="msg", N=200, D=5, seed=100),
    "sa": dict(kind="sa", N=200, D=5, group_all=False, seed=200),
    "sa_nopoints": dict(kind="sa", N=200, D=0, group_all=False, seed=300),
    "sa_all": dict(kind="sa", N=200, D=5, group_all=True, seed=400),
    "sa_all_nopoints": dict(kind="sa", N=200, D=0, group_all=True, seed=500),
    "fp_s1": dict(kind="fp", N=50, S=1, D1=6, D2=7, seed=600),
    "fp_s1_nop1": dict(kind="fp", N=50, S=1, D1=0, D2=7, seed=700),
    "fp_s16": dict(kind="fp", N=200, S=16, D1=6, D2=7, seed=800),
    "fp_s16_nop1": dict(kind="fp", N=200, S=16, D1=0, D2=7, seed=900),
}
LAYERS = list(CONFIGS)
EXTRACTOR = dict(N=1024, seed=1000, weight_seed=11)
EXTRACTOR_GRADS = ["sa1.conv_blocks.0.0.weight", "sa1.bn_blocks.0.0.weight", "sa1.bn_blocks.0.0.bias", "sa2.bn_blocks.1.2.weight",
                   "sa2.bn_blocks.1.2.bias", "sa3.mlp_bns.1.weight", "sa3.mlp_bns.1.bias", "fp3.mlp_bns.0.weight", "fp3.mlp_bns.0.bias",
                   "fp2.mlp_bns.1.weight", "fp2.mlp_bns.1.bias", "fp1.mlp_bns.0.weight", "fp1.mlp_bns.0.bias", "fp1.mlp_convs.0.weight",
                   "conv1.weight", "bn1.bias"]


def make_module(ns, name):
    """The configuration's module from the namespace ``ns`` (the reference's pointnet2_utils, or ours)."""
    cfg = CONFIGS[name]
    if cfg["kind"] == "msg":
        return ns.PointNetSetAbstractionMsg(MSG["npoint"], MSG["radius_list"], MSG["nsample_list"], MSG["in_channel"], MSG["mlp_list"])
    if cfg["kind"] == "sa":
        if cfg["group_all"]:
            return ns.PointNetSetAbstraction(None, None, None, 3 + cfg["D"], [8, 16], True)
        return ns.PointNetSetAbstraction(16, 0.3, 16, 3 + cfg["D"], [8, 16], False)
    return ns.PointNetFeaturePropagation(cfg["D1"] + cfg["D2"], [16, 12])


def cloud(rng, n):
    """n points on a bumpy sphere of radius 0.5: ball queries of radius 0.2 .. 0.4 find from a few to more than nsample."""
    v = rng.normal(size=(B, n, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    return (v * (0.5 + 0.05 * rng.normal(size=(B, n, 1)))).astype(np.float32)


def inputs_of(name, seed):
    """Channel-first float32 numpy inputs of a layer configuration, in the order of its forward (None where absent)."""
    cfg, rng = CONFIGS[name], np.random.default_rng(seed)
    xyz = cloud(rng, cfg["N"])
    cf = lambda a: np.ascontiguousarray(np.transpose(a, (0, 2, 1)))
    if cfg["kind"] in ("msg", "sa"):
        pts = rng.normal(size=(B, cfg["N"], cfg["D"])).astype(np.float32) if cfg["D"] else None
        return dict(xyz=cf(xyz), points=None if pts is None else cf(pts))
    sub = np.stack([xyz[b, rng.permutation(cfg["N"])[:cfg["S"]]] for b in range(B)])
    p1 = rng.normal(size=(B, cfg["N"], cfg["D1"])).astype(np.float32) if cfg["D1"] else None
    p2 = rng.normal(size=(B, cfg["S"], cfg["D2"])).astype(np.float32)
    return dict(xyz1=cf(xyz), xyz2=cf(sub), points1=None if p1 is None else cf(p1), points2=cf(p2))


def upstream(name, shape):
    """U of the scalar (output * U).sum(): fixed by the configuration's name."""
    base = EXTRACTOR["seed"] if name == "extractor" else CONFIGS[name]["seed"]
    return np.random.default_rng(50000 + base).normal(size=shape).astype(np.float32)


def draw(n):
    """the start indices torch.randint hands the reference's FPS right after manual_seed(TORCH_SEED)"""
    torch.manual_seed(TORCH_SEED)
    return torch.randint(0, n, (B,), dtype=torch.long)


def draw_pair(n1, n2):
    """the extractor's two draws: sa1's FPS start, then sa2's"""
    torch.manual_seed(TORCH_SEED)
    a = torch.randint(0, n1, (B,), dtype=torch.long)
    return a.numpy(), torch.randint(0, n2, (B,), dtype=torch.long).numpy()


def weight_seed(name, seed):
    return 7 * seed + 1


def build_ours(name, z, dev):
    """Our module for a configuration with the generator's weights, its inputs on ``dev`` and the recorded FPS starts:
    (module, {argument: tensor or None} in forward order, starts) -- for "extractor": (net, xyz [B,3,N], (start1, start2))."""
    from reart_amd.networks import feature_extractor as fe
    from reart_amd.networks import pointnet2_utils as ours

    if name == "extractor":
        net = fe.PointNet2Msg2(64)
        net.load_state_dict(extractor_state(net, seed=EXTRACTOR["weight_seed"]))
        xyz = np.ascontiguousarray(np.transpose(cloud(np.random.default_rng(int(z["extractor/seed"])), EXTRACTOR["N"]), (0, 2, 1)))
        starts = (torch.from_numpy(z["extractor/start1"]).to(dev), torch.from_numpy(z["extractor/start2"]).to(dev))
        return net.to(dev).eval(), torch.from_numpy(xyz).to(dev), starts
    seed = int(z[name + "/seed"])
    mod = make_module(ours, name)
    mod.load_state_dict(extractor_state(mod, seed=weight_seed(name, seed)))
    inputs = {k: (None if v is None else torch.from_numpy(v).to(dev)) for k, v in inputs_of(name, seed).items()}
    starts = torch.from_numpy(z[name + "/start"]).to(dev) if name + "/start" in z.files else None
    return mod.to(dev).eval(), inputs, starts


def restate(name, seed, start):
    """tests/pointnet_grad_ref.Restatement of a layer configuration -> (restatement, output float64 [B,C,n], feature leaves)."""
    from tests import pointnet_grad_ref as G

    cfg = CONFIGS[name]
    mod = make_module(__import__("reart_amd.networks.pointnet2_utils", fromlist=["x"]), name)
    rs = G.Restatement({k: v.numpy() for k, v in extractor_state(mod, seed=weight_seed(name, seed)).items()})
    inp = inputs_of(name, seed)
    cl = lambda a: None if a is None else np.ascontiguousarray(np.transpose(a, (0, 2, 1)))
    leaves = {}

    def pair(key):
        if inp[key] is None:
            return None, None
        f32 = torch.from_numpy(cl(inp[key]))
        leaves[key] = f32.double().requires_grad_(True)
        return f32, leaves[key]
    if cfg["kind"] == "msg":
        f32, f64 = pair("points")
        _, _, y = rs.sa_msg("", cl(inp["xyz"]), f32, f64, MSG["npoint"], MSG["radius_list"], MSG["nsample_list"], 3, start)
    elif cfg["kind"] == "sa":
        f32, f64 = pair("points")
        _, _, y = rs.sa("", cl(inp["xyz"]), f32, f64, 16, 0.3, 16, 2, start, cfg["group_all"])
    else:
        a32, a64 = pair("points1")
        b32, b64 = pair("points2")
        _, y = rs.fp("", cl(inp["xyz1"]), cl(inp["xyz2"]), a32, a64, b32, b64, 2)
    return rs, y.permute(0, 2, 1), leaves


def main():
    sys.path.insert(0, REF)
    import tests.golden.make_golden as mg  # installs the stand-ins, imports the reference  # noqa: F401
    from networks import pointnet2_utils as ref
    from networks.feature_extractor import PointNet2Msg2

    out = {}
    for name, cfg in CONFIGS.items():
        sampled = cfg["kind"] == "msg" or (cfg["kind"] == "sa" and not cfg["group_all"])
        start = draw(cfg["N"]).numpy() if sampled else None
        for seed in range(cfg["seed"], cfg["seed"] + 50):
            rs, _, _ = restate(name, seed, start)
            if rs.margin >= MARGIN:
                break
            print(name, "seed", seed, "rejected: margin", rs.margin)
        else:
            raise SystemExit(f"no admitted seed for {name}")
        mod = make_module(ref, name)
        mod.load_state_dict(extractor_state(mod, seed=weight_seed(name, seed)))
        mod.eval()
        inputs = {k: (None if v is None else torch.from_numpy(v)) for k, v in inputs_of(name, seed).items()}
        for k, v in inputs.items():
            if v is not None and k.startswith("points"):
                v.requires_grad_(True)
        torch.manual_seed(TORCH_SEED)
        res = mod(*inputs.values())
        feats = res[1] if isinstance(res, tuple) else res
        (feats * torch.from_numpy(upstream(name, tuple(feats.shape)))).sum().backward()
        out[name + "/seed"] = np.int64(seed)
        out[name + "/margin"] = np.float64(rs.margin)
        if start is not None:
            out[name + "/start"] = start
        for k, v in inputs.items():
            if v is not None and v.grad is not None:
                out[f"{name}/grad/{k}"] = v.grad.numpy()
        for k, p in mod.named_parameters():
            out[f"{name}/grad/{k}"] = p.grad.numpy()
        print(name, "seed", seed, "margin %.3e" % rs.margin, "output", tuple(feats.shape))

    from tests import pointnet_grad_ref as G

    s1 = draw_pair(EXTRACTOR["N"], 512)
    for seed in range(EXTRACTOR["seed"], EXTRACTOR["seed"] + 20):
        net = PointNet2Msg2(out_dim=64)
        net.load_state_dict(extractor_state(net, seed=EXTRACTOR["weight_seed"]))
        net.eval()
        pts = cloud(np.random.default_rng(seed), EXTRACTOR["N"])
        xyz = torch.from_numpy(np.ascontiguousarray(np.transpose(pts, (0, 2, 1))))
        torch.manual_seed(TORCH_SEED)
        feat = net(xyz)
        U = torch.from_numpy(upstream("extractor", tuple(feat.shape)))
        (feat * U).sum().backward()
        params = dict(net.named_parameters())
        # the float32 decisions of a network this deep differ between two float32 evaluations somewhere (a ReLU or a group
        # maximum decided by the last bit); a cloud is admitted where the reference's own float32 gradients lie within
        # EXTRACTOR_MARGIN of their largest entry of the float64 restatement, i.e. where no such decision carries weight
        rs = G.Restatement({k: v.numpy() for k, v in extractor_state(net, seed=EXTRACTOR["weight_seed"]).items()})
        _, y = rs.extractor(pts, s1)
        (y.permute(0, 2, 1) * U.double()).sum().backward()
        worst = max(float((rs.p64[k].grad.reshape(params[k].shape) - params[k].grad.double()).abs().max() / params[k].grad.abs().max())
                    for k in EXTRACTOR_GRADS)
        print("extractor seed", seed, "worst |reference - float64| / largest entry = %.2e" % worst)
        if worst <= EXTRACTOR_MARGIN:
            break
    else:
        raise SystemExit("no admitted cloud for the extractor")
    out["extractor/seed"] = np.int64(seed)
    out["extractor/start1"], out["extractor/start2"] = s1
    for k in EXTRACTOR_GRADS:
        out["extractor/grad/" + k] = params[k].grad.numpy()
    path = os.path.join(HERE, "pointnet_grad.npz")
    np.savez_compressed(path, **out)
    print("wrote pointnet_grad.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
