#!/usr/bin/env python3
"""Golden vectors for the public PointNet++ layer classes (networks/pointnet2_utils.py:143-348 and the extractor with
normals, networks/feature_extractor.py:11-46): the REFERENCE's own classes on this container's CPU (CPU-fallback rules for
FPS / ball query) with seeded weights that carry non-trivial BatchNorm running statistics.  The weights are NOT stored: the
tests regenerate them from the same seeds with `reart_amd.synthetic.extractor_state`.  The FPS start indices the reference
draws from torch's generator are recorded by re-seeding.  Data only: inputs, sampled coordinates, grouping indices, features.

    python tests/golden/make_golden_pointnet_layers.py

Configurations (the tests build the same ones; SEEDS gives the weight seed of every module):
  A  PointNet2Msg2(64, normal_channel=True) on [2,6,1024]
  B  a single-scale trunk: PointNetSetAbstraction(512, 0.2, 24, 3, [64,64,128]) with points=None ->
     (128, 0.4, 64, 131, [128,128,256]) -> group_all [256,512,1024] over the 128 points, and over a 100-point slice
  C  PointNetSetAbstractionMsg(512, [0.1,0.2,0.4], [16,32,128], 0, [[32,32,64],[64,64,128],[64,96,128]]) with points=None
  D  PointNetFeaturePropagation: S == 1; points1=None; the ordinary three-neighbour case
  E  sample_and_group(returnfps=True), sample_and_group_all, square_distance on a 300 x 200 pair
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REART_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)

from reart_amd.synthetic import extractor_state  # noqa: E402

SEEDS = dict(a=31, b1=32, b2=33, b3=34, c=35, d1=36, d2=37, d3=38)
TORCH_SEED = 77


def unit_normals(shape, seed):
    n = np.random.default_rng(seed).normal(size=shape).astype(np.float32)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def seeded(module, seed):
    module.load_state_dict(extractor_state(module, seed=seed))
    return module.eval()


def draw(n, B=2):
    """the start indices torch.randint hands the reference's FPS right after manual_seed(TORCH_SEED)"""
    torch.manual_seed(TORCH_SEED)
    return torch.randint(0, n, (B,), dtype=torch.long)


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print("wrote", name, os.path.getsize(path), "bytes")


def main():
    sys.path.insert(0, REF)
    import tests.golden.make_golden as mg  # installs the stand-ins, imports the reference  # noqa: F401
    from dataset.dataset_robot import Sequence
    from networks import pointnet2_utils as ref
    from networks.feature_extractor import PointNet2Msg2

    sample = Sequence(os.path.join(REF, "demo_data/data/nao"), num_points=4096, cano_idx=2)[0]
    pts = torch.from_numpy(sample["complete_pc_list"][[0, 5]][:, :1024]).float()  # [2,1024,3]
    pts = pts - pts.mean(dim=1, keepdim=True)
    pts = pts / pts.norm(dim=-1).max()
    xyz = pts.permute(0, 2, 1).contiguous()                                        # [2,3,1024]
    i16 = lambda t: t.numpy().astype(np.int16)

    with torch.no_grad():
        # ---- A: the extractor on clouds that carry normals
        xyz6 = torch.cat([xyz, torch.from_numpy(unit_normals((2, 1024, 3), 5)).permute(0, 2, 1)], dim=1).contiguous()
        model = seeded(PointNet2Msg2(out_dim=64, normal_channel=True), SEEDS["a"])
        torch.manual_seed(TORCH_SEED)
        s1 = torch.randint(0, 1024, (2,), dtype=torch.long)
        s2 = torch.randint(0, 512, (2,), dtype=torch.long)
        torch.manual_seed(TORCH_SEED)
        l1_xyz, l1 = model.sa1(xyz, xyz6)
        l2_xyz, l2 = model.sa2(l1_xyz, l1)
        torch.manual_seed(TORCH_SEED)
        feat = model(xyz6)
        idx1 = [ref.query_ball_point(r, k, pts, l1_xyz.permute(0, 2, 1)) for r, k in zip(model.sa1.radius_list, model.sa1.nsample_list)]
        save("pointnet_layers_a.npz", xyz6=xyz6.numpy(), start1=s1.numpy(), start2=s2.numpy(), l1_xyz=l1_xyz.numpy(),
             l2_xyz=l2_xyz.numpy(), l2_points=l2.numpy(), feat=feat.numpy(), idx1_0=i16(idx1[0]), idx1_1=i16(idx1[1]), idx1_2=i16(idx1[2]),
             keys=np.array(list(model.state_dict().keys())))

        # ---- B: a single-scale trunk
        sa1 = seeded(ref.PointNetSetAbstraction(512, 0.2, 24, 3, [64, 64, 128], False), SEEDS["b1"])
        sa2 = seeded(ref.PointNetSetAbstraction(128, 0.4, 64, 128 + 3, [128, 128, 256], False), SEEDS["b2"])
        sa3 = seeded(ref.PointNetSetAbstraction(None, None, None, 256 + 3, [256, 512, 1024], True), SEEDS["b3"])
        b_s1, b_s2 = draw(1024), draw(512)
        torch.manual_seed(TORCH_SEED)
        b1_xyz, b1 = sa1(xyz, None)
        torch.manual_seed(TORCH_SEED)
        b2_xyz, b2 = sa2(b1_xyz, b1)
        b3_xyz, b3 = sa3(b2_xyz, b2)
        _, b3_100 = sa3(b2_xyz[:, :, :100].contiguous(), b2[:, :, :100].contiguous())
        b_idx1 = ref.query_ball_point(0.2, 24, pts, b1_xyz.permute(0, 2, 1))
        b_idx2 = ref.query_ball_point(0.4, 64, b1_xyz.permute(0, 2, 1), b2_xyz.permute(0, 2, 1))
        save("pointnet_layers_b.npz", xyz=xyz.numpy(), start1=b_s1.numpy(), start2=b_s2.numpy(), l1_xyz=b1_xyz.numpy(), l1_points=b1.numpy(),
             l2_xyz=b2_xyz.numpy(), l2_points=b2.numpy(), l3_xyz=b3_xyz.numpy(), l3_points=b3.numpy(), l3_points_100=b3_100.numpy(),
             idx1=i16(b_idx1), idx2=i16(b_idx2), keys1=np.array(list(sa1.state_dict().keys())), keys3=np.array(list(sa3.state_dict().keys())))

        # ---- C: multi-scale grouping without input features
        msg = seeded(ref.PointNetSetAbstractionMsg(512, [0.1, 0.2, 0.4], [16, 32, 128], 0, [[32, 32, 64], [64, 64, 128], [64, 96, 128]]),
                     SEEDS["c"])
        c_s = draw(1024)
        torch.manual_seed(TORCH_SEED)
        c_xyz, c_pts = msg(xyz, None)
        c_idx = [ref.query_ball_point(r, k, pts, c_xyz.permute(0, 2, 1)) for r, k in zip([0.1, 0.2, 0.4], [16, 32, 128])]
        save("pointnet_layers_c.npz", xyz=xyz.numpy(), start=c_s.numpy(), new_xyz=c_xyz.numpy(), new_points=c_pts.numpy(),
             idx_0=i16(c_idx[0]), idx_1=i16(c_idx[1]), idx_2=i16(c_idx[2]), keys=np.array(list(msg.state_dict().keys())))

        # ---- D: feature propagation three ways (coarse clouds: B's sampled levels, FPS subsets of the finer ones)
        rng = np.random.default_rng(9)
        f = lambda *shape: torch.from_numpy(rng.normal(size=shape).astype(np.float32))
        fp_one = seeded(ref.PointNetFeaturePropagation(24 + 40, [64, 32]), SEEDS["d1"])
        d1_p1, d1_p2 = f(2, 24, 128), f(2, 40, 1)
        d1 = fp_one(b2_xyz, b3_xyz, d1_p1, d1_p2)
        fp_none = seeded(ref.PointNetFeaturePropagation(40, [64, 32]), SEEDS["d2"])
        d2_p2 = f(2, 40, 128)
        d2 = fp_none(b1_xyz, b2_xyz, None, d2_p2)
        fp_three = seeded(ref.PointNetFeaturePropagation(20 + 52, [96, 48]), SEEDS["d3"])
        d3_p1, d3_p2 = f(2, 20, 512), f(2, 52, 128)
        d3 = fp_three(b1_xyz, b2_xyz, d3_p1, d3_p2)

        # ---- E: the grouping functions and square_distance
        e_pts = f(2, 1024, 5)
        e_s = draw(1024)
        torch.manual_seed(TORCH_SEED)
        g_xyz, g_pts, g_grouped, g_fps = ref.sample_and_group(64, 0.3, 16, pts, e_pts, returnfps=True)
        a_xyz, a_pts = ref.sample_and_group_all(pts[:, :100].contiguous(), e_pts[:, :100].contiguous())
        sq = ref.square_distance(pts[:, :300].contiguous(), pts[:, 300:500].contiguous())
        save("pointnet_layers_de.npz", xyz=xyz.numpy(), l1_xyz=b1_xyz.numpy(), l2_xyz=b2_xyz.numpy(), l3_xyz=b3_xyz.numpy(),
             d1_points1=d1_p1.numpy(), d1_points2=d1_p2.numpy(), d1_out=d1.numpy(), d2_points2=d2_p2.numpy(), d2_out=d2.numpy(),
             d3_points1=d3_p1.numpy(), d3_points2=d3_p2.numpy(), d3_out=d3.numpy(), keys_fp=np.array(list(fp_three.state_dict().keys())),
             e_points=e_pts.numpy(), e_start=e_s.numpy(), sg_new_xyz=g_xyz.numpy(), sg_new_points=g_pts.numpy(),
             sg_grouped_xyz=g_grouped.numpy(), sg_fps_idx=i16(g_fps), sga_new_xyz=a_xyz.numpy(), sga_new_points=a_pts.numpy(),
             sq_dist=sq.numpy())


if __name__ == "__main__":
    main()
