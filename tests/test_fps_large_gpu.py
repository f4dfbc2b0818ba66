"""GPU parity of farthest point sampling on clouds above 12 288 points (csrc/fps_large.hip, reart_fps_temp) against the
CPU oracle under both tie rules, the pointnet2_cuda wrapper with a caller-allocated temp buffer, the PointNet++ extractor
on a large cloud, and the new ceiling."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cloud(rng, B, N):
    xyz = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    xyz[:, 5] = xyz[:, 40]                                          # duplicated points
    xyz[:, N - 1] = xyz[:, min(13000, N - 2)]                       # ... across the register / temp border
    xyz[B - 1, : N // 2] = np.round(xyz[B - 1, : N // 2] * 4) / 4   # lattice half: many exact distance ties
    return xyz


@pytest.mark.parametrize("cuda_mode", [False, True])
@pytest.mark.parametrize("N,M", [(12289, 64), (16384, 512), (65537, 1024), (200000, 2048), (1 << 21, 256)])
def test_fps_large_vs_oracle(oracle, dev, cuda_mode, N, M):
    from reart_amd.networks.pointnet2_utils import farthest_point_sample

    rng = np.random.default_rng(N + M + int(cuda_mode))
    B = 2 if N <= 65537 else 1
    xyz = _cloud(rng, B, N)
    start = rng.integers(0, N, B).astype(np.int32)
    ref = oracle.fps(xyz, M, start=start, cuda_mode=cuda_mode)
    got = farthest_point_sample(t(xyz, dev), M, start=t(start, dev), cuda_mode=cuda_mode)
    assert got.dtype == torch.int64
    np.testing.assert_array_equal(got.cpu().numpy(), ref)


def test_fps_large_all_ties_cuda_rule(oracle, dev):
    """Coincident points at N = 20 000: every distance ties, so the block-tree rule (lowest k % 1024, then lowest k)
    decides the whole sequence."""
    from reart_amd.networks.pointnet2_utils import farthest_point_sample

    N, M = 20000, 64
    xyz = np.zeros((2, N, 3), np.float32)
    xyz[1, 1::2] = 1.0                                              # two-value cloud
    ref = oracle.fps(xyz, M, cuda_mode=True)
    got = farthest_point_sample(t(xyz, dev), M, cuda_mode=True)
    np.testing.assert_array_equal(got.cpu().numpy(), ref)


def test_furthest_point_sampling_wrapper_large_garbage_temp(oracle, dev):
    from reart_amd import pointnet2_cuda as pc

    rng = np.random.default_rng(5)
    B, N, M = 2, 50000, 300
    xyz = _cloud(rng, B, N)
    temp = torch.full((B, N), -3.0, device=dev)                    # garbage: the kernel must initialise what it uses
    temp[:, ::3] = float("nan")
    idx = torch.full((B, M), -1, dtype=torch.int32, device=dev)
    assert pc.furthest_point_sampling_wrapper(B, N, M, t(xyz, dev), temp, idx) == 1
    np.testing.assert_array_equal(idx.cpu().numpy(), oracle.fps(xyz, M, cuda_mode=True))


def test_extractor_large_cloud_cuda_rules(oracle, dev):
    """PointNet2Msg2 on a 16 384-point cloud pair (its FPS runs the large-cloud kernel), against the oracle's forward with
    the bounds of test_extractor_vs_oracle_other_size_cuda_rules."""
    from oracle import extractor as ox
    from reart_amd.networks.feature_extractor import PointNet2Msg2
    from reart_amd.synthetic import extractor_state, make_sequence

    seq = make_sequence(T=2, n_parts=4, pts_per_part=4096, seed=9, with_flow=False)
    pts = torch.from_numpy(seq["complete"]).float()
    assert pts.shape[1] == 16384
    pts = pts - pts.mean(dim=1, keepdim=True)
    pts = pts / pts.norm(dim=-1).max()
    xyz = pts.permute(0, 2, 1).contiguous()
    model = PointNet2Msg2(out_dim=64)
    sd = extractor_state(model, seed=23)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    got = model(xyz.to(dev), cuda_mode=True).cpu().numpy()
    ref = ox.forward({k: v.numpy() for k, v in sd.items()}, xyz.numpy(), cuda_mode=True)
    err = np.abs(got - ref)
    assert err.max() <= 1e-5 * np.abs(ref).max(), (err.max(), np.abs(ref).max())
    assert err.mean() <= 5e-6 * np.abs(ref).mean()


def test_fps_above_ceiling_raises(dev):
    from reart_amd import _lib
    from reart_amd import pointnet2_cuda as pc
    from reart_amd.networks.pointnet2_utils import farthest_point_sample

    N = (1 << 21) + 1
    assert _lib.FPS_MAX_N == 1 << 21
    xyz = torch.zeros((1, N, 3), device=dev)
    with pytest.raises(NotImplementedError, match=str(1 << 21)):
        farthest_point_sample(xyz, 4, cuda_mode=True)
    idx = torch.zeros((1, 4), dtype=torch.int32, device=dev)
    with pytest.raises(NotImplementedError):
        pc.furthest_point_sampling_wrapper(1, N, 4, xyz, torch.zeros((1, N), device=dev), idx)
