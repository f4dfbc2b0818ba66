"""GPU tests of the public PointNet++ layer classes (reart_amd.networks.pointnet2_utils) and the kernels under them:
max-pooling over any group size, the fused gathered chain for arbitrary shapes (reart_mlp_chain), square_distance, the
extractor with normals.  Goldens: the reference's own classes on CPU (tests/golden/make_golden_pointnet_layers.py)."""
import os

import numpy as np
import pytest
import torch

from tests.golden.make_golden_pointnet_layers import SEEDS

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("cpu_rules")]   # goldens follow the CPU-fallback rules
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def seeded(module, seed, dev):
    from reart_amd.synthetic import extractor_state

    module.load_state_dict(extractor_state(module, seed=seed), strict=True)
    return module.to(dev).eval()


def close_intermediate(got, ref, what):
    """intermediate levels: the tolerance tests/test_extractor_gpu.py holds l1_points / l2_points to"""
    got = got.cpu().numpy()
    print(f"\n[{what}] max abs error {np.abs(got - ref).max():.3e} (max |ref| {np.abs(ref).max():.3e})")
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4)


def close_final(got, ref, what):
    """final features: the bound tests/test_extractor_gpu.py holds the descriptors to"""
    err = np.abs(got.cpu().numpy() - ref)
    print(f"\n[{what}] max error {err.max() / np.abs(ref).max():.3e} of the scale, mean {err.mean() / np.abs(ref).mean():.3e} of the mean magnitude")
    assert err.max() <= 2e-5 * np.abs(ref).max(), (what, err.max(), np.abs(ref).max())
    assert err.mean() <= 5e-6 * np.abs(ref).mean(), (what, err.mean(), np.abs(ref).mean())


def ball(radius, K, xyz_cf, new_xyz_cf):
    """the grouping indices a class used, from channel-first coordinates"""
    from reart_amd.networks.pointnet2_utils import query_ball_point

    return query_ball_point(radius, K, xyz_cf.permute(0, 2, 1).contiguous(), new_xyz_cf.permute(0, 2, 1).contiguous()).cpu().numpy()


# ------------------------------------------------------------------------------------------------ kernels

@pytest.mark.parametrize("pool_k", [1, 16, 24, 100, 128, 384])
def test_pooling_over_any_group_size_is_the_max_of_the_unpooled_rows(dev, pool_k):
    """The pooled call equals the group-wise maximum of the rows the un-pooled call writes, bit for bit, and writes
    nothing outside its columns -- plain and gathered input, narrow and seven-accumulator layers, with and without ReLU."""
    from reart_amd.networks.feature_extractor import mlp_layer

    rng = np.random.default_rng(pool_k)
    for groups, cin, cout, relu in ((7, 19, 70, True), (3, 131, 200, False), (11, 6, 32, True)):
        rows = groups * pool_k
        X = t(rng.normal(size=(rows, cin)).astype(np.float32), dev)
        W = t((rng.normal(size=(cin, cout)) + np.arange(cout)[None, :] * 0.01).astype(np.float32), dev)
        b = t(rng.normal(size=cout).astype(np.float32), dev)
        plain = mlp_layer(X, W, b, relu=relu)
        want = plain.reshape(groups, pool_k, cout).amax(dim=1)
        out = torch.full((groups, cout + 5), -7.0, device=dev)
        mlp_layer(X, W, b, relu=relu, pool_k=pool_k, out=out, out_col=3)
        assert torch.equal(out[:, 3:3 + cout], want), (pool_k, groups, cin, cout)
        assert torch.equal(out[:, :3], torch.full((groups, 3), -7.0, device=dev))
        assert torch.equal(out[:, 3 + cout:], torch.full((groups, 2), -7.0, device=dev))
    # gathered rows: group_all over pool_k points ([xyz | F]) and ball-query groups ([F | xyz - centre])
    B, Npts, S, D = 2, 50, 3, 5
    F = t(rng.normal(size=(B * Npts, D)).astype(np.float32), dev)
    Q = t(rng.normal(size=(B * Npts, 3)).astype(np.float32), dev)
    C = t(rng.normal(size=(B * S, 3)).astype(np.float32), dev)
    idx = t(rng.integers(0, Npts, (B, S, pool_k)), dev)
    W = t(rng.normal(size=(D + 3, 40)).astype(np.float32), dev)
    b = t(rng.normal(size=40).astype(np.float32), dev)
    for xyz_first in (0, 1):
        g = dict(idx=idx, F=F, Q=Q, C=None if xyz_first else C, Npts=Npts, xyz_first=xyz_first)
        want = mlp_layer(None, W, b, gather=g).reshape(B * S, pool_k, 40).amax(dim=1)
        assert torch.equal(mlp_layer(None, W, b, gather=g, pool_k=pool_k), want), (pool_k, xyz_first)


CHAIN_WIDTHS = ((32, 32, 64), (64, 96, 128), (128, 196, 256), (256, 256, 256), (160, 132, 192), (64, 64, 128), (32, 4, 32))


@pytest.mark.parametrize("D", [0, 3, 6, 131, 320])
def test_fused_chain_equals_three_layer_launches(dev, D):
    """reart_mlp_chain against three reart_mlp_layer launches, bit for bit: K in {16, 32, 64, 128}, both column orders, with and
    without centres, widths that exercise each layout of the kernel (no layer above 128 columns; a wide layer with all 128
    rows in flight; the widest hidden layers with 64); and float64 on the host."""
    from reart_amd import _lib
    from reart_amd.networks import feature_extractor as fe

    rng = np.random.default_rng(100 + D)
    B, Npts = 2, 200
    n = 0
    for K in (16, 32, 64, 128):
        for xyz_first in (0, 1):
            S = (128 // K) * 3
            for widths in (CHAIN_WIDTHS[n % len(CHAIN_WIDTHS)], CHAIN_WIDTHS[(n + 3) % len(CHAIN_WIDTHS)]):
                n += 1
                F = None if D == 0 else t(rng.normal(size=(B * Npts, D)).astype(np.float32), dev)
                Q = t(rng.normal(size=(B * Npts, 3)).astype(np.float32), dev)
                C = None if (xyz_first and n % 2) else t(rng.normal(size=(B * S, 3)).astype(np.float32), dev)
                idx = t(rng.integers(0, Npts, (B, S, K)), dev)
                folded, cin = [], D + 3
                for cout in widths:
                    folded.append((t((rng.normal(size=(cin, cout)) * np.sqrt(2.0 / cin)).astype(np.float32), dev),
                                   t(rng.normal(0, 0.1, cout).astype(np.float32), dev)))
                    cin = cout
                g = dict(idx=idx, F=F, Q=Q, C=C, Npts=Npts, xyz_first=xyz_first)
                C3 = widths[2]
                got = torch.full((B * S, C3 + 7), -3.0, device=dev)
                if not fe.chain_serves(D, K, widths, B * S * K, xyz_first):
                    # a shape the older kernels own: the new entry point refuses it
                    with pytest.raises(_lib.ReartHipError, match="unsupported"):
                        fe.mlp_chain(folded, g, got, 5)
                    continue
                h = fe.mlp_layer(None, *folded[0], gather=g)
                h = fe.mlp_layer(h, *folded[1])
                ref = torch.full((B * S, C3 + 7), -3.0, device=dev)
                fe.mlp_layer(h, *folded[2], pool_k=K, out=ref, out_col=5)
                fe.mlp_chain(folded, g, got, 5)
                assert torch.equal(got, ref), (D, K, xyz_first, widths, float((got - ref).abs().max()))
                if n % 4 == 0:
                    Qg = Q.cpu().numpy().reshape(B, Npts, 3)[np.arange(B)[:, None, None], idx.cpu().numpy()]
                    if C is not None:
                        Qg = Qg - C.cpu().numpy().reshape(B, S, 1, 3)
                    parts = [Qg]
                    if D:
                        Fg = F.cpu().numpy().reshape(B, Npts, D)[np.arange(B)[:, None, None], idx.cpu().numpy()]
                        parts = [Qg, Fg] if xyz_first else [Fg, Qg]
                    X = np.concatenate(parts, -1).reshape(-1, D + 3).astype(np.float64)
                    for W, bvec in folded:
                        X = np.maximum(X @ W.cpu().numpy().astype(np.float64) + bvec.cpu().numpy(), 0)
                    want = X.reshape(B * S, K, C3).max(1)
                    np.testing.assert_allclose(got[:, 5:5 + C3].cpu().numpy(), want, rtol=5e-5, atol=5e-5 * np.abs(want).max())


def test_the_extractors_scales_stay_with_their_kernels(dev):
    """A shape reart_mlp_chain3 / reart_mlp_chain3_wide takes never reaches the new kernel: the predicate says no, the entry
    point returns REART_ERR_UNSUPPORTED, and the routing of the layer classes still picks the old kernels."""
    from reart_amd import _lib
    from reart_amd.networks import feature_extractor as fe

    for D, (C1, C2, C3, K) in [(3, w) for w in sorted(fe.CHAIN3)] + [(320, w) for w in sorted(fe.CHAIN3_WIDE)]:
        assert not fe.chain_serves(D, K, (C1, C2, C3), 1024, 0)
        assert fe.chain_serves(D + 2, K, (C1, C2, C3), 1024, 0) and fe.chain_serves(D, K, (C1, C2, C3), 1024, 1)   # their neighbours are served
    called = []
    old3, oldw, oldc = fe.mlp_chain3, fe.mlp_chain3_wide, fe.mlp_chain
    fe.mlp_chain3 = lambda *a: (called.append("chain3"), old3(*a))[1]
    fe.mlp_chain3_wide = lambda *a: (called.append("wide"), oldw(*a))[1]
    fe.mlp_chain = lambda *a: (called.append("chain"), oldc(*a))[1]
    try:
        g = np.load(os.path.join(G, "extractor.npz"))
        model = seeded(fe.PointNet2Msg2(out_dim=64), 11, dev)
        model(t(g["xyz"], dev), fps_start=(t(g["start1"], dev), t(g["start2"], dev)))
        assert called == ["chain3"] * 3 + ["wide"] * 2, called
        del called[:]
        a = np.load(os.path.join(G, "pointnet_layers_a.npz"))
        model = seeded(fe.PointNet2Msg2(out_dim=64, normal_channel=True), SEEDS["a"], dev)
        model(t(a["xyz6"], dev), fps_start=(t(a["start1"], dev), t(a["start2"], dev)))
        assert called == ["chain"] * 3 + ["wide"] * 2, called      # six feature columns: the new kernel; sa2 as before
    finally:
        fe.mlp_chain3, fe.mlp_chain3_wide, fe.mlp_chain = old3, oldw, oldc
    assert _lib.lib().reart_mlp_chain_serves(3, 32, 32, 32, 64, 1024, 0) == 0


def test_square_distance_bits_and_other_dimensions(dev):
    from reart_amd.networks.pointnet2_utils import square_distance

    g = np.load(os.path.join(G, "pointnet_layers_de.npz"))
    pts = t(g["xyz"], dev).permute(0, 2, 1).contiguous()
    got = square_distance(pts[:, :300].contiguous(), pts[:, 300:500].contiguous())
    np.testing.assert_array_equal(got.cpu().numpy(), g["sq_dist"])           # every bit
    rng = np.random.default_rng(4)
    a, b = rng.normal(size=(2, 40, 5)).astype(np.float32), rng.normal(size=(2, 30, 5)).astype(np.float32)
    want = ((a[:, :, None, :].astype(np.float64) - b[:, None, :, :]) ** 2).sum(-1)
    np.testing.assert_allclose(square_distance(t(a, dev), t(b, dev)).cpu().numpy(), want, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ fixtures A - E

def test_a_extractor_with_normals_matches_reference(dev):
    from reart_amd.networks.feature_extractor import PointNet2Msg2

    g = np.load(os.path.join(G, "pointnet_layers_a.npz"))
    model = PointNet2Msg2(out_dim=64, normal_channel=True)
    assert list(model.state_dict().keys()) == list(g["keys"])
    model = seeded(model, SEEDS["a"], dev)
    xyz6 = t(g["xyz6"], dev)
    s1, s2 = t(g["start1"], dev), t(g["start2"], dev)
    l1_xyz, l1 = model.sa1(xyz6[:, :3].contiguous(), xyz6, fps_start=s1)
    np.testing.assert_array_equal(l1_xyz.cpu().numpy(), g["l1_xyz"])
    for i, (r, K) in enumerate(zip(model.sa1.radius_list, model.sa1.nsample_list)):
        np.testing.assert_array_equal(ball(r, K, xyz6[:, :3], l1_xyz), g[f"idx1_{i}"])
    l2_xyz, l2 = model.sa2(l1_xyz, l1, fps_start=s2)
    np.testing.assert_array_equal(l2_xyz.cpu().numpy(), g["l2_xyz"])
    close_intermediate(l2, g["l2_points"], "A l2_points")
    feat = model(xyz6, fps_start=(s1, s2))
    assert tuple(feat.shape) == (2, 64, 1024)
    close_final(feat, g["feat"], "A feat")
    with pytest.raises(ValueError):
        model(xyz6[:, :3].contiguous())


def b_trunk(dev):
    from reart_amd.networks.pointnet2_utils import PointNetSetAbstraction as SA

    return (seeded(SA(512, 0.2, 24, 3, [64, 64, 128], False), SEEDS["b1"], dev),
            seeded(SA(128, 0.4, 64, 128 + 3, [128, 128, 256], False), SEEDS["b2"], dev),
            seeded(SA(None, None, None, 256 + 3, [256, 512, 1024], True), SEEDS["b3"], dev))


def test_b_single_scale_trunk_matches_reference(dev):
    g = np.load(os.path.join(G, "pointnet_layers_b.npz"))
    sa1, sa2, sa3 = b_trunk(dev)
    assert list(sa1.state_dict().keys()) == list(g["keys1"]) and list(sa3.state_dict().keys()) == list(g["keys3"])
    xyz = t(g["xyz"], dev)
    l1_xyz, l1 = sa1(xyz, None, fps_start=t(g["start1"], dev))
    np.testing.assert_array_equal(l1_xyz.cpu().numpy(), g["l1_xyz"])
    np.testing.assert_array_equal(ball(0.2, 24, xyz, l1_xyz), g["idx1"])
    close_intermediate(l1, g["l1_points"], "B l1_points")
    l2_xyz, l2 = sa2(l1_xyz, l1, fps_start=t(g["start2"], dev))
    np.testing.assert_array_equal(l2_xyz.cpu().numpy(), g["l2_xyz"])
    np.testing.assert_array_equal(ball(0.4, 64, l1_xyz, l2_xyz), g["idx2"])
    close_intermediate(l2, g["l2_points"], "B l2_points")
    l3_xyz, l3 = sa3(l2_xyz, l2)
    np.testing.assert_array_equal(l3_xyz.cpu().numpy(), g["l3_xyz"])
    assert tuple(l3.shape) == (2, 1024, 1)
    close_final(l3, g["l3_points"], "B group_all over 128 points")
    _, l3s = sa3(l2_xyz[:, :, :100].contiguous(), l2[:, :, :100].contiguous())
    close_final(l3s, g["l3_points_100"], "B group_all over 100 points")


def c_msg(dev):
    from reart_amd.networks.pointnet2_utils import PointNetSetAbstractionMsg as Msg

    return seeded(Msg(512, [0.1, 0.2, 0.4], [16, 32, 128], 0, [[32, 32, 64], [64, 64, 128], [64, 96, 128]]), SEEDS["c"], dev)


def test_c_multi_scale_without_features_matches_reference(dev):
    g = np.load(os.path.join(G, "pointnet_layers_c.npz"))
    msg = c_msg(dev)
    assert list(msg.state_dict().keys()) == list(g["keys"])
    xyz = t(g["xyz"], dev)
    new_xyz, new_points = msg(xyz, None, fps_start=t(g["start"], dev))
    np.testing.assert_array_equal(new_xyz.cpu().numpy(), g["new_xyz"])
    for i, (r, K) in enumerate(zip([0.1, 0.2, 0.4], [16, 32, 128])):
        np.testing.assert_array_equal(ball(r, K, xyz, new_xyz), g[f"idx_{i}"])
    assert tuple(new_points.shape) == (2, 320, 512)
    close_final(new_points, g["new_points"], "C new_points")


def d_layers(dev):
    from reart_amd.networks.pointnet2_utils import PointNetFeaturePropagation as FP

    return (seeded(FP(24 + 40, [64, 32]), SEEDS["d1"], dev), seeded(FP(40, [64, 32]), SEEDS["d2"], dev),
            seeded(FP(20 + 52, [96, 48]), SEEDS["d3"], dev))


def d_inputs(g, dev):
    l1, l2, l3 = t(g["l1_xyz"], dev), t(g["l2_xyz"], dev), t(g["l3_xyz"], dev)
    return ((l2, l3, t(g["d1_points1"], dev), t(g["d1_points2"], dev)), (l1, l2, None, t(g["d2_points2"], dev)),
            (l1, l2, t(g["d3_points1"], dev), t(g["d3_points2"], dev)))


def test_d_feature_propagation_three_ways_matches_reference(dev):
    g = np.load(os.path.join(G, "pointnet_layers_de.npz"))
    layers = d_layers(dev)
    assert list(layers[2].state_dict().keys()) == list(g["keys_fp"])
    for fp, args, name in zip(layers, d_inputs(g, dev), ("d1", "d2", "d3")):
        close_final(fp(*args), g[name + "_out"], "D " + name)


def test_e_grouping_functions_match_reference(dev):
    from reart_amd.networks import pointnet2_utils as pu

    g = np.load(os.path.join(G, "pointnet_layers_de.npz"))
    pts = t(g["xyz"], dev).permute(0, 2, 1).contiguous()
    feats = t(g["e_points"], dev)
    new_xyz, new_points, grouped_xyz, fps_idx = pu.sample_and_group(64, 0.3, 16, pts, feats, returnfps=True, fps_start=t(g["e_start"], dev))
    np.testing.assert_array_equal(fps_idx.cpu().numpy(), g["sg_fps_idx"])
    np.testing.assert_array_equal(new_xyz.cpu().numpy(), g["sg_new_xyz"])
    np.testing.assert_array_equal(grouped_xyz.cpu().numpy(), g["sg_grouped_xyz"])
    np.testing.assert_array_equal(new_points.cpu().numpy(), g["sg_new_points"])
    two = pu.sample_and_group(64, 0.3, 16, pts, feats, fps_start=t(g["e_start"], dev))
    assert len(two) == 2 and torch.equal(two[0], new_xyz) and torch.equal(two[1], new_points)
    none = pu.sample_and_group(64, 0.3, 16, pts, None, fps_start=t(g["e_start"], dev))
    assert torch.equal(none[1], new_points[..., :3])
    a_xyz, a_points = pu.sample_and_group_all(pts[:, :100].contiguous(), feats[:, :100].contiguous())
    np.testing.assert_array_equal(a_xyz.cpu().numpy(), g["sga_new_xyz"])
    np.testing.assert_array_equal(a_points.cpu().numpy(), g["sga_new_points"])
    assert tuple(pu.sample_and_group_all(pts, None)[1].shape) == (2, 1, 1024, 3)


# ------------------------------------------------------------------------------------------------ identities

def test_every_class_gives_the_same_bits_fused_and_layer_by_layer(dev):
    from reart_amd.networks import feature_extractor as fe

    b, c, a = (np.load(os.path.join(G, f"pointnet_layers_{n}.npz")) for n in "bca")
    sa1, sa2, sa3 = b_trunk(dev)
    msg = c_msg(dev)
    ext = seeded(fe.PointNet2Msg2(out_dim=64, normal_channel=True), SEEDS["a"], dev)
    xyz = t(b["xyz"], dev)

    def everything():
        l1_xyz, l1 = sa1(xyz, None, fps_start=t(b["start1"], dev))
        l2_xyz, l2 = sa2(l1_xyz, l1, fps_start=t(b["start2"], dev))
        outs = [l1, l2, sa3(l2_xyz, l2)[1], sa3(l2_xyz[:, :, :64].contiguous(), l2[:, :, :64].contiguous())[1]]
        outs.append(msg(xyz, None, fps_start=t(c["start"], dev))[1])
        outs.append(ext(t(a["xyz6"], dev), fps_start=(t(a["start1"], dev), t(a["start2"], dev))))
        return outs

    fused = everything()
    fe.FUSE_CHAIN = False
    try:
        plain = everything()
    finally:
        fe.FUSE_CHAIN = True
    for i, (x, y) in enumerate(zip(fused, plain)):
        assert torch.equal(x, y), i


def test_extractor_without_normals_keeps_its_outputs(dev):
    """PointNet2Msg2(normal_channel=False), now built from the public classes, against the parent's fixture: the sampled
    coordinates exactly, the features within extractor.npz's existing tolerances."""
    from reart_amd.networks.feature_extractor import PointNet2Msg2

    g = np.load(os.path.join(G, "extractor.npz"))
    model = seeded(PointNet2Msg2(out_dim=64), 11, dev)
    xyz = t(g["xyz"], dev)
    l1_xyz, l1 = model.sa1(xyz, xyz, fps_start=t(g["start1"], dev))
    np.testing.assert_array_equal(l1_xyz.cpu().numpy(), g["l1_xyz"])
    np.testing.assert_allclose(l1.cpu().numpy(), g["l1_points"], rtol=1e-4, atol=1e-4)
    l2_xyz, l2 = model.sa2(l1_xyz, l1, fps_start=t(g["start2"], dev))
    np.testing.assert_array_equal(l2_xyz.cpu().numpy(), g["l2_xyz"])
    np.testing.assert_allclose(l2.cpu().numpy(), g["l2_points"], rtol=1e-4, atol=1e-4)
    close_final(model(xyz, fps_start=(t(g["start1"], dev), t(g["start2"], dev))), g["feat"], "extractor, no normals")


def composed(convs, bns, gather, K):
    """one mlp_layer launch per layer over the gathered rows, the last one pooled: the operators tested on their own"""
    from reart_amd.networks import feature_extractor as fe

    h = None
    for j, (conv, bn) in enumerate(zip(convs, bns)):
        Wt, bias = fe._fold_now(conv, bn)
        h = fe.mlp_layer(h, Wt, bias, gather=gather if j == 0 else None, pool_k=K if j == len(convs) - 1 else 0)
    return h


def test_cuda_rules_equal_the_composition_of_the_operators(dev):
    """The reference cannot run its CUDA rules here: each class under cuda_mode=True is held, bit for bit, to
    farthest_point_sample -> query_ball_point -> mlp_layer per layer, which are tested separately under those rules."""
    from reart_amd.networks import pointnet2_utils as pu

    b = np.load(os.path.join(G, "pointnet_layers_b.npz"))
    xyz = t(b["xyz"], dev)
    pts = xyz.permute(0, 2, 1).contiguous()
    B, N, _ = pts.shape
    feats = t(np.random.default_rng(2).normal(size=(B, 7, N)).astype(np.float32), dev)
    F = feats.permute(0, 2, 1).contiguous().reshape(B * N, 7)
    sa1, _, sa3 = b_trunk(dev)
    msg = c_msg(dev)
    # single scale, points=None: [xyz - centre]
    new_xyz, out = sa1(xyz, None, cuda_mode=True)
    fps = pu.farthest_point_sample(pts, 512, cuda_mode=True)
    assert int(fps[0, 0]) == 0 and int(fps[1, 0]) == 0
    centres = pu.index_points(pts, fps).contiguous()
    assert torch.equal(new_xyz, centres.permute(0, 2, 1))
    idx = pu.query_ball_point(0.2, 24, pts, centres, cuda_mode=True)
    want = composed(sa1.mlp_convs, sa1.mlp_bns, dict(idx=idx, F=None, Q=pts.reshape(B * N, 3), C=centres.reshape(-1, 3), Npts=N, xyz_first=1), 24)
    assert torch.equal(out, want.reshape(B, 512, -1).permute(0, 2, 1))
    # multi scale, points=None: [xyz - centre] per scale, side by side
    new_xyz, out = msg(xyz, None, cuda_mode=True)
    assert torch.equal(new_xyz, centres.permute(0, 2, 1))
    cols = []
    for i, (r, K) in enumerate(zip(msg.radius_list, msg.nsample_list)):
        idx = pu.query_ball_point(r, K, pts, centres, cuda_mode=True)
        cols.append(composed(msg.conv_blocks[i], msg.bn_blocks[i],
                             dict(idx=idx, F=None, Q=pts.reshape(B * N, 3), C=centres.reshape(-1, 3), Npts=N, xyz_first=0), K))
    assert torch.equal(out, torch.cat(cols, dim=1).reshape(B, 512, -1).permute(0, 2, 1))
    # with features: Msg puts them first, the single-scale class the coordinates
    msg7 = seeded(pu.PointNetSetAbstractionMsg(128, [0.3], [48], 7, [[32, 48]]), 41, dev)
    sa7 = seeded(pu.PointNetSetAbstraction(128, 0.3, 48, 7 + 3, [32, 48], False), 42, dev)
    fps = pu.farthest_point_sample(pts, 128, cuda_mode=True)
    centres = pu.index_points(pts, fps).contiguous()
    idx = pu.query_ball_point(0.3, 48, pts, centres, cuda_mode=True)
    for layer, convs, bns, first in ((msg7, msg7.conv_blocks[0], msg7.bn_blocks[0], 0), (sa7, sa7.mlp_convs, sa7.mlp_bns, 1)):
        want = composed(convs, bns, dict(idx=idx, F=F, Q=pts.reshape(B * N, 3), C=centres.reshape(-1, 3), Npts=N, xyz_first=first), 48)
        assert torch.equal(layer(xyz, feats, cuda_mode=True)[1], want.reshape(B, 128, -1).permute(0, 2, 1))
    # group_all samples nothing: the two rule sets agree
    l2_xyz, l2 = t(b["l2_xyz"], dev), t(b["l2_points"], dev)
    assert torch.equal(sa3(l2_xyz, l2, cuda_mode=True)[1], sa3(l2_xyz, l2, cuda_mode=False)[1])


def test_checkpoints_training_mode_and_host_tensors(dev):
    from reart_amd.networks import pointnet2_utils as pu
    from reart_amd.networks.feature_extractor import PointNet2Msg2, rec_freeze
    from reart_amd.synthetic import extractor_state

    layers = [pu.PointNetSetAbstraction(16, 0.3, 16, 3, [32, 32, 64], False), pu.PointNetSetAbstraction(None, None, None, 3, [32], True),
              pu.PointNetSetAbstractionMsg(16, [0.2, 0.3], [16, 32], 0, [[32, 32, 64], [32, 32]]), pu.PointNetFeaturePropagation(8, [16])]
    prefixes = [{"mlp_convs", "mlp_bns"}, {"mlp_convs", "mlp_bns"}, {"conv_blocks", "bn_blocks"}, {"mlp_convs", "mlp_bns"}]
    xyz = torch.rand(2, 3, 64)
    for layer, names in zip(layers, prefixes):
        assert {k.split(".")[0] for k in layer.state_dict()} == names
        sd = extractor_state(layer, seed=3)
        layer.load_state_dict(sd, strict=True)
        assert all(torch.equal(v, sd[k]) for k, v in layer.state_dict().items())
    args = [(xyz, None), (xyz, None), (xyz, None), (xyz, xyz[:, :, :16].contiguous(), None, torch.rand(2, 8, 16))]
    for layer, a in zip(layers, args):
        layer.eval()
        with pytest.raises(RuntimeError, match="no CPU fallback"):       # host tensors, as every other operator
            layer(*a)
        layer.to(dev).train()
        with pytest.raises(RuntimeError, match="inference-only"):
            layer(*[None if x is None else x.to(dev) for x in a])
        layer.eval()
        out = layer(*[None if x is None else x.to(dev) for x in a])
        assert torch.isfinite(out[1] if isinstance(out, tuple) else out).all()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pu.square_distance(torch.rand(1, 4, 3), torch.rand(1, 5, 3))
    model = PointNet2Msg2(out_dim=64, normal_channel=True)
    rec_freeze(model)
    assert all(not p.requires_grad for p in model.parameters())
    assert all(m.momentum == 0 for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm))
