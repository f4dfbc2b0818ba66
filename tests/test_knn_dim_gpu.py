"""GPU parity of the K-nearest search and its backward for points of any dimension D != 3 (csrc/knn_anyd.hip,
knn_bwd_kernel of csrc/knn.hip) against the CPU oracle: bit-exact indices, distances and gradients through knn_points / chamferdist_C / ChamferDistance /
knn_cuda.KNN, the reference's own mutual-nearest-descriptor matches, and the D ceiling."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _clouds(rng, N, P1, P2, D, scale=0.35):
    a = rng.uniform(-scale, scale, (N, P1, D)).astype(np.float32)
    b = rng.uniform(-scale, scale, (N, P2, D)).astype(np.float32)
    return a, b


def _check(out, d_ref, i_ref):
    assert out.idx.dtype == torch.int64 and out.dists.dtype == torch.float32
    np.testing.assert_array_equal(out.idx.cpu().numpy(), i_ref)
    np.testing.assert_array_equal(out.dists.cpu().numpy(), d_ref)


# every D meets K = 1, one K <= 16 and one K > 16
DK = [(1, 1), (1, 16), (1, 200), (2, 1), (2, 5), (2, 1024), (4, 1), (4, 16), (4, 64), (6, 1), (6, 5), (6, 17),
      (7, 1), (7, 16), (7, 200), (16, 1), (16, 5), (16, 64), (33, 1), (33, 16), (33, 17), (64, 1), (64, 5),
      (64, 1024), (128, 1), (128, 16), (128, 64), (256, 1), (256, 5), (256, 200)]


@pytest.mark.parametrize("D,K", DK)
def test_knn_points_dim_bit_exact(oracle, dev, D, K):
    from reart_amd.utils.chamfer import knn_points

    rng = np.random.default_rng(100 * D + K)
    a, b = _clouds(rng, 2, 150, 1100, D)                         # 1100 targets: not a multiple of 64
    d_ref, i_ref = oracle.knn_points(a, b, K=K)
    _check(knn_points(t(a, dev), t(b, dev), K=K), d_ref, i_ref)


# enough query groups for launches with 8 and 4 queries per wave (K = 800: the list LDS caps it at 4), group tails
@pytest.mark.parametrize("N,P1,P2,D,K", [(3, 2777, 900, 64, 1), (8, 4100, 300, 7, 64), (4, 4100, 500, 33, 5),
                                         (8, 4100, 850, 16, 800), (2, 2777, 900, 256, 17)])
def test_knn_points_dim_wide_launch(oracle, dev, N, P1, P2, D, K):
    from reart_amd.utils.chamfer import knn_points

    rng = np.random.default_rng(7 * D + K)
    a, b = _clouds(rng, N, P1, P2, D)
    d_ref, i_ref = oracle.knn_points(a, b, K=K)
    _check(knn_points(t(a, dev), t(b, dev), K=K), d_ref, i_ref)


@pytest.mark.parametrize("D,K", [(2, 17), (5, 5), (64, 200)])
def test_knn_points_dim_k_equals_p2(oracle, dev, D, K):
    from reart_amd.utils.chamfer import knn_points

    rng = np.random.default_rng(D + K)
    a, b = _clouds(rng, 3, 90, K, D)
    d_ref, i_ref = oracle.knn_points(a, b, K=K)
    out = knn_points(t(a, dev), t(b, dev), K=K)
    _check(out, d_ref, i_ref)
    assert (np.sort(out.idx.cpu().numpy(), axis=-1) == np.arange(K)).all()


@pytest.mark.parametrize("D,K", [(6, 5), (6, 33), (64, 5), (64, 33)])
def test_knn_points_dim_ragged(oracle, dev, D, K):
    """Ragged lengths: lengths2 < K (zero-filled slots), an empty query set, a ragged target count."""
    from reart_amd.utils.chamfer import knn_points

    rng = np.random.default_rng(D * K)
    a, b = _clouds(rng, 4, 190, 700, D)
    l1 = np.array([190, 17, 0, 150], np.int64)
    l2 = np.array([700, 3, 600, K - 1], np.int64)
    d_ref, i_ref = oracle.knn_points(a, b, l1, l2, K=K)
    out = knn_points(t(a, dev), t(b, dev), lengths1=t(l1, dev), lengths2=t(l2, dev), K=K)
    _check(out, d_ref, i_ref)
    assert (out.idx[1, :, 3:] == 0).all() and (out.dists[1, :, 3:] == 0).all()
    assert (out.idx[2] == 0).all() and (out.dists[2] == 0).all()


@pytest.mark.parametrize("D", [2, 64])
def test_knn_points_dim_no_targets(dev, D):
    from reart_amd import chamferdist_C

    a = torch.rand((2, 33, D), device=dev)
    idx, dists = chamferdist_C.knn_points_idx(a, torch.empty((2, 0, D), device=dev), None, None, 4)
    assert tuple(idx.shape) == (2, 33, 4)
    assert (idx == 0).all() and (dists == 0).all()


@pytest.mark.parametrize("D,K", [(2, 1), (2, 5), (2, 17), (6, 1), (6, 16), (6, 64), (64, 1), (64, 5), (64, 40)])
def test_knn_points_dim_ties(oracle, dev, D, K):
    """Integer-grid coordinates and every target present twice: exact ties are frequent, the lower index wins."""
    from reart_amd.utils.chamfer import knn_points

    rng = np.random.default_rng(D + 1000 * K)
    levels = {2: 10, 6: 3, 64: 2}[D]
    g = rng.integers(0, levels, (1, 600, D)).astype(np.float32)
    b = np.concatenate([g, g[:, ::-1]], axis=1)                      # 1200 targets, each at least twice
    a = np.concatenate([g[:, :100], rng.integers(0, levels, (1, 100, D)) + 0.5 * rng.integers(0, 2, (1, 100, D))],
                       axis=1).astype(np.float32)
    d_ref, i_ref = oracle.knn_points(a, b, K=K)
    out = knn_points(t(a, dev), t(b, dev), K=K)
    _check(out, d_ref, i_ref)
    d_next, _ = oracle.knn_points(a, b, K=K + 1)
    assert (d_next[..., K] == d_next[..., K - 1]).any()              # some row ties at the K-th slot


@pytest.mark.parametrize("D", [2, 6, 64])
def test_knn_points_backward_dim_bit_exact(oracle, dev, D):
    from reart_amd import chamferdist_C

    rng = np.random.default_rng(D)
    N, P1, P2, K = 3, 1500, 7, 3
    a = rng.uniform(-1, 1, (N, P1, D)).astype(np.float32)
    b = rng.uniform(-1, 1, (N, P2, D)).astype(np.float32)          # 7 targets: ~650 (i, k) pairs per bucket
    l1 = np.array([P1, 900, 0], np.int64)
    l2 = np.array([P2, 5, 2], np.int64)
    _, i_ref = oracle.knn_points(a, b, l1, l2, K=K)
    g = rng.normal(size=(N, P1, K)).astype(np.float32)
    g1_ref, g2_ref = oracle.knn_points_backward(a, b, i_ref, g, l1, l2)
    g1, g2 = chamferdist_C.knn_points_backward(t(a, dev), t(b, dev), t(l1, dev), t(l2, dev), t(i_ref, dev), t(g, dev))
    assert tuple(g1.shape) == (N, P1, D) and tuple(g2.shape) == (N, P2, D)
    np.testing.assert_array_equal(g1.cpu().numpy(), g1_ref)
    np.testing.assert_array_equal(g2.cpu().numpy(), g2_ref)


@pytest.mark.parametrize("D,K", [(2, 4), (6, 1), (64, 20)])
def test_knn_points_dim_autograd(oracle, dev, D, K):
    from reart_amd.utils.chamfer import knn_gather, knn_points

    rng = np.random.default_rng(50 + D)
    a, b = _clouds(rng, 2, 300, 120, D)
    b[:, 60:] = b[:, :60]                                            # repeated targets
    at = t(a, dev).requires_grad_(True)
    bt = t(b, dev).requires_grad_(True)
    out = knn_points(at, bt, K=K, return_nn=True)
    out.dists.sum().backward()
    _, i_ref = oracle.knn_points(a, b, K=K)
    np.testing.assert_array_equal(out.idx.cpu().numpy(), i_ref)
    g1, g2 = oracle.knn_points_backward(a, b, i_ref, np.ones((2, 300, K), np.float32))
    np.testing.assert_array_equal(at.grad.cpu().numpy(), g1)
    np.testing.assert_array_equal(bt.grad.cpu().numpy(), g2)
    assert torch.equal(out.knn, knn_gather(bt.detach(), out.idx))


@pytest.mark.parametrize("D", [2, 6])
def test_chamfer_distance_dim(oracle, dev, D):
    from reart_amd.utils.chamfer import ChamferDistance

    rng = np.random.default_rng(70 + D)
    x, y = _clouds(rng, 2, 500, 500, D)
    d_xy, i_xy = oracle.knn_points(x, y)
    d_yx, i_yx = oracle.knn_points(y, x)
    cd = ChamferDistance()
    xt, yt = t(x, dev), t(y, dev)
    np.testing.assert_array_equal(cd(xt, yt).cpu().numpy(), d_xy[..., 0])
    d, i = cd(xt, yt, return_index=True)
    np.testing.assert_array_equal(d.cpu().numpy(), d_xy[..., 0])
    np.testing.assert_array_equal(i.cpu().numpy(), i_xy[..., 0])
    d, i = cd(xt, yt, reverse=True, return_index=True)
    np.testing.assert_array_equal(d.cpu().numpy(), d_yx[..., 0])
    np.testing.assert_array_equal(i.cpu().numpy(), i_yx[..., 0])
    xg, yg = xt.clone().requires_grad_(True), yt.clone().requires_grad_(True)
    tot, i1, i2 = cd(xg, yg, bidirectional=True, return_index=True)
    np.testing.assert_array_equal(tot.detach().cpu().numpy(), d_xy[..., 0] + d_yx[..., 0])
    np.testing.assert_array_equal(i1.cpu().numpy(), i_xy[..., 0])
    np.testing.assert_array_equal(i2.cpu().numpy(), i_yx[..., 0])
    tot.sum().backward()
    ones = np.ones((2, 500, 1), np.float32)
    gx_f, gy_f = oracle.knn_points_backward(x, y, i_xy, ones)
    gy_b, gx_b = oracle.knn_points_backward(y, x, i_yx, ones)
    np.testing.assert_array_equal(xg.grad.cpu().numpy(), gx_f + gx_b)
    np.testing.assert_array_equal(yg.grad.cpu().numpy(), gy_f + gy_b)


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("D,k", [(64, 1), (64, 24), (128, 1), (128, 8)])
def test_knn_cuda_dim(oracle, dev, D, k, squared):
    from reart_amd.knn_cuda import KNN

    rng = np.random.default_rng(D + k + int(squared))
    ref = rng.normal(size=(2, 1333, D)).astype(np.float32)
    qry = rng.normal(size=(2, 401, D)).astype(np.float32)
    qry[:, :20] = ref[:, 100:120]                                  # zero distances
    d_ref, i_ref = oracle.knn_cuda(ref, qry, k, euclidean=not squared)
    d, i = KNN(k=k, transpose_mode=True, squared=squared)(t(ref, dev), t(qry, dev))
    np.testing.assert_array_equal(i.cpu().numpy(), i_ref)
    np.testing.assert_array_equal(d.cpu().numpy(), d_ref)
    d, i = KNN(k=k, transpose_mode=False, squared=squared)(t(ref, dev).transpose(1, 2), t(qry, dev).transpose(1, 2))
    assert tuple(i.shape) == (2, k, 401)
    np.testing.assert_array_equal(i.cpu().numpy(), i_ref.transpose(0, 2, 1))
    np.testing.assert_array_equal(d.cpu().numpy(), d_ref.transpose(0, 2, 1))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_knn_cuda_mutual_descriptor_matches_vs_reference_golden(dev, tag):
    """tests/golden/mnn.npz holds the reference's matching="mnn" pairs on the 64-D descriptors of smnn.npz: a k = 1
    KNN in both directions ([1, 64, n] layout, transpose_mode=False) followed by the mutual filter."""
    from reart_amd.knn_cuda import KNN

    g, m = np.load(os.path.join(GOLDEN, "smnn.npz")), np.load(os.path.join(GOLDEN, "mnn.npz"))
    n = int(m[f"n_{tag}"])
    f1 = t(g[f"d1_{tag}"][:n].T[None], dev)                          # [1, 64, n]
    f2 = t(g[f"d2_{tag}"][:n].T[None], dev)
    knn = KNN(k=1, transpose_mode=False)
    _, i12 = knn(f2, f1)                                             # [1, 1, n]: nearest frame-2 point of each frame-1 point
    _, i21 = knn(f1, f2)
    nn12, nn21 = i12[0, 0], i21[0, 0]
    src = torch.nonzero(nn21[nn12] == torch.arange(n, device=dev))[:, 0]
    np.testing.assert_array_equal(src.cpu().numpy(), m[f"src_{tag}"])
    np.testing.assert_array_equal(nn12[src].cpu().numpy(), m[f"tgt_{tag}"])


def test_knn_dim_above_ceiling_raises(dev):
    from reart_amd import _lib
    from reart_amd.knn_cuda import KNN
    from reart_amd.utils.chamfer import ChamferDistance, knn_points

    x = torch.zeros((1, 50, 257), device=dev)
    assert _lib.MAX_D == 256
    with pytest.raises(NotImplementedError, match="256"):
        knn_points(x, x)
    with pytest.raises(NotImplementedError, match="256"):
        KNN(k=1, transpose_mode=True)(x, x)
    with pytest.raises(NotImplementedError, match="256"):
        KNN(k=1, transpose_mode=False)(x.transpose(1, 2), x.transpose(1, 2))
    with pytest.raises(NotImplementedError, match="256"):
        ChamferDistance()(x, x)
    L = _lib.lib()
    assert L.reart_knn_points_workspace_bytes_d(1, 50, 50, 257, 1) == 0
    assert L.reart_knn_points_workspace_bytes_d(1, 50, 50, 64, 1025) == 0
    assert L.reart_knn_points_workspace_bytes_d(1, 50, 50, 256, 1024) > 0
    for N, P1, P2, K in [(1, 1, 1, 1), (2, 77, 1500, 3), (19, 4096, 4096, 16), (3, 301, 1100, 200), (1, 5, 2000, 1024)]:
        assert L.reart_knn_points_workspace_bytes_d(N, P1, P2, 3, K) == L.reart_knn_points_workspace_bytes(N, P1, P2, K)
