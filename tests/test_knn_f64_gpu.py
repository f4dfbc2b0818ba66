"""GPU parity of the float64 K-nearest search (csrc/knn_anyd.hip, reart_knn_points_idx_f64) against the float64 numpy
restatement of its contract (tests/knn_f64_ref.py): bit-exact indices and distances through chamferdist_C /
knn_points / knn_gather / ChamferDistance, orders that only float64 resolves, ties and ragged lengths, wide launches,
gradients through the float32 backward, and the dtype / size errors."""
import numpy as np
import pytest
import torch

from tests.knn_f64_ref import knn_ref

pytestmark = pytest.mark.gpu


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _clouds(rng, N, P1, P2, D, scale=0.35):
    a = rng.uniform(-scale, scale, (N, P1, D))
    b = rng.uniform(-scale, scale, (N, P2, D))
    return a, b


def _check(dists, idx, d_ref, i_ref):
    assert dists.dtype == torch.float64 and idx.dtype == torch.int64
    np.testing.assert_array_equal(idx.cpu().numpy(), i_ref)
    np.testing.assert_array_equal(dists.cpu().numpy(), d_ref)


@pytest.mark.parametrize("K", [1, 3, 16, 17, 200, 1024])
@pytest.mark.parametrize("D", [1, 2, 3, 7, 64, 256])
def test_knn_f64_bit_exact(dev, D, K):
    from reart_amd.utils.chamfer import knn_points

    rng = np.random.default_rng(1000 * D + K)
    a, b = _clouds(rng, 2, 150, 1100, D)                          # 1100 targets: not a multiple of 64
    d_ref, i_ref = knn_ref(a, b, K)
    out = knn_points(t(a, dev), t(b, dev), K=K)
    _check(out.dists, out.idx, d_ref, i_ref)


@pytest.mark.parametrize("D,K", [(1, 1), (3, 16), (64, 100)])
def test_knn_f64_resolves_what_float32_merges(dev, D, K):
    """Targets at x = 1 + delta_j with delta_j < 2^-25 descending in j: in float32 every distance rounds to 1 and the
    lowest indices win; in float64 the order is reversed.  A search that casts to float32 fails here."""
    from reart_amd import chamferdist_C

    P2 = 100
    a = np.zeros((1, 5, D))
    b = np.zeros((1, P2, D))
    b[0, :, 0] = 1.0 + (P2 - np.arange(P2)) * 2.0 ** -40
    d64, i64 = knn_ref(a, b, K)
    d32, i32 = knn_ref(a.astype(np.float32), b.astype(np.float32), K)
    assert not np.array_equal(i32, i64)
    assert (i64[0, :, 0] == P2 - 1).all() and (i32[0, :, 0] == 0).all()
    idx, dists = chamferdist_C.knn_points_idx(t(a, dev), t(b, dev), None, None, K)
    _check(dists, idx, d64, i64)


@pytest.mark.parametrize("D,K", [(3, 5), (3, 40), (16, 33), (64, 1024)])
def test_knn_f64_ties_and_ragged(dev, D, K):
    """Duplicate targets and exact distance ties go to the lower index; lengths1 / lengths2 of 0, below K and full;
    rows and slots past them are zero."""
    from reart_amd.utils.chamfer import knn_points

    rng = np.random.default_rng(D * K)
    P1, P2 = 190, 1100
    a = rng.integers(-4, 5, (4, P1, D)) / 8.0                     # coarse grid: many equal distances
    b = rng.integers(-4, 5, (4, P2, D)) / 8.0
    b[:, 600:900] = b[:, 0:300]                                   # duplicated targets
    l1 = np.array([P1, 17, 0, P1 - 5], np.int64)
    l2 = np.array([P2, K - 1, P2 - 7, 0], np.int64)
    d_ref, i_ref = knn_ref(a, b, K, l1, l2)
    out = knn_points(t(a, dev), t(b, dev), t(l1, dev), t(l2, dev), K=K)
    _check(out.dists, out.idx, d_ref, i_ref)
    d, i = out.dists.cpu().numpy(), out.idx.cpu().numpy()
    assert (d[1, :, K - 1:] == 0).all() and (i[1, :, K - 1:] == 0).all()     # slots past lengths2 < K
    assert (d[1, 17:] == 0).all() and (i[1, 17:] == 0).all()                 # rows past lengths1
    assert (d[2] == 0).all() and (i[2] == 0).all()                           # lengths1 = 0
    assert (d[3] == 0).all() and (i[3] == 0).all()                           # lengths2 = 0
    # a duplicated target (600 + m) only ever follows its original m
    for row in i[0]:
        for k, j in enumerate(row):
            if 600 <= j < 900:
                assert j - 600 in row[:k]


@pytest.mark.parametrize("D,K", [(2, 100), (64, 1024)])
def test_knn_f64_k_above_p2(dev, D, K):
    from reart_amd.utils.chamfer import knn_points

    rng = np.random.default_rng(D + K)
    a, b = _clouds(rng, 2, 70, 70, D)
    d_ref, i_ref = knn_ref(a, b, K)
    out = knn_points(t(a, dev), t(b, dev), K=K)
    _check(out.dists, out.idx, d_ref, i_ref)
    assert (out.dists[..., 70:] == 0).all() and (out.idx[..., 70:] == 0).all()
    assert (np.sort(out.idx[..., :70].cpu().numpy(), axis=-1) == np.arange(70)).all()


@pytest.mark.parametrize("D,K", [(3, 1), (3, 64), (64, 17), (256, 1024)])
def test_knn_f64_wide_launch(dev, D, K):
    """N = 8, P1 = 4100: full query groups of 8 and 4 and a tail, and K = 1024 (two queries per wave)."""
    from reart_amd import chamferdist_C

    rng = np.random.default_rng(7 * D + K)
    a, b = _clouds(rng, 8, 4100, 4096, D)
    rows = np.concatenate([np.arange(64), np.sort(rng.choice(np.arange(64, 4030), 64, replace=False)),
                           np.arange(4030, 4100)])
    d_ref, i_ref = knn_ref(a, b, K, rows=rows)
    idx, dists = chamferdist_C.knn_points_idx(t(a, dev), t(b, dev), None, None, K)
    _check(dists[:, rows], idx[:, rows], d_ref, i_ref)


@pytest.mark.parametrize("D", [3, 7])
def test_chamfer_f64(dev, D):
    from reart_amd.utils.chamfer import ChamferDistance, knn_points

    rng = np.random.default_rng(D)
    a, b = _clouds(rng, 2, 300, 300, D)
    ta, tb = t(a, dev), t(b, dev)
    d_f, i_f = knn_ref(a, b, 1)
    d_b, i_b = knn_ref(b, a, 1)
    cd = ChamferDistance()
    d, i = cd(ta, tb, return_index=True)
    _check(d, i, d_f[..., 0], i_f[..., 0])
    d, i = cd(ta, tb, reverse=True, return_index=True)
    _check(d, i, d_b[..., 0], i_b[..., 0])
    tot, i1, i2 = cd(ta, tb, bidirectional=True, return_index=True)
    _check(tot, i1, d_f[..., 0] + d_b[..., 0], i_f[..., 0])
    np.testing.assert_array_equal(i2.cpu().numpy(), i_b[..., 0])

    out = knn_points(ta, tb, K=5, return_nn=True)
    d5, i5 = knn_ref(a, b, 5)
    _check(out.dists, out.idx, d5, i5)
    assert out.knn.dtype == torch.float64
    np.testing.assert_array_equal(out.knn.cpu().numpy(), b[np.arange(2)[:, None, None], i5])


def test_chamfer_f64_autograd(dev):
    """Gradients reach float64 clouds through the float32 backward (as upstream) and come back as float64."""
    from reart_amd import chamferdist_C
    from reart_amd.utils.chamfer import ChamferDistance

    rng = np.random.default_rng(5)
    a, b = _clouds(rng, 2, 400, 400, 3)
    a64 = t(a, dev).requires_grad_(True)
    b64 = t(b, dev).requires_grad_(True)
    ChamferDistance()(a64, b64, bidirectional=True).sum().backward()
    assert a64.grad.dtype == torch.float64 and b64.grad.dtype == torch.float64

    af, bf = a64.detach().float(), b64.detach().float()
    i_ab, _ = chamferdist_C.knn_points_idx(a64.detach(), b64.detach(), None, None, 1)
    i_ba, _ = chamferdist_C.knn_points_idx(b64.detach(), a64.detach(), None, None, 1)
    ones = torch.ones((2, 400, 1), dtype=torch.float32, device=dev)
    ga_f, gb_f = chamferdist_C.knn_points_backward(af, bf, None, None, i_ab, ones)
    gb_b, ga_b = chamferdist_C.knn_points_backward(bf, af, None, None, i_ba, ones)
    assert torch.equal(a64.grad, ga_f.double() + ga_b.double())
    assert torch.equal(b64.grad, gb_f.double() + gb_b.double())


def test_knn_f64_errors(dev):
    from reart_amd import chamferdist_C
    from reart_amd.utils.chamfer import ChamferDistance, knn_points

    a64 = torch.rand((1, 20, 3), dtype=torch.float64, device=dev)
    a32 = a64.float()
    with pytest.raises(TypeError):
        knn_points(a64, a32)
    with pytest.raises(TypeError):
        chamferdist_C.knn_points_idx(a32, a64, None, None, 1)
    with pytest.raises(TypeError):
        ChamferDistance()(a32, a64)
    with pytest.raises(TypeError):
        knn_points(a64.half(), a64.half())
    with pytest.raises(TypeError):
        knn_points(a64.bfloat16(), a64.bfloat16())
    w = torch.rand((1, 20, 257), dtype=torch.float64, device=dev)
    with pytest.raises(NotImplementedError):
        knn_points(w, w)
    with pytest.raises(NotImplementedError):
        knn_points(a64, torch.rand((1, 1100, 3), dtype=torch.float64, device=dev), K=1025)
    idx, _ = chamferdist_C.knn_points_idx(a64, a64, None, None, 1)
    g = torch.ones((1, 20, 1), dtype=torch.float64, device=dev)
    with pytest.raises(TypeError):
        chamferdist_C.knn_points_backward(a64, a64, None, None, idx, g)
    with pytest.raises(TypeError):
        chamferdist_C.knn_points_backward(a32, a32, None, None, idx, g)
