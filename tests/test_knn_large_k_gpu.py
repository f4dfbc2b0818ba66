"""GPU parity of the K-nearest search for 16 < K <= 1024 (csrc/knn_list.hip) against the CPU oracle: bit-exact
indices and distances through knn_points / chamferdist_C / knn_cuda.KNN, the autograd path through the existing
backward, and the new ceiling."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _clouds(rng, N, P1, P2, scale=0.35):
    a = rng.uniform(-scale, scale, (N, P1, 3)).astype(np.float32)
    b = rng.uniform(-scale, scale, (N, P2, 3)).astype(np.float32)
    return a, b


def _check(out, d_ref, i_ref):
    assert out.idx.dtype == torch.int64 and out.dists.dtype == torch.float32
    np.testing.assert_array_equal(out.idx.cpu().numpy(), i_ref)
    np.testing.assert_array_equal(out.dists.cpu().numpy(), d_ref)


@pytest.mark.parametrize("K", [17, 24, 33, 64, 200, 1024])
@pytest.mark.parametrize("N,P1,P2", [(1, 77, 1500), (3, 301, 1100)])
def test_knn_points_large_k_bit_exact(oracle, dev, N, P1, P2, K):
    from reart_amd.utils.chamfer import knn_points

    rng = np.random.default_rng(1000 * N + K)
    a, b = _clouds(rng, N, P1, P2)
    d_ref, i_ref = oracle.knn_points(a, b, K=K)
    _check(knn_points(t(a, dev), t(b, dev), K=K), d_ref, i_ref)


@pytest.mark.parametrize("K", [17, 33, 200, 1024])
def test_knn_points_large_k_ragged(oracle, dev, K):
    """Ragged lengths, including lengths2 < K (zero-filled slots) and an empty query row set."""
    from reart_amd.utils.chamfer import knn_points

    rng = np.random.default_rng(K)
    a, b = _clouds(rng, 4, 190, 1300)
    l1 = np.array([190, 17, 0, 150], np.int64)
    l2 = np.array([1300, 5, 600, K - 1], np.int64)
    d_ref, i_ref = oracle.knn_points(a, b, l1, l2, K=K)
    out = knn_points(t(a, dev), t(b, dev), lengths1=t(l1, dev), lengths2=t(l2, dev), K=K)
    _check(out, d_ref, i_ref)
    assert (out.idx[1, :, 5:] == 0).all() and (out.dists[1, :, 5:] == 0).all()


@pytest.mark.parametrize("K", [17, 64, 200, 1024])
def test_knn_points_large_k_ties(oracle, dev, K):
    """A lattice with many exact distance ties and every target duplicated: ties keep the lower index."""
    from reart_amd.utils.chamfer import knn_points

    rng = np.random.default_rng(40 + K)
    g = np.stack(np.meshgrid(*[np.arange(10, dtype=np.float32) * 0.125] * 3, indexing="ij"), -1).reshape(1, -1, 3)
    b = np.concatenate([g, g[:, ::-1]], axis=1)                    # 2000 targets, each twice
    a = np.concatenate([g[:, ::7], np.round(rng.uniform(0, 1.2, (1, 60, 3)) * 16) / 16], axis=1).astype(np.float32)
    d_ref, i_ref = oracle.knn_points(a, b, K=K)
    _check(knn_points(t(a, dev), t(b, dev), K=K), d_ref, i_ref)


def test_knn_points_prefix_matches_register_kernel(dev):
    """The first 16 columns of K = 40 (LDS list) equal K = 16 (the existing register-list kernel)."""
    from reart_amd.utils.chamfer import knn_points

    rng = np.random.default_rng(11)
    a, b = _clouds(rng, 2, 513, 2000)
    a, b = t(a, dev), t(b, dev)
    big, small = knn_points(a, b, K=40), knn_points(a, b, K=16)
    assert torch.equal(big.idx[..., :16], small.idx) and torch.equal(big.dists[..., :16], small.dists)


def test_knn_points_large_k_autograd(oracle, dev):
    from reart_amd.utils.chamfer import knn_gather, knn_points

    rng = np.random.default_rng(12)
    a, b = _clouds(rng, 2, 300, 700)
    K = 32
    at = t(a, dev).requires_grad_(True)
    bt = t(b, dev).requires_grad_(True)
    out = knn_points(at, bt, K=K, return_nn=True)
    g = rng.normal(size=(2, 300, K)).astype(np.float32)
    (out.dists * t(g, dev)).sum().backward()
    d_ref, i_ref = oracle.knn_points(a, b, K=K)
    np.testing.assert_array_equal(out.idx.cpu().numpy(), i_ref)
    g1, g2 = oracle.knn_points_backward(a, b, i_ref, g)
    np.testing.assert_allclose(at.grad.cpu().numpy(), g1, rtol=0, atol=1e-6)
    np.testing.assert_allclose(bt.grad.cpu().numpy(), g2, rtol=0, atol=1e-6)
    assert torch.equal(out.knn, knn_gather(bt.detach(), out.idx))


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("k", [17, 64, 200])
def test_knn_cuda_large_k(oracle, dev, k, squared):
    from reart_amd.knn_cuda import KNN

    rng = np.random.default_rng(k + int(squared))
    ref = rng.uniform(-0.3, 0.3, (2, 1777, 3)).astype(np.float32)
    qry = rng.uniform(-0.3, 0.3, (2, 333, 3)).astype(np.float32)
    qry[:, :20] = ref[:, 100:120]                                  # zero distances
    d_ref, i_ref = oracle.knn_cuda(ref, qry, k, euclidean=not squared)
    d, i = KNN(k=k, transpose_mode=True, squared=squared)(t(ref, dev), t(qry, dev))
    np.testing.assert_array_equal(i.cpu().numpy(), i_ref)
    np.testing.assert_array_equal(d.cpu().numpy(), d_ref)
    d, i = KNN(k=k, transpose_mode=False, squared=squared)(t(ref, dev).transpose(1, 2), t(qry, dev).transpose(1, 2))
    assert tuple(i.shape) == (2, k, 333)
    np.testing.assert_array_equal(i.cpu().numpy(), i_ref.transpose(0, 2, 1))
    np.testing.assert_array_equal(d.cpu().numpy(), d_ref.transpose(0, 2, 1))


def test_knn_cuda_large_k_more_than_references(dev):
    from reart_amd import _lib
    from reart_amd.knn_cuda import KNN

    ref = torch.zeros((1, 40, 3), device=dev)
    with pytest.raises(_lib.ReartHipError, match="invalid argument"):
        KNN(k=41, transpose_mode=True)(ref, ref)


def test_knn_k_above_ceiling_raises(dev):
    from reart_amd import _lib
    from reart_amd.knn_cuda import KNN
    from reart_amd.utils.chamfer import knn_points

    x = torch.zeros((1, 2000, 3), device=dev)
    assert _lib.MAX_K_LIST == 1024
    with pytest.raises(NotImplementedError, match="1024"):
        knn_points(x, x, K=1025)
    with pytest.raises(NotImplementedError, match="1024"):
        KNN(k=1025, transpose_mode=True)(x, x)
    assert _lib.lib().reart_knn_points_workspace_bytes(1, 2000, 2000, 1025) == 0
    assert _lib.lib().reart_knn_points_workspace_bytes(1, 2000, 2000, 1024) > 0
