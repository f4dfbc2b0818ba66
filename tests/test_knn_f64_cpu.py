"""Host-side checks of the float64 K-nearest search (no GPU): the numpy restatement the GPU tests compare against agrees
with a plain per-pair brute force, the float64 entry point rejects bad sizes with a status code before any device work,
its workspace query covers the float64 images, and float64 CPU tensors still find no CPU fallback."""
import numpy as np
import pytest
import torch

from tests.knn_f64_ref import knn_ref

INVALID, UNSUPPORTED = -1, -2


def _brute(a, b, K, l1=None, l2=None):
    """One Python float (IEEE double) at a time: d = ((d0*d0) + (d1*d1)) + ..., ranked by the tuple (d, j)."""
    N, P1, D = a.shape
    P2 = b.shape[1]
    dists = np.zeros((N, P1, K))
    idx = np.zeros((N, P1, K), np.int64)
    for n in range(N):
        n1 = P1 if l1 is None else min(int(l1[n]), P1)
        n2 = P2 if l2 is None else min(int(l2[n]), P2)
        for i in range(n1):
            keys = []
            for j in range(n2):
                d = 0.0
                for c in range(D):
                    diff = float(a[n, i, c]) - float(b[n, j, c])
                    d = d + diff * diff
                keys.append((d, j))
            keys.sort()
            for k, (d, j) in enumerate(keys[:K]):
                dists[n, i, k], idx[n, i, k] = d, j
    return dists, idx


@pytest.mark.parametrize("D,K", [(1, 3), (3, 1), (3, 8), (5, 40), (17, 6)])
def test_restatement_matches_brute_force(D, K):
    rng = np.random.default_rng(D * 100 + K)
    a = rng.uniform(-0.35, 0.35, (2, 23, D))
    b = rng.uniform(-0.35, 0.35, (2, 31, D))
    b[:, 20:25] = b[:, 0:5]                                        # exact ties: the lower index first
    l1, l2 = np.array([23, 9]), np.array([31, 4])
    d_ref, i_ref = knn_ref(a, b, K, l1, l2)
    d_bf, i_bf = _brute(a, b, K, l1, l2)
    assert d_ref.dtype == np.float64
    np.testing.assert_array_equal(i_ref, i_bf)
    np.testing.assert_array_equal(d_ref, d_bf)
    rows = np.array([0, 5, 22])
    d_r, i_r = knn_ref(a, b, K, l1, l2, rows=rows, chunk=2)
    np.testing.assert_array_equal(d_r, d_ref[:, rows])
    np.testing.assert_array_equal(i_r, i_ref[:, rows])


def test_restatement_rounds_in_its_dtype():
    """float32 inputs are summed in float32: the targets x = 1 + delta_j (delta_j < 2^-25) all tie there."""
    a = np.zeros((1, 1, 1))
    b = np.zeros((1, 10, 1))
    b[0, :, 0] = 1.0 + (10 - np.arange(10)) * 2.0 ** -40
    d64, i64 = knn_ref(a, b, 3)
    d32, i32 = knn_ref(a.astype(np.float32), b.astype(np.float32), 3)
    assert d32.dtype == np.float32 and (d32 == 1).all() and (i32[0, 0] == [0, 1, 2]).all()
    assert (i64[0, 0] == [9, 8, 7]).all() and (d64 > 1).all()


def test_f64_entry_point_rejects_bad_sizes_without_a_gpu():
    from reart_amd import _lib

    L = _lib.lib()
    for D, K, rc in ((0, 1, INVALID), (3, 0, INVALID), (257, 1, UNSUPPORTED), (3, 1025, UNSUPPORTED)):
        assert L.reart_knn_points_idx_f64(None, None, None, None, 1, 8, 8, D, K, None, None, None, 0, None) == rc
    assert L.reart_knn_points_idx_f64(None, None, None, None, 0, 8, 8, 64, 1, None, None, None, 0, None) == 0


def test_f64_workspace_bytes():
    from reart_amd import _lib

    L = _lib.lib()
    for N, P1, P2, K in [(1, 1, 1, 1), (2, 77, 1500, 3), (8, 4100, 4096, 1024), (1, 5, 2000, 17)]:
        for D in (1, 3, 64, 256):
            # at least the [N, D, P2] target image and the [N, P1, D] query image, in doubles
            assert L.reart_knn_points_workspace_bytes_f64(N, P1, P2, D, K) >= 8 * N * D * (P1 + P2)
    for D, K in ((0, 1), (257, 1), (3, 0), (3, 1025)):
        assert L.reart_knn_points_workspace_bytes_f64(1, 50, 50, D, K) == 0


def test_f64_has_no_cpu_fallback():
    from reart_amd import chamferdist_C
    from reart_amd.utils.chamfer import ChamferDistance, knn_points

    a = torch.zeros(1, 8, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        knn_points(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ChamferDistance()(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        chamferdist_C.knn_points_idx(a, a, None, None, 1)
