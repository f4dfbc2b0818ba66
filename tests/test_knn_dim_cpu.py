"""Host-side contract of the any-D K-nearest search (no GPU): the D ceiling agrees between include/reart_hip.h and
reart_amd/_lib.py, the entry points reject a bad D with a status code before any device work, and the D-aware
workspace query agrees with the D = 3 one."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2


def test_max_d_matches_the_header():
    from reart_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "reart_hip.h")).read()
    assert int(re.search(r"#define\s+REART_MAX_D\s+(\d+)", hdr).group(1)) == _lib.MAX_D == 256


def test_entry_points_reject_bad_dimension_without_a_gpu():
    from reart_amd import _lib

    L = _lib.lib()
    for D, rc in ((0, INVALID), (-1, INVALID), (257, UNSUPPORTED)):
        assert L.reart_knn_points_idx(None, None, None, None, 1, 8, 8, D, 1, None, None, None, 0, None) == rc
        assert L.reart_knn_cuda(None, None, 1, 8, 8, D, 1, 1, None, None, None, 0, None) == rc
        assert L.reart_knn_points_backward(None, None, None, None, None, None, 1, 8, 8, D, 1, None, None, None, 0,
                                           None) == rc
    # the other limits keep their codes at any D
    assert L.reart_knn_points_idx(None, None, None, None, 1, 8, 8, 64, 1025, None, None, None, 0, None) == UNSUPPORTED
    assert L.reart_knn_cuda(None, None, 1, 8, 8, 64, 9, 1, None, None, None, 0, None) == INVALID       # k > nr
    # empty problems are fine
    assert L.reart_knn_points_idx(None, None, None, None, 0, 8, 8, 64, 1, None, None, None, 0, None) == 0
    assert L.reart_knn_cuda(None, None, 1, 8, 0, 128, 1, 1, None, None, None, 0, None) == 0


def test_workspace_bytes_d():
    from reart_amd import _lib

    L = _lib.lib()
    for N, P1, P2, K in [(1, 1, 1, 1), (2, 77, 1500, 3), (19, 4096, 4096, 16), (3, 301, 1100, 200), (1, 5, 2000, 1024),
                         (8, 4096, 4096, 17)]:
        assert L.reart_knn_points_workspace_bytes_d(N, P1, P2, 3, K) == L.reart_knn_points_workspace_bytes(N, P1, P2, K)
        for D in (1, 2, 64, 256):
            # at least the [N, D, P2] target image and the [N, P1, D] query image
            assert L.reart_knn_points_workspace_bytes_d(N, P1, P2, D, K) >= 4 * N * D * (P1 + P2)
    assert L.reart_knn_points_workspace_bytes_d(1, 50, 50, 257, 1) == 0
    assert L.reart_knn_points_workspace_bytes_d(1, 50, 50, 0, 1) == 0
    assert L.reart_knn_points_workspace_bytes_d(1, 50, 50, 64, 1025) == 0
    assert L.reart_knn_points_workspace_bytes_d(1, 50, 50, 64, 0) == 0
