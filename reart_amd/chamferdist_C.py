"""Drop-in for the ``chamferdist._C`` extension module the reference imports at
``utils/chamfer.py:12`` and calls at ``utils/chamfer.py:174`` / ``:206-208``.

Same two functions, same argument order, same return order; backed by
``reart_knn_points_idx`` / ``reart_knn_points_backward`` in libreart_hip.so.
"""
import torch

from . import _lib


def _as_len(lengths, n, full, device):
    if lengths is None:
        return None
    if lengths.dtype != torch.int64:
        lengths = lengths.long()
    # a full-length vector is the reference's default (utils/chamfer.py:266-275)
    return lengths.contiguous()


def _check_dim(what, D):
    if D > _lib.MAX_D:
        raise NotImplementedError(f"{what}: D = {D} > {_lib.MAX_D} (REART_MAX_D)")


def knn_points_idx(p1, p2, lengths1, lengths2, K, version=-1):
    """-> (idx int64 [N,P1,K], dists [N,P1,K] squared L2 in the clouds' dtype), cf. utils/chamfer.py:174.

    p1 [N,P1,D], p2 [N,P2,D], both float32 or both float64 (like the upstream forward, which dispatches on float and
    double); mixed or other dtypes raise TypeError.  1 <= D <= 256 (REART_MAX_D); D > 256 raises NotImplementedError.
    1 <= K <= 1024; K > 1024 raises NotImplementedError.  float32: at D = 3, K <= 16 keeps each query's list in
    registers, larger K in LDS; other D keep it in LDS (same result, bit for bit).  float64: one LDS-list kernel for
    every D and K (``reart_knn_points_idx_f64``), distances summed in fp64."""
    _lib.require_gpu(p1, p2, lengths1, lengths2)
    if p1.dtype != p2.dtype or p1.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"knn_points_idx expects float32 or float64 point clouds of one dtype, got {p1.dtype} and "
                        f"{p2.dtype}")
    p1, p2 = p1.contiguous(), p2.contiguous()
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    if K > _lib.MAX_K_LIST:
        raise NotImplementedError(f"knn_points_idx: K = {K} > {_lib.MAX_K_LIST} (REART_MAX_K_LIST)")
    _check_dim("knn_points_idx", D)
    l1 = _as_len(lengths1, N, P1, p1.device)
    l2 = _as_len(lengths2, N, P2, p1.device)
    dists = torch.empty((N, P1, K), dtype=p1.dtype, device=p1.device)
    idx = torch.empty((N, P1, K), dtype=torch.int64, device=p1.device)
    L = _lib.lib()
    if p1.dtype == torch.float64:
        nbytes, run, name = L.reart_knn_points_workspace_bytes_f64(N, P1, P2, D, K), L.reart_knn_points_idx_f64, \
            "reart_knn_points_idx_f64"
    else:
        nbytes, run, name = L.reart_knn_points_workspace_bytes_d(N, P1, P2, D, K), L.reart_knn_points_idx, \
            "reart_knn_points_idx"
    ws = _lib.workspace(nbytes, p1.device)
    rc = run(_lib.ptr(p1), _lib.ptr(p2), _lib.ptr(l1), _lib.ptr(l2), N, P1, P2, D, K,
             _lib.ptr(dists), _lib.ptr(idx), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, name)
    return idx, dists


def knn_points_backward(p1, p2, lengths1, lengths2, idx, grad_dists):
    """-> (grad_p1 [N,P1,D], grad_p2 [N,P2,D]), cf. utils/chamfer.py:206-208; 1 <= D <= 256 (REART_MAX_D).

    float32 only, like the upstream backward: p1, p2 and grad_dists of any other dtype raise TypeError (the autograd
    wrapper in utils/chamfer.py casts float64 clouds to float32 before this call, as the reference does)."""
    _lib.require_gpu(p1, p2, idx, grad_dists)
    if p1.dtype != torch.float32 or p2.dtype != torch.float32 or grad_dists.dtype != torch.float32:
        raise TypeError(f"knn_points_backward expects float32 p1, p2 and grad_dists, got {p1.dtype}, {p2.dtype} and "
                        f"{grad_dists.dtype}")
    p1, p2 = p1.contiguous(), p2.contiguous()
    idx, grad_dists = idx.contiguous(), grad_dists.contiguous()
    N, P1, D = p1.shape
    _check_dim("knn_points_backward", D)
    P2 = p2.shape[1]
    K = idx.shape[2]
    l1 = _as_len(lengths1, N, P1, p1.device)
    l2 = _as_len(lengths2, N, P2, p1.device)
    g1 = torch.empty_like(p1)
    g2 = torch.empty_like(p2)
    L = _lib.lib()
    nbytes = L.reart_knn_points_backward_workspace_bytes(N, P1, P2, K)
    ws = _lib.workspace(nbytes, p1.device)
    rc = L.reart_knn_points_backward(_lib.ptr(p1), _lib.ptr(p2), _lib.ptr(l1), _lib.ptr(l2), _lib.ptr(idx),
                                     _lib.ptr(grad_dists), N, P1, P2, D, K, _lib.ptr(g1), _lib.ptr(g2),
                                     _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "reart_knn_points_backward")
    return g1, g2


def chamfer_bidir(x, y):
    """Fused two-direction K=1 search: -> (d_xy, i_xy, d_yx, i_yx), each [N,P]."""
    _lib.require_gpu(x, y)
    x, y = x.contiguous(), y.contiguous()
    N, Pn, _ = x.shape
    d_xy = torch.empty((N, Pn), dtype=torch.float32, device=x.device)
    d_yx = torch.empty_like(d_xy)
    i_xy = torch.empty((N, Pn), dtype=torch.int64, device=x.device)
    i_yx = torch.empty_like(i_xy)
    L = _lib.lib()
    ws = _lib.workspace(L.reart_chamfer_bidir_workspace_bytes(N, Pn), x.device)
    rc = L.reart_chamfer_bidir(_lib.ptr(x), _lib.ptr(y), N, Pn, _lib.ptr(d_xy), _lib.ptr(i_xy), _lib.ptr(d_yx),
                               _lib.ptr(i_yx), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "reart_chamfer_bidir")
    return d_xy, i_xy, d_yx, i_yx


def knn_points_idx_warm(p1, p2, K, seed=None):
    """Warm-started exact search (``reart_knn_points_idx_warm``): same (idx, dists) as
    ``knn_points_idx(p1, p2, None, None, K)`` for K in {1, 3}, bit for bit, whatever ``seed`` holds.
    ``seed`` [N,P1,K] int32 is updated in place with the new neighbour indices (pass it to the next
    call on the moved clouds); ``None`` starts cold.  Not part of the reference's ``_C`` module: it is
    the stand-alone form of the search the fused relaxation step runs every iteration.
    -> (idx int64 [N,P1,K], dists float32 [N,P1,K], seed)"""
    _lib.require_gpu(p1, p2)
    if p1.dtype != torch.float32 or p2.dtype != torch.float32:
        raise TypeError("knn_points_idx_warm expects float32 point clouds")
    p1, p2 = p1.contiguous(), p2.contiguous()
    N, P1, _ = p1.shape
    P2 = p2.shape[1]
    if seed is None:
        seed = torch.full((N, P1, K), -1, dtype=torch.int32, device=p1.device)
    if seed.dtype != torch.int32 or not seed.is_contiguous() or tuple(seed.shape) != (N, P1, K):
        raise TypeError("seed must be a contiguous int32 tensor [N,P1,K]")
    dists = torch.empty((N, P1, K), dtype=torch.float32, device=p1.device)
    idx = torch.empty((N, P1, K), dtype=torch.int64, device=p1.device)
    L = _lib.lib()
    nbytes = L.reart_knn_points_warm_workspace_bytes(N, P1, P2, K)
    ws = _lib.workspace(nbytes, p1.device)
    rc = L.reart_knn_points_idx_warm(_lib.ptr(p1), _lib.ptr(p2), N, P1, P2, K, _lib.ptr(seed), _lib.ptr(dists),
                                     _lib.ptr(idx), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "reart_knn_points_idx_warm")
    return idx, dists, seed
