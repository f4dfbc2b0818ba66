"""Host-side mirror of the reference's ``utils/chamfer.py`` (ChamferDistance, knn_points,
knn_gather) over the HIP K-NN kernels.

Same names, argument meaning, return shapes and error behaviour as the reference module
(``utils/chamfer.py:20-337``); the native calls at ``:174`` and ``:206-208`` go to
``reart_amd.chamferdist_C`` instead of ``chamferdist._C``.
"""
import warnings
from collections import namedtuple

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib
from .. import chamferdist_C as _C

_KNN = namedtuple("KNN", "dists idx knn")


class _knn_points(Function):
    """autograd wrapper, cf. utils/chamfer.py:135-209."""

    @staticmethod
    def forward(ctx, p1, p2, lengths1, lengths2, K, version, return_sorted=True):
        idx, dists = _C.knn_points_idx(p1, p2, lengths1, lengths2, K, version)
        # The HIP kernel already returns neighbours ascending by (distance, index) and
        # zero-fills slots beyond lengths2, which is what the reference's post-sort
        # (utils/chamfer.py:177-189) produces.
        ctx.save_for_backward(p1, p2, lengths1, lengths2, idx)
        ctx.mark_non_differentiable(idx)
        return dists, idx

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_dists, grad_idx):
        # The native backward is float32 only, as upstream (utils/chamfer.py:196-208 casts too); autograd casts the
        # gradients back to a float64 input's dtype.
        p1, p2, lengths1, lengths2, idx = ctx.saved_tensors
        grad_p1, grad_p2 = _C.knn_points_backward(
            p1.float(), p2.float(), lengths1, lengths2, idx, grad_dists.float()
        )
        return grad_p1, grad_p2, None, None, None, None, None


def knn_points(p1, p2, lengths1=None, lengths2=None, K=1, version=-1, return_nn=False, return_sorted=True):
    """K nearest neighbours of every p1 point in p2 (utils/chamfer.py:212-286).

    p1 [N,P1,D], p2 [N,P2,D] with 1 <= D <= 256 and 1 <= K <= 1024 (above: NotImplementedError), both float32 or
    both float64 (otherwise TypeError).  Returns the namedtuple ``(dists [N,P1,K] squared in the clouds' dtype,
    idx [N,P1,K] int64, knn or None)``; gradients reach float64 clouds through the float32 backward, as upstream.
    """
    if p1.shape[0] != p2.shape[0]:
        raise ValueError("pts1 and pts2 must have the same batch dimension.")
    if p1.shape[2] != p2.shape[2]:
        raise ValueError("pts1 and pts2 must have the same point dimension.")
    p1, p2 = p1.contiguous(), p2.contiguous()
    n = p1.shape[0]
    if lengths1 is None:
        lengths1 = torch.full((n,), p1.shape[1], dtype=torch.int64, device=p1.device)
    if lengths2 is None:
        lengths2 = torch.full((n,), p2.shape[1], dtype=torch.int64, device=p1.device)
    dists, idx = _knn_points.apply(p1, p2, lengths1, lengths2, K, version, return_sorted)
    nn = knn_gather(p2, idx, lengths2) if return_nn else None
    return _KNN(dists=dists, idx=idx, knn=nn)


def knn_gather(x, idx, lengths=None):
    """x [N,M,U], idx [N,L,K] -> [N,L,K,U] with x_out[n,l,k] = x[n, idx[n,l,k]]
    (utils/chamfer.py:289-337); entries with k >= lengths[n] are zero.  Any dtype of x (the result keeps it)."""
    N, M, U = x.shape
    n2, L, K = idx.shape
    if N != n2:
        raise ValueError("x and idx must have same batch dimension.")
    if lengths is None:
        lengths = torch.full((N,), M, dtype=torch.int64, device=x.device)
    out = x.gather(1, idx.reshape(N, L * K, 1).expand(-1, -1, U)).reshape(N, L, K, U)
    if lengths.min() < K:
        dead = lengths[:, None] <= torch.arange(K, device=x.device)[None]
        out = out.masked_fill(dead[:, None, :, None], 0.0)
    return out


class ChamferDistance(torch.nn.Module):
    """Per-point (un-reduced) Chamfer distance, cf. utils/chamfer.py:19-132, for clouds of any dimension D <= 256,
    both float32 or both float64 (the distances come back in that dtype; otherwise TypeError).

    ``reduction`` is validated and then ignored, exactly like the reference (its reduction
    block is commented out, utils/chamfer.py:104-117): the result has shape [B, P].
    """

    def forward(self, source_cloud, target_cloud, bidirectional=False, reverse=False,
                reduction="mean", return_index=False):
        for cloud in (source_cloud, target_cloud):
            if not isinstance(cloud, torch.Tensor):
                raise TypeError("Expected input type torch.Tensor. Got {} instead".format(type(cloud)))
        if source_cloud.device != target_cloud.device:
            raise ValueError(
                "Source and target clouds must be on the same device. "
                f"Got {source_cloud.device} and {target_cloud.device}."
            )
        bs, ns, ds = source_cloud.shape
        bt, nt, dt = target_cloud.shape
        if bs != bt:
            raise ValueError("Source and target pointclouds must have the same batchsize.")
        if ds != dt:
            raise ValueError("Source and target pointclouds must have the same dimensionality.")
        if bidirectional and reverse:
            warnings.warn("Both bidirectional and reverse set to True. bidirectional behavior takes precedence.")
        if reduction not in ("sum", "mean"):
            raise ValueError('Reduction must either be "sum" or "mean".')

        len_s = torch.full((bs,), ns, dtype=torch.long, device=source_cloud.device)
        len_t = torch.full((bt,), nt, dtype=torch.long, device=target_cloud.device)
        fwd = knn_points(source_cloud, target_cloud, lengths1=len_s, lengths2=len_t, K=1)
        d_fwd, i_fwd = fwd.dists[..., 0], fwd.idx[..., 0]
        if reverse or bidirectional:
            bwd = knn_points(target_cloud, source_cloud, lengths1=len_t, lengths2=len_s, K=1)
            d_bwd, i_bwd = bwd.dists[..., 0], bwd.idx[..., 0]
        if bidirectional:
            total = d_fwd + d_bwd  # element-wise: needs ns == nt (utils/chamfer.py:119-123)
            return (total, i_fwd, i_bwd) if return_index else total
        if reverse:
            return (d_bwd, i_bwd) if return_index else d_bwd
        return (d_fwd, i_fwd) if return_index else d_fwd


class _ChamferLossFn(Function):
    """Pattern of networks/loss.py's _FlowLoss: the forward has computed the loss and both gradients, the backward
    scales them by the upstream scalar."""

    @staticmethod
    def forward(ctx, x, y, mod):
        loss, gx, gy = mod._run(x, y, y.requires_grad)
        ctx.save_for_backward(gx, gy)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gx, gy = ctx.saved_tensors
        return gx * g, (gy * g if gy is not None else None), None


class ChamferLoss(torch.nn.Module):
    """``forward(x, y) -> scalar``: the value of ``recon_loss(x, y, ChamferDistance())`` -- the sum over both directions
    of the squared distance of every point to its nearest neighbour in the other cloud -- with its gradient, as one
    warm-started native call (``reart_chamfer_loss``).  x [N,P1,3], y [N,P2,3] float32 on the GPU; P1 != P2 is allowed.

    The module keeps, per (shapes, device): the neighbour indices of its previous call (they bound the next search and
    never change its result), the native workspace with y's prepared image, and -- unless ``spatial_sort=False`` -- a
    storage order per cloud (``relax.kd_order`` of the first x and of the first y, computed on the host once), in which
    the box-pruned search is fastest.  Results are always in the caller's point numbering; ``.last`` holds the detached
    ``(d_xy, i_xy, d_yx, i_yx)`` of the latest call.  With ``spatial_sort`` a tie between DISTINCT equidistant targets goes
    to the one stored first (coincident points keep the caller's order, so copies of a point resolve to the lowest index).

    State is never trusted for correctness: y's image is rebuilt whenever y is another tensor (``data_ptr``, shape,
    device) or was modified in place (``_version``).  After the first call on a shape there is no host synchronisation.
    Gradient reaches y only when ``y.requires_grad``.

    Host tensors raise ``RuntimeError: ... no CPU fallback``.  Inputs the warm search does not serve (D != 3, float64)
    go through two ``knn_points`` calls inside the module: the same value and gradients, without warm state (``.last``
    is filled as well)."""

    def __init__(self, spatial_sort=True):
        super().__init__()
        self.spatial_sort = bool(spatial_sort)
        self._state = {}
        self._last = self._raw = None

    def reset(self):
        """Forget seeds, orders, y's image and ``.last`` (the next call is a first call)."""
        self._state = {}
        self._last = self._raw = None

    def forward(self, x, y, bidirectional=True):
        for cloud in (x, y):
            if not isinstance(cloud, torch.Tensor):
                raise TypeError("Expected input type torch.Tensor. Got {} instead".format(type(cloud)))
        if not bidirectional:
            raise ValueError("ChamferLoss is the bidirectional sum")
        _lib.require_gpu(x, y)
        if x.dim() != 3 or y.dim() != 3 or x.shape[0] != y.shape[0] or x.shape[2] != y.shape[2]:
            raise ValueError("ChamferLoss: x [N,P1,D] and y [N,P2,D]")
        if x.device != y.device:
            raise ValueError("Source and target clouds must be on the same device.")
        if x.shape[2] != 3 or x.dtype != torch.float32 or y.dtype != torch.float32:
            fwd = knn_points(x, y, K=1)
            bwd = knn_points(y, x, K=1)
            self._raw, self._last = None, (fwd.dists[..., 0].detach(), fwd.idx[..., 0], bwd.dists[..., 0].detach(), bwd.idx[..., 0])
            return torch.sum(fwd.dists) + torch.sum(bwd.dists)
        return _ChamferLossFn.apply(x, y, self)

    @staticmethod
    def _orders(c):
        from ..relax import kd_order

        perm = torch.stack([kd_order(c[n]) for n in range(c.shape[0])]).to(torch.int64)
        inv = torch.empty_like(perm)
        inv.scatter_(1, perm, torch.arange(perm.shape[1], device=perm.device).expand_as(perm).contiguous())
        return perm, inv

    def _prepare(self, x, y):
        """(state, ykey) of these shapes on this device (created on the first call), with the stored copy of y up to date.
        Whether the NATIVE image of y in the workspace is up to date is a separate fact, ``st["built"]``: it is set by
        ``_run`` alone, after a native call that built it has returned without an error."""
        N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
        dev = x.device
        if N == 0 or P1 == 0 or P2 == 0:
            raise ValueError("ChamferLoss: empty clouds")
        key = (N, P1, P2, dev)
        st = self._state.get(key)
        if st is None:
            nbytes = _lib.lib().reart_chamfer_loss_workspace_bytes(N, P1, P2)
            if nbytes == 0:
                raise NotImplementedError("ChamferLoss: shape beyond reart_chamfer_loss")
            st = {"ws": torch.empty(int(nbytes), dtype=torch.uint8, device=dev),
                  "seed_xy": torch.full((N, P1), -1, dtype=torch.int32, device=dev),
                  "seed_yx": torch.full((N, P2), -1, dtype=torch.int32, device=dev),
                  "bits": torch.zeros((N,), dtype=torch.int32, device=dev), "ykey": None, "built": None, "px": None, "py": None}
            if self.spatial_sort:
                st["px"] = self._orders(x.detach())
            self._state[key] = st
        yd = y.detach()
        ykey = (y.data_ptr(), tuple(y.shape), tuple(y.stride()), y.device, y._version)
        if st["ykey"] != ykey:
            if self.spatial_sort:
                if st["py"] is None:
                    st["py"] = self._orders(yd)
                st["ys"] = torch.gather(yd, 1, st["py"][0][..., None].expand(-1, -1, 3)).contiguous()
            else:
                st["ys"] = yd.contiguous()
            # the detached alias keeps y's storage (not its autograd graph) alive: an equal data_ptr later is this storage,
            # never a recycled block
            st["ykey"], st["yref"] = ykey, yd
        return st, ykey

    def seed(self, x, y, seed_xy=None, seed_yx=None):
        """Install neighbour guesses for the next call on clouds of these shapes (caller numbering: seed_xy [N,P1] indices
        into y, seed_yx [N,P2] indices into x; None: forget that direction's).  Any values are allowed -- seeds bound the
        search, they never change its result."""
        _lib.require_gpu(x, y)
        st, _ = self._prepare(x, y)      # orders and the stored y; the native image is (re)built by the next forward
        for name, sd, rows, other in (("seed_xy", seed_xy, st["px"], st["py"]), ("seed_yx", seed_yx, st["py"], st["px"])):
            if sd is None:
                st[name].fill_(-1)
                continue
            sd = sd.to(device=x.device, dtype=torch.int64).reshape(st[name].shape)
            if self.spatial_sort:
                Po = other[1].shape[1]
                ok = (sd >= 0) & (sd < Po)
                sd = torch.where(ok, torch.gather(other[1], 1, sd.clamp(0, Po - 1)), sd)   # index -> its stored position
                sd = torch.gather(sd, 1, rows[0])                                          # row of the stored point
            st[name].copy_(sd.to(torch.int32))

    def _run(self, x, y, want_gy):
        N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
        dev = x.device
        L = _lib.lib()
        st, ykey = self._prepare(x, y)
        same_y = st["built"] == ykey     # y's SoA image and boxes in THIS workspace were built from exactly this y
        st["built"] = None               # until the call below has returned without an error
        xd = x.detach()
        if self.spatial_sort:
            xs = torch.gather(xd, 1, st["px"][0][..., None].expand(-1, -1, 3))
        else:
            xs = xd.contiguous()
        ys = st["ys"]
        d_xy = torch.empty((N, P1), dtype=torch.float32, device=dev)
        i_xy = torch.empty((N, P1), dtype=torch.int64, device=dev)
        d_yx = torch.empty((N, P2), dtype=torch.float32, device=dev)
        i_yx = torch.empty((N, P2), dtype=torch.int64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        gx = torch.empty((N, P1, 3), dtype=torch.float32, device=dev)
        gy = torch.empty((N, P2, 3), dtype=torch.float32, device=dev) if want_gy else None
        with torch.cuda.device(dev):
            rc = L.reart_chamfer_loss(_lib.ptr(xs), _lib.ptr(ys), N, P1, P2, _lib.ptr(st["seed_xy"]), _lib.ptr(st["seed_yx"]),
                                      int(same_y), _lib.ptr(d_xy), _lib.ptr(i_xy), _lib.ptr(d_yx), _lib.ptr(i_yx),
                                      _lib.ptr(loss), _lib.ptr(gx), _lib.ptr(gy), _lib.ptr(st["bits"]), _lib.ptr(st["ws"]),
                                      st["ws"].numel(), _lib.stream())
        _lib.check(rc, "reart_chamfer_loss")
        st["built"] = ykey
        self._last, self._raw = None, (d_xy, i_xy, d_yx, i_yx, st["px"], st["py"])
        if self.spatial_sort:
            # stored -> caller numbering: rows through the inverse order
            gx = torch.gather(gx, 1, st["px"][1][..., None].expand(-1, -1, 3))
            if gy is not None:
                gy = torch.gather(gy, 1, st["py"][1][..., None].expand(-1, -1, 3))
        self.fx_bits = st["bits"]
        return loss, gx, gy

    @property
    def last(self):
        """Detached ``(d_xy [N,P1], i_xy [N,P1] int64, d_yx [N,P2], i_yx [N,P2] int64)`` of the latest call, in the caller's
        numbering (None before the first call).  With ``spatial_sort`` they are renumbered on first access, not in the call."""
        if self._last is None and self._raw is not None:
            d_xy, i_xy, d_yx, i_yx, px, py = self._raw
            if px is not None:
                # rows through the inverse order, neighbour indices through the other cloud's order
                (px, ix), (py, iy) = px, py
                d_xy, i_xy = torch.gather(d_xy, 1, ix), torch.gather(torch.gather(py, 1, i_xy), 1, ix)
                d_yx, i_yx = torch.gather(d_yx, 1, iy), torch.gather(torch.gather(px, 1, i_yx), 1, iy)
            self._last = (d_xy, i_xy, d_yx, i_yx)
        return self._last
