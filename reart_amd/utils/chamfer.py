"""Host-side mirror of the reference's ``utils/chamfer.py`` (ChamferDistance, knn_points,
knn_gather) over the HIP K-NN kernels.

Same names, argument meaning, return shapes and error behaviour as the reference module
(``utils/chamfer.py:20-337``); the native calls at ``:174`` and ``:206-208`` go to
``reart_amd.chamferdist_C`` instead of ``chamferdist._C``.

Beyond the reference: the warm-started operators ``ChamferLoss`` (the bidirectional sum with a fused backward),
``ChamferPoints`` (the per-point distances with a backward for per-point upstream gradients) and ``WarmChamferDistance``
(``ChamferDistance``'s interface over a ``ChamferPoints``).
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

    @staticmethod
    def _check(source_cloud, target_cloud, bidirectional, reverse, reduction):
        """The reference's validation (utils/chamfer.py:34-76), shared with ``WarmChamferDistance`` -> (bs, ns, bt, nt)."""
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
        return bs, ns, bt, nt

    @staticmethod
    def _select(d_fwd, i_fwd, d_bwd, i_bwd, bidirectional, reverse, return_index):
        """What the reference returns for the mode (utils/chamfer.py:119-132) from the per-direction results."""
        if bidirectional:
            total = d_fwd + d_bwd  # element-wise: needs ns == nt (utils/chamfer.py:119-123)
            return (total, i_fwd, i_bwd) if return_index else total
        if reverse:
            return (d_bwd, i_bwd) if return_index else d_bwd
        return (d_fwd, i_fwd) if return_index else d_fwd

    def forward(self, source_cloud, target_cloud, bidirectional=False, reverse=False,
                reduction="mean", return_index=False):
        bs, ns, bt, nt = self._check(source_cloud, target_cloud, bidirectional, reverse, reduction)
        len_s = torch.full((bs,), ns, dtype=torch.long, device=source_cloud.device)
        len_t = torch.full((bt,), nt, dtype=torch.long, device=target_cloud.device)
        fwd = knn_points(source_cloud, target_cloud, lengths1=len_s, lengths2=len_t, K=1)
        d_fwd, i_fwd = fwd.dists[..., 0], fwd.idx[..., 0]
        d_bwd = i_bwd = None
        if reverse or bidirectional:
            bwd = knn_points(target_cloud, source_cloud, lengths1=len_t, lengths2=len_s, K=1)
            d_bwd, i_bwd = bwd.dists[..., 0], bwd.idx[..., 0]
        return self._select(d_fwd, i_fwd, d_bwd, i_bwd, bidirectional, reverse, return_index)


class _WarmChamfer(torch.nn.Module):
    """State of the warm-started Chamfer operators (``ChamferLoss``, ``ChamferPoints``), per (shapes, device, lengths): the
    seeds, the native workspace with y's prepared image and the key of the y it was built from, the storage orders, ``.last``."""

    _LEN_CACHE = 16     # lengths tensors whose host copy is remembered

    def __init__(self, spatial_sort=True):
        super().__init__()
        self.spatial_sort = bool(spatial_sort)
        self._state = {}
        self._lens = {}
        self._last = self._raw = None

    def reset(self):
        """Forget seeds, orders, y's image, the lengths read so far and ``.last`` (the next call is a first call)."""
        self._state = {}
        self._lens = {}
        self._last = self._raw = None

    def _length(self, arg, name, N, P):
        """A lengths argument -> tuple of N ints in [0, P], or None (no lengths).
        A tensor is read on the host when it is new to the module (identity, shape, ``_version``, as for y): one
        synchronisation the first time, none afterwards.  Nothing is launched before the checks have passed."""
        if arg is None:
            return None
        who = type(self).__name__
        if isinstance(arg, torch.Tensor):
            if arg.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
                raise TypeError(f"{who}: {name} must be an integer tensor, got {arg.dtype}")
            if tuple(arg.shape) != (N,):
                raise ValueError(f"{who}: {name} must have shape [{N}], got {list(arg.shape)}")
            key = (id(arg), arg.data_ptr(), arg.device, arg._version)
            hit = self._lens.get(key)
            if hit is not None and hit[0] is arg:
                vals = hit[1]
            else:
                vals = tuple(int(v) for v in arg.detach().cpu().tolist())
                if len(self._lens) >= self._LEN_CACHE:
                    self._lens.pop(next(iter(self._lens)))
                self._lens[key] = (arg, vals)       # the reference keeps id(arg) from being recycled
        else:
            try:
                seq = list(arg)
            except TypeError:
                raise TypeError(f"{who}: {name} must be None, a sequence of ints or an integer tensor") from None
            if len(seq) != N:
                raise ValueError(f"{who}: {name} must have {N} entries, got {len(seq)}")
            import numbers

            for v in seq:
                if isinstance(v, bool) or not isinstance(v, numbers.Integral):
                    raise TypeError(f"{who}: {name} must hold ints, got {type(v).__name__}")
            vals = tuple(int(v) for v in seq)
        for v in vals:
            if v < 0 or v > P:
                raise ValueError(f"{who}: {name} holds {v}, outside [0, {P}]")
        return vals

    def _lengths(self, x, y, x_lengths, y_lengths):
        """(lx, ly): the two validated length tuples (None where a cloud is dense)."""
        return (self._length(x_lengths, "x_lengths", x.shape[0], x.shape[1]),
                self._length(y_lengths, "y_lengths", y.shape[0], y.shape[1]))

    @staticmethod
    def _orders(c, lengths=None):
        """Storage order per element and its inverse.  With lengths: ``kd_order`` of the live prefix, the padding rows in place,
        so a trimmed cloud and the same cloud inside a padded batch are stored in the same order."""
        from ..relax import kd_order

        if lengths is None:
            perm = torch.stack([kd_order(c[n]) for n in range(c.shape[0])]).to(torch.int64)
        else:
            tail = torch.arange(c.shape[1], device=c.device, dtype=torch.int64)
            perm = torch.stack([torch.cat([kd_order(c[n, :l]).to(torch.int64), tail[l:]]) if l > 0 else tail
                                for n, l in enumerate(lengths)])
        inv = torch.empty_like(perm)
        inv.scatter_(1, perm, torch.arange(perm.shape[1], device=perm.device).expand_as(perm).contiguous())
        return perm, inv

    def _prepare(self, x, y, lens=(None, None)):
        """(state, ykey) of these shapes and lengths on this device (created on the first call), with the stored copy of y up to date.
        Whether the NATIVE image of y in the workspace is up to date is a separate fact, ``st["built"]``: it is set by
        ``_run`` alone, after a native call that built it has returned without an error."""
        N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
        dev = x.device
        if N == 0 or P1 == 0 or P2 == 0:
            raise ValueError(f"{type(self).__name__}: empty clouds")
        lx, ly = lens
        ragged = lx is not None or ly is not None
        key = (N, P1, P2, dev, lx, ly) if ragged else (N, P1, P2, dev)
        st = self._state.get(key)
        if st is None:
            L = _lib.lib()
            nbytes = L.reart_chamfer_ragged_bytes(N, P1, P2) if ragged else L.reart_chamfer_loss_workspace_bytes(N, P1, P2)
            if nbytes == 0:
                raise NotImplementedError(f"{type(self).__name__}: shape beyond reart_chamfer_loss")
            st = {"ws": torch.empty(int(nbytes), dtype=torch.uint8, device=dev),
                  "seed_xy": torch.full((N, P1), -1, dtype=torch.int32, device=dev),
                  "seed_yx": torch.full((N, P2), -1, dtype=torch.int32, device=dev),
                  "bits": torch.zeros((N,), dtype=torch.int32, device=dev), "ykey": None, "built": None, "px": None, "py": None,
                  "lens": lens,
                  "lenx": None if lx is None else torch.tensor(lx, dtype=torch.int32, device=dev),
                  "leny": None if ly is None else torch.tensor(ly, dtype=torch.int32, device=dev)}
            if self.spatial_sort:
                st["px"] = self._orders(x.detach(), lx)
            self._state[key] = st
        yd = y.detach()
        ykey = (y.data_ptr(), tuple(y.shape), tuple(y.stride()), y.device, y._version)
        if st["ykey"] != ykey:
            if self.spatial_sort:
                if st["py"] is None:
                    st["py"] = self._orders(yd, ly)
                st["ys"] = torch.gather(yd, 1, st["py"][0][..., None].expand(-1, -1, 3)).contiguous()
            else:
                st["ys"] = yd.contiguous()
            # the detached alias keeps y's storage (not its autograd graph) alive: an equal data_ptr later is this storage,
            # never a recycled block
            st["ykey"], st["yref"] = ykey, yd
        return st, ykey

    def seed(self, x, y, seed_xy=None, seed_yx=None, x_lengths=None, y_lengths=None):
        """Install neighbour guesses for the next call on clouds of these shapes and lengths (caller numbering: seed_xy [N,P1]
        indices into y, seed_yx [N,P2] indices into x; None: forget that direction's).  Any values are allowed -- seeds bound
        the search, they never change its result (one that names a padding point is unusable)."""
        _lib.require_gpu(x, y)
        lens = self._lengths(x, y, x_lengths, y_lengths)
        st, _ = self._prepare(x, y, lens)      # orders and the stored y; the native image is (re)built by the next forward
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

    @staticmethod
    def _dead(idx, len_own, len_other):
        """[N,P] mask of the rows of a ragged call that have no neighbour: beyond their own length, or the other cloud is empty."""
        dead = torch.zeros_like(idx, dtype=torch.bool)
        if len_own is not None:
            dead |= torch.arange(idx.shape[1], device=idx.device)[None] >= len_own[:, None]
        if len_other is not None:
            dead |= (len_other == 0)[:, None]
        return dead

    @staticmethod
    def _long_lengths(lens, dev):
        """The length tuples as ``knn_points``'s int64 device tensors (None stays None)."""
        return tuple(None if l is None else torch.tensor(l, dtype=torch.int64, device=dev) for l in lens)

    @property
    def last(self):
        """Detached ``(d_xy [N,P1], i_xy [N,P1] int64, d_yx [N,P2], i_yx [N,P2] int64)`` of the latest call, in the caller's
        numbering (None before the first call; a direction that was not computed is None).  With ``spatial_sort`` they are
        renumbered on first access, not in the call."""
        if self._last is None and self._raw is not None:
            d_xy, i_xy, d_yx, i_yx, px, py, lenx, leny = self._raw
            if px is not None:
                # rows through the inverse order, neighbour indices through the other cloud's order
                (px, ix), (py, iy) = px, py
                if d_xy is not None:
                    d_xy, i_xy = torch.gather(d_xy, 1, ix), torch.gather(torch.gather(py, 1, i_xy), 1, ix)
                if d_yx is not None:
                    d_yx, i_yx = torch.gather(d_yx, 1, iy), torch.gather(torch.gather(px, 1, i_yx), 1, iy)
                # a row without a neighbour (padding, or an empty other cloud: distance 0) names index 0 in the caller's
                # numbering too, not the point stored first
                if i_xy is not None and (lenx is not None or leny is not None):
                    i_xy = i_xy.masked_fill(self._dead(i_xy, lenx, leny), 0)
                if i_yx is not None and (lenx is not None or leny is not None):
                    i_yx = i_yx.masked_fill(self._dead(i_yx, leny, lenx), 0)
            self._last = (d_xy, i_xy, d_yx, i_yx)
        return self._last


class _ChamferLossFn(Function):
    """Pattern of networks/loss.py's _FlowLoss: the forward has computed the loss and both gradients, the backward
    scales them by the upstream scalar."""

    @staticmethod
    def forward(ctx, x, y, mod, lens=(None, None)):
        loss, gx, gy = mod._run(x, y, y.requires_grad, lens)
        ctx.save_for_backward(gx, gy)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gx, gy = ctx.saved_tensors
        return gx * g, (gy * g if gy is not None else None), None, None


class ChamferLoss(_WarmChamfer):
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
    is filled as well).

    Clouds of differing lengths in one batch: ``x_lengths`` / ``y_lengths`` (None, a sequence of N ints, or an integer
    tensor [N] on the host or the device, each length in [0, P]; validated before anything is launched) say how many leading
    points of every element are real -- the call is ``knn_points(x, y, lengths1, lengths2, K=1)`` in both directions
    (``reart_chamfer_loss_ragged``).  Live rows are bit for bit the oracle's; padding rows, and every row of an element whose
    other cloud is empty, come back as distance 0, index 0, gradient exactly 0; whatever the padding rows of x and y hold
    (NaN included) changes no output bit; element n equals a dense call on the two trimmed clouds in every bit, ``fx_bits``
    included.  State is kept per (shapes, device, the two length tuples); a lengths tensor is read on the host when it is
    new to the module (identity, ``_version``) -- one synchronisation, none afterwards.  With ``spatial_sort`` an element is
    stored as ``kd_order`` of its live prefix followed by its padding rows, so the tie rule is the trimmed cloud's."""

    def forward(self, x, y, bidirectional=True, x_lengths=None, y_lengths=None):
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
        lens = self._lengths(x, y, x_lengths, y_lengths)
        if x.shape[2] != 3 or x.dtype != torch.float32 or y.dtype != torch.float32:
            l1, l2 = self._long_lengths(lens, x.device)
            fwd = knn_points(x, y, l1, l2, K=1)
            bwd = knn_points(y, x, l2, l1, K=1)
            self._raw, self._last = None, (fwd.dists[..., 0].detach(), fwd.idx[..., 0], bwd.dists[..., 0].detach(), bwd.idx[..., 0])
            return torch.sum(fwd.dists) + torch.sum(bwd.dists)
        if lens == (None, None):
            return _ChamferLossFn.apply(x, y, self)
        return _ChamferLossFn.apply(x, y, self, lens)

    def _run(self, x, y, want_gy, lens=(None, None)):
        N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
        dev = x.device
        L = _lib.lib()
        st, ykey = self._prepare(x, y, lens)
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
        args = (_lib.ptr(xs), _lib.ptr(ys), N, P1, P2, _lib.ptr(st["seed_xy"]), _lib.ptr(st["seed_yx"]),
                int(same_y), _lib.ptr(d_xy), _lib.ptr(i_xy), _lib.ptr(d_yx), _lib.ptr(i_yx),
                _lib.ptr(loss), _lib.ptr(gx), _lib.ptr(gy), _lib.ptr(st["bits"]), _lib.ptr(st["ws"]), st["ws"].numel())
        with torch.cuda.device(dev):
            if lens == (None, None):
                rc = L.reart_chamfer_loss(*args, _lib.stream())
            else:
                rc = L.reart_chamfer_loss_ragged(*args, _lib.stream(), _lib.ptr(st["lenx"]), _lib.ptr(st["leny"]))
        _lib.check(rc, "reart_chamfer_loss")
        st["built"] = ykey
        self._last, self._raw = None, (d_xy, i_xy, d_yx, i_yx, st["px"], st["py"], st["lenx"], st["leny"])
        if self.spatial_sort:
            # stored -> caller numbering: rows through the inverse order
            gx = torch.gather(gx, 1, st["px"][1][..., None].expand(-1, -1, 3))
            if gy is not None:
                gy = torch.gather(gy, 1, st["py"][1][..., None].expand(-1, -1, 3))
        self.fx_bits = st["bits"]
        return loss, gx, gy


_DIRECTIONS = {"xy": 1, "yx": 2, "both": 3}


class _ChamferPointsFn(Function):
    """The forward hands out the per-point distances of the searched directions; the backward takes whatever upstream
    arrives for them (None for an output that was not used) to ``reart_chamfer_points_backward``."""

    @staticmethod
    def forward(ctx, x, y, mod, directions, lens=(None, None)):
        ctx.set_materialize_grads(False)
        xs, ys, d_xy, i_xy, d_yx, i_yx, px, py, lenx, leny = mod._run(x, y, directions, lens)
        ctx.save_for_backward(xs, ys, d_xy, i_xy, d_yx, i_yx)
        ctx.mod, ctx.orders, ctx.lens = mod, (px, py), (lenx, leny)
        if px is not None:
            # stored -> caller numbering: rows through the inverse order
            o_xy = None if d_xy is None else torch.gather(d_xy, 1, px[1])
            o_yx = None if d_yx is None else torch.gather(d_yx, 1, py[1])
        else:
            # fresh tensors for autograd to mark as outputs; the saved ones and .last stay plain
            o_xy = None if d_xy is None else d_xy.clone()
            o_yx = None if d_yx is None else d_yx.clone()
        return o_xy, o_yx

    @staticmethod
    @once_differentiable
    def backward(ctx, g_xy, g_yx):
        if g_xy is None and g_yx is None:
            return None, None, None, None, None
        xs, ys, d_xy, i_xy, d_yx, i_yx = ctx.saved_tensors
        px, py = ctx.orders
        N, P1, P2 = xs.shape[0], xs.shape[1], ys.shape[1]
        dev = xs.device
        # an expanded tensor (from .sum()) is the common upstream: dense float32, in the stored numbering
        if g_xy is not None:
            g_xy = g_xy.to(torch.float32).contiguous() if px is None else torch.gather(g_xy.to(torch.float32), 1, px[0])
        if g_yx is not None:
            g_yx = g_yx.to(torch.float32).contiguous() if py is None else torch.gather(g_yx.to(torch.float32), 1, py[0])
        gx = torch.empty((N, P1, 3), dtype=torch.float32, device=dev)
        gy = torch.empty((N, P2, 3), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        bits = torch.empty((N, 2), dtype=torch.int32, device=dev)
        args = (_lib.ptr(xs), _lib.ptr(ys), N, P1, P2, _lib.ptr(i_xy), _lib.ptr(i_yx), _lib.ptr(d_xy), _lib.ptr(d_yx),
                _lib.ptr(g_xy), _lib.ptr(g_yx), _lib.ptr(gx), _lib.ptr(gy), _lib.ptr(bits))
        lenx, leny = ctx.lens
        with torch.cuda.device(dev):
            if lenx is None and leny is None:
                rc = _lib.lib().reart_chamfer_points_backward(*args, _lib.stream())
            else:
                rc = _lib.lib().reart_chamfer_points_backward_ragged(*args, _lib.stream(), _lib.ptr(lenx), _lib.ptr(leny))
        _lib.check(rc, "reart_chamfer_points_backward")
        ctx.mod.fx_bits = bits
        if px is not None:
            gx = torch.gather(gx, 1, px[1][..., None].expand(-1, -1, 3))
            if gy is not None:
                gy = torch.gather(gy, 1, py[1][..., None].expand(-1, -1, 3))
        return (gx if ctx.needs_input_grad[0] else None), gy, None, None, None


class ChamferPoints(_WarmChamfer):
    """``forward(x, y, directions="both") -> (d_xy [N,P1], d_yx [N,P2])``: the per-point squared distances to the nearest
    neighbour in the other cloud, as ``ChamferDistance`` returns them, from the warm-started search of ``ChamferLoss``
    (``reart_chamfer_points``), differentiable with respect to x -- and y, when it requires grad -- for ANY per-point
    upstream gradient (``reart_chamfer_points_backward``): weights, masks, means over clouds of different sizes, robust
    functions of the distances.  x [N,P1,3], y [N,P2,3] float32 on the GPU; P1 != P2 is allowed.  With ``directions``
    "xy" or "yx" only that direction is searched and the other result is None.

    State, its keys, ``seed()``, ``reset()``, ``spatial_sort`` and the tie rule are ``ChamferLoss``'s; results and
    gradients are always in the caller's numbering.  ``.last`` holds the detached ``(d_xy, i_xy, d_yx, i_yx)`` of the
    latest call (None for a direction that was not computed), ``.fx_bits`` the [N,2] fractional bits of the latest
    backward's fixed-point sums into x and into y.  An output that is not used contributes nothing and costs nothing in
    the backward; the backward reads only what its own forward returned, never the module's state.

    Host tensors raise ``RuntimeError: ... no CPU fallback``; D != 3 or float64 go through ``knn_points(..., K=1)`` (same
    values, gradients through its backward, no warm state); a shape beyond the workspace raises NotImplementedError.

    ``x_lengths`` / ``y_lengths``: clouds of differing lengths in one batch, with ``ChamferLoss``'s rules
    (``reart_chamfer_points_ragged``, ``reart_chamfer_points_backward_ragged``): padding rows come back as distance 0 with
    gradient exactly 0, and an upstream gradient at a padding row is never read."""

    def forward(self, x, y, directions="both", x_lengths=None, y_lengths=None):
        for cloud in (x, y):
            if not isinstance(cloud, torch.Tensor):
                raise TypeError("Expected input type torch.Tensor. Got {} instead".format(type(cloud)))
        _lib.require_gpu(x, y)
        if directions not in _DIRECTIONS:
            raise ValueError('ChamferPoints: directions must be "both", "xy" or "yx"')
        if x.dim() != 3 or y.dim() != 3 or x.shape[0] != y.shape[0] or x.shape[2] != y.shape[2]:
            raise ValueError("ChamferPoints: x [N,P1,D] and y [N,P2,D]")
        if x.device != y.device:
            raise ValueError("Source and target clouds must be on the same device.")
        mask = _DIRECTIONS[directions]
        lens = self._lengths(x, y, x_lengths, y_lengths)
        if x.shape[2] != 3 or x.dtype != torch.float32 or y.dtype != torch.float32:
            l1, l2 = self._long_lengths(lens, x.device)
            fwd = knn_points(x, y, l1, l2, K=1) if mask & 1 else None
            bwd = knn_points(y, x, l2, l1, K=1) if mask & 2 else None
            d_xy, i_xy = (fwd.dists[..., 0], fwd.idx[..., 0]) if fwd is not None else (None, None)
            d_yx, i_yx = (bwd.dists[..., 0], bwd.idx[..., 0]) if bwd is not None else (None, None)
            self._raw = None
            self._last = (None if d_xy is None else d_xy.detach(), i_xy, None if d_yx is None else d_yx.detach(), i_yx)
            return d_xy, d_yx
        if lens == (None, None):
            return _ChamferPointsFn.apply(x, y, self, mask)
        return _ChamferPointsFn.apply(x, y, self, mask, lens)

    def _run(self, x, y, directions, lens=(None, None)):
        """One native forward in the stored numbering -> (xs, ys, d_xy, i_xy, d_yx, i_yx, px, py, lenx, leny)."""
        N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
        dev = x.device
        st, ykey = self._prepare(x, y, lens)
        same_y = st["built"] == ykey     # y's SoA image and boxes in THIS workspace were built from exactly this y
        if directions & 1:               # a y -> x search alone neither reads nor writes y's image
            st["built"] = None           # until the call below has returned without an error
        xd = x.detach()
        if self.spatial_sort:
            xs = torch.gather(xd, 1, st["px"][0][..., None].expand(-1, -1, 3))
        else:
            xs = xd.contiguous()
        ys = st["ys"]
        d_xy = i_xy = d_yx = i_yx = None
        if directions & 1:
            d_xy = torch.empty((N, P1), dtype=torch.float32, device=dev)
            i_xy = torch.empty((N, P1), dtype=torch.int64, device=dev)
        if directions & 2:
            d_yx = torch.empty((N, P2), dtype=torch.float32, device=dev)
            i_yx = torch.empty((N, P2), dtype=torch.int64, device=dev)
        args = (_lib.ptr(xs), _lib.ptr(ys), N, P1, P2, directions, _lib.ptr(st["seed_xy"]), _lib.ptr(st["seed_yx"]), int(same_y),
                _lib.ptr(d_xy), _lib.ptr(i_xy), _lib.ptr(d_yx), _lib.ptr(i_yx), _lib.ptr(st["ws"]), st["ws"].numel())
        with torch.cuda.device(dev):
            if lens == (None, None):
                rc = _lib.lib().reart_chamfer_points(*args, _lib.stream())
            else:
                rc = _lib.lib().reart_chamfer_points_ragged(*args, _lib.stream(), _lib.ptr(st["lenx"]), _lib.ptr(st["leny"]))
        _lib.check(rc, "reart_chamfer_points")
        if directions & 1:
            st["built"] = ykey
        self._last, self._raw = None, (d_xy, i_xy, d_yx, i_yx, st["px"], st["py"], st["lenx"], st["leny"])
        return xs, ys, d_xy, i_xy, d_yx, i_yx, st["px"], st["py"], st["lenx"], st["leny"]


class WarmChamferDistance(ChamferDistance):
    """``ChamferDistance`` over a ``ChamferPoints``: the same signature, validation, warnings, errors and return shapes, with
    only the direction(s) the mode needs searched, warm from the module's previous call.  For float32 [B,P,3] clouds on
    the GPU the distances equal ``ChamferDistance``'s bit for bit, the indices too except for a tie between DISTINCT
    equidistant targets under ``spatial_sort=True`` (the caveat of ``ChamferLoss``).  ``recon_loss(x, y,
    WarmChamferDistance())`` goes through the per-point branch."""

    def __init__(self, spatial_sort=True):
        super().__init__()
        self.points = ChamferPoints(spatial_sort=spatial_sort)

    def forward(self, source_cloud, target_cloud, bidirectional=False, reverse=False,
                reduction="mean", return_index=False):
        self._check(source_cloud, target_cloud, bidirectional, reverse, reduction)
        d_fwd, d_bwd = self.points(source_cloud, target_cloud, "both" if bidirectional else ("yx" if reverse else "xy"))
        _, i_fwd, _, i_bwd = self.points.last if return_index else (None,) * 4
        return self._select(d_fwd, i_fwd, d_bwd, i_bwd, bidirectional, reverse, return_index)
