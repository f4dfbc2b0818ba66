"""Host-side mirror of the reference's ``networks/loss.py`` (recon_loss ``:24-29``, flow_loss
``:10-21``, structure_loss ``:32-57``, compute_connection_loss ``:60-78``) over the HIP kernels; ``StructureTerm`` and
``ConnectionTerm`` are the last two as one native operator each."""
import torch

from .. import _lib


def recon_loss(pc_trans_list, pc_list, chamfer_dist):
    """Sum of the bidirectional per-point Chamfer distance (networks/loss.py:24-29).
    pc_trans_list, pc_list: [T-1, N, 3].  A ``utils.chamfer.ChamferLoss`` as ``chamfer_dist`` returns that sum itself
    (one warm-started native call with a fused backward)."""
    from ..utils.chamfer import ChamferLoss

    if isinstance(chamfer_dist, ChamferLoss):
        return chamfer_dist(pc_trans_list, pc_list)
    cd = chamfer_dist(pc_trans_list, pc_list, bidirectional=True)  # [T-1, N]
    return torch.sum(cd)


class _FlowLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gt, pred, mask, robust, smooth_weight):
        _lib.require_gpu(gt, pred, mask)
        gt, pred = gt.contiguous().float(), pred.contiguous().float()
        B, N, _ = pred.shape
        m = None if mask is None else (mask != 0).contiguous()  # bool: one byte per point
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        grad = torch.empty_like(pred)
        L = _lib.lib()
        ws = _lib.workspace(L.reart_flow_loss_workspace_bytes(), pred.device)
        rc = L.reart_flow_loss(_lib.ptr(gt), _lib.ptr(pred), _lib.ptr(m), B, N, int(bool(robust)),
                               float(smooth_weight), _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(ws), ws.numel(),
                               _lib.stream())
        _lib.check(rc, "reart_flow_loss")
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        gp = grad * g
        return None, gp, None, None, None


def flow_loss(gt_flow_list, pred_flow_list, flow_mask_list=None, robust=False, smooth_weight=1e-2):
    """networks/loss.py:10-21: masked MSE (or Huber, delta=1) between predicted and blended flow
    plus ``smooth_weight`` x |pred|^2 on the un-masked points; returns the scalar sum.
    Gradient flows to ``pred_flow_list`` (the reference computes ``gt_flow_list`` under no_grad)."""
    if gt_flow_list.requires_grad:
        raise NotImplementedError("flow_loss: gt_flow_list is a constant in the reference (run_robot.py:195)")
    return _FlowLoss.apply(gt_flow_list, pred_flow_list, flow_mask_list, robust, smooth_weight)


# ------------------------------------------------------------------------------------------------ structure term
def _structure_term_call(tr, pairs, weight, want_grad):
    """One ``reart_structure_term`` call on a contiguous float32 device tensor: ``tr`` [T,P,4,4] with ``pairs`` [E,2] int32,
    or the relative motions [T,E,4,4] with ``pairs=None`` -> (loss, edge_cost [E], prismatic [E] uint8, grad or None)."""
    T = tr.shape[0]
    if pairs is None:
        P, E = 1, tr.shape[1]
    else:
        P, E = tr.shape[1], pairs.shape[0]
        if E == 0:                                     # an empty tensor has no address: the call would read it as "no pairs"
            pairs = torch.zeros((1, 2), dtype=torch.int32, device=tr.device)
    if T > _lib.MAX_POSE_LEN:
        raise NotImplementedError(f"structure term: T = {T} frames above REART_MAX_POSE_LEN = {_lib.MAX_POSE_LEN}")
    if P > _lib.STRUCT_MAX_P:
        raise NotImplementedError(f"structure term: P = {P} parts above {_lib.STRUCT_MAX_P}")
    if E > _lib.STRUCT_MAX_E:
        raise NotImplementedError(f"structure term: E = {E} edges above {_lib.STRUCT_MAX_E}")
    dev = tr.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    cost = torch.empty((E,), dtype=torch.float32, device=dev)
    pris = torch.empty((E,), dtype=torch.uint8, device=dev)
    grad = torch.empty_like(tr) if want_grad else None
    L = _lib.lib()
    ws = _lib.workspace(L.reart_structure_term_workspace_bytes(T, P, E), dev)
    rc = L.reart_structure_term(_lib.ptr(tr), T, P, _lib.ptr(pairs), E, float(weight), _lib.ptr(loss), _lib.ptr(cost),
                                _lib.ptr(pris), _lib.ptr(grad), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "reart_structure_term")
    return loss, cost, pris, grad


def _check_transforms(t, what):
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: float32 transforms, not {t.dtype}")
    if t.dim() != 4 or tuple(t.shape[2:]) != (4, 4) or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what}: transforms [T,P,4,4], not {tuple(t.shape)}")


class _StructureTermFn(torch.autograd.Function):
    """Pattern of utils/flow_utils.py's _FlowTermFn: the forward has computed the value and its gradient, the backward
    scales the gradient by the upstream scalar."""

    @staticmethod
    def forward(ctx, trans, pairs, weight, sink):
        want = ctx.needs_input_grad[0]
        loss, cost, pris, grad = _structure_term_call(trans.detach().contiguous(), pairs, weight, want)
        if sink is not None:
            sink._last = (cost, pris)
        if want:
            ctx.save_for_backward(grad)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None


class StructureTerm(torch.nn.Module):
    """``forward(trans_list [T,P,4,4]) -> scalar``: ``weight`` x the reference's

        axis, moment, theta, distance, rel = compute_relative_trans(trans_list, return_trans=True)
        structure_loss(rel, axis, moment, theta, distance, edge_list)

    i.e. every edge's relative motion inv(T_src) T_tgt pulled towards the one-degree-of-freedom screw motion fitted to it
    over all frames (networks/loss.py:32-57), with its gradient for ``trans_list`` as one native call
    (``reart_structure_term``: two launches, no host synchronisation, the same bits on every run).  ``edge_list`` [E,2]
    (src, tgt) part indices; the fitted target is a constant, as in the reference.  Row 3 of a transform holds constants:
    its gradient is zero here (the reference's full 4x4 products leave a value there that reaches no parameter).  Without
    ``trans_list.requires_grad`` no gradient is computed.  ``.last`` holds ``(edge_cost [E], prismatic [E] bool)`` of the
    latest call.

    Limits: float32 (``TypeError`` otherwise), T <= 1024, P <= 64, E <= 4096 (``NotImplementedError``); an edge index
    outside [0, P) raises ``ValueError``; host tensors raise ``RuntimeError: ... no CPU fallback``."""

    def __init__(self, edge_list, weight=1.0):
        super().__init__()
        el = torch.as_tensor(edge_list).detach().cpu().to(torch.int64).reshape(-1, 2)
        self.weight = float(weight)
        self._lo = int(el.min()) if el.numel() else 0
        self._hi = int(el.max()) if el.numel() else -1
        self._edges = el.to(torch.int32).contiguous()
        self._pairs = {}
        self._last = None

    @property
    def last(self):
        return None if self._last is None else (self._last[0], self._last[1].bool())

    def forward(self, trans_list):
        _check_transforms(trans_list, "StructureTerm")
        if self._lo < 0 or self._hi >= trans_list.shape[1]:
            raise ValueError(f"StructureTerm: edge indices in [{self._lo}, {self._hi}] for P = {trans_list.shape[1]} parts")
        _lib.require_gpu(trans_list)
        pairs = self._pairs.get(trans_list.device)
        if pairs is None:
            pairs = self._pairs[trans_list.device] = self._edges.to(trans_list.device)
        return _StructureTermFn.apply(trans_list, pairs, self.weight, self)


def structure_loss(rel_trans_list, axis, moment, theta, distance, edge_list):
    """networks/loss.py:32-57 with the reference's signature: ``rel_trans_list`` [T,P,P,4,4] (of
    ``utils.graph_utils.compute_relative_trans(trans_list, return_trans=True)``), ``edge_list`` [E,2] -> the scalar sum over
    frames and edges of |rel inv(target) - I|^2.  The edges' relative motions are selected with torch indexing (the scatter
    back to [T,P,P,4,4] is autograd's) and go through ``reart_structure_term`` in its relative-motion form.  ``axis``,
    ``moment``, ``theta`` and ``distance`` are accepted for signature parity: the screw parameters are recomputed inside the
    kernel from ``rel_trans_list``, as ``compute_geo_cost`` does.  The range of ``edge_list`` is read on the host in every call
    (``ValueError`` outside [0, P)); ``StructureTerm`` reads it once, at construction, and needs no relative transforms."""
    if rel_trans_list.dtype != torch.float32:
        raise TypeError(f"structure_loss: float32 transforms, not {rel_trans_list.dtype}")
    if rel_trans_list.dim() != 5 or rel_trans_list.shape[1] != rel_trans_list.shape[2] or tuple(rel_trans_list.shape[3:]) != (4, 4):
        raise ValueError(f"structure_loss: rel_trans_list [T,P,P,4,4], not {tuple(rel_trans_list.shape)}")
    P = rel_trans_list.shape[1]
    el = torch.as_tensor(edge_list).reshape(-1, 2).long()
    if el.numel() and (int(el.min()) < 0 or int(el.max()) >= P):
        raise ValueError(f"structure_loss: edge indices in [{int(el.min())}, {int(el.max())}] for P = {P} parts")
    _lib.require_gpu(rel_trans_list)
    el = el.to(rel_trans_list.device)
    sel = rel_trans_list[:, el[:, 0], el[:, 1]]
    return _StructureTermFn.apply(sel, None, 1.0, None)


def compute_connection_loss(cano_pc, seg_part, joint_connection, pc_trans_list, chamfer_dist, k=10):
    """networks/loss.py:60-78: per edge the ``k`` closest (source point, nearest target point) pairs between the two parts in
    the canonical cloud, and the mean squared distance of those pairs in every frame of ``pc_trans_list`` [T,N,3]; summed
    over edges and frames.  A composition of what exists (``chamfer_dist(..., return_index=True)``, ``torch.topk``, gathers):
    differentiable w.r.t. ``pc_trans_list`` through torch indexing, one search per edge."""
    _lib.require_gpu(cano_pc, seg_part, pc_trans_list)
    loss = 0
    for edge in joint_connection:
        src_mask, tgt_mask = seg_part == edge[0], seg_part == edge[1]
        src_pc, tgt_pc = cano_pc[src_mask], cano_pc[tgt_mask]
        src_cano_idx, tgt_cano_idx = torch.where(src_mask)[0], torch.where(tgt_mask)[0]
        dist, nn_idx = chamfer_dist(src_pc[None], tgt_pc[None], return_index=True)
        dist, nn_idx = dist.squeeze(dim=0), nn_idx.squeeze(dim=0)
        _, src_idx = torch.topk(dist, k=k, dim=0, largest=False)
        raw_src, raw_tgt = src_cano_idx[src_idx], tgt_cano_idx[nn_idx[src_idx].long()]
        d = ((pc_trans_list[:, raw_src, :] - pc_trans_list[:, raw_tgt, :]) ** 2).sum(dim=2).mean(dim=1)
        loss = loss + d
    return loss.sum(dim=0)


# ----------------------------------------------------------------------------------------------- connection term
def _connection_select_call(cano, seg, pairs, P, k):
    """One ``reart_connection_select`` call on contiguous device tensors -> (src_idx [E,k] i32, tgt_idx [E,k] i32, valid [E] u8)."""
    N, E, dev = cano.shape[0], pairs.shape[0], cano.device
    src = torch.empty((E, k), dtype=torch.int32, device=dev)
    tgt = torch.empty((E, k), dtype=torch.int32, device=dev)
    valid = torch.empty((E,), dtype=torch.uint8, device=dev)
    L = _lib.lib()
    ws = _lib.workspace(L.reart_connection_select_workspace_bytes(N, P, E, k), dev)
    rc = L.reart_connection_select(_lib.ptr(cano), _lib.ptr(seg), N, P, _lib.ptr(pairs), E, k, _lib.ptr(src), _lib.ptr(tgt), None,
                                   _lib.ptr(valid), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "reart_connection_select")
    return src, tgt, valid


def _connection_term_call(pc, src, tgt, valid, k, weight, want_grad):
    """One ``reart_connection_term`` call -> (loss, edge_cost [E], grad or None)."""
    T, N, E, dev = pc.shape[0], pc.shape[1], src.shape[0], pc.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    cost = torch.empty((E,), dtype=torch.float32, device=dev)
    grad = torch.empty_like(pc) if want_grad else None
    L = _lib.lib()
    ws = _lib.workspace(L.reart_connection_term_workspace_bytes(T, N, E, k), dev)
    rc = L.reart_connection_term(_lib.ptr(pc), _lib.ptr(src), _lib.ptr(tgt), _lib.ptr(valid), T, N, E, k, float(weight),
                                 _lib.ptr(loss), _lib.ptr(cost), _lib.ptr(grad), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "reart_connection_term")
    return loss, cost, grad


class _ConnectionTermFn(torch.autograd.Function):
    """The _StructureTermFn pattern: the forward has computed the value and its gradient, the backward scales it."""

    @staticmethod
    def forward(ctx, pc, src, tgt, valid, k, weight, sink):
        want = ctx.needs_input_grad[0]
        loss, cost, grad = _connection_term_call(pc.detach().contiguous(), src, tgt, valid, k, weight, want)
        sink._last = (cost, src, tgt, valid)
        if want:
            ctx.save_for_backward(grad)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None, None, None, None


class ConnectionTerm(torch.nn.Module):
    """``forward(cano_pc [N,3], seg_part [N], pc_trans_list [T,N,3]) -> scalar``: ``weight`` x the reference's

        compute_connection_loss(cano_pc, seg_part, joint_connection, pc_trans_list, chamfer_dist, k)

    (networks/loss.py:60-78) as two native calls on the current stream, ``reart_connection_select`` and
    ``reart_connection_term`` (six launches, no host synchronisation, the same bits on every run): per edge (a, b) of
    ``joint_connection`` [E,2] the ``k`` points of part a closest to part b, each with its nearest point of part b, in the
    canonical cloud; then the mean over those pairs of their squared distance in every frame, summed over frames and edges.
    Differentiable w.r.t. ``pc_trans_list``; the selection is a constant, as in the reference.  Without
    ``pc_trans_list.requires_grad`` no gradient buffer is allocated.

    Ties, where ``topk`` and the search of the composition leave the choice open: the nearest point is the one of lowest
    index, the ``k`` sources are the smallest (distance, index).  An edge whose source part has fewer than ``k`` points or
    whose target part is empty (the reference raises) is invalid: it costs nothing and has no gradient.  A label outside
    [0, P) belongs to no part.

    ``select(cano_pc, seg_part)`` computes and keeps the tables; ``forward(pc_trans_list)`` with one argument then reuses
    them (one native call; a KinematicModel's cloud and labels never change) until ``reset()``.
    ``.last`` holds ``(edge_cost [E], src_idx [E,k], tgt_idx [E,k], valid [E] bool)`` of the latest call.

    P is the largest edge index + 1 unless ``num_parts`` is given.  Limits: float32 clouds (``TypeError`` otherwise);
    T <= 1024, P <= 64, E <= 4096, 1 <= k <= 64, N <= 65 536 (``NotImplementedError``); an edge index outside [0, P) or a
    shape mismatch raises ``ValueError``; host tensors raise ``RuntimeError: ... no CPU fallback``."""

    def __init__(self, joint_connection, k=10, weight=1.0, num_parts=None):
        super().__init__()
        el = torch.as_tensor(joint_connection).detach().cpu().to(torch.int64).reshape(-1, 2)
        self.k, self.weight = int(k), float(weight)
        self._lo = int(el.min()) if el.numel() else 0
        self._hi = int(el.max()) if el.numel() else -1
        self.num_parts = int(num_parts) if num_parts is not None else max(self._hi + 1, 1)
        self._edges = el.to(torch.int32).contiguous()
        self._pairs = {}
        self._kept = None      # (src_idx, tgt_idx, valid, N) of select()
        self._last = None

    @property
    def last(self):
        return None if self._last is None else self._last[:3] + (self._last[3].bool(),)

    def reset(self):
        self._kept = None

    def _check_static(self):
        if self._lo < 0 or self._hi >= self.num_parts:
            raise ValueError(f"ConnectionTerm: edge indices in [{self._lo}, {self._hi}] for P = {self.num_parts} parts")

    def _check_limits(self, N, T=1):
        E = self._edges.shape[0]
        if T > _lib.MAX_POSE_LEN:
            raise NotImplementedError(f"connection term: T = {T} frames above REART_MAX_POSE_LEN = {_lib.MAX_POSE_LEN}")
        if self.num_parts > _lib.STRUCT_MAX_P:
            raise NotImplementedError(f"connection term: P = {self.num_parts} parts above {_lib.STRUCT_MAX_P}")
        if E > _lib.STRUCT_MAX_E:
            raise NotImplementedError(f"connection term: E = {E} edges above {_lib.STRUCT_MAX_E}")
        if not 1 <= self.k <= _lib.CONN_MAX_K:
            raise NotImplementedError(f"connection term: k = {self.k} outside [1, {_lib.CONN_MAX_K}]")
        if N > _lib.CONN_MAX_N:
            raise NotImplementedError(f"connection term: N = {N} points above {_lib.CONN_MAX_N}")

    @staticmethod
    def _check_cloud(cano, seg):
        if cano.dtype != torch.float32:
            raise TypeError(f"ConnectionTerm: a float32 canonical cloud, not {cano.dtype}")
        if seg.dtype.is_floating_point or seg.dtype.is_complex or seg.dtype == torch.bool:
            raise TypeError(f"ConnectionTerm: integer labels, not {seg.dtype}")
        if cano.dim() != 2 or cano.shape[1] != 3 or cano.shape[0] < 1 or tuple(seg.shape) != (cano.shape[0],):
            raise ValueError(f"ConnectionTerm: cano_pc [N,3] and seg_part [N], not {tuple(cano.shape)} and {tuple(seg.shape)}")

    @staticmethod
    def _check_frames(pc, N):
        if pc.dtype != torch.float32:
            raise TypeError(f"ConnectionTerm: float32 frames, not {pc.dtype}")
        if pc.dim() != 3 or pc.shape[0] < 1 or tuple(pc.shape[1:]) != (N, 3):
            raise ValueError(f"ConnectionTerm: pc_trans_list [T,{N},3], not {tuple(pc.shape)}")

    def _select(self, cano, seg):
        pairs = self._pairs.get(cano.device)
        if pairs is None:
            pairs = self._pairs[cano.device] = self._edges.to(cano.device)
        return _connection_select_call(cano.detach().contiguous(), seg.to(torch.int64).contiguous(), pairs, self.num_parts, self.k)

    def select(self, cano_pc, seg_part):
        self._check_cloud(cano_pc, seg_part)
        self._check_static()
        self._check_limits(cano_pc.shape[0])
        _lib.require_gpu(cano_pc, seg_part)
        self._kept = self._select(cano_pc, seg_part) + (cano_pc.shape[0],)
        return self

    def forward(self, *args):
        if len(args) == 1:
            (pc,) = args
            if self._kept is None:
                raise RuntimeError("ConnectionTerm: forward(pc_trans_list) needs the tables of select(cano_pc, seg_part)")
            src, tgt, valid, N = self._kept
            self._check_frames(pc, N)
            self._check_limits(N, pc.shape[0])
            _lib.require_gpu(pc)
            if pc.device != src.device:
                raise ValueError(f"ConnectionTerm: tables on {src.device}, frames on {pc.device}")
        else:
            cano, seg, pc = args
            self._check_cloud(cano, seg)
            self._check_frames(pc, cano.shape[0])
            self._check_static()
            self._check_limits(cano.shape[0], pc.shape[0])
            _lib.require_gpu(cano, seg, pc)
            src, tgt, valid = self._select(cano, seg)
        return _ConnectionTermFn.apply(pc, src, tgt, valid, self.k, self.weight, self)


# ------------------------------------------------------------------------------------------- descriptor InfoNCE
def _infonce_forward_call(f1, f2, pos, mask, tau):
    """One ``reart_infonce_forward`` call on contiguous device tensors -> (loss, row_loss [B,N1], lse [B,N1], top [B,N1], count)."""
    (B, N1, C), N2, dev = f1.shape, f2.shape[1], f1.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    row_loss = torch.empty((B, N1), dtype=torch.float32, device=dev)
    lse = torch.empty((B, N1), dtype=torch.float32, device=dev)
    top = torch.empty((B, N1), dtype=torch.int64, device=dev)
    count = torch.empty((), dtype=torch.int64, device=dev)
    L = _lib.lib()
    ws = _lib.workspace(L.reart_infonce_scratch_bytes(B, N1, N2, C), dev)
    rc = L.reart_infonce_forward(_lib.ptr(f1), _lib.ptr(f2), _lib.ptr(pos), _lib.ptr(mask), B, N1, N2, C, float(tau), _lib.ptr(loss),
                                 _lib.ptr(row_loss), _lib.ptr(lse), _lib.ptr(top), _lib.ptr(count), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "reart_infonce_forward")
    return loss, row_loss, lse, top, count


def _infonce_backward_call(f1, f2, pos, mask, lse, count, g, tau, want1, want2):
    """One ``reart_infonce_backward`` call -> (dF1 or None, dF2 or None); ``g`` a float32 device scalar or None (= 1)."""
    (B, N1, C), N2, dev = f1.shape, f2.shape[1], f1.device
    d1 = torch.empty_like(f1) if want1 else None
    d2 = torch.empty_like(f2) if want2 else None
    if (want1 and d1.numel()) or (want2 and d2.numel()):
        L = _lib.lib()
        ws = _lib.workspace(L.reart_infonce_scratch_bytes(B, N1, N2, C), dev)
        rc = L.reart_infonce_backward(_lib.ptr(f1), _lib.ptr(f2), _lib.ptr(pos), _lib.ptr(mask), _lib.ptr(lse), _lib.ptr(count), _lib.ptr(g),
                                      B, N1, N2, C, float(tau), _lib.ptr(d1) if want1 and d1.numel() else None,
                                      _lib.ptr(d2) if want2 and d2.numel() else None, _lib.ptr(ws), ws.numel(), _lib.stream())
        _lib.check(rc, "reart_infonce_backward")
    return d1, d2


class _InfoNCEFn(torch.autograd.Function):
    """The forward keeps the operands, lse and count; the backward is one native call that recomputes the logits, for the
    operands that need a gradient only."""

    @staticmethod
    def forward(ctx, f1, f2, pos, mask, tau, sink):
        ctx.set_materialize_grads(False)
        f1c, f2c = f1.detach().contiguous(), f2.detach().contiguous()
        loss, row_loss, lse, top, count = _infonce_forward_call(f1c, f2c, pos, mask, tau)
        if sink is not None:
            sink._last = (row_loss, top, count, pos)
        ctx.tau, ctx.has_mask = tau, mask is not None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(*((f1c, f2c, pos, lse, count) + ((mask,) if mask is not None else ())))
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None, None
        f1c, f2c, pos, lse, count = ctx.saved_tensors[:5]
        mask = ctx.saved_tensors[5] if ctx.has_mask else None
        d1, d2 = _infonce_backward_call(f1c, f2c, pos, mask, lse, count, g.detach().to(torch.float32).contiguous(), ctx.tau,
                                        ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return d1, d2, None, None, None, None


class DescriptorInfoNCE(torch.nn.Module):
    """``forward(f1 [B,N1,C], f2 [B,N2,C], pos [B,N1] int64, col_mask=None) -> scalar``: the contrastive descriptor loss
    (PointInfoNCE) on two descriptor sets.  With s_ij = <f1_i, f2_j> / tau the loss is the mean over the used rows of

        log sum_j exp(s_ij) - s_i,pos(i)        (``F.cross_entropy(f1 @ f2.T / tau, pos)`` with masked columns at -inf)

    as one native operator (``reart_infonce_forward`` / ``reart_infonce_backward``): the logits are formed tile by tile on
    the fp32 matrix cores and never stored, the backward recomputes them, every sum has a fixed order (the same bits on
    every run), nothing synchronises with the host.  ``pos[b, i]`` is the column of ``f2`` that is the positive of row i; an
    entry outside [0, N2), the conventional -1 included, means the row is not used.  ``col_mask`` [B,N2] bool / uint8: a
    false column takes part in no row's sum, and a row whose positive is masked out is not used.  With no used row the
    loss is exactly 0.  First-order gradients reach ``f1`` and ``f2``, whichever require them; nothing is computed for one
    that does not.

    The descriptors are used as given: for cosine logits apply ``F.normalize`` to them first, autograd carries it.

    ``symmetric=True`` adds the loss of the transposed problem (``f2`` against ``f1``) and halves the sum: there the
    positive of column j is the lowest row i with ``pos(i) = j`` among the used rows, columns no used row names (masked
    ones among them) are unused and no column of ``f1`` is masked; two native calls, the inverse map built on the device.

    ``.last`` holds ``(row_loss [B,N1], top [B,N1], count)`` of the latest call (of ``f1`` against ``f2``): ``top`` is the
    lowest live column attaining the row's maximum, -1 on unused rows; ``accuracy()`` is the share of used rows with
    ``top == pos``, a 0-d device tensor.

    Limits: float32 descriptors, int64 ``pos``, bool / uint8 mask (``TypeError`` otherwise); 1 <= C <= 256, N1 and
    N2 <= 65 536, B <= 1024 (``NotImplementedError``); shape mismatches and ``tau <= 0`` raise ``ValueError``; host tensors
    raise ``RuntimeError: ... no CPU fallback``."""

    def __init__(self, tau=0.07, symmetric=False):
        super().__init__()
        if not float(tau) > 0.0:
            raise ValueError(f"DescriptorInfoNCE: tau = {tau} must be positive")
        self.tau, self.symmetric = float(tau), bool(symmetric)
        self._last = None

    @property
    def last(self):
        return None if self._last is None else self._last[:3]

    def accuracy(self):
        if self._last is None:
            raise RuntimeError("DescriptorInfoNCE: accuracy() follows a forward call")
        _, top, count, pos = self._last
        hit = ((top == pos) & (top >= 0)).sum()
        return hit.to(torch.float32) / count.clamp(min=1).to(torch.float32)

    @staticmethod
    def _check(f1, f2, pos, col_mask):
        if f1.dtype != torch.float32 or f2.dtype != torch.float32:
            raise TypeError(f"DescriptorInfoNCE: float32 descriptors, not {f1.dtype} and {f2.dtype}")
        if pos.dtype != torch.int64:
            raise TypeError(f"DescriptorInfoNCE: int64 positives, not {pos.dtype}")
        if col_mask is not None and col_mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"DescriptorInfoNCE: a bool or uint8 column mask, not {col_mask.dtype}")
        if f1.dim() != 3 or f2.dim() != 3 or f1.shape[0] != f2.shape[0] or f1.shape[2] != f2.shape[2] or f1.shape[2] < 1:
            raise ValueError(f"DescriptorInfoNCE: f1 [B,N1,C] and f2 [B,N2,C], not {tuple(f1.shape)} and {tuple(f2.shape)}")
        if tuple(pos.shape) != tuple(f1.shape[:2]):
            raise ValueError(f"DescriptorInfoNCE: pos {tuple(f1.shape[:2])}, not {tuple(pos.shape)}")
        if col_mask is not None and tuple(col_mask.shape) != tuple(f2.shape[:2]):
            raise ValueError(f"DescriptorInfoNCE: col_mask {tuple(f2.shape[:2])}, not {tuple(col_mask.shape)}")
        B, N1, C = f1.shape
        if C > _lib.MAX_D:
            raise NotImplementedError(f"DescriptorInfoNCE: C = {C} above REART_MAX_D = {_lib.MAX_D}")
        if max(N1, f2.shape[1]) > _lib.NCE_MAX_N:
            raise NotImplementedError(f"DescriptorInfoNCE: N1 = {N1}, N2 = {f2.shape[1]} above {_lib.NCE_MAX_N}")
        if B > _lib.NCE_MAX_B:
            raise NotImplementedError(f"DescriptorInfoNCE: B = {B} above {_lib.NCE_MAX_B}")
        _lib.require_gpu(f1, f2, pos, col_mask)

    @staticmethod
    def _transposed_positives(pos, mask, N2):
        """[B,N2]: the lowest used row naming each column, -1 where none does."""
        B, N1 = pos.shape
        if N2 == 0 or N1 == 0:
            return torch.full((B, N2), -1, dtype=torch.int64, device=pos.device)
        used = (pos >= 0) & (pos < N2)
        col = torch.where(used, pos, torch.zeros_like(pos))
        if mask is not None:
            used = used & (mask.gather(1, col) != 0)
            col = torch.where(used, col, torch.zeros_like(pos))
        row = torch.arange(N1, dtype=torch.int64, device=pos.device).expand(B, N1)
        row = torch.where(used, row, torch.full_like(row, N1))
        inv = torch.full((B, N2), N1, dtype=torch.int64, device=pos.device)
        inv.scatter_reduce_(1, col, row, "amin", include_self=True)           # a minimum of integers: any order, one result
        return torch.where(inv >= N1, torch.full_like(inv, -1), inv)

    def forward(self, f1, f2, pos, col_mask=None):
        if not self.tau > 0.0:
            raise ValueError(f"DescriptorInfoNCE: tau = {self.tau} must be positive")
        self._check(f1, f2, pos, col_mask)
        pos = pos.detach().contiguous()
        mask = None if col_mask is None else col_mask.detach().to(torch.uint8).contiguous()
        loss = _InfoNCEFn.apply(f1, f2, pos, mask, self.tau, self)
        if self.symmetric:
            pos_t = self._transposed_positives(pos, mask, f2.shape[1])
            loss = 0.5 * (loss + _InfoNCEFn.apply(f2, f1, pos_t, None, self.tau, None))
        return loss
