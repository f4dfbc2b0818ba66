"""Host-side mirror of the reference's ``networks/loss.py`` (recon_loss ``:24-29``, flow_loss
``:10-21``, structure_loss ``:32-57``, compute_connection_loss ``:60-78``) over the HIP kernels."""
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
