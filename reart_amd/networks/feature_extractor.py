"""Host-side mirror of the reference's ``networks/feature_extractor.py`` (PointNet2Msg2, the
64-d per-point correspondence descriptor net, ``:10-49``) over the HIP kernels: FPS and ball
query (``reart_fps`` / ``reart_ball_query``), gather-fused 1x1-conv stacks with max-pool on the
fp32 matrix cores (``reart_mlp_layer``) and 3-NN interpolation (``reart_three_interpolate``).

Module / parameter names equal the reference's (``sa1.conv_blocks.0.0.weight``, ``sa1.bn_blocks...``,
``sa3.mlp_convs.0``, ``fp1.mlp_bns.1``, ``conv1``, ``bn1``) so ``corr_model.pth.tar``-style checkpoints
load with ``strict=True`` (feature_extractor.py:62-86).  ``eval()`` only (the reference freezes the
extractor, ``rec_freeze`` :52-59): BatchNorm uses running statistics and is folded into the conv.

``forward(..., grad=True)`` builds a first-order autograd graph from the descriptors to the conv / BatchNorm parameters (and,
for the layer classes, to the incoming features) over ``reart_mlp_layer_backward`` / ``reart_three_interpolate_backward``
(csrc/pointnet_grad.hip): fine-tuning a checkpoint in ``eval()`` mode.  Coordinates get no gradient -- neither the
``xyz - centre`` columns, nor the centres, nor the interpolation weights, nor the extractor's level-0 features (which ARE the
input cloud); the parameters' gradients are complete all the same, because parameters are reached through features only.
Training-mode BatchNorm (batch statistics) and second derivatives are not built.  The default, ``grad=False``, is the
inference path as it always was.
"""
import torch
import torch.nn as nn

from .. import _lib


def _fold(conv, bn):
    """eval-mode BN folded into the 1x1 conv -> (Wt [Cin, Cout] contiguous, bias [Cout]).  The folded pair is kept on the
    conv module until one of the six tensors it was made from changes (in-place updates and ``load_state_dict`` bump
    ``_version``; a re-assigned tensor is another object): nine tiny launches per layer and forward otherwise,
    a sixth of the extractor's device time.  The entry holds references to its source tensors, so an address cannot be
    recycled under it.  NOT seen: writes through ``.data`` (``p.data.copy_()``, ``p.data.mul_()`` -- they bypass the
    version counter); after such an update call ``PointNet2Msg2.invalidate_fold()`` (``.train()``, ``.to()`` / ``.cuda()``
    / ``.float()`` and ``load_state_dict`` on the extractor do it themselves)."""
    src = (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)
    key = tuple((id(t), t.data_ptr(), t._version) if t is not None else None for t in src) + (bn.eps,)
    hit = getattr(conv, "_reart_folded", None)
    if hit is not None and hit[0] == key:
        return hit[1], hit[2]
    Wt, bf = _fold_now(conv, bn)
    conv._reart_folded = (key, Wt, bf, src)          # src: keeps the keyed tensors (and their addresses) alive
    return Wt, bf


def _fold_now(conv, bn):
    w = conv.weight.detach().reshape(conv.weight.shape[0], -1).float()
    b = conv.bias.detach().float() if conv.bias is not None else torch.zeros(w.shape[0], device=w.device)
    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    wf = w * scale[:, None]
    bf = (b - bn.running_mean.detach().float()) * scale + bn.bias.detach().float()
    return wf.t().contiguous(), bf.contiguous()


def _fold_grad(conv, bn):
    """The differentiable twin of ``_fold_now``: the same tensor expression, operation for operation (the same bits), WITHOUT the
    detach -- the folded pair carries a graph to conv.weight, conv.bias, bn.weight and bn.bias (whichever require grad).  The
    running statistics are constants.  Never cached."""
    w = conv.weight.reshape(conv.weight.shape[0], -1).float()
    b = conv.bias.float() if conv.bias is not None else torch.zeros(w.shape[0], device=w.device)
    scale = bn.weight.float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    wf = w * scale[:, None]
    bf = (b - bn.running_mean.detach().float()) * scale + bn.bias.float()
    return wf.t().contiguous(), bf.contiguous()


def _grad_operand(name, t):
    """What the differentiable path takes: float32, contiguous, on the GPU -- refused before anything is launched."""
    if t is None:
        return
    _lib.require_gpu(t)
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: float32 expected, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: a contiguous tensor expected")


def require_grad_mode(what):
    if not torch.is_grad_enabled():
        raise RuntimeError(f"{what}: grad=True needs autograd enabled (called under torch.no_grad())")


def _layer_args(X, gather):
    """The operand description of reart_mlp_layer / reart_mlp_layer_backward -> (arguments, rows, (B, Npts, D))."""
    if gather is None:
        rows, ldx = X.shape
        return (_lib.ptr(X), ldx, None, 0, 0, 0, None, 0, None, None, 0), rows, (0, 0, 0)
    B, S, K = gather["idx"].shape
    F = gather.get("F")
    D = 0 if F is None else F.shape[1]
    return ((None, 0, _lib.ptr(gather["idx"]), K, S, gather["Npts"], _lib.ptr(F), D, _lib.ptr(gather["Q"]), _lib.ptr(gather.get("C")),
             int(gather.get("xyz_first", 0))), B * S * K, (B, gather["Npts"], D))


GRAD_CALLS = {"parameter": 0, "feature": 0}    # layer backwards that computed dWt / dbias, and dX / dF (a frozen module: no "parameter")


class _MlpLayerGrad(torch.autograd.Function):
    """``mlp_layer`` with a first-order backward (reart_mlp_layer_backward).  ``feat`` is the plain X, or the gathered form's F
    (None for D = 0); ``gather`` holds the constants of the gathered form (idx, Q, C, Npts, xyz_first): coordinates get no
    gradient.  The forward is the launch of ``mlp_layer``.  An un-pooled layer keeps its output, which is the activation the
    backward selects by; a pooled layer keeps its operands only and the backward runs the un-pooled launch again."""

    @staticmethod
    def forward(ctx, feat, Wt, bias, gather, relu, pool_k):
        ctx.set_materialize_grads(False)
        g = None if gather is None else dict(gather, F=feat)
        out = mlp_layer(feat if g is None else None, Wt, bias, relu=relu, pool_k=pool_k, gather=g)
        ctx.pooled = pool_k > 1
        ctx.save_for_backward(feat, Wt, bias, None if ctx.pooled else out)
        ctx.gather, ctx.relu, ctx.pool_k = gather, relu, pool_k
        return out

    @staticmethod
    def backward(ctx, dY):
        feat, Wt, bias, A = ctx.saved_tensors
        need_f, need_w, need_b = (ctx.needs_input_grad[0] and feat is not None and feat.shape[1] > 0, ctx.needs_input_grad[1],
                                  ctx.needs_input_grad[2] and bias is not None)
        if dY is None or not (need_f or need_w or need_b):
            return None, None, None, None, None, None
        L = _lib.lib()
        gather, relu, pool_k = ctx.gather, ctx.relu, ctx.pool_k
        g = None if gather is None else dict(gather, F=feat)
        X = feat if g is None else None
        dY = dY.contiguous()
        Cin, Cout = Wt.shape
        if A is None:
            A = mlp_layer(X, Wt, bias, relu=relu, pool_k=0, gather=g)
        args, rows, (B, Npts, D) = _layer_args(X, g)
        dWt = torch.empty_like(Wt) if need_w else None
        db = torch.empty_like(bias) if need_b else None
        dfeat = torch.empty_like(feat) if need_f else None
        GRAD_CALLS["parameter"] += int(need_w or need_b)
        GRAD_CALLS["feature"] += int(need_f)
        ws = _lib.workspace(L.reart_mlp_layer_backward_scratch_bytes(rows, Cin, Cout, B, Npts, D), Wt.device)
        rc = L.reart_mlp_layer_backward(*args, _lib.ptr(Wt), rows, Cin, Cout, int(relu), pool_k if ctx.pooled else 0, _lib.ptr(A),
                                        _lib.ptr(dY), dY.shape[1], 0, _lib.ptr(dWt), _lib.ptr(db),
                                        _lib.ptr(dfeat) if g is None else None, Cin, _lib.ptr(dfeat) if g is not None else None,
                                        _lib.ptr(ws), ws.numel(), _lib.stream())
        _lib.check(rc, "reart_mlp_layer_backward")
        return dfeat, dWt, db, None, None, None


class _ThreeInterpolateGrad(torch.autograd.Function):
    """``three_interpolate`` into a tensor of its own with a backward to ``points2`` (reart_three_interpolate_backward, which finds
    the three neighbours again from the coordinates: nothing but the operands is kept)."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, points2):
        ctx.set_materialize_grads(False)
        B, N, _ = xyz1.shape
        out = torch.empty((B * N, points2.shape[2]), dtype=torch.float32, device=points2.device)
        three_interpolate(xyz1, xyz2, points2, out, 0)
        ctx.save_for_backward(xyz1, xyz2)
        ctx.shape = tuple(points2.shape)
        return out

    @staticmethod
    def backward(ctx, dOut):
        if dOut is None or not ctx.needs_input_grad[2]:
            return None, None, None
        xyz1, xyz2 = ctx.saved_tensors
        L = _lib.lib()
        B, S2, D = ctx.shape
        N = xyz1.shape[1]
        dOut = dOut.contiguous()
        dP2 = torch.empty(ctx.shape, dtype=torch.float32, device=dOut.device)
        ws = _lib.workspace(L.reart_three_interpolate_backward_scratch_bytes(B, N, S2), dOut.device)
        rc = L.reart_three_interpolate_backward(_lib.ptr(xyz1), _lib.ptr(xyz2), _lib.ptr(dOut), dOut.shape[1], 0, B, N, S2, D,
                                                _lib.ptr(dP2), None, _lib.ptr(ws), ws.numel(), _lib.stream())
        _lib.check(rc, "reart_three_interpolate_backward")
        return None, None, dP2


def mlp_layer(X, Wt, bias, relu=True, pool_k=0, out=None, out_col=0, gather=None, grad=False):
    """Y = relu(X Wt + bias) [max over pool_k consecutive rows] via reart_mlp_layer.
    gather = dict(idx [B,S,K] i64, F [B*Npts,D] or None, Q [B*Npts,3], C [B*S,3] or None, Npts, xyz_first).
    ``grad=True``: the same launch and bits, in a tensor of its own (``out`` must be None) that carries a first-order graph to
    X (or gather["F"]), Wt and bias, whichever require grad; coordinates (Q, C) get none."""
    if grad:
        require_grad_mode("mlp_layer")
        if out is not None:
            raise ValueError("mlp_layer(grad=True) returns a tensor of its own: out must be None")
        feat = X if gather is None else gather.get("F")
        for name, t in (("X" if gather is None else "F", feat), ("Wt", Wt), ("bias", bias)):
            _grad_operand(name, t)
        if gather is not None:
            for name in ("Q", "C"):
                _grad_operand(name, gather.get(name))
            gather = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in gather.items() if k != "F"}
        return _MlpLayerGrad.apply(feat, Wt, bias, gather, bool(relu), int(pool_k))
    L = _lib.lib()
    Cin, Cout = Wt.shape
    if gather is None:
        rows, ldx = X.shape
        args = (_lib.ptr(X), ldx, None, 0, 0, 0, None, 0, None, None, 0)
    else:
        B, S, K = gather["idx"].shape
        rows = B * S * K
        F = gather.get("F")
        args = (None, 0, _lib.ptr(gather["idx"]), K, S, gather["Npts"], _lib.ptr(F), 0 if F is None else F.shape[1],
                _lib.ptr(gather["Q"]), _lib.ptr(gather.get("C")), int(gather.get("xyz_first", 0)))
    orows = rows // pool_k if pool_k else rows
    if out is None:
        out = torch.empty((orows, Cout), dtype=torch.float32, device=Wt.device)
    rc = L.reart_mlp_layer(*args, _lib.ptr(Wt), _lib.ptr(bias), rows, Cin, Cout, int(relu), pool_k, _lib.ptr(out),
                           out.shape[1], out_col, _lib.stream())
    _lib.check(rc, "reart_mlp_layer")
    return out


OVERLAP_SAMPLING = True      # the second level's FPS / ball queries on a side stream under the first level's GEMMs
_SIDE = {}


def _side_stream(device):
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=device)
    return _SIDE[key]


CHAIN3 = {(32, 32, 64, 32), (64, 64, 128, 64), (64, 96, 128, 128)}    # (C1, C2, C3, nsample) built into reart_mlp_chain3
CHAIN3_WIDE = {(128, 128, 256, 64), (128, 196, 256, 128)}             # sa2's scales, built into reart_mlp_chain3_wide
FUSE_CHAIN = True      # False: every layer its own launch (the same bits; tests compare the two)


def mlp_chain3(folded, gather, out, out_col):
    """Three gathered 1x1-conv layers + max over the group in ONE launch (reart_mlp_chain3): ``folded`` = [(Wt, bias)] x 3,
    ``gather`` as for ``mlp_layer`` with 3 feature columns; the result lands in out[:, out_col:out_col + C3]."""
    L = _lib.lib()
    (W1, b1), (W2, b2), (W3, b3) = folded
    B, S, K = gather["idx"].shape
    rc = L.reart_mlp_chain3(_lib.ptr(gather["idx"]), K, S, gather["Npts"], _lib.ptr(gather["F"]), _lib.ptr(gather["Q"]),
                            _lib.ptr(gather["C"]), _lib.ptr(W1), _lib.ptr(b1), W1.shape[1], _lib.ptr(W2), _lib.ptr(b2), W2.shape[1],
                            _lib.ptr(W3), _lib.ptr(b3), W3.shape[1], B * S * K, _lib.ptr(out), out.shape[1], out_col, _lib.stream())
    _lib.check(rc, "reart_mlp_chain3")
    return out


def mlp_chain3_wide(folded, gather, out, out_col):
    """The same for a scale with D (% 4 == 0) feature columns and wide layers (reart_mlp_chain3_wide: the weights stream
    through LDS, a workgroup carries 128 rows through the three layers)."""
    L = _lib.lib()
    (W1, b1), (W2, b2), (W3, b3) = folded
    B, S, K = gather["idx"].shape
    F = gather["F"]
    ws = _lib.workspace(L.reart_mlp_chain3_wide_workspace_bytes(F.shape[1], W1.shape[1], W2.shape[1], W3.shape[1]), F.device)
    rc = L.reart_mlp_chain3_wide(_lib.ptr(gather["idx"]), K, S, gather["Npts"], _lib.ptr(F), F.shape[1], _lib.ptr(gather["Q"]),
                                 _lib.ptr(gather["C"]), _lib.ptr(W1), _lib.ptr(b1), W1.shape[1], _lib.ptr(W2), _lib.ptr(b2),
                                 W2.shape[1], _lib.ptr(W3), _lib.ptr(b3), W3.shape[1], B * S * K, _lib.ptr(out), out.shape[1], out_col,
                                 _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "reart_mlp_chain3_wide")
    return out


def three_interpolate(xyz1, xyz2, points2, out, out_col, grad=False):
    """PointNetFeaturePropagation's 3-NN interpolation written into out[:, out_col:out_col+D].
    ``grad=True``: returned as a [B*N, D] tensor of its own (``out`` must be None) with a first-order graph to ``points2``; the
    neighbours and their weights are functions of the coordinates and get no gradient."""
    if grad:
        require_grad_mode("three_interpolate")
        if out is not None:
            raise ValueError("three_interpolate(grad=True) returns a tensor of its own: out must be None")
        for name, t in (("xyz1", xyz1), ("xyz2", xyz2), ("points2", points2)):
            _grad_operand(name, t)
        return _ThreeInterpolateGrad.apply(xyz1.detach(), xyz2.detach(), points2)
    L = _lib.lib()
    B, N, _ = xyz1.shape
    S2, D = points2.shape[1], points2.shape[2]
    ws = _lib.workspace(L.reart_three_interpolate_workspace_bytes(B, N, S2), xyz1.device)
    rc = L.reart_three_interpolate(_lib.ptr(xyz1), _lib.ptr(xyz2), _lib.ptr(points2), B, N, S2, D, _lib.ptr(out),
                                   out.shape[1], out_col, _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "reart_three_interpolate")


def mlp_chain(folded, gather, out, out_col):
    """The fused chain for every other shape ``reart_mlp_chain_serves`` accepts (reart_mlp_chain): any D (``F`` None: D = 0),
    either column order (``gather["xyz_first"]``), centres optional."""
    L = _lib.lib()
    (W1, b1), (W2, b2), (W3, b3) = folded
    B, S, K = gather["idx"].shape
    F = gather.get("F")
    D = 0 if F is None else F.shape[1]
    ws = _lib.workspace(L.reart_mlp_chain_workspace_bytes(D, W1.shape[1], W2.shape[1], W3.shape[1]), W1.device)
    rc = L.reart_mlp_chain(_lib.ptr(gather["idx"]), K, S, gather["Npts"], _lib.ptr(F), D, _lib.ptr(gather["Q"]), _lib.ptr(gather.get("C")),
                           int(gather.get("xyz_first", 0)), _lib.ptr(W1), _lib.ptr(b1), W1.shape[1], _lib.ptr(W2), _lib.ptr(b2), W2.shape[1],
                           _lib.ptr(W3), _lib.ptr(b3), W3.shape[1], B * S * K, _lib.ptr(out), out.shape[1], out_col,
                           _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "reart_mlp_chain")
    return out


def chain_serves(D, K, widths, rows, xyz_first):
    """``reart_mlp_chain_serves``: the one predicate the launcher and this layer both ask."""
    return len(widths) == 3 and bool(_lib.lib().reart_mlp_chain_serves(D, K, widths[0], widths[1], widths[2], rows, int(xyz_first)))


def grouped_mlp(convs, bns, gather, out, col, grad=False):
    """The 1x1-conv + BatchNorm + ReLU stack of one scale over the gathered rows of ``gather`` (see ``mlp_layer``) and the max over
    each group of K rows, written into out[:, col:col + C_last].  Three-layer stacks run as ONE launch where a fused kernel
    serves the shape (the extractor's scales: reart_mlp_chain3 / _wide; whatever ``reart_mlp_chain_serves`` accepts:
    reart_mlp_chain), everything else layer by layer -- the same bits either way.
    ``grad=True``: layer by layer through ``mlp_layer(grad=True)`` with differentiable folds (``_fold_grad``); the [groups, C_last]
    result is returned as a tensor of its own (``out`` / ``col`` are not used) with a graph to gather["F"] and the parameters."""
    if grad:
        h = None
        for j, (conv, bn) in enumerate(zip(convs, bns)):
            Wt, b = _fold_grad(conv, bn)
            last = j == len(convs) - 1
            h = mlp_layer(h, Wt, b, gather=gather if j == 0 else None, pool_k=gather["idx"].shape[2] if last else 0, grad=True)
        return h
    idx, F = gather["idx"], gather.get("F")
    B, S, K = idx.shape
    D = 0 if F is None else F.shape[1]
    xyz_first = int(gather.get("xyz_first", 0))
    n_layers = len(convs)
    widths = tuple(c.weight.shape[0] for c in convs)
    if FUSE_CHAIN and n_layers == 3:
        folded = None
        if not xyz_first and D == 3 and widths + (K,) in CHAIN3:
            # sa1: the activations between the three layers stay in LDS (one launch per scale instead of three)
            folded = [_fold(conv, bn) for conv, bn in zip(convs, bns)]
            mlp_chain3(folded, gather, out, col)
        elif (not xyz_first and widths + (K,) in CHAIN3_WIDE and D >= 4 and D % 4 == 0 and (B * S * K) % 128 == 0
              and F.data_ptr() % 16 == 0):
            # sa2: the same with the weights streamed through LDS
            folded = [_fold(conv, bn) for conv, bn in zip(convs, bns)]
            mlp_chain3_wide(folded, gather, out, col)
        elif chain_serves(D, K, widths, B * S * K, xyz_first):
            folded = [_fold(conv, bn) for conv, bn in zip(convs, bns)]
            mlp_chain(folded, gather, out, col)
        if folded is not None:
            return out
    h = None
    for j, (conv, bn) in enumerate(zip(convs, bns)):
        Wt, b = _fold(conv, bn)
        last = j == n_layers - 1
        h = mlp_layer(h, Wt, b, gather=gather if j == 0 else None, pool_k=K if last else 0, out=out if last else None,
                      out_col=col if last else 0)
    return out


from .pointnet2_utils import (PointNetFeaturePropagation, PointNetSetAbstraction,  # noqa: E402  (they use the helpers above)
                              PointNetSetAbstractionMsg)

# the names these layers had while they were private to the extractor
_SAMsg = PointNetSetAbstractionMsg
_FP = PointNetFeaturePropagation


class _SAAll(PointNetSetAbstraction):
    """PointNetSetAbstraction with group_all=True under its former constructor."""

    def __init__(self, in_channel, mlp):
        super().__init__(None, None, None, in_channel, mlp, True)


class PointNet2Msg2(nn.Module):
    """feature_extractor.py:10-49; forward(xyz [B,3,N]) -> [B,out_dim,N]."""

    def __init__(self, out_dim, normal_channel=False):
        super().__init__()
        extra = 3 if normal_channel else 0          # normals ride along as three more input features (:13-16)
        self.out_dim, self.normal_channel = out_dim, normal_channel
        self.sa1 = PointNetSetAbstractionMsg(512, [0.05, 0.1, 0.2], [32, 64, 128], 3 + extra,
                                             [[32, 32, 64], [64, 64, 128], [64, 96, 128]])
        self.sa2 = PointNetSetAbstractionMsg(128, [0.2, 0.4], [64, 128], 128 + 128 + 64, [[128, 128, 256], [128, 196, 256]])
        self.sa3 = PointNetSetAbstraction(None, None, None, 512 + 3, [256, 512, 1024], True)
        self.fp3 = PointNetFeaturePropagation(1536, [256, 256])
        self.fp2 = PointNetFeaturePropagation(576, [256, 128])
        self.fp1 = PointNetFeaturePropagation(134 + extra, [128, 128])
        self.conv1 = nn.Conv1d(128, out_dim, 1)
        self.bn1 = nn.BatchNorm1d(out_dim)

    def invalidate_fold(self):
        """Drop every cached BatchNorm fold (see ``_fold``): needed by hand only after writes through ``.data``."""
        for m in self.modules():
            if hasattr(m, "_reart_folded"):
                del m._reart_folded
        return self

    def train(self, mode=True):
        self.invalidate_fold()
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):         # .to() / .cuda() / .float() / .half()
        self.invalidate_fold()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self.invalidate_fold()
        return super().load_state_dict(*args, **kwargs)

    def forward(self, xyz, fps_start=None, cuda_mode=None, grad=False):
        """``cuda_mode`` None follows ``pointnet2_utils.CUDA`` (True: the rules of a GPU run of the reference);
        ``cuda_mode=False`` selects the CPU-fallback rules, for which ``fps_start`` = (start1 [B], start2 [B])
        injects the FPS start indices the reference draws from torch's RNG.

        ``grad=True`` (``eval()`` only, autograd enabled): the same descriptors, bit for bit, with a first-order graph to every
        conv / BatchNorm parameter that requires grad.  The stacks run layer by layer on the current stream (no fused chain, no
        side stream).  The input cloud gets no gradient (``xyz.requires_grad`` is ignored): it enters as coordinates, and the
        level-0 features are the cloud itself."""
        if self.training:
            raise RuntimeError("PointNet2Msg2 is inference-only here (call .eval()); the reference freezes it")
        if grad:
            require_grad_mode("PointNet2Msg2.forward")
            return self._forward_grad(xyz.detach(), fps_start, cuda_mode)
        with torch.no_grad():
            return self._forward(xyz, fps_start, cuda_mode)

    def _forward_grad(self, xyz, fps_start, cuda_mode):
        _lib.require_gpu(xyz)
        B, _, N = xyz.shape
        if xyz.shape[1] != (6 if self.normal_channel else 3):
            raise ValueError(f"PointNet2Msg2(normal_channel={self.normal_channel}) takes [B,{6 if self.normal_channel else 3},N] input")
        with torch.no_grad():
            feats0 = xyz.permute(0, 2, 1).contiguous().float()
            pts = feats0[:, :, :3].contiguous() if self.normal_channel else feats0
            skip0 = torch.cat([pts, feats0], dim=2)
        s1, s2 = fps_start if fps_start is not None else (None, None)
        l1_xyz, l1 = self.sa1.run(pts, feats0, start=s1, cuda_mode=cuda_mode, grad=True)
        l2_xyz, l2 = self.sa2.run(l1_xyz, l1, start=s2, cuda_mode=cuda_mode, grad=True)
        l3 = self.sa3.pool_all(l2_xyz, l2, grad=True)
        l2n = self.fp3.run(l2_xyz, l2_xyz[:, :1], l2, l3[:, None, :], grad=True)
        l1n = self.fp2.run(l1_xyz, l2_xyz, l1, l2n, grad=True)
        l0n = self.fp1.run(pts, l1_xyz, skip0, l1n, grad=True)
        Wt, b = _fold_grad(self.conv1, self.bn1)
        feat = mlp_layer(l0n.reshape(B * N, -1), Wt, b, grad=True)
        return feat.reshape(B, N, self.out_dim).permute(0, 2, 1).contiguous()

    def _forward(self, xyz, fps_start, cuda_mode):
        _lib.require_gpu(xyz)
        B, _, N = xyz.shape
        if xyz.shape[1] != (6 if self.normal_channel else 3):
            raise ValueError(f"PointNet2Msg2(normal_channel={self.normal_channel}) takes [B,{6 if self.normal_channel else 3},N] input")
        pts = xyz.permute(0, 2, 1).contiguous().float()  # [B,N,3] (with normals: [B,N,6] = xyz | normal)
        feats0 = pts                                     # level-0 features: the input itself (:34-39)
        if self.normal_channel:
            pts = feats0[:, :, :3].contiguous()
        s1, s2 = fps_start if fps_start is not None else (None, None)
        samp1 = self.sa1.sample(pts, start=s1, cuda_mode=cuda_mode)
        samp2 = None
        if OVERLAP_SAMPLING:
            # the second level's sampling (FPS 512 -> 128: a latency chain on B workgroups; its ball queries) needs the first
            # level's coordinates only: it runs on a side stream under the first level's feature stacks
            main, side = torch.cuda.current_stream(xyz.device), _side_stream(xyz.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                samp2 = self.sa2.sample(samp1[0], start=s2, cuda_mode=cuda_mode)
                for t_ in (samp2[0], *samp2[1]):
                    t_.record_stream(main)           # allocated on the side stream, consumed on the main one
        l1_xyz, l1 = self.sa1.run(pts, feats0, sampled=samp1)                         # [B,512,3], [B,512,320]
        if samp2 is not None:
            main.wait_stream(side)
        l2_xyz, l2 = self.sa2.run(l1_xyz, l1, start=s2, cuda_mode=cuda_mode, sampled=samp2)   # [B,128,3], [B,128,512]
        l3 = self.sa3.pool_all(l2_xyz, l2)                                           # [B,1024]
        l2n = self.fp3.run(l2_xyz, l2_xyz[:, :1], l2, l3[:, None, :])                # [B,128,256]
        l1n = self.fp2.run(l1_xyz, l2_xyz, l1, l2n)                                  # [B,512,128]
        l0n = self.fp1.run(pts, l1_xyz, torch.cat([pts, feats0], dim=2), l1n)           # [B,N,128]
        Wt, b = _fold(self.conv1, self.bn1)
        feat = mlp_layer(l0n.reshape(B * N, -1), Wt, b)                              # [B*N,64]
        return feat.reshape(B, N, self.out_dim).permute(0, 2, 1).contiguous()


def rec_freeze(model):
    """feature_extractor.py:52-59: BatchNorm momentum 0 and no parameter of any descendant trainable."""
    for m in model.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.momentum = 0
    for child in model.children():           # the parameters of every descendant; the root's own, if any, stay as they are
        for p in child.parameters():
            p.requires_grad = False


def get_extractor(args):
    """feature_extractor.py:62-86 without the DataParallel wrapper: checkpoints saved from the
    wrapped model carry a ``module.`` prefix, which is stripped here."""
    import warnings

    model = PointNet2Msg2(out_dim=64)
    ckpt = torch.load(args.corr_model_path, map_location="cpu")
    sd = ckpt["state_dict"] if "state_dict" in ckpt else ckpt
    sd = {k.replace("net.", "").replace("module.", "", 1): v for k, v in sd.items()}
    missing = set(model.state_dict().keys()) - set(sd.keys())
    if missing:
        warnings.warn("Missing keys ! : {}".format(missing))
    model.load_state_dict(sd, strict=True)
    model.eval()
    for p in model.parameters():
        p.requires_grad = False
    return model.cuda()
