"""Host-side mirror of the sampling / grouping functions of the reference's
``networks/pointnet2_utils.py`` over the HIP kernels (``reart_fps``, ``reart_ball_query``).

The reference picks its sampling rules with a module-level switch (``CUDA``, networks/pointnet2_utils.py:7-12:
true whenever a GPU is present) -- mirrored here as ``CUDA = True``, because this package only runs on a GPU:
  * ``CUDA`` rules (default): the vendored CUDA kernels -- FPS starts at index 0 with the block-tree tie rule
    (sampling_gpu.cu:93-209), ball query keeps ``d2 < r*r`` on coordinate differences and pads with the first hit
    (ball_query_gpu.cu:9-45);
  * CPU-fallback rules (``cuda_mode=False`` per call, or ``pointnet2_utils.CUDA = False``): FPS starts at a
    ``torch.randint`` draw, arg-max = first maximum (:88-99); ball query keeps ``d2 <= r^2`` on the matmul-expanded
    ``square_distance`` and pads with the nearest point (:102-140) -- BASELINE's "reference CPU/PyTorch path", the
    rules the CPU-generated golden vectors follow.

The layer classes (``PointNetSetAbstraction``, ``PointNetSetAbstractionMsg``, ``PointNetFeaturePropagation``) carry the
reference's constructor arguments, channel-first ``forward`` shapes and parameter names (``mlp_convs`` / ``mlp_bns``,
``conv_blocks`` / ``bn_blocks``: its checkpoints load with ``strict=True``).  They run in ``eval()`` only (``forward`` in
training mode raises: batch statistics are not built): BatchNorm uses its running statistics, folded into the 1x1 conv, and
the grouped tensor is never built -- the gather, the conv stack and the max over a group run in ``reart_mlp_layer`` / the
fused chain kernels.
``forward`` takes keyword-only extras: ``fps_start`` ([B] first index of the farthest point sampling) and ``cuda_mode``
(the sampling rules, None: the module switch ``CUDA``), with the meaning they have in ``PointNet2Msg2.forward``, and ``grad``.

``grad=False`` (the default) is inference: nothing returned requires grad.  ``grad=True`` (``forward``, ``run``, ``pool_all``;
``eval()`` only, autograd enabled, float32 contiguous operands) returns the same bits with a FIRST-ORDER graph from the feature
output to the incoming features (``points`` / ``points1`` / ``points2``) and to ``conv.weight``, ``conv.bias``, ``bn.weight``,
``bn.bias`` of the stacks, whichever require grad (``reart_mlp_layer_backward`` / ``reart_three_interpolate_backward``).
Coordinates get NO gradient and ``xyz.requires_grad`` is ignored: not the ``xyz - centre`` columns, not the centres
(``new_xyz`` carries no graph), not the interpolation weights.  The stacks run layer by layer on the current stream; two runs
agree in every bit; nothing synchronises with the host.
"""
import torch
import torch.nn as nn

from .. import _lib

CUDA = True   # networks/pointnet2_utils.py:7-12


def _rules(cuda_mode):
    return CUDA if cuda_mode is None else bool(cuda_mode)


def index_points(points, idx):
    """points [B,N,C], idx [B,S] or [B,S,K] -> [B,S,(K,)C] (networks/pointnet2_utils.py:54-71)."""
    B = points.shape[0]
    flat = idx.reshape(B, -1)
    out = torch.gather(points, 1, flat[..., None].expand(-1, -1, points.shape[-1]))
    return out.reshape(*idx.shape, points.shape[-1])


def farthest_point_sample(xyz, npoint, start=None, cuda_mode=None):
    """xyz [B,N,3] -> int64 [B,npoint] (networks/pointnet2_utils.py:74-99).

    ``start`` [B]: first index of every cloud.  The reference's CPU fallback draws it with
    ``torch.randint`` from the global generator (:90) -- reproduced here when ``start`` is None and
    ``cuda_mode`` is False; its CUDA kernel always starts at 0 (sampling_gpu.cu:113).

    N <= 12 288 runs ``reart_fps`` (cloud in LDS), larger clouds up to 2^21 points ``reart_fps_temp`` with a
    [B,N] distance buffer allocated here; N > 2^21 raises NotImplementedError."""
    _lib.require_gpu(xyz)
    cuda_mode = _rules(cuda_mode)
    xyz = xyz.contiguous().float()
    B, N, _ = xyz.shape
    if N > _lib.FPS_MAX_N:
        raise NotImplementedError(f"farthest_point_sample: N = {N} > {_lib.FPS_MAX_N} points (REART_FPS_MAX_N)")
    if start is None and not cuda_mode:
        start = torch.randint(0, N, (B,), dtype=torch.long, device=xyz.device)
    st = None if start is None else start.to(device=xyz.device, dtype=torch.int32).contiguous()
    idx = torch.empty((B, npoint), dtype=torch.int64, device=xyz.device)
    if N <= _lib.FPS_MAX_N_LDS:
        rc = _lib.lib().reart_fps(_lib.ptr(xyz), B, N, npoint, _lib.ptr(st), int(bool(cuda_mode)), None, _lib.ptr(idx),
                                  _lib.stream())
        _lib.check(rc, "reart_fps")
        return idx
    temp = torch.empty((B, N), dtype=torch.float32, device=xyz.device)   # running minima beyond the registers
    rc = _lib.lib().reart_fps_temp(_lib.ptr(xyz), B, N, npoint, _lib.ptr(st), int(bool(cuda_mode)), _lib.ptr(temp),
                                   None, _lib.ptr(idx), _lib.stream())
    _lib.check(rc, "reart_fps_temp")
    return idx


def query_ball_point(radius, nsample, xyz, new_xyz, cuda_mode=None):
    """xyz [B,N,3], new_xyz [B,S,3] -> int64 [B,S,nsample] (networks/pointnet2_utils.py:102-140)."""
    _lib.require_gpu(xyz, new_xyz)
    cuda_mode = _rules(cuda_mode)
    xyz, new_xyz = xyz.contiguous().float(), new_xyz.contiguous().float()
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    idx = torch.empty((B, S, nsample), dtype=torch.int64, device=xyz.device)
    rc = _lib.lib().reart_ball_query(_lib.ptr(xyz), _lib.ptr(new_xyz), B, N, S, float(radius), nsample,
                                     int(bool(cuda_mode)), None, _lib.ptr(idx), _lib.stream())
    _lib.check(rc, "reart_ball_query")
    return idx


def square_distance(src, dst):
    """src [B,N,C], dst [B,M,C] -> squared distances [B,N,M] by the matmul expansion -2 src.dst + |src|^2 + |dst|^2
    (networks/pointnet2_utils.py:30-51).  C = 3 runs ``reart_square_distance`` (torch's CPU rounding of that expansion, the
    expression ball query and 3-NN interpolation use); any other C is evaluated with tensor expressions."""
    _lib.require_gpu(src, dst)
    B, N, C = src.shape
    M = dst.shape[1]
    if C != 3 or src.dtype != torch.float32 or dst.dtype != torch.float32:
        dist = -2 * torch.matmul(src, dst.transpose(1, 2))
        dist += (src * src).sum(-1)[:, :, None]
        dist += (dst * dst).sum(-1)[:, None, :]
        return dist
    src, dst = src.contiguous(), dst.contiguous()
    out = torch.empty((B, N, M), dtype=torch.float32, device=src.device)
    rc = _lib.lib().reart_square_distance(_lib.ptr(src), _lib.ptr(dst), B, N, M, _lib.ptr(out), _lib.stream())
    _lib.check(rc, "reart_square_distance")
    return out


def sample_and_group(npoint, radius, nsample, xyz, points, returnfps=False, *, fps_start=None, cuda_mode=None):
    """xyz [B,N,3], points [B,N,D] or None -> new_xyz [B,npoint,3], new_points [B,npoint,nsample,3+D] = [xyz - centre | points]
    (networks/pointnet2_utils.py:143-171); with ``returnfps`` also the grouped absolute xyz and the sampled indices."""
    B = xyz.shape[0]
    fps_idx = farthest_point_sample(xyz, npoint, start=fps_start, cuda_mode=cuda_mode)
    new_xyz = index_points(xyz, fps_idx)
    idx = query_ball_point(radius, nsample, xyz, new_xyz, cuda_mode=cuda_mode)
    grouped_xyz = index_points(xyz, idx)
    new_points = grouped_xyz - new_xyz[:, :, None, :]
    if points is not None:
        new_points = torch.cat([new_points, index_points(points, idx)], dim=-1)
    if returnfps:
        return new_xyz, new_points, grouped_xyz, fps_idx
    return new_xyz, new_points


def sample_and_group_all(xyz, points):
    """One group of all N points around the origin: new_xyz zeros [B,1,3], new_points [B,1,N,3+D] = [xyz | points]
    (networks/pointnet2_utils.py:174-191)."""
    B, N, C = xyz.shape
    new_xyz = torch.zeros((B, 1, C), dtype=xyz.dtype, device=xyz.device)
    new_points = xyz.reshape(B, 1, N, C)
    if points is not None:
        new_points = torch.cat([new_points, points.reshape(B, 1, N, -1)], dim=-1)
    return new_xyz, new_points


class _InferenceLayer(nn.Module):
    """What the three layer classes share: eval() only, cached BatchNorm folds dropped when the parameters move."""

    def invalidate_fold(self):
        for m in self.modules():
            if hasattr(m, "_reart_folded"):
                del m._reart_folded
        return self

    def train(self, mode=True):
        self.invalidate_fold()
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_fold()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self.invalidate_fold()
        return super().load_state_dict(*args, **kwargs)

    def _check(self, *tensors):
        if self.training:
            raise RuntimeError(f"{type(self).__name__} is inference-only here (call .eval())")
        _lib.require_gpu(*tensors)

    def _call(self, grad, fn):
        """``fn(grad)`` under torch.no_grad() (inference), or -- grad=True -- with autograd, which must be enabled."""
        if not grad:
            with torch.no_grad():
                return fn(False)
        from .feature_extractor import require_grad_mode

        require_grad_mode(type(self).__name__)
        return fn(True)


def _coords(t):
    """Coordinates take no part in the graph."""
    return None if t is None else t.detach()


def _last(t):
    """channel-first [B,C,N] -> contiguous float channel-last [B,N,C] (None stays None)."""
    return None if t is None else t.permute(0, 2, 1).contiguous().float()


def _flat(t):
    return None if t is None else t.reshape(t.shape[0] * t.shape[1], -1).contiguous()


class PointNetSetAbstractionMsg(_InferenceLayer):
    """Multi-scale grouping (networks/pointnet2_utils.py:238-295): FPS, one ball query per radius, per scale a conv stack over
    [features | xyz - centre] (features FIRST) and the max over the group; the scales' outputs side by side."""

    def __init__(self, npoint, radius_list, nsample_list, in_channel, mlp_list):
        super().__init__()
        self.npoint, self.radius_list, self.nsample_list = npoint, radius_list, nsample_list
        self.conv_blocks, self.bn_blocks = nn.ModuleList(), nn.ModuleList()
        for mlp in mlp_list:
            convs, bns, last = nn.ModuleList(), nn.ModuleList(), in_channel + 3
            for out in mlp:
                convs.append(nn.Conv2d(last, out, 1))
                bns.append(nn.BatchNorm2d(out))
                last = out
            self.conv_blocks.append(convs)
            self.bn_blocks.append(bns)
        self.out_channels = sum(m[-1] for m in mlp_list)

    def sample(self, xyz, start=None, cuda_mode=None):
        """The part of the level that depends on COORDINATES only: farthest point sampling and the ball queries of every
        scale -> (new_xyz [B,S,3], [idx [B,S,K] per scale]).  The caller may run it ahead of the previous level's
        feature stacks (another stream)."""
        fps = farthest_point_sample(xyz, self.npoint, start=start, cuda_mode=cuda_mode)
        new_xyz = index_points(xyz, fps).contiguous()
        return new_xyz, [query_ball_point(radius, K, xyz, new_xyz, cuda_mode=cuda_mode)
                         for radius, K in zip(self.radius_list, self.nsample_list)]

    def run(self, xyz, feats, start=None, cuda_mode=None, sampled=None, grad=False):
        """xyz [B,N,3], feats [B,N,D] (channel-last) or None -> new_xyz [B,S,3], new_feats [B,S,sum C]."""
        from .feature_extractor import grouped_mlp

        B, N, _ = xyz.shape
        S = self.npoint
        if grad:
            self._check(xyz, feats)
            xyz = _coords(xyz)
            with torch.no_grad():
                new_xyz, idx_list = sampled if sampled is not None else self.sample(xyz, start=start, cuda_mode=cuda_mode)
            Q, F, C = xyz.reshape(B * N, 3), _flat(feats), new_xyz.reshape(B * S, 3)
            outs = [grouped_mlp(self.conv_blocks[i], self.bn_blocks[i], dict(idx=idx, F=F, Q=Q, C=C, Npts=N, xyz_first=0), None, 0,
                                grad=True) for i, idx in enumerate(idx_list)]
            return new_xyz, torch.cat(outs, dim=1).reshape(B, S, self.out_channels)
        new_xyz, idx_list = sampled if sampled is not None else self.sample(xyz, start=start, cuda_mode=cuda_mode)
        out = torch.empty((B * S, self.out_channels), dtype=torch.float32, device=xyz.device)
        col = 0
        Q, F, C = xyz.reshape(B * N, 3), _flat(feats), new_xyz.reshape(B * S, 3)
        for i, idx in enumerate(idx_list):
            # grouped [features | xyz - centre], features first (:277-281)
            grouped_mlp(self.conv_blocks[i], self.bn_blocks[i], dict(idx=idx, F=F, Q=Q, C=C, Npts=N, xyz_first=0), out, col)
            col += self.conv_blocks[i][-1].weight.shape[0]
        return new_xyz, out.reshape(B, S, self.out_channels)

    def forward(self, xyz, points, *, fps_start=None, cuda_mode=None, grad=False):
        """xyz [B,3,N], points [B,D,N] or None -> new_xyz [B,3,S], new_points [B,sum C,S]."""
        self._check(xyz, points)

        def fn(g):
            new_xyz, out = self.run(_last(_coords(xyz) if g else xyz), _last(points), start=fps_start, cuda_mode=cuda_mode, grad=g)
            return new_xyz.permute(0, 2, 1), out.permute(0, 2, 1)
        return self._call(grad, fn)


class PointNetSetAbstraction(_InferenceLayer):
    """Single-scale grouping (networks/pointnet2_utils.py:194-235): a conv stack over [xyz - centre | features] (xyz FIRST)
    of npoint ball-query groups, or -- ``group_all`` -- over [xyz | features] of ONE group of all points, and the max over it."""

    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all):
        super().__init__()
        self.npoint, self.radius, self.nsample, self.group_all = npoint, radius, nsample, group_all
        self.mlp_convs, self.mlp_bns = nn.ModuleList(), nn.ModuleList()
        last = in_channel
        for out in mlp:
            self.mlp_convs.append(nn.Conv2d(last, out, 1))
            self.mlp_bns.append(nn.BatchNorm2d(out))
            last = out

    def pool_all(self, xyz, feats, grad=False):
        """group_all on channel-last input: xyz [B,N,3], feats [B,N,D] or None -> [B,C] (any N)."""
        from .feature_extractor import grouped_mlp

        B, N, _ = xyz.shape
        idx = torch.arange(N, device=xyz.device, dtype=torch.int64).expand(B, 1, N).contiguous()
        if grad:
            self._check(xyz, feats)
            return grouped_mlp(self.mlp_convs, self.mlp_bns, dict(idx=idx, F=_flat(feats), Q=_coords(xyz).reshape(B * N, 3), C=None,
                                                                  Npts=N, xyz_first=1), None, 0, grad=True)
        out = torch.empty((B, self.mlp_convs[-1].weight.shape[0]), dtype=torch.float32, device=xyz.device)
        # [xyz | features], xyz first, nothing subtracted (sample_and_group_all :186-188)
        return grouped_mlp(self.mlp_convs, self.mlp_bns, dict(idx=idx, F=_flat(feats), Q=xyz.reshape(B * N, 3), C=None, Npts=N,
                                                              xyz_first=1), out, 0)

    def run(self, xyz, feats, start=None, cuda_mode=None, grad=False):
        """xyz [B,N,3], feats [B,N,D] (channel-last) or None -> new_xyz [B,S,3], new_feats [B,S,C]."""
        from .feature_extractor import grouped_mlp

        B, N, _ = xyz.shape
        if self.group_all:
            return torch.zeros((B, 1, 3), dtype=torch.float32, device=xyz.device), self.pool_all(xyz, feats, grad=grad)[:, None, :]
        S = self.npoint
        if grad:
            self._check(xyz, feats)
            xyz = _coords(xyz)
            with torch.no_grad():
                fps = farthest_point_sample(xyz, S, start=start, cuda_mode=cuda_mode)
                new_xyz = index_points(xyz, fps).contiguous()
                idx = query_ball_point(self.radius, self.nsample, xyz, new_xyz, cuda_mode=cuda_mode)
            out = grouped_mlp(self.mlp_convs, self.mlp_bns, dict(idx=idx, F=_flat(feats), Q=xyz.reshape(B * N, 3),
                                                                 C=new_xyz.reshape(B * S, 3), Npts=N, xyz_first=1), None, 0, grad=True)
            return new_xyz, out.reshape(B, S, -1)
        fps = farthest_point_sample(xyz, S, start=start, cuda_mode=cuda_mode)
        new_xyz = index_points(xyz, fps).contiguous()
        idx = query_ball_point(self.radius, self.nsample, xyz, new_xyz, cuda_mode=cuda_mode)
        out = torch.empty((B * S, self.mlp_convs[-1].weight.shape[0]), dtype=torch.float32, device=xyz.device)
        # [xyz - centre | features], xyz first (sample_and_group :160-165)
        grouped_mlp(self.mlp_convs, self.mlp_bns, dict(idx=idx, F=_flat(feats), Q=xyz.reshape(B * N, 3), C=new_xyz.reshape(B * S, 3),
                                                       Npts=N, xyz_first=1), out, 0)
        return new_xyz, out.reshape(B, S, -1)

    def forward(self, xyz, points, *, fps_start=None, cuda_mode=None, grad=False):
        """xyz [B,3,N], points [B,D,N] or None -> new_xyz [B,3,S], new_points [B,C,S] (group_all: S = 1, new_xyz zeros)."""
        self._check(xyz, points)

        def fn(g):
            new_xyz, out = self.run(_last(_coords(xyz) if g else xyz), _last(points), start=fps_start, cuda_mode=cuda_mode, grad=g)
            return new_xyz.permute(0, 2, 1), out.permute(0, 2, 1)
        return self._call(grad, fn)


class PointNetFeaturePropagation(_InferenceLayer):
    """Feature propagation (networks/pointnet2_utils.py:298-348): the coarse level's features interpolated onto the fine points
    from their three nearest coarse points with inverse squared-distance weights (one coarse point: repeated), joined behind
    the fine level's own features, then a Conv1d stack."""

    def __init__(self, in_channel, mlp):
        super().__init__()
        self.mlp_convs, self.mlp_bns = nn.ModuleList(), nn.ModuleList()
        last = in_channel
        for out in mlp:
            self.mlp_convs.append(nn.Conv1d(last, out, 1))
            self.mlp_bns.append(nn.BatchNorm1d(out))
            last = out

    def run(self, xyz1, xyz2, points1, points2, grad=False):
        """xyz1 [B,N,3], xyz2 [B,S,3], points1 [B,N,D1] or None, points2 [B,S,D2] -> [B,N,C]."""
        from .feature_extractor import _fold, _fold_grad, mlp_layer, three_interpolate

        B, N, _ = xyz1.shape
        S, D2 = points2.shape[1], points2.shape[2]
        D1 = 0 if points1 is None else points1.shape[2]
        if grad:
            self._check(xyz1, xyz2, points1, points2)
            # the copy of points1 and the S = 1 repeat are tensor expressions; the interpolation is its own operator
            if S == 1:
                h = points2.expand(B, N, D2).reshape(B * N, D2)
            else:
                h = three_interpolate(_coords(xyz1).contiguous(), _coords(xyz2).contiguous(), points2.contiguous(), None, 0, grad=True)
            if D1:
                h = torch.cat([points1.reshape(B * N, D1), h], dim=1)
            h = h.contiguous()
            for conv, bn in zip(self.mlp_convs, self.mlp_bns):
                Wt, b = _fold_grad(conv, bn)
                h = mlp_layer(h, Wt, b, grad=True)
            return h.reshape(B, N, -1)
        X = torch.empty((B * N, D1 + D2), dtype=torch.float32, device=xyz1.device)
        if D1:
            X[:, :D1] = points1.reshape(B * N, D1)
        if S == 1:
            X[:, D1:] = points2.expand(B, N, D2).reshape(B * N, D2)
        else:
            three_interpolate(xyz1.contiguous(), xyz2.contiguous(), points2.contiguous(), X, D1)
        h = X
        for conv, bn in zip(self.mlp_convs, self.mlp_bns):
            Wt, b = _fold(conv, bn)
            h = mlp_layer(h, Wt, b)
        return h.reshape(B, N, -1)

    def forward(self, xyz1, xyz2, points1, points2, *, fps_start=None, cuda_mode=None, grad=False):
        """xyz1 [B,3,N], xyz2 [B,3,S], points1 [B,D1,N] or None, points2 [B,D2,S] -> [B,C,N].  (Nothing is sampled here:
        ``fps_start`` and ``cuda_mode`` are accepted for a uniform signature and have no effect.)"""
        self._check(xyz1, xyz2, points1, points2)
        return self._call(grad, lambda g: self.run(_last(xyz1), _last(xyz2), _last(points1), _last(points2), grad=g).permute(0, 2, 1))
