"""Host-side mirror of the per-iteration part of the reference's ``utils/flow_utils.py``."""
import torch

from .. import _lib


@torch.no_grad()
def blend_anchor_motion(query_loc, reference_loc, reference_flow, knn, return_mask=False):
    """Inverse-distance blending of the k nearest anchors' flow (utils/flow_utils.py:147-170).
    query_loc [m,3], reference_loc [n,3], reference_flow [n,3]; ``knn`` is a ``KNN`` instance
    (only its ``k`` and distance convention are used: search and blend are one fused call)."""
    _lib.require_gpu(query_loc, reference_loc, reference_flow)
    q = query_loc.contiguous().float()
    r = reference_loc.contiguous().float()
    f = reference_flow.contiguous().float()
    nq, nr, k = q.shape[0], r.shape[0], knn.k
    flow = torch.empty((nq, 3), dtype=torch.float32, device=q.device)
    mask = torch.empty((nq,), dtype=torch.bool, device=q.device)
    L = _lib.lib()
    ws = _lib.workspace(L.reart_blend_anchor_motion_workspace_bytes(nq, nr, k), q.device)
    euclid = 0 if getattr(knn, "_squared", False) else 1
    rc = L.reart_blend_anchor_motion(_lib.ptr(q), _lib.ptr(r), _lib.ptr(f), nq, nr, k, euclid, _lib.ptr(flow),
                                     _lib.ptr(mask), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "reart_blend_anchor_motion")
    return (flow, mask) if return_mask else flow


def pad_reference_sets(reference_locs, reference_flows):
    """The ragged per-frame reference sets of ``blend_anchor_motion_batch`` as padded tensors, built once:
    (ref [B,nr_max,3], ref_flow [B,nr_max,3], ref_len [B] int64 or None when all sets have nr_max points)."""
    B, nr = len(reference_locs), max(int(r.shape[0]) for r in reference_locs)
    dev = reference_locs[0].device
    ref = torch.zeros((B, nr, 3), dtype=torch.float32, device=dev)
    flo = torch.zeros((B, nr, 3), dtype=torch.float32, device=dev)
    for b, (r, f) in enumerate(zip(reference_locs, reference_flows)):
        ref[b, :r.shape[0]] = r.float()
        flo[b, :f.shape[0]] = f.float()
    lens = [int(r.shape[0]) for r in reference_locs]
    ref_len = None if min(lens) == nr else torch.tensor(lens, dtype=torch.int64, device=dev)
    return ref, flo, ref_len


@torch.no_grad()
def blend_anchor_motion_batch(query_locs, ref, ref_flow, ref_len, knn, return_mask=False):
    """The B calls ``blend_anchor_motion(query_locs[b], reference_loc[b], reference_flow[b], knn)`` of an iteration
    (run_robot.py:194-201) as one native call (``reart_blend_anchor_motion_batch``), bit for bit the per-frame results.
    query_locs [B,m,3]; ref, ref_flow [B,nr_max,3] and ref_len [B] int64 or None from ``pad_reference_sets``.
    Returns flow [B,m,3] (and mask [B,m] bool)."""
    _lib.require_gpu(query_locs, ref, ref_flow, ref_len)
    q = query_locs.contiguous().float()
    r, f = ref.contiguous().float(), ref_flow.contiguous().float()
    B, nq, nr, k = q.shape[0], q.shape[1], r.shape[1], knn.k
    if r.shape[0] != B or f.shape != r.shape:
        raise ValueError("blend_anchor_motion_batch: query_locs [B,m,3], ref and ref_flow [B,nr_max,3]")
    flow = torch.empty((B, nq, 3), dtype=torch.float32, device=q.device)
    mask = torch.empty((B, nq), dtype=torch.bool, device=q.device)
    L = _lib.lib()
    ws = _lib.workspace(L.reart_blend_anchor_motion_batch_workspace_bytes(B, nq, nr, k), q.device)
    euclid = 0 if getattr(knn, "_squared", False) else 1
    rc = L.reart_blend_anchor_motion_batch(_lib.ptr(q), _lib.ptr(r), _lib.ptr(f), _lib.ptr(ref_len), B, nq, nr, k, euclid,
                                           _lib.ptr(flow), _lib.ptr(mask), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "reart_blend_anchor_motion_batch")
    return (flow, mask) if return_mask else flow


class _FlowTermFn(torch.autograd.Function):
    """Pattern of utils/chamfer.py's _ChamferLossFn: the forward has computed the loss and its gradient, the backward scales it
    by the upstream scalar."""

    @staticmethod
    def forward(ctx, pc_trans_list, cano_pc, mod):
        loss, G = mod._run(pc_trans_list, cano_pc)
        ctx.save_for_backward(G)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (G,) = ctx.saved_tensors
        return G * g, None, None


class _Knn3:
    """What ``blend_anchor_motion_batch`` reads of a ``KNN`` instance."""

    def __init__(self, squared):
        self.k, self._squared = 3, bool(squared)


class FlowTerm(torch.nn.Module):
    """``forward(pc_trans_list [B,N,3], cano_pc [N,3]) -> scalar``: one iteration's flow term (run_robot.py:194-209),

        comp = cat(pc_trans_list[:cano_idx], cano_pc[None], pc_trans_list[cano_idx:])
        gt_flow, mask = blend_anchor_motion(comp[f], pc_ref_list[f], flow_ref_list[f], KNN(k=3))   for every pair f
        weight * flow_loss(gt_flow, comp[1:] - comp[:-1], mask, robust, smooth_weight)

    with its gradient for ``pc_trans_list`` as one warm-started native call (``reart_flow_term``): the same neighbours, blended
    flow, mask and gradient bit for bit, the loss as one double sum rounded once.  ``pc_ref_list`` / ``flow_ref_list`` are the
    B = T - 1 ragged reference sets ([n_f,3] each, n_f >= 3) and never change; ``knn_squared`` selects squared distances in the
    blend (``KNN``'s default is their square root).  Gradient reaches ``pc_trans_list`` only.

    The module owns, per (N, device): the native workspace with the references' searchable image (built on the first call
    with that N, again after ``reset()``), the neighbour indices of its previous call (they bound the next search and never
    change its result) and -- unless ``spatial_sort=False`` -- the storage orders in which the box-pruned search is fastest:
    every reference set is stored once in ``relax.kd_order``, and the queries are visited in the k-d order of the first
    ``cano_pc``.  Results are always in the caller's numbering; ``.last`` holds the detached ``(gt_flow, mask, dists, idx)`` of
    the latest call.  With ``spatial_sort`` a tie between DISTINCT equidistant reference points goes to the one stored first
    (coincident points keep the caller's order, so copies of a point resolve to the lowest index), as ``ChamferLoss``.

    Host tensors raise ``RuntimeError: ... no CPU fallback``.  What the native call does not serve -- float64 input, a query
    cloud that is not [B,N,3] float32, a shape beyond its limits -- goes through ``blend_anchor_motion_batch`` + ``flow_loss``
    inside the module: the same value and gradient, without warm state (``.last`` then holds ``(gt_flow, mask, None, None)``)."""

    def __init__(self, pc_ref_list, flow_ref_list, cano_idx, weight=1.0, robust=False, smooth_weight=1e-2, knn_squared=False,
                 spatial_sort=True):
        super().__init__()
        if len(pc_ref_list) != len(flow_ref_list) or len(pc_ref_list) == 0:
            raise ValueError("FlowTerm: one flow set per reference set, at least one")
        _lib.require_gpu(*pc_ref_list, *flow_ref_list)
        for r, f in zip(pc_ref_list, flow_ref_list):
            if r.dim() != 2 or r.shape[1] != 3 or f.shape != r.shape or r.shape[0] < 3:
                raise ValueError("FlowTerm: reference sets and flows [n,3] with n >= 3")
        self.B, self.cano_idx = len(pc_ref_list), int(cano_idx)
        if not 0 <= self.cano_idx <= self.B:
            raise ValueError("FlowTerm: cano_idx in [0, B]")
        self.weight, self.robust, self.smooth_weight = float(weight), bool(robust), float(smooth_weight)
        self.knn_squared, self.spatial_sort = bool(knn_squared), bool(spatial_sort)
        refs, flows = [r.detach().float() for r in pc_ref_list], [f.detach().float() for f in flow_ref_list]
        self._caller = pad_reference_sets(refs, flows)              # the composition's operands, caller numbering
        self._rperm = None
        if self.spatial_sort:
            from ..relax import kd_order

            perms = [kd_order(r).to(torch.int64) for r in refs]
            self._stored = pad_reference_sets([r[p] for r, p in zip(refs, perms)], [f[p] for f, p in zip(flows, perms)])
            nr = self._stored[0].shape[1]
            self._rperm = torch.zeros((self.B, nr), dtype=torch.int64, device=refs[0].device)   # stored position -> caller index
            self._rinv = torch.zeros_like(self._rperm)                                           # caller index -> stored position
            for b, p in enumerate(perms):
                self._rperm[b, :p.shape[0]] = p
                self._rinv[b, p] = torch.arange(p.shape[0], device=p.device)
        else:
            self._stored = self._caller
        self._lens = torch.tensor([int(r.shape[0]) for r in refs], dtype=torch.int64, device=refs[0].device)
        self._state = {}
        self._last = self._raw = None

    def reset(self):
        """Forget seeds, visiting orders, workspaces and ``.last`` (the next call is a first call)."""
        self._state = {}
        self._last = self._raw = None

    def _served(self, x, cano):
        if x.dtype != torch.float32 or cano.dtype != torch.float32 or x.dim() != 3 or cano.dim() != 2:
            return False
        if x.shape[0] != self.B or x.shape[2] != 3 or tuple(cano.shape) != (x.shape[1], 3) or x.device != self._stored[0].device:
            return False
        return _lib.lib().reart_flow_term_workspace_bytes(self.B, x.shape[1], self._stored[0].shape[1]) > 0

    def forward(self, pc_trans_list, cano_pc):
        _lib.require_gpu(pc_trans_list, cano_pc)
        if self._served(pc_trans_list, cano_pc):
            return _FlowTermFn.apply(pc_trans_list, cano_pc, self)
        from ..networks.loss import flow_loss

        c = self.cano_idx
        comp = torch.cat((pc_trans_list[:c], cano_pc[None], pc_trans_list[c:]), dim=0)
        gt_flow, mask = blend_anchor_motion_batch(comp[:-1].detach(), *self._caller, _Knn3(self.knn_squared), return_mask=True)
        self._raw, self._last = None, (gt_flow, mask, None, None)
        return self.weight * flow_loss(gt_flow, comp[1:] - comp[:-1], flow_mask_list=mask, robust=self.robust,
                                       smooth_weight=self.smooth_weight)

    def _get_state(self, N, cano):
        dev = cano.device
        st = self._state.get((N, dev))
        if st is None:
            L = _lib.lib()
            ref, flo, ref_len = self._stored
            nbytes = int(L.reart_flow_term_workspace_bytes(self.B, N, ref.shape[1]))
            st = {"ws": torch.empty(nbytes, dtype=torch.uint8, device=dev),     # exactly: the size tells the call nr_max
                  "seed": torch.full((self.B, N, 3), -1, dtype=torch.int32, device=dev), "order": None}
            if self.spatial_sort:
                from ..relax import kd_order

                st["order"] = kd_order(cano.detach()).to(torch.int32).contiguous()
            with torch.cuda.device(dev):
                rc = L.reart_flow_term_prepare(_lib.ptr(ref), _lib.ptr(flo), _lib.ptr(ref_len), self.B, ref.shape[1],
                                               _lib.ptr(st["ws"]), nbytes, _lib.stream())
            _lib.check(rc, "reart_flow_term_prepare")
            self._state[(N, dev)] = st
        return st

    def seed(self, cano_pc, idx=None):
        """Install neighbour guesses for the next call on clouds of ``cano_pc``'s size: idx [B,N,3], caller numbering (row n of
        pair f: indices into ``pc_ref_list[f]``); None forgets them.  Any values are allowed -- seeds bound the search, they
        never change its result."""
        _lib.require_gpu(cano_pc, idx)
        st = self._get_state(int(cano_pc.shape[0]), cano_pc)
        if idx is None:
            st["seed"].fill_(-1)
            return
        sd = idx.to(device=cano_pc.device, dtype=torch.int64).reshape(st["seed"].shape)
        if self.spatial_sort:
            B, N = sd.shape[0], sd.shape[1]
            ok = (sd >= 0) & (sd < self._lens[:, None, None])
            pos = torch.gather(self._rinv, 1, sd.clamp(0, self._rinv.shape[1] - 1).reshape(B, N * 3)).reshape(B, N, 3)
            sd = torch.where(ok, pos, sd)                        # index -> its stored position
            sd = sd[:, st["order"].long()]                       # row of the point visited at each position
        st["seed"].copy_(sd.clamp(-1, 2 ** 31 - 1).to(torch.int32))

    def _call(self, xd, cd, st, gt, mask, dists, idx, loss, G, accumulate):
        with torch.cuda.device(xd.device):
            rc = _lib.lib().reart_flow_term(_lib.ptr(xd), _lib.ptr(cd), _lib.ptr(st["order"]), self.B, xd.shape[1], self.cano_idx,
                                            0 if self.knn_squared else 1, int(self.robust), self.smooth_weight, self.weight,
                                            _lib.ptr(st["seed"]), _lib.ptr(gt), _lib.ptr(mask), _lib.ptr(dists), _lib.ptr(idx),
                                            _lib.ptr(loss), _lib.ptr(G), int(accumulate), _lib.ptr(st["ws"]), st["ws"].numel(),
                                            _lib.stream())
        _lib.check(rc, "reart_flow_term")

    def _run(self, x, cano):
        B, N, dev = self.B, x.shape[1], x.device
        st = self._get_state(N, cano)
        xd, cd = x.detach().contiguous(), cano.detach().contiguous()
        gt = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
        mask = torch.empty((B, N), dtype=torch.bool, device=dev)
        dists = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
        idx = torch.empty((B, N, 3), dtype=torch.int64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        G = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
        self._call(xd, cd, st, gt, mask, dists, idx, loss, G, 0)
        self._last, self._raw = None, (gt, mask, dists, idx)
        return loss, G

    def serves(self, pc_trans_list, cano_pc):
        """Whether these clouds take the native call (otherwise ``forward`` computes the composition)."""
        return self._served(pc_trans_list, cano_pc)

    @torch.no_grad()
    def add_gradient(self, pc_trans_list, cano_pc, G, loss):
        """The native call for a caller that keeps its own gradient buffer (``KinematicEngine``): ADDS d loss / d pc_trans_list
        onto ``G`` [B,N,3] and writes the value into ``loss`` (a float32 device scalar); nothing else is written, nothing is
        allocated, ``.last`` is left alone.  Contiguous float32 operands the native call serves only."""
        if not self._served(pc_trans_list, cano_pc) or not (pc_trans_list.is_contiguous() and cano_pc.is_contiguous() and G.is_contiguous()):
            raise NotImplementedError("FlowTerm.add_gradient: contiguous float32 [B,N,3] clouds within reart_flow_term's limits")
        if G.shape != pc_trans_list.shape or G.dtype != torch.float32 or loss.dtype != torch.float32:
            raise ValueError("FlowTerm.add_gradient: G like pc_trans_list, loss a float32 scalar")
        _lib.require_gpu(G, loss)
        self._call(pc_trans_list, cano_pc, self._get_state(pc_trans_list.shape[1], cano_pc), None, None, None, None, loss, G, 1)

    @property
    def last(self):
        """Detached ``(gt_flow [B,N,3], mask [B,N] bool, dists [B,N,3], idx [B,N,3] int64)`` of the latest call, in the caller's
        numbering (None before the first call).  With ``spatial_sort`` the indices are renumbered on first access, not in the call."""
        if self._last is None and self._raw is not None:
            gt, mask, dists, idx = self._raw
            if self._rperm is not None:
                B, N = idx.shape[0], idx.shape[1]
                idx = torch.gather(self._rperm, 1, idx.reshape(B, N * 3)).reshape(B, N, 3)
            self._last = (gt, mask, dists, idx)
        return self._last


@torch.no_grad()
def find_mutual_correspondences(nns01, nns10):
    """utils/flow_utils.py:102-113: the pairs (i, nns01[i]) whose target points back at i."""
    idx0 = torch.arange(len(nns01), device=nns10.device)
    keep = nns10[nns01] == idx0
    return idx0[keep], nns01[keep]


def normalize_pc_list(pc_list, centroid, scale):
    """utils/flow_utils.py:173-175."""
    return (pc_list - centroid) * scale


@torch.no_grad()
def match_smnn(desc1, desc2, th=0.9):
    """Mutual second-nearest-neighbour ratio matching (utils/flow_utils.py:48-100).
    desc1 [B1,D], desc2 [B2,D] -> (match_dists [B3,1], matches_idxs [B3,2]) sorted by the desc1 index.
    (match_dists is the larger of the two ratios like the reference; its callers ignore it.)"""
    if desc1.shape[0] < 2 or desc2.shape[0] < 2:
        raise AssertionError
    keep, tgt = _smnn_batched(desc1[None], desc2[None], th)
    src = torch.nonzero(keep[0], as_tuple=False)[:, 0]
    idx = torch.stack([src, tgt[0][src]], dim=1)
    return torch.empty((idx.shape[0], 1), device=desc1.device), idx


def _smnn_batched(d1, d2, th):
    _lib.require_gpu(d1, d2)
    d1, d2 = d1.contiguous().float(), d2.contiguous().float()
    E, N1, D = d1.shape
    N2 = d2.shape[1]
    keep = torch.empty((E, N1), dtype=torch.bool, device=d1.device)
    tgt = torch.empty((E, N1), dtype=torch.int64, device=d1.device)
    L = _lib.lib()
    ws = _lib.workspace(L.reart_match_smnn_workspace_bytes(E, N1, N2), d1.device)
    rc = L.reart_match_smnn(_lib.ptr(d1), _lib.ptr(d2), E, N1, N2, D, float(th), _lib.ptr(keep), _lib.ptr(tgt),
                            _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "reart_match_smnn")
    return keep, tgt


@torch.no_grad()
def compute_corr_list_filter(norm_pc_list, feature_extractor, knn=None, matching="smnn"):
    """One-time correspondence extraction (utils/flow_utils.py:116-143): descriptors of frames
    [:-1] and [1:], then per pair the mutual SMNN matches.  norm_pc_list [T,N,3] ->
    (corrs_src_list, corrs_tgt_list): ragged index lists per consecutive frame pair.
    Every frame's descriptors are computed once (the reference evaluates interior frames twice)."""
    if matching not in ("smnn", "mnn"):
        raise ValueError("matching is 'smnn' (the reference's default, run_robot.py:80) or 'mnn'")
    feats = feature_extractor(norm_pc_list.transpose(1, 2).contiguous())   # [T,64,N]
    feats = feats.permute(0, 2, 1).contiguous()                            # point-major rows
    # "mnn" (utils/flow_utils.py:126-137): nearest descriptor in both directions + the mutual filter, no ratio test --
    # the same two top-2 passes with the test switched off (th < 0); ``knn`` is not needed (the reference's k = 1 KNN)
    keep, tgt = _smnn_batched(feats[:-1], feats[1:], 0.9 if matching == "smnn" else -1.0)
    src_list, tgt_list = [], []
    for e in range(keep.shape[0]):
        src = torch.nonzero(keep[e], as_tuple=False)[:, 0]
        src_list.append(src)
        tgt_list.append(tgt[e][src])
    return src_list, tgt_list


@torch.no_grad()
def correspondence_targets(pred, obs, max_dist):
    """Positives for ``networks.loss.DescriptorInfoNCE`` from a fitted model: ``pred`` [B,N,3] is where the model puts the
    canonical points in every frame (``pc_trans_list``), ``obs`` [B,M,3] the observed frames -> ``pos`` [B,N] int64, the
    index of the observed point nearest to each predicted one (``knn_points``, K = 1: the lowest index on a tie), or -1
    where their squared distance exceeds ``max_dist`` ** 2.  A composition of what exists; no gradient."""
    if pred.dim() != 3 or obs.dim() != 3 or pred.shape[0] != obs.shape[0] or pred.shape[2] != 3 or obs.shape[2] != 3:
        raise ValueError(f"correspondence_targets: pred [B,N,3] and obs [B,M,3], not {tuple(pred.shape)} and {tuple(obs.shape)}")
    if not float(max_dist) >= 0.0:
        raise ValueError(f"correspondence_targets: max_dist = {max_dist} is not a distance")
    _lib.require_gpu(pred, obs)
    from .chamfer import knn_points
    if pred.shape[1] == 0 or obs.shape[1] == 0 or pred.shape[0] == 0:
        return torch.full(tuple(pred.shape[:2]), -1, dtype=torch.int64, device=pred.device)
    nn = knn_points(pred.detach(), obs.detach(), K=1)
    far = nn.dists[..., 0] > float(max_dist) ** 2
    return torch.where(far, torch.full_like(nn.idx[..., 0], -1), nn.idx[..., 0])
