"""Kinematic projection loop without autograd: the reference's loop body (run_robot.py:154-221) for ``--model kinematic``
(networks/model.py:137-166, utils/kinematic_utils.py:151-198) as a fixed sequence of operator calls on the launch
stream -- forward kinematics + rigid apply, assignment re-solve, assignment / flow gradients, the hand-derived FK backward
and Adam (``reart_adam_step``) on the model's own parameter tensors, in place.  ``run_robot.OperatorLoop`` is the same
iteration through PyTorch autograd and ``torch.optim.Adam``; ``tests/test_kinematic_engine_gpu.py`` holds the two together.

What an iteration costs the host here: a dozen ctypes calls and, when the assignment is refreshed, the copy of its result.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .utils import lap
from .utils.flow_utils import blend_anchor_motion
from .utils.kinematic_utils import _effective_joint_values


class KinematicEngine:
    """State of one kinematic projection on one GPU.

    ``model``: a ``KinematicModel`` (any joint types; with or without root motion, networks/model.py:113-166) whose ``axis_list`` /
    ``moment_list`` / ``theta_list`` (and ``distance_list``, ``root_6d``, ``root_t``) are optimised IN PLACE; ``cano_pc`` [N,3], ``pc_list`` [T-1,N,3]; ``pc_ref_list`` / ``flow_ref_list``:
    the flow references of run_robot.py:81-84 or None.  Hyper-parameters carry the reference's flag names
    (run_robot.py:362-420): ``trans_lr`` (Adam lr of every kinematic parameter, :150-151), ``weight_decay``,
    ``use_assign_loss`` / ``assign_iter`` / ``assign_gap`` / ``downsample`` / ``lambda_assign``, ``lambda_flow``,
    ``use_robust_loss``.  Before ``assign_iter`` (or with ``use_assign_loss=False``) the iteration takes the Chamfer branch
    (run_robot.py:187-190): two exact K = 1 searches and ``knn_points_backward`` for dL/d pc_trans, no autograd there either.

    ``recon_with_assign=True`` (off by default: nothing new is allocated, the attributes below are None, every launch is the
    default mode's): the objective of the reference's real-scan and SAPIEN recipes (run_real.py:175-203, run_sapien.py:174-203) --
    the Chamfer loss in EVERY iteration, the assignment loss added to it from ``assign_iter`` on, as ``OperatorLoop`` computes it
    under ``--recon_with_assign``.  The Chamfer term is the warm exact search with its gradient as one call
    (``reart_chamfer_loss``) on clouds stored in k-d order -- one order of the canonical cloud for every predicted frame, each
    observed frame in its own --, in front of the re-solve (queued eagerly between the two captured graphs); ``reart_kin_post_recon`` adds
    its gradient, the pairs' term and the flow term in one write.  Neighbours and distances are bit for bit ``knn_points``'s; a
    tie between distinct equidistant targets goes to the one stored first in the k-d order (``ChamferLoss``'s rule).  The loss
    dictionary has ``OperatorLoop``'s keys in its order: [opt assignment loss,] recon Loss, [flow Loss,] total Loss.
    ``recon_grad()``: the latest Chamfer gradient in the caller's numbering; ``last_fx_bits``: its fixed-point bits.  One
    lambda_assign, no weight on the Chamfer term, K = 1.  The Chamfer gradient is discontinuous where a point has two nearest
    neighbours, so this mode keeps to the bits of an autograd loop over the model: the root motion is applied with the model's
    own expression (product, then addition) and the step is ``reart_amd.optim.Adam`` (torch.optim.Adam's bits, one launch; the
    parameters' ``.grad`` are then the engine's gradient buffers).  Shapes beyond the warm call (frames x (points + 512) >= 2^30) raise
    ``NotImplementedError`` from the constructor.
    """

    def __init__(self, model, cano_pc, pc_list, cano_idx, pc_ref_list=None, flow_ref_list=None, trans_lr=1e-2,
                 weight_decay=0.0, assign_iter=0, assign_gap=5, downsample=4, lambda_assign=3e-1, lambda_flow=1.0,
                 use_robust_loss=False, smooth_weight=1e-2, knn_squared=False, use_assign_loss=True, src_idx=None, tgt_idx=None,
                 warm_flow=False, recon_with_assign=False):
        _lib.require_gpu(cano_pc, pc_list)
        self.recon_with_assign = bool(recon_with_assign)
        self._cham_bytes = 0
        if self.recon_with_assign:      # a shape the warm Chamfer call does not take: refused before anything is launched
            B_, N_ = int(pc_list.shape[0]), int(pc_list.shape[1])
            self._cham_bytes = int(_lib.lib().reart_chamfer_loss_workspace_bytes(B_, N_, N_))
            if self._cham_bytes == 0:
                raise NotImplementedError(f"KinematicEngine(recon_with_assign=True): {B_} frames of {N_} points are beyond "
                                          "reart_chamfer_loss (frames <= 65535, frames x (points + 512) < 2^30)")
        self.root = hasattr(model, "root_6d") and hasattr(model, "root_t")      # networks/model.py:153-158
        self._pris = None
        if model.joint_type_list is not None:
            # utils/kinematic_utils.py:174-186: prismatic joints run with theta = 1e-6 and their distance, revolute joints with
            # their theta and distance = 1e-6; the masked entries take no gradient (torch.where's backward in the autograd loop)
            if not hasattr(model, "distance_list"):
                raise NotImplementedError("joint types without distance_list")
            self._pris = torch.tensor([jt == "prismatic" for jt in model.joint_type_list], device=cano_pc.device)[None, :]
        self.model, self.dev = model, cano_pc.device
        self.cano = cano_pc.contiguous().float()
        self.pc_list = pc_list.contiguous().float()
        self.cano_idx = int(cano_idx)
        self.B, self.N = self.pc_list.shape[:2]
        self.lr, self.wd = float(trans_lr), float(weight_decay)
        self.assign_iter, self.assign_gap, self.lambda_assign = int(assign_iter), int(assign_gap), float(lambda_assign)
        self.use_assign = bool(use_assign_loss)
        self.lambda_flow, self.robust, self.smooth = float(lambda_flow), bool(use_robust_loss), float(smooth_weight)
        self.euclid = 0 if knn_squared else 1
        self.refs = None
        if pc_ref_list is not None:
            self.refs = [(r.reshape(-1, 3).contiguous().float(), f.reshape(-1, 3).contiguous().float())
                         for r, f in zip(pc_ref_list, flow_ref_list)]
            assert len(self.refs) == self.B
        with torch.no_grad():
            self.part = model.seg_forward(self.cano).contiguous().long()      # fixed: label transfer from the model's own cloud
        self.parent, self.edge_of, self.order = model._tree(self.dev)
        self.P = int(self.parent.shape[0])
        # parameters in the order torch.optim.Adam would see them (model.parameters())
        self.params = [p for p in model.parameters() if p.requires_grad]
        for p in self.params:
            assert p.is_cuda and p.is_contiguous() and p.dtype == torch.float32
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        self.grads = {id(p): torch.zeros_like(p) for p in self.params}
        self.lap_steps_log = []
        self.step_count = 0
        # run_robot.py:167-169: both FPS calls sample fixed clouds (start 0 on the reference's CUDA path): once
        # (``src_idx`` [n] / ``tgt_idx`` [T-1,n]: samples handed in instead -- the reference's CPU sampler starts from a random point,
        # networks/pointnet2_utils.py:90, so a trajectory the reference produced on a CPU comes with its samples:
        # tests/golden/kinematic_loop.npz)
        # the sampled targets are the COLUMNS of every re-solve of the run: numbered along a Z-order curve (lap.spatial_order)
        sample = lap.AssignmentSample(self.cano, self.pc_list, downsample, src_idx, tgt_idx)
        self.src_idx, self.tgt_order = sample.src_idx, sample.tgt_order                 # [n]; [B,n] into the FPS order
        self.tgt_idx, self.tgt_pts = sample.tgt_idx, sample.tgt_pts                     # [B,n]; [B,n,3]
        self.matched = None
        self.lap_state = {}
        self.lap_solves = self.lap_fallbacks = 0
        self.lap_events = None
        self.lap_stats = None
        self.lap_winners = np.zeros(32, np.int64)      # wins per racer (JV_RACE_MAX = 28 racers, 5 bits in the statistics)
        self.trans = torch.empty((self.B, self.P, 4, 4), dtype=torch.float32, device=self.dev)
        self.pc_trans = torch.empty((self.B, self.N, 3), dtype=torch.float32, device=self.dev)
        self.G = torch.zeros((self.B, self.N, 3), dtype=torch.float32, device=self.dev)
        # root motion: the articulated cloud before the per-frame rigid motion, and dL/d of it
        self.pc_fk = torch.empty_like(self.pc_trans) if self.root else self.pc_trans
        self.G_fk = torch.empty_like(self.G) if self.root else self.G
        self.losses = {}
        self._pc_src, self._inplace, self._g_pre, self._g_post = None, None, None, None
        self._adam_tab = self._src_idx32 = None
        self._side = None
        # reart_kin_post's inputs that never change: the sample slot of every canonical point, the frames' flow references padded
        # to one length; its buffers (owned here: a captured graph keeps their addresses)
        n, self._slot = sample.n, sample.slot
        self._ref_pad = self._flow_pad = self._ref_len = None
        self._nr_max = 0
        if self.refs is not None:
            lens = [int(r.shape[0]) for r, _ in self.refs]
            self._nr_max = max(lens)
            self._ref_pad = torch.zeros((self.B, self._nr_max, 3), dtype=torch.float32, device=self.dev)
            self._flow_pad = torch.zeros((self.B, self._nr_max, 3), dtype=torch.float32, device=self.dev)
            for f, (r, fl) in enumerate(self.refs):
                self._ref_pad[f, :lens[f]] = r
                self._flow_pad[f, :lens[f]] = fl
            if min(lens) != self._nr_max:
                self._ref_len = torch.tensor(lens, dtype=torch.int64, device=self.dev)
        # warm_flow: the flow term of the fused post as one warm-started call over references prepared once (utils.flow_utils.
        # FlowTerm) behind a reart_kin_post without its flow branch; shapes that call does not serve keep the branch
        self._flow_term = None
        if warm_flow and self.refs is not None and min(int(r.shape[0]) for r, _ in self.refs) >= 3:
            from .utils.flow_utils import FlowTerm

            ft = FlowTerm([r for r, _ in self.refs], [f for _, f in self.refs], self.cano_idx, weight=self.lambda_flow,
                          robust=self.robust, smooth_weight=self.smooth, knn_squared=bool(knn_squared))
            if ft.serves(self.pc_trans, self.cano):
                self._flow_term = ft
        self._matched_buf = torch.zeros((self.B, n, 3), dtype=torch.float32, device=self.dev)
        self._loss3 = torch.zeros((3,), dtype=torch.float32, device=self.dev)
        self._post_ws = torch.empty((max(int(_lib.lib().reart_kin_post_workspace_bytes(self.B, self.N, self._nr_max, 3)), 256),),
                                    dtype=torch.uint8, device=self.dev)
        # recon_with_assign: the state of the warm Chamfer term (reart_chamfer_loss), built once.  One storage order serves the
        # predicted cloud of every frame -- the parts move rigidly, the canonical cloud's locality carries over --, every observed
        # frame is stored in its own; the buffers are owned here (a captured graph keeps their addresses)
        self._order_x = self._inv_x = self._ys = self._seed_xy = self._seed_yx = self._fx_bits = self._cham_ws = None
        self._xs = self._g_recon = self._loss_recon = self._loss4 = self._loss_tmp = None
        self._cham_calls = 0
        self._opt = None        # recon_with_assign: reart_amd.optim.Adam over self.params (created at the first step)
        if self.recon_with_assign:
            from .relax import kd_order

            order = kd_order(self.cano).to(torch.int64)
            inv = torch.empty_like(order)
            inv[order] = torch.arange(self.N, dtype=torch.int64, device=self.dev)
            self._order_x, self._inv_x = order.int().contiguous(), inv.int().contiguous()
            self._ys = torch.stack([self.pc_list[b][kd_order(self.pc_list[b]).long()] for b in range(self.B)]).contiguous()
            self._seed_xy = torch.full((self.B, self.N), -1, dtype=torch.int32, device=self.dev)
            self._seed_yx = torch.full((self.B, self.N), -1, dtype=torch.int32, device=self.dev)
            self._fx_bits = torch.zeros((self.B,), dtype=torch.int32, device=self.dev)
            self._cham_ws = torch.empty((self._cham_bytes,), dtype=torch.uint8, device=self.dev)
            self._xs = torch.empty((self.B, self.N, 3), dtype=torch.float32, device=self.dev)
            self._g_recon = torch.zeros((self.B, self.N, 3), dtype=torch.float32, device=self.dev)
            self._loss_recon = torch.zeros((), dtype=torch.float32, device=self.dev)
            self._loss4 = torch.zeros((4,), dtype=torch.float32, device=self.dev)
            self._loss_tmp = torch.zeros((), dtype=torch.float32, device=self.dev)

    # ---- pieces -----------------------------------------------------------------------------------------------------
    def _joint_values(self):
        m = self.model
        dist = m.distance_list if hasattr(m, "distance_list") else None
        if self._pris is None:
            return _effective_joint_values(m.theta_list, dist, None)
        # (the mask is built once: _effective_joint_values uploads it on every call, which a captured graph cannot hold)
        return (torch.where(self._pris, torch.full_like(m.theta_list, 1e-6), m.theta_list).detach(),
                torch.where(self._pris, dist, torch.full_like(dist, 1e-6)).detach())

    def forward(self):
        """pc_trans [T-1,N,3] and trans_list of the current parameters (no graph kept)."""
        L = _lib.lib()
        m = self.model
        theta, dist = self._joint_values()
        B, E = theta.shape
        rc = L.reart_fk_forward(_lib.ptr(self.parent), _lib.ptr(self.edge_of), _lib.ptr(self.order), self.P,
                                _lib.ptr(m.axis_list), _lib.ptr(m.moment_list), _lib.ptr(theta), _lib.ptr(dist), B, E,
                                _lib.ptr(self.trans), _lib.stream())
        _lib.check(rc, "reart_fk_forward")
        rc = L.reart_compute_pc_transform(_lib.ptr(self.cano), _lib.ptr(self.trans), _lib.ptr(self.part), self.N, self.P,
                                          B, _lib.ptr(self.pc_fk), _lib.stream())
        _lib.check(rc, "reart_compute_pc_transform")
        if self.root:                                     # networks/model.py:153-158: x R^T + t per frame
            R = self._root_rotation()[0]
            if self.recon_with_assign:
                # the model's own expression, product then addition (KinematicModel.forward): the Chamfer term is discontinuous
                # where a point has two nearest neighbours, so this mode computes the cloud bit for bit as the model does and a
                # last-bit difference cannot send the engine and an autograd loop over the model down different branches
                torch.matmul(self.pc_fk, R.transpose(1, 2), out=self.pc_trans)
                self.pc_trans.add_(m.root_t.detach()[:, None, :])
                return self.pc_trans
            torch.baddbmm(m.root_t.detach()[:, None, :], self.pc_fk, R.transpose(1, 2), out=self.pc_trans)
        return self.pc_trans

    def trans_list(self):
        """The parts' transforms of the last forward, root motion included (what the model's forward returns third)."""
        if not self.root:
            return self.trans
        root = torch.zeros((self.B, 4, 4), dtype=torch.float32, device=self.dev)
        root[:, :3, :3], root[:, :3, 3], root[:, 3, 3] = self._root_rotation()[0], self.model.root_t.detach(), 1.0
        return torch.matmul(root[:, None], self.trans)

    def _root_rotation(self):
        """R [T-1,3,3] of the 6-D parameters (Gram-Schmidt, rows b1, b2, b1 x b2) and what its backward needs."""
        r6 = self.model.root_6d.detach()
        a1, a2 = r6[:, :3], r6[:, 3:]
        n1 = a1.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        b1 = a1 / n1
        s = (b1 * a2).sum(-1, keepdim=True)
        v = a2 - s * b1
        n2 = v.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        b2 = v / n2
        return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2), (a2, n1, b1, s, n2, b2)

    def _root_backward(self):
        """self.G = dL/d pc_trans -> gradients of root_6d / root_t, and self.G_fk = dL/d (the cloud before the root motion):
        the hand-derived backward of x R^T + t and of the Gram-Schmidt step (autograd's in OperatorLoop)."""
        m = self.model
        R, (a2, n1, b1, s, n2, b2) = self._root_rotation()
        self.grads[id(m.root_t)].copy_(self.G.sum(dim=1))
        dR = torch.matmul(self.G.transpose(1, 2), self.pc_fk)           # [T-1,3,3]: rows = gradients of b1, b2, b3
        torch.matmul(self.G, R, out=self.G_fk)
        g1, g2, g3 = dR[:, 0], dR[:, 1], dR[:, 2]
        g_b1 = g1 + torch.cross(b2, g3, dim=-1)                         # b3 = b1 x b2
        g_b2 = g2 + torch.cross(g3, b1, dim=-1)
        g_v = (g_b2 - (g_b2 * b2).sum(-1, keepdim=True) * b2) / n2      # b2 = v / |v|
        gvb = (g_v * b1).sum(-1, keepdim=True)
        g_a2 = g_v - gvb * b1                                           # v = a2 - (b1 . a2) b1
        g_b1 = g_b1 - gvb * a2 - s * g_v
        g_a1 = (g_b1 - (g_b1 * b1).sum(-1, keepdim=True) * b1) / n1     # b1 = a1 / |a1|
        self.grads[id(m.root_6d)].copy_(torch.cat((g_a1, g_a2), dim=-1))

    def _backward(self):
        """dL/d pc_trans (self.G) -> gradients of axis / moment / theta (/ distance)."""
        L = _lib.lib()
        m = self.model
        theta, dist = self._joint_values()
        B, E = theta.shape
        g_axis, g_moment, g_theta = self.grads[id(m.axis_list)], self.grads[id(m.moment_list)], self.grads[id(m.theta_list)]
        g_dist = self.grads[id(m.distance_list)] if hasattr(m, "distance_list") else None
        if self.root:
            self._root_backward()
        ws = _lib.workspace(L.reart_fk_backward_workspace_bytes(self.P, B, E), self.dev)
        rc = L.reart_fk_backward(_lib.ptr(self.cano), _lib.ptr(self.part), _lib.ptr(self.G_fk), self.N, _lib.ptr(self.parent),
                                 _lib.ptr(self.edge_of), _lib.ptr(self.order), self.P, _lib.ptr(m.axis_list),
                                 _lib.ptr(m.moment_list), _lib.ptr(theta), _lib.ptr(dist), B, E, _lib.ptr(self.trans),
                                 _lib.ptr(g_axis), _lib.ptr(g_moment), _lib.ptr(g_theta), _lib.ptr(g_dist), _lib.ptr(ws),
                                 ws.numel(), _lib.stream())
        _lib.check(rc, "reart_fk_backward")
        if self._pris is not None:
            g_theta.masked_fill_(self._pris, 0.0)
            g_dist.masked_fill_(~self._pris, 0.0)

    def _adam(self):
        """torch.optim.Adam's step on every parameter tensor (run_robot.py:219-221) in one launch (reart_adam_step_multi)."""
        import ctypes

        L = _lib.lib()
        self.step_count += 1
        if self.recon_with_assign:
            # torch.optim.Adam's step in torch's own bits (reart_amd.optim.Adam: one launch, no synchronisation; its weight decay
            # is torch's L2 form).  reart_adam_step_multi rounds a step differently in the last bit, and with the Chamfer term in
            # every iteration one last bit can switch a point's nearest neighbour, where the gradient is discontinuous: this mode
            # stays on the trajectory of an autograd loop with torch.optim.Adam.  The parameters' .grad are the engine's buffers.
            if self._opt is None:
                from .optim import Adam

                self._opt = Adam(self.params, lr=self.lr, weight_decay=self.wd)
            for p in self.params:
                if p.grad is not self.grads[id(p)]:
                    p.grad = self.grads[id(p)]
            self._opt.step()
            return
        grads = []
        for p in self.params:
            g = self.grads[id(p)]
            if self.wd != 0.0:
                g = g + self.wd * p.detach()          # torch.optim.Adam's L2 form
            grads.append(g)
        if self._adam_tab is None or self.wd != 0.0:      # per launch of at most eight tensors: host arrays of pointers, sizes, rates
            self._adam_tab = []
            for a in range(0, len(self.params), 8):
                ps, gs, ms, vs = self.params[a:a + 8], grads[a:a + 8], self.m[a:a + 8], self.v[a:a + 8]
                k = len(ps)
                vp = ctypes.c_void_p * k
                self._adam_tab.append((k, vp(*[p.data_ptr() for p in ps]), vp(*[g.data_ptr() for g in gs]), vp(*[m_.data_ptr() for m_ in ms]),
                                       vp(*[v_.data_ptr() for v_ in vs]), (ctypes.c_int * k)(*[p.numel() for p in ps]),
                                       (ctypes.c_float * k)(*([self.lr] * k))))
        for k, tp, tg, tm, tv, tn, tl in self._adam_tab:
            rc = L.reart_adam_step_multi(k, tp, tg, tm, tv, tn, tl, self.step_count, 0.9, 0.999, 1e-8, _lib.stream())
            _lib.check(rc, "reart_adam_step_multi")

    def _flow_terms(self):
        """lambda_flow * flow_loss and its gradient added to self.G (run_robot.py:194-209)."""
        from .networks.loss import _FlowLoss  # the operator below it is reart_flow_loss

        L = _lib.lib()
        c = self.cano_idx
        comp = torch.cat((self.pc_trans[:c], self.cano[None], self.pc_trans[c:]), dim=0)          # [T,N,3]
        gt = torch.empty((self.B, self.N, 3), dtype=torch.float32, device=self.dev)
        mask = torch.empty((self.B, self.N), dtype=torch.bool, device=self.dev)
        # the T-1 blends are independent and small (16 workgroups each, a chain of gathers): dealt to a few side streams they
        # run side by side -- in a captured graph as parallel branches -- instead of one after the other
        cur = torch.cuda.current_stream()
        if self._side is None:
            self._side = [torch.cuda.Stream(device=self.dev) for _ in range(min(self.SIDE_STREAMS, len(self.refs)))]
        for st in self._side:
            st.wait_stream(cur)
        for f, (r, fl) in enumerate(self.refs):
            with torch.cuda.stream(self._side[f % len(self._side)]):
                ws = _lib.workspace(L.reart_blend_anchor_motion_workspace_bytes(self.N, r.shape[0], 3), self.dev)
                rc = L.reart_blend_anchor_motion(_lib.ptr(comp[f]), _lib.ptr(r), _lib.ptr(fl), self.N, r.shape[0], 3, self.euclid,
                                                 _lib.ptr(gt[f]), _lib.ptr(mask[f]), _lib.ptr(ws), ws.numel(), _lib.stream())
                _lib.check(rc, "reart_blend_anchor_motion")
        for st in self._side:
            cur.wait_stream(st)
        pred = (comp[1:] - comp[:-1]).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=self.dev)
        gp = torch.empty_like(pred)
        ws = _lib.workspace(L.reart_flow_loss_workspace_bytes(), self.dev)
        rc = L.reart_flow_loss(_lib.ptr(gt), _lib.ptr(pred), _lib.ptr(mask), self.B, self.N, int(self.robust), self.smooth,
                               _lib.ptr(loss), _lib.ptr(gp), _lib.ptr(ws), ws.numel(), _lib.stream())
        _lib.check(rc, "reart_flow_loss")
        gp = gp * self.lambda_flow
        # pred = comp[1:] - comp[:-1]: +gp to frame f+1, -gp to frame f; the canonical frame takes no gradient
        gc = torch.zeros_like(comp)
        gc[1:] += gp
        gc[:-1] -= gp
        self.G += torch.cat((gc[:c], gc[c + 1:]), dim=0)
        return loss * self.lambda_flow

    # ---- the iteration ----------------------------------------------------------------------------------------------
    GRAPHS = True       # replay the launches around the solve from two captured graphs (False: every launch eagerly)
    SIDE_STREAMS = 6    # streams the per-frame flow blends of an iteration are dealt to

    def _solve(self, pc_src, timer, behind=None):
        """The assignment refresh (run_robot.py:165-178) -> the solver's [B,4] statistics; the optimum is in lap_state["cols"].
        ``timer``: the started ``lap.EventPair`` of this solve; its end is recorded behind the solve's launches, before the host waits.
        ``behind``: launches that only READ the optimum (the replay of the post graph), queued behind the re-solve BEFORE the host
        waits for its flags -- the GPU goes straight on while the host wakes up and reads them (75-85 us of every iteration
        otherwise: tools/solve_gaps.py) -- and queued once more in the rare case that the host then changed the columns (a tied
        or an uncertified problem).  Returns True when ``behind`` ran."""
        B, n = pc_src.shape[:2]
        ran = False
        if lap.InPlaceResolve.usable(self.lap_state, B, n):
            if self._inplace is None:
                self._inplace = lap.InPlaceResolve(B, n, self.dev)
            self._inplace.begin(pc_src, self.tgt_pts, self.lap_state, stats=True)
            timer.end()
            if behind is not None:
                behind()
                ran = True
            fb, raw, changed = self._inplace.finish()
            if changed and ran:
                behind()
            st = lap.unpack_chain_stats(raw, self.lap_state)
        else:       # the first solve (cold), sizes outside the chain forms: the general entry (its columns are a new tensor)
            _, fb, st = lap.linear_sum_assignment_points(pc_src.contiguous(), self.tgt_pts, self.lap_state, return_stats="full", device_cols=True)
            self._g_post = None                     # a graph that reads the columns must see the new tensor
            timer.end()
        self.lap_solves += 1
        self.lap_fallbacks += fb
        self.lap_stats = st
        # sequential steps of this solve per problem (slowest, mean) and the slowest problem's search steps alone -- the latency
        # roofline of bench.py multiplies them by the measured floor of one step
        search, reduction, winner = lap.stats_fields(st)
        seq = search.astype(np.int64)
        search_only = int(seq.max())
        if self.lap_state.get("resolve_form", "jv") == "jv":           # one row at a time: the row reduction's steps are sequential too
            seq = seq + reduction.astype(np.int64)
        elif self.lap_state.get("backward_rounds") is not None:        # the backward growth before the searches: the same kind of step
            seq = seq + np.asarray(self.lap_state["backward_rounds"], dtype=np.int64)
        self.lap_steps_log.append((int(seq.max()), float(seq.mean()), search_only))
        self.lap_winners += np.bincount(winner, minlength=32)[:32]                  # raced re-solves: who finished first
        return ran

    def _pre(self):
        """Forward of the current parameters and the sampled source points (the solver's input)."""
        self.forward()
        if self._src_idx32 is None:
            self._src_idx32 = self.src_idx.int().contiguous()
        rc = _lib.lib().reart_gather_points(_lib.ptr(self.pc_trans), _lib.ptr(self._src_idx32), self.B, self.N, int(self._src_idx32.numel()),
                                            _lib.ptr(self._pc_src), _lib.stream())                 # pc_trans[:, src_idx], one launch
        _lib.check(rc, "reart_gather_points")

    def _recon_term(self):
        """recon_with_assign: recon_loss(pc_trans, pc_list) (networks/loss.py:24-29) and its gradient w.r.t. pc_trans as the warm
        exact search's one call, on the stored clouds: self._loss_recon, self._g_recon (rows in the stored order), self._fx_bits.
        Neighbours and distances are bit for bit ``knn_points``'s; a tie between distinct equidistant targets goes to the one stored
        first in the k-d order (``ChamferLoss``'s rule).  The seeds are in/out and never change a result."""
        L = _lib.lib()
        B, N = self.B, self.N
        rc = L.reart_gather_points(_lib.ptr(self.pc_trans), _lib.ptr(self._order_x), B, N, N, _lib.ptr(self._xs), _lib.stream())
        _lib.check(rc, "reart_gather_points")
        # y_unchanged: 0 on the first call with this workspace, 1 afterwards
        rc = L.reart_chamfer_loss(_lib.ptr(self._xs), _lib.ptr(self._ys), B, N, N, _lib.ptr(self._seed_xy), _lib.ptr(self._seed_yx),
                                  int(self._cham_calls > 0), None, None, None, None, _lib.ptr(self._loss_recon), _lib.ptr(self._g_recon),
                                  None, _lib.ptr(self._fx_bits), _lib.ptr(self._cham_ws), self._cham_ws.numel(), _lib.stream())
        _lib.check(rc, "reart_chamfer_loss")
        self._cham_calls += 1

    def recon_grad(self):
        """recon_with_assign: the latest Chamfer gradient d recon_loss / d pc_trans [T-1,N,3] in the caller's point numbering."""
        return self._g_recon.index_select(1, self._inv_x.long())

    @property
    def last_fx_bits(self):
        """recon_with_assign: the fractional bits [T-1] of the latest Chamfer gradient's fixed-point sums (reart_chamfer_loss)."""
        return self._fx_bits

    FUSED_POST = True   # reart_kin_post (nine launches); False: the same values as tensor expressions (_post_expressions)

    def _post_recon(self, assign):
        """_post of a recon_with_assign engine (reart_kin_post_recon: the launches of reart_kin_post): G = Chamfer gradient + the
        pairs' term + the flow term, four losses.  ``assign`` False: the Chamfer-only form (n = 0) of the iterations before
        assign_iter."""
        L = _lib.lib()
        n = int(self.src_idx.numel()) if assign else 0
        warm = self._flow_term is not None
        rc = L.reart_kin_post_recon(_lib.ptr(self.pc_trans), _lib.ptr(self.cano), self.B, self.N, self.cano_idx,
                                    _lib.ptr(self._pc_src) if assign else None, _lib.ptr(self.tgt_pts) if assign else None,
                                    _lib.ptr(self.lap_state["cols"]) if assign else None, _lib.ptr(self._slot) if assign else None, n,
                                    self.lambda_assign, None if warm else _lib.ptr(self._ref_pad), None if warm else _lib.ptr(self._flow_pad),
                                    None if warm else _lib.ptr(self._ref_len), self._nr_max, 3, self.euclid, self.lambda_flow,
                                    int(self.robust), self.smooth, _lib.ptr(self._g_recon), _lib.ptr(self._inv_x), _lib.ptr(self._loss_recon),
                                    _lib.ptr(self.G), _lib.ptr(self._matched_buf) if assign else None, _lib.ptr(self._loss4),
                                    _lib.ptr(self._post_ws), self._post_ws.numel(), _lib.stream())
        _lib.check(rc, "reart_kin_post_recon")
        l4 = self._loss4
        if warm:        # flow gradient onto G, its value into losses[1], the total redone in the order of losses[3]
            self._flow_term.add_gradient(self.pc_trans, self.cano, self.G, l4[1])
            torch.add(l4[0], l4[2], out=self._loss_tmp)
            torch.add(self._loss_tmp, l4[1], out=l4[3])
        losses = {}
        if assign:
            self.matched = self._matched_buf
            losses["opt assignment loss"] = l4[0]
        losses["recon Loss"] = l4[2]
        if self.refs is not None:
            losses["flow Loss"] = l4[1]
        losses["total Loss"] = l4[3]
        self._backward()
        self.losses = losses

    def _post(self, assign=True):
        """Everything between the solve and Adam: matched targets, assignment (+ flow) loss, dL/d pc_trans, the FK backward.
        ``assign`` False (recon_with_assign engines only): no pairs, the Chamfer-only form."""
        if (not self.FUSED_POST or (assign and self.lap_state["cols"].dtype != torch.int32)
                or (self.refs is not None and min(int(r.shape[0]) for r, _ in self.refs) < 3)):
            return self._post_expressions(assign)
        if self.recon_with_assign:
            return self._post_recon(assign)
        L = _lib.lib()
        n = int(self.src_idx.numel())
        warm = self._flow_term is not None     # then reart_kin_post runs without references: its assignment branch overwrites G
        rc = L.reart_kin_post(_lib.ptr(self.pc_trans), _lib.ptr(self.cano), self.B, self.N, self.cano_idx, _lib.ptr(self._pc_src),
                              _lib.ptr(self.tgt_pts), _lib.ptr(self.lap_state["cols"]), _lib.ptr(self._slot), n, self.lambda_assign,
                              None if warm else _lib.ptr(self._ref_pad), None if warm else _lib.ptr(self._flow_pad),
                              None if warm else _lib.ptr(self._ref_len), self._nr_max, 3, self.euclid,
                              self.lambda_flow, int(self.robust), self.smooth, _lib.ptr(self.G), _lib.ptr(self._matched_buf),
                              _lib.ptr(self._loss3), _lib.ptr(self._post_ws), self._post_ws.numel(), _lib.stream())
        _lib.check(rc, "reart_kin_post")
        if warm:
            # the flow gradient is added onto the G just written, the value into losses[1], and the total is redone: replaying
            # the pair twice around a re-solve gives the same buffers (seeds never change a result)
            self._flow_term.add_gradient(self.pc_trans, self.cano, self.G, self._loss3[1])
            torch.add(self._loss3[0], self._loss3[1], out=self._loss3[2])
        self.matched = self._matched_buf
        losses = {"opt assignment loss": self._loss3[0]}
        if self.refs is not None:
            losses["flow Loss"] = self._loss3[1]
        losses["total Loss"] = self._loss3[2]
        self._backward()
        self.losses = losses

    def _post_expressions(self, assign=True):
        """_post as the reference's tensor expressions (run_robot.py:177-209) over the per-frame operators: the form reart_kin_post
        replaced, kept as its check (tests/test_kinematic_engine_gpu.py)."""
        if self.recon_with_assign:
            return self._post_recon_expressions(assign)
        cols = self.lap_state["cols"].long()
        self.matched = self.tgt_pts.gather(1, cols[..., None].expand(-1, -1, 3))
        diff = self._pc_src - self.matched
        ass = self.lambda_assign * (diff * diff).sum()                                            # run_robot.py:181-184
        self.G.zero_()
        self.G[:, self.src_idx] = (2.0 * self.lambda_assign) * diff
        losses = {"opt assignment loss": ass}
        total = ass
        if self.refs is not None:
            fl = self._flow_terms()
            losses["flow Loss"] = fl
            total = total + fl
        losses["total Loss"] = total
        self._backward()
        self.losses = losses

    def _post_recon_expressions(self, assign):
        """_post_recon as tensor expressions that round as reart_kin_post_recon does (its check, and the path when FUSED_POST is
        off or the columns are not int32): G = the Chamfer gradient in the caller's numbering, the pairs' term added at the
        sampled points, then the flow term; total = (assignment + Chamfer) + flow, OperatorLoop's order."""
        self.G.copy_(self._g_recon.index_select(1, self._inv_x.long()))
        losses = {}
        total = self._loss_recon
        if assign:
            cols = self.lap_state["cols"].long()
            self.matched = self.tgt_pts.gather(1, cols[..., None].expand(-1, -1, 3))
            diff = self._pc_src - self.matched
            ass = self.lambda_assign * (diff * diff).sum()
            self.G[:, self.src_idx] = self.G[:, self.src_idx] + (2.0 * self.lambda_assign) * diff
            losses["opt assignment loss"] = ass
            total = ass + total
        losses["recon Loss"] = self._loss_recon
        if self.refs is not None:
            fl = self._flow_terms()
            losses["flow Loss"] = fl
            total = total + fl
        losses["total Loss"] = total
        self._backward()
        self.losses = losses

    def _post_chamfer(self):
        """The Chamfer branch (run_robot.py:187-190: recon_loss = sum of the bidirectional per-point Chamfer distance,
        networks/loss.py:24-29) without autograd: both searches, then the gradient of each direction's distances w.r.t. the
        predicted cloud (utils/chamfer.py:195-209 with grad_dists = 1), flow terms, FK backward.  (The default mode's branch; a
        recon_with_assign engine never runs it.)"""
        from . import chamferdist_C as _C

        X, Y = self.pc_trans, self.pc_list
        i1, d1 = _C.knn_points_idx(X, Y, None, None, 1)
        i2, d2 = _C.knn_points_idx(Y, X, None, None, 1)
        rec = d1.sum() + d2.sum()
        ones = torch.ones_like(d1)
        g1, _ = _C.knn_points_backward(X, Y, None, None, i1, ones)
        _, g2 = _C.knn_points_backward(Y, X, None, None, i2, ones)
        self.G.copy_(g1)
        self.G += g2
        losses = {"recon Loss": rec}
        total = rec
        if self.refs is not None:
            fl = self._flow_terms()
            losses["flow Loss"] = fl
            total = total + fl
        losses["total Loss"] = total
        self._backward()
        self.losses = losses

    @staticmethod
    def _graph(fn):
        fn()                                        # warm-up outside the capture (lazy loads, workspace growth)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            fn()
        return g

    @torch.no_grad()
    def iteration(self, i):
        """Iteration i of run_robot.py:154-221 in the assignment-loss branch; returns the loss dictionary (device tensors).
        From the third iteration on the launches before and after the solve replay from two captured graphs (the solve itself
        and Adam, whose step count is a host value, stay eager): same launches, same results, a tenth of the host work."""
        if not self.use_assign or i < self.assign_iter:                   # run_robot.py:187-190
            self.forward()
            if self.recon_with_assign:      # the warm Chamfer term and the consumer's Chamfer-only form; eager, as this branch is
                self._recon_term()
                self._post(assign=False)
            else:
                self._post_chamfer()
            self._adam()
            return self.losses
        if self._pc_src is None:
            self._pc_src = torch.empty((self.B, self.src_idx.numel(), 3), dtype=torch.float32, device=self.dev)
        if self._g_pre is not None:
            self._g_pre.replay()
        else:
            self._pre()
            if self.GRAPHS and self.lap_solves >= 2:
                self._g_pre = self._graph(self._pre)                      # (the warm-up inside recomputes the same forward)
        if self.recon_with_assign:
            # The Chamfer term does not depend on the optimum: in front of the re-solve.  Queued eagerly (five launches and the
            # 4-byte memset of its reduction's counter), not captured with _pre: replayed from the captured graph beside an
            # autograd loop in the same process, the call stopped writing its loss from the sixth iteration on (the gradient
            # stayed right) -- measured on the MI355X, deterministic, cause not found; tests/test_kinematic_both_gpu.py
            # (test_the_recon_loss_is_current_in_every_iteration) holds the eager form
            self._recon_term()
        posted = False
        if self.lap_state.get("cols") is None or i % self.assign_gap == 0:                       # run_robot.py:165-178
            timer = lap.EventPair(self.lap_events).start()      # (_solve records the end right behind the re-solve's launches)
            posted = self._solve(self._pc_src, timer, behind=self._g_post.replay if self._g_post is not None else None)
        if posted:
            pass                                        # (the post graph went in behind the re-solve)
        elif self._g_post is not None:
            self._g_post.replay()
        elif self.GRAPHS and self.lap_solves >= 2 and self._inplace is not None:
            self._g_post = self._graph(self._post)                        # (warm-up + capture; the replay below does the work once more:
            self._g_post.replay()                                         #  _post only writes buffers it fully overwrites)
        else:
            self._post()
        self._adam()
        return self.losses
