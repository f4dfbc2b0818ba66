#!/usr/bin/env python3
"""Drop-in counterpart of the reference's ``run_robot.py`` optimisation loop (``:154-221``) on the
HIP path: same command-line flags and defaults (``run_robot.py:362-420``), same checkpoint keys
(``:340-356``), same loss branches.

What is built: the loop itself.
  * ``--model base`` without assignment loss (the first ``--assign_iter`` iterations of every run,
    and whole runs without ``--use_assign_loss``): the fused ``RelaxEngine`` -- five kernel launches
    per iteration replayed from a graph, no host sync inside the loop.
  * ``--model base`` with ``--use_assign_loss`` after ``--assign_iter``: the same engine in its
    assignment-loss mode; every ``--assign_gap`` iterations the host refreshes the pairs (forward of the
    coming iteration, FPS, cost matrices, GPU linear assignment), in between the engine runs alone.
    With ``--recon_with_assign`` (off by default) the assignment loss is added to the Chamfer loss instead of taking
    its place, as the reference's ``run_real.py:175-203`` does; ``--model kinematic`` then runs through ``OperatorLoop``.
  * ``--model kinematic``: the reference's own loop structure with
    the HIP operators underneath (``BaseModel`` / ``KinematicModel``, ``ChamferDistance``,
    ``blend_anchor_motion``, ``flow_loss``, FPS) and ``torch.optim.Adam``; the linear assignment of the
    reference (``run_robot.py:172-176``, scipy on a process pool) runs on the GPU (``reart_lap_auction``:
    auction + exact dual certificate, host fallback for an uncertified matrix).
  * end of run (``run_robot.py:224-330``): ``reart_amd.tail`` -- denoise / merge / spanning tree / renumbering,
    the model-selection energy (assignment, screw and group errors), ``result.pkl`` / ``result.txt`` /
    ``model.pth.tar`` with the reference's keys; ``--model kinematic --base_result_path result.pkl`` builds the
    joint tree from a base result (``run_robot.py:101-124``).
What is NOT built (SURVEY.md section 8 out of scope): visualisation (gif / html) and the GT-graph tree edit distance
(``apted``); ground-truth metrics and the retargeting error (``ik``) are reported when the sequence carries them.

Data: ``--seq_path`` with the reference's pickle layout (``reart_amd.dataset.Sequence`` = ``dataset/dataset_robot.py``), or
``--synthetic`` for the generated articulated sequence of ``reart_amd/synthetic.py``.
"""
import argparse
import contextlib
import ctypes
import functools
import glob
import os
import pickle
import random

import numpy as np
import torch

from reart_amd.knn_cuda import KNN
from reart_amd.networks.loss import flow_loss, recon_loss
from reart_amd.networks.model import BaseModel, KinematicModel
from reart_amd.networks.pointnet2_utils import index_points
from reart_amd.relax import RelaxEngine
from reart_amd.utils.chamfer import ChamferDistance, ChamferLoss
from reart_amd.utils.flow_utils import FlowTerm, blend_anchor_motion, blend_anchor_motion_batch, pad_reference_sets
from reart_amd.utils.model_utils import tau_cosine


def load_sequence(seq_path, num_points, cano_idx):
    """The reference's sample dictionary (dataset/dataset_robot.py:9-100) through the mirror loader."""
    from reart_amd.dataset import Sequence

    return Sequence(seq_path, num_points=num_points, cano_idx=cano_idx)[0]


def synthetic_sequence(num_points, cano_idx, frames, with_flow, seed=2):
    from reart_amd.synthetic import make_sequence, split_canonical

    seq = make_sequence(T=frames, n_parts=8, pts_per_part=num_points // 8, seed=seed, with_flow=with_flow)
    cano, pc_list = split_canonical(seq["complete"], cano_idx)
    out = dict(cano_pc=cano, pc_list=pc_list, complete_pc_list=seq["complete"], gt_cano_part=seq["part"])
    if with_flow:
        out.update(ref_loc=seq["ref_loc"], ref_flow=seq["ref_flow"])
    return out


def flow_references(args, sample, device, seq_path=None):
    """The flow branch's reference sets (run_robot.py:64-84) -> (pc_ref_list, flow_ref_list), lists of [M_i,3] tensors:
    the generator's own references for a synthetic sample, otherwise descriptors -> SMNN matches -> reference flows."""
    if "ref_loc" in sample:  # synthetic references (true motion + noise)
        return ([torch.from_numpy(r).to(device) for r in sample["ref_loc"]],
                [torch.from_numpy(f).to(device) for f in sample["ref_flow"]])
    from reart_amd.networks.feature_extractor import get_extractor
    from reart_amd.utils.dataset_utils import load_normalize_dict
    from reart_amd.utils.flow_utils import compute_corr_list_filter, normalize_pc_list

    extractor = get_extractor(args)
    info = load_normalize_dict(args.normalize_file)[os.path.basename(seq_path.rstrip("/"))]
    centroid = torch.from_numpy(info["centroid"]).float().to(device)
    complete = torch.from_numpy(sample["complete_pc_list"]).float().to(device)
    norm = normalize_pc_list(complete, centroid, info["scale"].item())
    src_list, tgt_list = compute_corr_list_filter(norm, extractor, None, matching="smnn")
    return ([complete[i][s] for i, s in enumerate(src_list)],
            [complete[i + 1][t] - complete[i][s] for i, (s, t) in enumerate(zip(src_list, tgt_list))])


def _cat(parts):
    """torch.cat along dim 0; a single part is returned as it is (no copy, no launch)."""
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)


class AssignmentPhase:
    """The base model's assignment-loss phase (run_robot.py:164-187) on the fused ``RelaxEngine``.  Every ``assign_gap``
    iterations: forward of the coming iteration (``peek_forward``: the temperature and noise the step will use) -> the sampled
    source points (FPS of the canonical cloud, run_robot.py:167) -> optimal assignment to the sampled target points
    (``cdist`` + ``linear_sum_assignment`` in the reference, :170-176) -> the pairs go to the engine, which then runs the
    iterations up to the next refresh from a captured graph without touching the host.
    Both FPS calls of the reference sample fixed clouds from a fixed start (its CUDA FPS starts at index 0): computed once
    (``lap.AssignmentSample``, one per engine in ``parts``).
    The first refresh is a cold solve (raced auction + exact certificate); every later one re-solves from the previous
    optimum and potentials (``linear_sum_assignment_points``: shortest augmenting paths, the row reduction one chain per
    wave, costs recomputed from the points, same certificate).  ``fallbacks`` counts matrices that went to the host solver.

    The phase drives 1..K engines of one shape through a *stepper*, the object whose ``step(n)`` and
    ``capture(steps_per_graph)`` advance them: this constructor takes one engine, which is its own stepper;
    ``AssignmentPhaseBatch`` takes the K engines of a ``RelaxBatch``.  With K engines every refresh gathers the sampled source
    points of all of them and solves their K x (T-1) problems in ONE call -- one set of launches, every problem its own
    workgroup(s) --, then hands each engine its pairs: rows k (T-1) ... of ``tgt_idx`` / ``tgt_order`` / ``tgt_pts`` /
    ``lap_state["cols"]`` and row k of ``src_idx`` belong to engine k.  Each engine ends exactly as it would alone (the optimal
    assignment does not depend on who else is in the call)."""

    NATIVE = os.environ.get("REART_ASSIGN_NATIVE", "1") != "0"      # "0": every refresh through the host path's tensor operations

    def __init__(self, eng, cano_pc, pc_list, downsample, assign_gap, lambda_assign):
        self._setup(eng, [eng], [(cano_pc, pc_list)], downsample, assign_gap, lambda_assign)

    def _setup(self, stepper, engines, clouds, downsample, assign_gap, lambda_assign):
        """clouds: [(cano_pc, pc_list)] per engine, in the caller's point order."""
        from reart_amd.utils.lap import AssignmentSample

        self.stepper, self.engines = stepper, list(engines)
        self.gap, self.lam = int(assign_gap), float(lambda_assign)
        # the sampled targets are the COLUMNS of every refresh: numbered along a Z-order curve (lap.spatial_order: the searches'
        # waves then hold neighbouring columns); the pairs a refresh returns are the same whatever the numbering
        self.parts = [AssignmentSample(c, p, downsample) for c, p in clouds]
        if len({tuple(s.tgt_idx.shape) for s in self.parts}) != 1:
            raise ValueError("AssignmentPhase: the engines must share one shape")
        self.B, self.n = self.parts[0].tgt_idx.shape
        self.src_idx = _cat([s.src_idx[None] for s in self.parts])                                                   # [K, n]
        self.tgt_order, self.tgt_idx, self.tgt_pts = (_cat([getattr(s, a) for s in self.parts]) for a in ("tgt_order", "tgt_idx", "tgt_pts"))
        self.lap_state = {}
        self.refreshes = self.fallbacks = 0
        self.events = None          # set to [] to collect a (start, end) torch.cuda.Event pair around every solve
        self.collect_stats = False  # True: the solver's per-problem statistics of every refresh are read (B x 4 ints) into stats_log
        self.stats_log = []         # per refresh: (sequential steps of the slowest problem = search steps + backward rounds, mean search
                                    # steps, mean row-reduction steps, most search steps, mean backward rounds)
        self.stats_raw = []         # per device-side refresh: the solver's [B,4] statistics words as written (tools/exp_tail.py)
        self.capture_guard = None   # a context-manager factory entered around the graph capture (the sweep's _CaptureGate)
        self.work_guard = None      # a context-manager factory entered around every refresh (the sweep's gate, reader side)
        self._have = False
        # the device path's tables (_native_tables)
        self._src_stored = self._slot = self._tgt_stored = self._src_pts = self._inplace = None

    def _native_tables(self):
        """What the device-side refresh needs, built once.  Per engine, in the engine's STORAGE order: the stored position of
        every sampled canonical point, the sample slot of every stored point (-1: not sampled), the stored position of every
        sampled target point.  For all: the solver's source points and the re-solve itself."""
        from reart_amd.utils import lap

        dev, N = self.engines[0].device, self.parts[0].N
        stored = [e.stored_indices(s.src_idx, s.tgt_idx) for e, s in zip(self.engines, self.parts)]
        self._src_stored = [src.int().contiguous() for src, _ in stored]
        self._slot = [lap.slot_table(src, N) for src, _ in stored]
        self._tgt_stored = [tgt.int().contiguous() for _, tgt in stored]
        self._src_pts = torch.empty((len(self.engines) * self.B, self.n, 3), device=dev)
        self._inplace = lap.InPlaceResolve(len(self.engines) * self.B, self.n, dev)

    def _refresh_on_device(self):
        """A refresh after the first, without a host-side tensor operation: a gather per engine into one source batch
        (reart_gather_points) -> ONE re-solve of all problems from the previous optimum in place (lap.InPlaceResolve) -> a pair
        map per engine (reart_assign_pairs), all queued behind the forward; the host waits for the certificate flags only (an
        uncertified problem goes to scipy, as everywhere)."""
        from reart_amd import _lib
        from reart_amd.utils import lap

        st, L, B, n, N = self.lap_state, _lib.lib(), self.B, self.n, self.parts[0].N
        self._inplace.launches.guard = self.capture_guard
        cols = st["cols"]

        def gather():
            for k, e in enumerate(self.engines):
                _lib.check(L.reart_gather_points(_lib.ptr(e._pc_trans), _lib.ptr(self._src_stored[k]), B, N, n,
                                                 _lib.ptr(self._src_pts[k * B:]), _lib.stream()), "reart_gather_points")

        def pairs():
            for k, e in enumerate(self.engines):
                _lib.check(L.reart_assign_pairs(_lib.ptr(cols[k * B:]), _lib.ptr(self._slot[k]), _lib.ptr(self._tgt_stored[k]), B, N, n,
                                                _lib.ptr(e._assign_map), _lib.stream()), "reart_assign_pairs")

        key = tuple(e._pc_trans.data_ptr() for e in self.engines) + tuple(e._assign_map.data_ptr() for e in self.engines)
        self._inplace.begin(self._src_pts, self.tgt_pts, st, stats=bool(self.collect_stats), before=gather, after=pairs, key=key)
        # the refresh's own graph (lap.ReplayedLaunches) is captured here -- or, under a work_guard, by refresh() once the guard
        # is left: a capture is the gate's writer
        fb, raw, changed = self._inplace.finish(capture=self.work_guard is None)
        if changed:                                                       # the host rewrote columns (a tie, a host solve): the maps again
            pairs()
        if raw is not None:
            self.stats_raw.append(raw)
            self._log_stats(lap.unpack_chain_stats(raw, st))
        return fb

    def _log_stats(self, st):
        from reart_amd.utils import lap

        search, reduction, _ = lap.stats_fields(st)
        back = np.asarray(self.lap_state.get("backward_rounds", np.zeros(len(st), np.int64)), dtype=np.int64)
        self.stats_log.append((int((search + back).max()), float(search.mean()), float(reduction.mean()), int(search.max()), float(back.mean())))

    def _device_path(self):
        from reart_amd.utils import lap

        lam32 = ctypes.c_float(self.lam).value
        return (self.NATIVE and all(e.cfg.use_assign and e.cfg.lambda_assign == lam32 for e in self.engines)
                and lap.InPlaceResolve.usable(self.lap_state, len(self.engines) * self.B, self.n))

    def refresh(self):
        """New pairs for every engine -> True when that changed the engines' loss mode (their graphs were dropped)."""
        if self.work_guard is None:
            return self._refresh()
        with self.work_guard():
            first = self._refresh()
        if self._inplace is not None:           # the capture a finish(capture=False) left due: OUTSIDE the guard's reader section
            self._inplace.capture()
        return first

    def _refresh(self):
        from reart_amd.utils import lap

        B, n = self.B, self.n
        for e in self.engines:
            e.peek_forward()
        if self._device_path():
            if self._slot is None:
                self._native_tables()
            with lap.EventPair(self.events):
                fb = self._refresh_on_device()
            first = False
        else:
            src_pts = _cat([index_points(e.pc_trans, s.src_idx.expand(B, n)) for e, s in zip(self.engines, self.parts)]).contiguous()
            with lap.EventPair(self.events):
                if self.collect_stats:
                    cols, fb, st = lap.linear_sum_assignment_points(src_pts, self.tgt_pts, self.lap_state, device_cols=True, return_stats="full")
                    self._log_stats(st)
                else:
                    cols, fb = lap.linear_sum_assignment_points(src_pts, self.tgt_pts, self.lap_state, device_cols=True)
            first = not self.engines[0].cfg.use_assign
            for k, (e, s) in enumerate(zip(self.engines, self.parts)):
                e.set_assignment(s.src_idx, s.tgt_idx.gather(1, cols[k * B:(k + 1) * B]), self.lam)
            self._have = True
        self.fallbacks += fb
        self.refreshes += 1
        return first

    def run(self, i, n_iter, snapshot_gap=0, on_snapshot=None):
        """Iterations i .. n_iter-1 -> n_iter.  ``on_snapshot(k)`` after iteration k-1 whenever k % snapshot_gap == 0 or k == n_iter."""
        while i < n_iter:
            if not self._have or i % self.gap == 0:
                if self.refresh() and n_iter - i > 1 and self.gap > 1:
                    # the engines' mode changed (their graph was dropped): one eager iteration, then a graph of the iterations
                    # between two refreshes
                    with (self.capture_guard() if self.capture_guard else contextlib.nullcontext()):
                        i += self.stepper.capture(steps_per_graph=self.gap - 1)
                    # the capture's eager iteration has moved i: a refresh or a snapshot may be due right here
                    # (assign_iter % assign_gap == assign_gap - 1: run_robot.py:165 refreshes at every i % gap == 0)
                    if on_snapshot is not None and (i == n_iter or (snapshot_gap and i % snapshot_gap == 0)):
                        on_snapshot(i)
                    continue
            nxt = (i // self.gap + 1) * self.gap                                       # next refresh
            snap = (i // snapshot_gap + 1) * snapshot_gap if snapshot_gap else n_iter
            chunk = max(1, min(nxt, snap, n_iter) - i)
            self.stepper.step(chunk)
            i += chunk
            if on_snapshot is not None and (i == n_iter or (snapshot_gap and i % snapshot_gap == 0)):
                on_snapshot(i)
        return i

    def report(self):
        out = {"assign_refreshes": self.refreshes, "lap_fallbacks": self.fallbacks}
        if self.events:
            torch.cuda.synchronize()
            ms = [a.elapsed_time(b) for a, b in self.events]
            out.update(ms_per_solve=sum(ms[1:]) / max(len(ms) - 1, 1), first_solve_ms=ms[0])
        return out


class AssignmentPhaseBatch(AssignmentPhase):
    """``AssignmentPhase`` for the K instances of one shape that step in shared launches (``RelaxBatch``; the sweep over
    canonical frames): the batch is the stepper, the iterations between refreshes replay one graph for all instances.
    Nothing but the constructor differs."""

    def __init__(self, batch, clouds, downsample, assign_gap, lambda_assign):
        """clouds: [(cano_pc, pc_list)] per engine of ``batch``, in the caller's point order."""
        self._setup(batch, batch.engines, clouds, downsample, assign_gap, lambda_assign)


class OperatorLoop:
    """The reference's loop body (run_robot.py:154-221) over the HIP operators with PyTorch autograd and
    ``torch.optim.Adam``: the path of ``--model kinematic`` (and of a base model outside the fused engine).
    ``iteration(i)`` runs iteration i -- forward, assignment (re-solved on the GPU every ``assign_gap`` iterations) or
    Chamfer loss, optional flow loss, backward, Adam -- and returns the loss dictionary of tensors (no host sync)."""

    def __init__(self, args, model, cano_pc, pc_list, pc_ref_list=None, flow_ref_list=None, tau_func=None):
        self.args, self.model, self.cano_pc, self.pc_list = args, model, cano_pc, pc_list
        self.pc_ref_list, self.flow_ref_list, self.tau_func = pc_ref_list, flow_ref_list, tau_func
        # --fused_adam: the same optimiser with its step as one launch (reart_amd.optim.Adam; same groups, options and state)
        Adam = torch.optim.Adam
        if getattr(args, "fused_adam", False):
            from reart_amd.optim import Adam
        if args.model == "base":
            seg_params = [p for p in model.seg_head.parameters() if p.requires_grad]
            self.optimizer = Adam([{"params": [model.proposal_6d, model.proposal_t], "lr": args.trans_lr},
                                   {"params": seg_params, "lr": args.seg_lr}], lr=1e-3, weight_decay=args.weight_decay)
        else:
            self.optimizer = Adam([p for p in model.parameters() if p.requires_grad], lr=args.trans_lr,
                                  weight_decay=args.weight_decay)
        # --fused_losses: the Chamfer term as one warm-started call with a fused backward (utils.chamfer.ChamferLoss), the
        # T - 1 blends of the flow term as one call (flow_utils.blend_anchor_motion_batch, bit for bit the per-frame calls).
        # --fused_flow: the whole flow term -- cat, blends, cat, subtraction, flow_loss, lambda_flow -- as one warm-started
        # call (flow_utils.FlowTerm: the same gradient bit for bit); ``flow_term = None`` after construction puts the
        # expressions back (what the tests compare FlowTerm with)
        self.fused_losses = bool(getattr(args, "fused_losses", False))
        self.chamfer_dist = ChamferLoss() if self.fused_losses else ChamferDistance()
        self.knn_flow = KNN(k=3, transpose_mode=True)
        self.ref_batch = self.flow_term = None
        if self.fused_losses and args.use_flow_loss and pc_ref_list is not None:
            self.ref_batch = pad_reference_sets(pc_ref_list, flow_ref_list)
        if getattr(args, "fused_flow", False) and args.use_flow_loss and pc_ref_list is not None:
            self.flow_term = FlowTerm(pc_ref_list, flow_ref_list, args.cano_idx, weight=args.lambda_flow,
                                      robust=args.use_robust_loss)
        self.matched = None
        # the kinematic model moves the cost matrices smoothly: the previous solve's pairs and potentials start the next
        # (shortest augmenting paths, reart_lap_resolve); the base model's resampled labels make them jump: cold solves
        self.lap_state = {} if args.model == "kinematic" else None
        self.lap_solves = self.lap_fallbacks = 0
        self.lap_events = None      # set to [] to collect a (start, end) torch.cuda.Event pair around every re-solve
        if args.use_assign_loss:
            # run_robot.py:167-169: both FPS calls sample fixed clouds (start 0 on the reference's CUDA path): once.  The columns
            # stay in FPS order: this loop only gathers the matched points, and its potentials and ties are pinned to that order
            from reart_amd.utils.lap import AssignmentSample

            sample = AssignmentSample(cano_pc, pc_list, args.downsample, z_order=False)
            self.src_idx = sample.src_idx.expand(pc_list.shape[0], sample.n)
            self.tgt_idx, self.tgt_order, self.tgt_pts = sample.tgt_idx, sample.tgt_order, sample.tgt_pts

    def iteration(self, i):
        from reart_amd.utils.lap import EventPair, cdist, linear_sum_assignment_batch, linear_sum_assignment_points

        args, model, cano_pc, pc_list = self.args, self.model, self.cano_pc, self.pc_list
        kwargs = {"tau": self.tau_func(cur_iter=i + 1)} if args.model == "base" else {}
        pc_trans_list, seg_part, trans_list = model(cano_pc, **kwargs)
        losses, loss = {}, 0
        if args.use_assign_loss and i >= args.assign_iter:
            pc_src = index_points(pc_trans_list, self.src_idx)
            if self.matched is None or i % args.assign_gap == 0:  # run_robot.py:165-178
                # certified optimum on the GPU; an uncertified matrix falls back to scipy on the host, so this is
                # always the assignment the reference's linear_sum_assignment / parallel_lap returns
                timer = EventPair(self.lap_events).start()
                if self.lap_state is not None:      # slowly moving problems: re-solve from the previous optimum
                    cols, fb, self.lap_stats = linear_sum_assignment_points(pc_src.detach(), self.tgt_pts, self.lap_state,
                                                                            return_stats="full", device_cols=True)
                else:
                    from reart_amd.utils import lap as lap_

                    st_ = {} if lap_.CANONICAL_TIES else None      # --deterministic: the potentials the tie check needs
                    assign, fb = linear_sum_assignment_batch(cdist(pc_src.detach(), self.tgt_pts), points=(pc_src.detach(), self.tgt_pts),
                                                             race=True, return_stats=True, state=st_, warm_assignment=st_ is not None)
                    if st_ is not None and lap_.canonicalize(pc_src.detach().contiguous(), self.tgt_pts.contiguous(), st_):
                        rows_ = np.arange(pc_src.shape[1], dtype=np.int64)
                        assign = [(rows_, c_) for c_ in st_["cols"].cpu().numpy().astype(np.int64)]
                timer.end()
                self.lap_solves += 1
                self.lap_fallbacks += fb
                if self.lap_state is None:
                    cols = torch.from_numpy(np.stack([c for _, c in assign])).to(cano_pc.device)    # rows are 0..n-1 in order
                self.matched = self.tgt_pts.gather(1, cols[..., None].expand(-1, -1, 3))
            ass = args.lambda_assign * ((pc_src - self.matched) ** 2).sum(-1).sum()
            losses["opt assignment loss"] = ass
            loss = loss + ass
            if getattr(args, "recon_with_assign", False):   # run_real.py:175-203: the Chamfer loss in every iteration
                rec = recon_loss(pc_trans_list, pc_list, self.chamfer_dist)
                losses["recon Loss"] = rec
                loss = loss + rec
        else:
            rec = recon_loss(pc_trans_list, pc_list, self.chamfer_dist)
            losses["recon Loss"] = rec
            loss = loss + rec
        if args.use_flow_loss and self.flow_term is not None:
            fl = self.flow_term(pc_trans_list, cano_pc)
            losses["flow Loss"] = fl
            loss = loss + fl
        elif args.use_flow_loss:
            c = args.cano_idx
            with torch.no_grad():
                comp = torch.cat((pc_trans_list[:c], cano_pc[None], pc_trans_list[c:]), dim=0)
                if self.ref_batch is not None:
                    gt_flow, gt_mask = blend_anchor_motion_batch(comp[:-1], *self.ref_batch, self.knn_flow, return_mask=True)
                else:
                    blended = [blend_anchor_motion(q, r, f, self.knn_flow, return_mask=True)
                               for q, r, f in zip(comp[:-1], self.pc_ref_list, self.flow_ref_list)]
                    gt_flow, gt_mask = torch.stack([b[0] for b in blended]), torch.stack([b[1] for b in blended])
            comp = torch.cat((pc_trans_list[:c], cano_pc[None], pc_trans_list[c:]), dim=0)
            fl = args.lambda_flow * flow_loss(gt_flow, comp[1:] - comp[:-1], flow_mask_list=gt_mask,
                                              robust=args.use_robust_loss)
            losses["flow Loss"] = fl
            loss = loss + fl
        losses["total Loss"] = loss
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        return losses


def make_projection_loop(args, model, cano_pc, pc_list, pc_ref_list=None, flow_ref_list=None, tau_func=None):
    """The loop object for phase 2: the autograd-free ``KinematicEngine`` for every ``--model kinematic`` run -- the projection
    as the reference's README runs it (``--use_assign_loss --assign_iter 0``), its Chamfer branch (iterations before
    ``assign_iter``, runs without ``--use_assign_loss``), mixed joint types and root motion (the SAPIEN / real-scan variant of
    the model, networks/model.py:113-166); the base model outside the fused engine goes through ``OperatorLoop`` (PyTorch
    autograd + torch.optim.Adam over the same operators), which also remains the engine's reference in the tests.
    ``--recon_with_assign`` (Chamfer and assignment loss together) goes through ``OperatorLoop`` too, unless ``--fused_recon``
    asks for the engine's ``recon_with_assign`` mode."""
    # --recon_with_assign alone: the operator loop computes that objective (the routing tests/test_relax_both_gpu.py pins);
    # with --fused_recon the engine does, in its recon_with_assign mode (the warm Chamfer term + reart_kin_post_recon)
    both = bool(getattr(args, "recon_with_assign", False))
    fused_recon = bool(getattr(args, "fused_recon", False))
    if fused_recon and not (both and args.model == "kinematic"):
        raise ValueError("--fused_recon is the kinematic engine's form of --recon_with_assign: it needs --model kinematic "
                         "--recon_with_assign")
    if args.model == "kinematic" and (not both or fused_recon):
        from reart_amd.kinematic_engine import KinematicEngine

        mode = {"recon_with_assign": True} if fused_recon else {}
        return KinematicEngine(model, cano_pc, pc_list, args.cano_idx, pc_ref_list if args.use_flow_loss else None,
                               flow_ref_list if args.use_flow_loss else None, trans_lr=args.trans_lr,
                               weight_decay=args.weight_decay, assign_iter=args.assign_iter, assign_gap=args.assign_gap,
                               downsample=args.downsample, lambda_assign=args.lambda_assign, lambda_flow=args.lambda_flow,
                               use_robust_loss=args.use_robust_loss, use_assign_loss=args.use_assign_loss,
                               warm_flow=bool(getattr(args, "fused_flow", False)), **mode)
    return OperatorLoop(args, model, cano_pc, pc_list, pc_ref_list, flow_ref_list, tau_func)


class SnapshotPrinter:
    """What the reference prints at ``i % snapshot_gap == 0`` and at the last iteration (run_robot.py:224-266): the loss line
    (the reference prints it every iteration, :216; here with the snapshot -- the fused loop does not meet the host in between)
    and, when the sample carries ground truth, `Flow eval: EPE | Acc 5 | Acc 10 | Angle`, `Seg eval: RI`, `Recon eval: recon`
    with the reference's formats and centimetre scaling.  The metrics are taken on a forward of the model as it stands after
    iteration i (the reference uses the forward iteration i itself ran: one Adam step and one noise draw earlier).
    ``lines`` keeps the metrics of every snapshot; ``out``: where the lines go (default stdout)."""

    GRAPH = os.environ.get("REART_SNAPSHOT_GRAPH", "1") != "0"

    def __init__(self, args, model, cano_pc, pc_list, sample=None, tau_func=None, out=None, graph=None):
        self.args, self.model, self.cano_pc, self.pc_list, self.sample = args, model, cano_pc, pc_list, sample
        self.tau_func, self.out = tau_func, out
        self.count, self.lines = 0, []
        # the metrics are ~80 small launches (elementwise / reductions / one matrix product): from the third snapshot on they are
        # ONE replay of a captured graph on copies of (seg_part, trans_list) -- README.md:125 prints 1 501 snapshots per run
        self.graph = self.GRAPH if graph is None else bool(graph)
        self._g = self._g_in = self._g_out = self._g_names = None
        # the ground truth the metrics compare with, on the device once (tail.snapshot_metrics would upload it at every snapshot)
        if sample is not None:
            keys = ("gt_flow_list", "gt_cano_part", "complete_gt_pc_list")
            self.sample = {k: torch.as_tensor(sample[k]).to(cano_pc.device) for k in keys if k in sample}

    def state(self, i):
        with torch.no_grad():
            if self.args.model == "base":
                _, seg_part, trans_list = self.model(self.cano_pc, tau=self.tau_func(cur_iter=i + 1))
            else:
                _, seg_part, trans_list = self.model(self.cano_pc)
        return seg_part, trans_list.detach()

    def __call__(self, i, losses):
        from reart_amd import tail

        import sys
        out = self.out if self.out is not None else sys.stdout
        if losses:
            print(f"iteration: {i} | " + " | ".join(f"{k}: {float(v.detach() if torch.is_tensor(v) else v):.3f}" for k, v in losses.items()),
                  file=out)
        seg_part, trans_list = self.state(i)
        has_gt = self.sample is not None and any(k in self.sample for k in ("gt_flow_list", "gt_cano_part", "complete_gt_pc_list"))
        m = self._metrics(seg_part, trans_list) if has_gt else {}
        if "epe" in m:
            print(f"Flow eval: EPE: {m['epe']:.3f} | Acc 5: {m['acc5']:.3f} | Acc 10: {m['acc10']:.3f} | Angle: {m['angle']:.3f}", file=out)
        if "ri" in m:
            print(f"Seg eval: RI: {m['ri']:.3f}", file=out)
        if "recon_err" in m:
            print(f"Recon eval: recon: {m['recon_err']:.3f}", file=out)
        self.count += 1
        self.lines.append((i, m))
        return m

    def _metrics(self, seg_part, trans_list):
        from reart_amd import tail

        c = self.args.cano_idx
        if not self.graph or self.count < 2:
            return tail.snapshot_metrics(self.cano_pc, self.pc_list, seg_part, trans_list, c, self.sample, chamfer=False)
        if self._g is None:
            try:
                self._g_in = (seg_part.clone(), trans_list.clone())
                g = torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                with torch.cuda.graph(g):
                    self._g_names, self._g_out = tail.snapshot_values(self.cano_pc, self._g_in[0], self._g_in[1], c, self.sample)
                self._g = g
            except Exception:           # a capture the runtime refuses: the eager form from here on
                self.graph, self._g = False, None
                torch.cuda.synchronize()
                return tail.snapshot_metrics(self.cano_pc, self.pc_list, seg_part, trans_list, c, self.sample, chamfer=False)
        if seg_part.shape != self._g_in[0].shape or trans_list.shape != self._g_in[1].shape:
            return tail.snapshot_metrics(self.cano_pc, self.pc_list, seg_part, trans_list, c, self.sample, chamfer=False)
        self._g_in[0].copy_(seg_part)
        self._g_in[1].copy_(trans_list)
        self._g.replay()
        return tail.snapshot_scaled(self._g_names, self._g_out.cpu().tolist()) if self._g_out is not None else {}


def build_kinematic_from_base(result, cano_pc, pc_list, args):
    """run_robot.py:101-124: KinematicModel from a base result (dict with pred_cano_part, pred_pose_list and, when the
    base run already extracted it, joint_connection)."""
    from reart_amd import tail

    device = cano_pc.device
    seg_part = torch.from_numpy(np.asarray(result["pred_cano_part"])).long().to(device)
    trans_list = torch.from_numpy(np.asarray(result["pred_pose_list"])).float().to(device)
    if "joint_connection" in result:
        joint_connection = torch.from_numpy(np.array(result["joint_connection"])).long().to(device)
    else:
        seg_part, trans_list, joint_connection = tail.extract_structure(
            seg_part, trans_list, cano_pc, merge_thr=args.merge_thr, cano_dist_thr=args.cano_dist_thr,
            lambda_joint=args.lambda_joint, min_num=0)
    new_seg, kin_kwargs = tail.kinematic_init(seg_part, trans_list, joint_connection)
    return KinematicModel(pose_len=pc_list.shape[0], seg_part=new_seg, cano_pc=cano_pc,
                          knn=KNN(k=1, transpose_mode=True), **kin_kwargs)


def project_from_base(args, sample, result, device, save_dir, dataset=None):
    """The projection of a base result onto a kinematic model (README.md:125, run_robot.py:101-124 + the loop + the end of the
    run), as ONE function for ``main`` (``--model kinematic --base_result_path``) and for the sweep's second stage: seeds,
    KinematicModel from ``result`` (the dict of a base run's result.pkl), ``args.n_iter`` iterations of the projection loop
    with the snapshots, ``finish`` (prints + result.pkl / model.pth.tar / result.txt under ``save_dir``).
    -> dict: the energy terms, cd_err, parts, joint_connection, assign_refreshes, lap_fallbacks, iterations, model."""
    torch.cuda.manual_seed_all(args.manual_seed)
    torch.manual_seed(args.manual_seed)
    np.random.seed(args.manual_seed)
    random.seed(args.manual_seed)
    from reart_amd.utils import lap as _lap

    _lap.CANONICAL_TIES = bool(getattr(args, "deterministic", True))
    assert args.cano_idx == result["cano_idx"]
    cano_pc = torch.from_numpy(sample["cano_pc"]).float().to(device)
    pc_list = torch.from_numpy(sample["pc_list"]).float().to(device)
    os.makedirs(save_dir, exist_ok=True)
    pc_ref_list = flow_ref_list = None
    if args.use_flow_loss:
        pc_ref_list, flow_ref_list = flow_references(args, sample, device, args.seq_path)
    tau_func = functools.partial(tau_cosine, max_iter=args.n_iter, end_temp=args.end_tau, start_temp=args.start_tau)
    model = build_kinematic_from_base(result, cano_pc, pc_list, args)
    model.to(device)
    snapshot = SnapshotPrinter(args, model, cano_pc, pc_list, None if args.synthetic and "gt_flow_list" not in sample else sample, tau_func)
    n_iter = args.n_iter
    loop = make_projection_loop(args, model, cano_pc, pc_list, pc_ref_list, flow_ref_list, tau_func)
    i = 0
    while i < n_iter:
        losses = loop.iteration(i)
        if i % args.snapshot_gap == 0 or i == n_iter - 1:
            snapshot(i, losses)
        i += 1
    lap_report = None       # assignment problems solved in the loop / how many of them went to the host solver
    if args.use_assign_loss:
        lap_report = {"assign_refreshes": loop.lap_solves, "lap_fallbacks": loop.lap_fallbacks}
    out = finish(args, model, cano_pc, pc_list, sample, save_dir, tau_func(cur_iter=n_iter), dataset, lap_report)
    out.update(lap_report or {"assign_refreshes": 0, "lap_fallbacks": 0}, iterations=i, model=model)
    return out


def main(args):
    torch.cuda.manual_seed_all(args.manual_seed)
    torch.manual_seed(args.manual_seed)
    np.random.seed(args.manual_seed)
    random.seed(args.manual_seed)
    if not torch.cuda.is_available():
        raise SystemExit("reart_amd runs on an AMD GPU only (no CPU fallback)")
    from reart_amd.utils import lap as _lap

    _lap.CANONICAL_TIES = bool(getattr(args, "deterministic", True))
    if args.evaluate and args.resume is None:
        raise ValueError("need model path to evaluate!")      # run_robot.py:86-87
    device = torch.device("cuda")
    dataset = None
    if args.synthetic:
        sample = synthetic_sequence(args.num_points, args.cano_idx, args.synthetic_frames, args.use_flow_loss)
    else:
        from reart_amd.dataset import Sequence

        dataset = Sequence(args.seq_path, num_points=args.num_points, cano_idx=args.cano_idx)
        sample = dataset[0]
    cano_pc = torch.from_numpy(sample["cano_pc"]).float().to(device)
    pc_list = torch.from_numpy(sample["pc_list"]).float().to(device)
    # --synthetic never shares a directory with a real sequence (seq_path keeps its default then)
    save_dir = os.path.join(args.save_root, "synthetic" if args.synthetic
                            else (os.path.basename(args.seq_path.rstrip("/")) or "sequence"))
    os.makedirs(save_dir, exist_ok=True)

    if args.model == "kinematic" and args.resume is None:  # run_robot.py:101-124: joint tree from a base result
        assert args.base_result_path is not None, "--model kinematic needs --base_result_path or --resume"
        with open(args.base_result_path, "rb") as f:
            result = pickle.load(f)
        print(f"load base result from {args.base_result_path}")
        model = project_from_base(args, sample, result, device, save_dir, dataset)["model"]
        print("all done!")
        return model

    pc_ref_list = flow_ref_list = None
    if args.use_flow_loss:
        pc_ref_list, flow_ref_list = flow_references(args, sample, device, args.seq_path)

    tau_func = functools.partial(tau_cosine, max_iter=args.n_iter, end_temp=args.end_tau, start_temp=args.start_tau)
    fixed_tau = 0.0
    if args.model == "base":
        model = BaseModel(num_parts=args.num_parts, pose_len=pc_list.shape[0])
        if args.resume is not None:
            ckpt = torch.load(args.resume[0], map_location=device, weights_only=False)
            model.load_state_dict(ckpt["state_dict"], strict=False)
            fixed_tau = float(ckpt["tau"])  # the reference freezes tau on resume (:96-97)
            tau_func = lambda cur_iter: fixed_tau
            assert args.cano_idx == ckpt.get("cano_idx", args.cano_idx)
    else:
        ckpt = torch.load(args.resume[0], map_location=device, weights_only=False)      # (without --resume: project_from_base, above)
        model = KinematicModel(pose_len=pc_list.shape[0], seg_part=ckpt["seg_part"].to(device),
                               cano_pc=ckpt["cano_pc"].to(device), knn=KNN(k=1, transpose_mode=True),
                               edge_index=ckpt["edge_index"], paths_to_base=ckpt["paths_to_base"],
                               reverse_topo=ckpt["reverse_topo"])
        model.load_state_dict(ckpt["state_dict"], strict=True)
    model.to(device)
    chamfer_dist = ChamferDistance()
    knn_flow = KNN(k=3, transpose_mode=True)

    snapshot = SnapshotPrinter(args, model, cano_pc, pc_list, None if args.synthetic and "gt_flow_list" not in sample else sample, tau_func)

    n_iter = 1 if args.evaluate else args.n_iter
    i = 0
    lap_report = None       # assignment problems solved in the loop / how many of them went to the host solver
    # ---- phase 1: fused engine (base model, Chamfer [+ flow]) until the assignment loss takes over
    fused_until = n_iter if not args.use_assign_loss else min(args.assign_iter, n_iter)
    if args.model == "base" and not args.evaluate:
        eng = RelaxEngine(cano_pc, pc_list, model, args.cano_idx, pc_ref_list, flow_ref_list, n_iter=args.n_iter,
                          start_tau=args.start_tau, end_tau=args.end_tau, trans_lr=args.trans_lr, seg_lr=args.seg_lr,
                          lambda_flow=args.lambda_flow, use_robust_loss=args.use_robust_loss, fixed_tau=fixed_tau,
                          seed=args.manual_seed, weight_decay=args.weight_decay,
                          recon_with_assign=bool(getattr(args, "recon_with_assign", False)))
        if fused_until > 0:
            i += eng.capture()
        while i < fused_until:
            chunk = min(args.snapshot_gap, fused_until - i)
            eng.step(chunk)
            i += chunk
            row = eng.last_losses().cpu().numpy()
            snapshot(i - 1, {"recon Loss": row[0], "flow Loss": row[1], "total Loss": row[2]})
        # ---- phase 2 (base model): assignment loss on the same engine (run_robot.py:164-187)
        if i < n_iter and args.use_assign_loss:
            phase = AssignmentPhase(eng, cano_pc, pc_list, args.downsample, args.assign_gap, args.lambda_assign)

            def on_snapshot(k):
                row = eng.last_losses().cpu().numpy()
                if eng.cfg.recon_with_assign:     # row[0] holds both terms (RelaxEngine.loss_log)
                    ass = float(eng.last_assign_loss().cpu())
                    snapshot(k - 1, {"recon Loss": row[0] - ass, "opt assignment loss": ass, "flow Loss": row[1], "total Loss": row[2]})
                    return
                snapshot(k - 1, {"opt assignment loss": row[0], "flow Loss": row[1], "total Loss": row[2]})

            i = phase.run(i, n_iter, args.snapshot_gap, on_snapshot)
            lap_report = phase.report()
            print(f"assignment phase: {lap_report['assign_refreshes']} refreshes, {lap_report['lap_fallbacks']} host fallbacks")
    # ---- phase 2 (kinematic model; base model without the engine): the reference's loop with HIP operators
    if i < n_iter and not args.evaluate:
        loop = make_projection_loop(args, model, cano_pc, pc_list, pc_ref_list, flow_ref_list, tau_func)
        while i < n_iter:
            losses = loop.iteration(i)
            if i % args.snapshot_gap == 0 or i == n_iter - 1:
                snapshot(i, losses)
            i += 1
        if args.use_assign_loss:
            lap_report = {"assign_refreshes": loop.lap_solves, "lap_fallbacks": loop.lap_fallbacks}
    if args.evaluate:
        snapshot(0, {})
    finish(args, model, cano_pc, pc_list, sample, save_dir, tau_func(cur_iter=n_iter), dataset, lap_report)
    print("all done!")
    return model


def finish(args, model, cano_pc, pc_list, sample, save_dir, tau, dataset=None, lap_report=None):
    """run_robot.py:227-356: structure, energies, result files (the reference's file names and keys).
    -> dict of what was printed: parts, joint_connection, cd_err and (not under --evaluate) the energy terms."""
    from reart_amd import tail
    from reart_amd.utils.kinematic_utils import edge_index2edges
    from reart_amd.utils.model_utils import compute_pc_transform

    device = cano_pc.device
    with torch.no_grad():
        _, seg_part, trans_list = model(cano_pc)
    trans_list = trans_list.detach()
    if isinstance(model, KinematicModel):   # the tree is the model's own (run_robot.py:235-237)
        from reart_amd.utils.graph_utils import denoise_seg_label

        seg_part = denoise_seg_label(seg_part.clone(), cano_pc, KNN(k=1, transpose_mode=True), min_num=20)
        conn = torch.tensor(edge_index2edges(model.edge_index), dtype=torch.long, device=device)
        from reart_amd.utils.kinematic_utils import extract_kinematic

        seg_part, trans_list, conn = extract_kinematic(seg_part, trans_list, conn)
    else:
        seg_part, trans_list, conn = tail.extract_structure(
            seg_part, trans_list, cano_pc, merge_thr=args.merge_thr, merge_it=args.merge_it,
            cano_dist_thr=args.cano_dist_thr, lambda_joint=args.lambda_joint)
    conn_list = conn.cpu().numpy().tolist()
    print("parts:", trans_list.shape[1], "| joint connection:", conn_list)
    metrics = tail.snapshot_metrics(cano_pc, pc_list, seg_part, trans_list, args.cano_idx, sample)
    if "epe" in metrics:
        print(f"Flow eval: EPE: {metrics['epe']:.3f} | Acc 5: {metrics['acc5']:.3f} | Acc 10: {metrics['acc10']:.3f} | "
              f"Angle: {metrics['angle']:.3f}")
    if "ri" in metrics:
        print(f"Seg eval: RI: {metrics['ri']:.3f}")
    if "recon_err" in metrics:
        print(f"Recon eval: recon: {metrics['recon_err']:.3f}")
    report = {"parts": int(trans_list.shape[1]), "joint_connection": conn_list,
              "cd_err": float(metrics["cd_err"]) if "cd_err" in metrics else None}
    retarget_err = 9999      # run_robot.py:287-291: retargeting to the sequence's novel poses (kinematic model only)
    if isinstance(model, KinematicModel) and dataset is not None and len(dataset.novel_pose_list):
        from reart_amd.utils.kinematic_utils import ik

        retarget_err = ik(dataset, model, device, verbose=False, vis=False, fused=bool(getattr(args, "fused_ik", False)))
    print("Retarget error: {:.3f}".format(retarget_err))
    with open(os.path.join(save_dir, "result.txt"), "w") as f_result:
        f_result.write(f"retarget_err: {retarget_err:.3f}\n")
        for k in ("recon_err", "epe", "acc5", "acc10", "angle", "ri", "cd_err"):
            if k in metrics:
                f_result.write(f"{k}: {metrics[k]:.3f}\n")
        if not args.evaluate:
            energy = tail.energy_terms(cano_pc, pc_list, seg_part, trans_list, conn, args.cano_idx)
            report.update({k: float(energy[k]) for k in ("ass_err", "screw_err", "group_err", "total_err")})
            print(f"Energy eval: total: {energy['total_err']:.3f}")
            for k in ("ass_err", "screw_err", "group_err", "total_err"):
                print(f"{k}: {energy[k]:.3f}")
                f_result.write(f"{k}: {energy[k]:.3f}\n")
            print(f"cd_err: {metrics['cd_err']:.3f}")
        if lap_report is not None:      # additions: how many assignment problems of the loop went to the host solver (0 = none)
            for k in ("assign_refreshes", "lap_fallbacks"):
                f_result.write(f"{k}: {lap_report[k]}\n")
    if args.evaluate:
        return report
    save_dict = {"pred_cano_part": seg_part.cpu().numpy(), "pred_pose_list": trans_list.cpu().numpy(),
                 "cano_idx": args.cano_idx, "joint_connection": conn_list}
    save_dict.update(sample)
    with open(os.path.join(save_dir, "result.pkl"), "wb") as f:
        pickle.dump(save_dict, f)
    model_dict = {"state_dict": model.state_dict(), "tau": tau, "cano_idx": args.cano_idx}
    if isinstance(model, KinematicModel):
        model_dict.update(seg_part=model.seg_part, cano_pc=model.cano_pc, edge_index=model.edge_index,
                          paths_to_base=model.paths_to_base, reverse_topo=model.reverse_topo)
    torch.save(model_dict, os.path.join(save_dir, "model.pth.tar"))
    print("saved", os.path.join(save_dir, "result.pkl"), "and", os.path.join(save_dir, "model.pth.tar"))
    return report


def build_parser():
    p = argparse.ArgumentParser(description="Robot (reart_amd)")
    # same flags and defaults as the reference, run_robot.py:362-420
    p.add_argument("--manual_seed", default=2, type=int)
    p.add_argument("--resume", type=str, nargs="+", metavar="PATH")
    p.add_argument("--evaluate", dest="evaluate", action="store_true")
    p.add_argument("--snapshot_gap", default=100, type=int)
    p.add_argument("--use_cuda", default=1, type=int)
    p.add_argument("--cano_idx", default=0, type=int)
    p.add_argument("--num_points", default=4096, type=int)
    p.add_argument("--seq_path", default="data/robot/nao", type=str)
    p.add_argument("--normalize_file", default="data/category_normalize_scale.pkl", type=str)
    p.add_argument("--start_tau", default=5, type=float)
    p.add_argument("--end_tau", default=1, type=float)
    p.add_argument("--seg_lr", default=1e-3, type=float)
    p.add_argument("--trans_lr", default=1e-2, type=float)
    p.add_argument("--weight_decay", default=0, type=float)
    p.add_argument("--n_iter", default=15000, type=int)
    p.add_argument("--assign_iter", default=5000, type=int)
    p.add_argument("--num_parts", default=20, type=int)
    p.add_argument("--model", default="base", type=str, choices=["base", "kinematic"])
    p.add_argument("--base_result_path", default=None, type=str)
    p.add_argument("--corr_model_path", default="pretrained/corr_model.pth.tar")
    p.add_argument("--use_flow_loss", action="store_true")
    p.add_argument("--use_robust_loss", action="store_true")
    p.add_argument("--use_assign_loss", action="store_true")
    p.add_argument("--use_nproc", action="store_true")
    p.add_argument("--downsample", default=4, type=int)
    p.add_argument("--assign_gap", default=5, type=int)
    p.add_argument("--lambda_assign", default=3e-1, type=float)
    p.add_argument("--lambda_flow", default=1, type=float)
    p.add_argument("--lambda_joint", default=100, type=float)
    p.add_argument("--cano_dist_thr", default=1e-2, type=float)
    p.add_argument("--merge_thr", default=3e-2, type=float)
    p.add_argument("--merge_it", default=2, type=int)
    p.add_argument("--save_root", default="exp", type=str)
    # additions
    p.add_argument("--synthetic", action="store_true", help="generated articulated sequence instead of --seq_path")
    p.add_argument("--synthetic_frames", default=20, type=int)
    p.add_argument("--deterministic", dest="deterministic", action="store_true", default=True,
                   help="(default) the assignment refreshes return a function of the cost matrix alone, like the reference's scipy "
                        "call (run_robot.py:172-176): when several assignments are optimal the raced GPU solvers return whichever "
                        "finished first, so every solve is checked for ties (reart_lap_ties) and a tied problem takes the "
                        "lexicographically smallest optimum -- two runs under one --manual_seed are the same run (run_robot.py:37-49)")
    p.add_argument("--no_deterministic", dest="deterministic", action="store_false",
                   help="skip the tie check (about 2 %% of a projection iteration): tied optima are settled by whichever racer wins")
    p.add_argument("--fused_ik", action="store_true",
                   help="retarget error of a kinematic model: fit all novel poses in one launch (kinematic_utils.ik_batch) instead of "
                        "one Adam loop per pose; same optimum, not bit-equal to the default")
    p.add_argument("--recon_with_assign", action="store_true",
                   help="with --use_assign_loss: from --assign_iter on the assignment loss is ADDED to the Chamfer loss instead of "
                        "taking its place, as the reference's run_real.py:175 and run_sapien.py:174 do (recon Loss in every "
                        "iteration); the fused engine runs both in its Chamfer consumer, --model kinematic goes through the "
                        "operator loop unless --fused_recon is given")
    p.add_argument("--fused_recon", action="store_true",
                   help="with --model kinematic --recon_with_assign: the autograd-free kinematic engine computes that objective "
                        "(KinematicEngine(recon_with_assign=True): the Chamfer term as one warm-started call in front of the re-solve, "
                        "its gradient, the pairs' term and the flow term added in one launch) instead of the operator loop; "
                        "anything else with this flag is an error")
    p.add_argument("--fused_losses", action="store_true",
                   help="operator loop (the base model outside the fused engine): the Chamfer term as one warm-started call with a "
                        "fused backward, the T-1 flow blends as one call; same losses up to the summation order of the Chamfer sum")
    p.add_argument("--fused_flow", action="store_true",
                   help="the flow term (blends, flow loss and its gradient) as one warm-started call over references prepared once "
                        "(flow_utils.FlowTerm): in the operator loop, and in the kinematic engine (warm_flow); the same gradients bit "
                        "for bit, the loss as one double sum")
    p.add_argument("--fused_adam", action="store_true",
                   help="operator loop: reart_amd.optim.Adam in place of torch.optim.Adam -- the same groups, options and state, "
                        "every parameter stepped in one launch; the same formula in float32, rounded as torch's multi-tensor kernels round it")
    return p


if __name__ == "__main__":
    a = build_parser().parse_args()
    os.makedirs(a.save_root, exist_ok=True)
    main(a)
