"""The fused step with the Chamfer loss AND the assignment loss in one iteration (reart_relax_config.recon_with_assign,
``RelaxEngine(recon_with_assign=True)``; the objective of the reference's run_real.py:175-203 and run_sapien.py:174-203):
against the restated oracle iteration (tests/relax_both_ref.py), against the pure modes bit for bit where the term is
absent, replayed from a graph, in shared launches, through ``AssignmentPhase`` and in the host loop.

Tolerances are those of tests/test_step_gpu.py::test_assignment_loss_step_matches_oracle for the two pure modes: loss terms
1e-5 relative, pc_trans 5e-7, parameters 2e-5 per iteration."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import relax_both_ref as R

pytestmark = pytest.mark.gpu
LAM = 0.3
PARAMS = ("p6d", "pt", "W2", "W1", "b1")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _model(dev, pb):
    from reart_amd.networks.model import BaseModel

    m = BaseModel(num_parts=pb["P"], pose_len=pb["B"]).to(dev)
    with torch.no_grad():
        m.seg_head.model[0].weight.copy_(t(pb["W1"], dev)[:, :, None])
        m.seg_head.model[0].bias.copy_(t(pb["b1"], dev))
        m.seg_head.model[2].weight.copy_(t(pb["W2"], dev)[:, :, None])
        m.proposal_6d.copy_(t(pb["p6d"], dev))
        m.proposal_t.copy_(t(pb["pt"], dev))
    return m


def _params(model):
    return dict(zip(PARAMS, (model.proposal_6d, model.proposal_t, model.seg_head.model[2].weight,
                             model.seg_head.model[0].weight, model.seg_head.model[0].bias)))


def _close(got, want, what):
    assert abs(got - want) <= 1e-5 * abs(want) + 1e-9, (what, got, want)


def _pair_sum(eng, pcs, src, tgt, lam):
    """lambda * sum |pc_trans[b, src] - pc_list[b, tgt[b]]|^2 in float64, from the engine's last forward."""
    x = eng.pc_trans.cpu().numpy().astype(np.float64)
    y = np.asarray(pcs, np.float64)
    return float(lam) * sum(float(((x[b, src] - y[b, tgt[b]]) ** 2).sum()) for b in range(y.shape[0]))


# name: N, flow, spatial_sort, use_grid, tuning, the consumer the launcher selects.  The brute-force path takes its slice
# count from the cloud (knn_pick_split: one slice up to 254 points, two up to 508, eight from 1021), so its three forms
# SL = 1 / 4 / 0 are three cloud sizes with tuning search_mode = 1, the switch of
# test_step_gpu.py::test_search_variants_give_identical_trajectories; N = 1100 is also two consumer workgroups per frame
# (CG_RANGE = 1024), the second with 76 live threads.
FORMS = {
    "merged": (260, True, True, False, {}),                            # post_kernel, single record
    "standalone": (260, False, True, False, {}),                       # chamfer_grad_kernel<1>
    "unsorted_flow": (260, True, False, False, {}),                    # use_boxes = 0: brute force, two slices (SL = 4)
    "unsorted": (260, False, False, False, {}),
    "grid": (260, True, True, True, {}),                               # x -> y through the grid (one record), y -> x two slices
    "brute_sl1": (200, True, True, False, {"search_mode": 1}),
    "brute_sl4": (260, True, True, False, {"search_mode": 1}),
    "brute_sl0": (1100, True, True, False, {"search_mode": 1}),
    "merged_two_workgroups": (1100, True, True, False, {}),
    "unsorted_two_workgroups": (1100, False, False, False, {}),
}


def _draw_pairs(rng, N, B, n=64):
    """n pairs per frame; beyond one consumer workgroup, sources and targets on both sides of index 1024 (and the ends)."""
    src = rng.permutation(N)[:n]
    tgt = np.stack([rng.permutation(N)[:n] for _ in range(B)])
    if N > 1024:
        edge = np.array([0, 1023, 1024, N - 1])
        src = np.concatenate([edge, np.setdiff1d(src, edge, assume_unique=True)[: n - 4]])
        for b in range(B):
            tgt[b] = np.concatenate([np.roll(edge, b + 1), np.setdiff1d(tgt[b], edge, assume_unique=True)[: n - 4]])
        assert (src < 1024).any() and (src >= 1024).any() and (tgt < 1024).any() and (tgt >= 1024).any()
    return src, tgt


@pytest.mark.parametrize("form", list(FORMS))
def test_combined_step_matches_the_restated_oracle(oracle, dev, form):
    """Two Chamfer iterations, then three with both losses, the 64 pairs redrawn before iterations 2 and 4: row[0] against
    recon + ass, last_assign_loss() against ass and against the float64 sum over the pairs, row[1], row[2], seg_part,
    pc_trans and the five parameter tensors after every iteration."""
    from oracle.step import RelaxOracle
    from reart_amd.relax import RelaxEngine

    N, flow, sort, grid, tuning = FORMS[form]
    pb = R.problem(N=N)
    rng, P, B = pb["rng"], pb["P"], pb["B"]
    refs, flows = (pb["refs"], pb["flows"]) if flow else (None, None)
    orc = RelaxOracle(pb["cano"], pb["pcs"], pb["W1"], pb["b1"], pb["W2"], pb["p6d"], pb["pt"], 2, refs, flows,
                      lambda_flow=0.7, n_iter=50)
    model = _model(dev, pb)
    eng = RelaxEngine(t(pb["cano"], dev), t(pb["pcs"], dev), model, 2, None if refs is None else [t(r, dev) for r in refs],
                      None if flows is None else [t(f, dev) for f in flows], n_iter=50, lambda_flow=0.7, spatial_sort=sort,
                      use_grid=grid, tuning=tuning, recon_with_assign=True)
    assert eng.cfg.recon_with_assign == 1 and eng.cfg.use_assign == 0
    assign = None
    for i in range(5):
        noise = R.gumbel(rng, N, P)
        eng.set_gumbel(t(noise, dev))
        if i in (2, 4):
            src, tgt = _draw_pairs(rng, N, B)
            assign = (src, tgt, LAM)
            eng.set_assignment(torch.from_numpy(src), torch.from_numpy(tgt), LAM)
            assert eng.cfg.use_assign == 1
        ref = R.step_both(orc, noise, assign=assign)
        eng.step()
        row = eng.last_losses().cpu().numpy()
        ass = float(eng.last_assign_loss().cpu())
        print(form, i, "row", row.tolist(), "ass", ass, "ref", ref["recon"], ref["ass"], ref["flow"])
        _close(row[0], ref["recon"] + ref["ass"], (i, "row0"))
        _close(ass, ref["ass"], (i, "ass"))
        if assign is None:
            assert ass == 0.0
        else:
            _close(ass, _pair_sum(eng, pb["pcs"], assign[0], assign[1], LAM), (i, "pair sum"))
        _close(row[1], ref["flow"], (i, "row1"))
        _close(row[2], ref["recon"] + ref["ass"] + ref["flow"], (i, "row2"))
        assert abs(row[3] - ref["tau"]) < 1e-6
        np.testing.assert_array_equal(eng.seg_part.cpu().numpy(), ref["seg_part"])
        np.testing.assert_allclose(eng.pc_trans.cpu().numpy(), ref["pc_trans"], rtol=0, atol=5e-7)
        for k, prm in _params(model).items():
            got = prm.detach().cpu().numpy().reshape(orc.params[k].shape)
            np.testing.assert_allclose(got, orc.params[k], rtol=0, atol=2e-5, err_msg=f"iter {i} param {k}")
    _, alog = eng.assign_loss_log()
    assert alog.shape == (5,) and (alog[:2] == 0).all() and (alog[2:] > 0).all()


def _synthetic(dev, flow, cano_idx=2, pts=75, seed=5):
    from reart_amd.synthetic import make_sequence, split_canonical

    seq = make_sequence(T=6, n_parts=4, pts_per_part=pts, seed=seed, n_ref=200, with_flow=True)
    cano, pcs = split_canonical(seq["complete"], cano_idx)
    refs = ([t(r, dev) for r in seq["ref_loc"]], [t(f, dev) for f in seq["ref_flow"]]) if flow else (None, None)
    return t(cano, dev), t(pcs, dev), refs


def _engine(dev, clouds, cano_idx=2, both=True, seed=7, model_seed=0, P=12, **kw):
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine

    cano, pcs, refs = clouds
    torch.manual_seed(model_seed)
    model = BaseModel(num_parts=P, pose_len=pcs.shape[0]).to(dev)
    eng = RelaxEngine(cano, pcs, model, cano_idx, refs[0], refs[1], n_iter=200, seed=seed, recon_with_assign=both, **kw)
    return eng, model


def _state(eng, model):
    it, log = eng.loss_log()
    return [log.cpu().numpy(), eng.assign_loss_log()[1].cpu().numpy(), eng.pc_trans.cpu().numpy(), eng.seg_part.cpu().numpy()] + \
           [p.detach().cpu().numpy().copy() for p in _params(model).values()]


def _same_state(a, b, skip=()):
    for k, (x, y) in enumerate(zip(a, b)):
        if k not in skip:
            np.testing.assert_array_equal(x, y, err_msg=f"state {k}")


@pytest.mark.parametrize("flow", [True, False])
def test_the_term_is_exactly_additive_and_skippable(dev, flow):
    """Bit for bit the Chamfer-only engine: a combined engine whose map is all -1, one with pairs and lambda_assign = 0, and
    one whose unpaired points carry out-of-range entries (N, 2^30, -7) against -1; after clear_assignment() a combined engine
    continues like a Chamfer-only engine started from its state."""
    clouds = _synthetic(dev, flow)
    B, N = clouds[1].shape[:2]
    rng = np.random.default_rng(3)
    src, tgt = torch.from_numpy(rng.permutation(N)[:64]), torch.from_numpy(np.stack([rng.permutation(N)[:64] for _ in range(B)]))
    plain, m0 = _engine(dev, clouds, both=False)
    plain.step(3)
    want = _state(plain, m0)
    for name, lam in (("all -1", LAM), ("lambda 0", 0.0)):
        eng, m = _engine(dev, clouds)
        eng.set_assignment(src, tgt, lam)
        if name == "all -1":
            eng._assign_map.fill_(-1)
        assert eng.cfg.use_assign == 1 and eng.cfg.recon_with_assign == 1
        eng.step(3)
        _same_state(want, _state(eng, m))
        assert (eng.assign_loss_log()[1] == 0).all(), name
    # out-of-range entries read as -1
    runs = []
    for bad in (False, True):
        eng, m = _engine(dev, clouds)
        eng.set_assignment(src, tgt, LAM)
        if bad:
            free = (eng._assign_map < 0).nonzero()
            assert free.shape[0] >= 3 * B
            for k, v in enumerate((N, 2 ** 30, -7)):
                rows = free[k::3]
                eng._assign_map[rows[:, 0], rows[:, 1]] = v
            assert (eng._assign_map >= N).any() and (eng._assign_map == -7).any()
        eng.step(3)
        runs.append(_state(eng, m))
    _same_state(*runs)
    assert (runs[0][1] > 0).all() and not np.array_equal(runs[0][-5], want[-5])      # the pairs did something
    # clear_assignment: on as a Chamfer engine
    from reart_amd.relax import RelaxEngine

    eng, m = _engine(dev, clouds)
    eng.step(2)
    eng.set_assignment(src, tgt, LAM)
    eng.step(2)
    eng.clear_assignment()
    assert eng.cfg.use_assign == 0
    import copy

    m2 = copy.deepcopy(m)
    cano, pcs, refs = clouds
    twin = RelaxEngine(cano, pcs, m2, 2, refs[0], refs[1], n_iter=200, seed=7, start_iter=4)
    twin.adam_m.copy_(eng.adam_m)
    twin.adam_v.copy_(eng.adam_v)
    for _ in range(3):
        eng.step()
        twin.step()
        np.testing.assert_array_equal(eng.last_losses().cpu().numpy(), twin.last_losses().cpu().numpy())
        assert float(eng.last_assign_loss()) == 0.0
        np.testing.assert_array_equal(eng.pc_trans.cpu().numpy(), twin.pc_trans.cpu().numpy())
        for a, b in zip(_params(m).values(), _params(m2).values()):
            assert torch.equal(a, b)


def test_graph_replay_equals_eager_and_two_runs_agree(dev):
    """Both losses with flow, in-kernel Philox noise: four iterations eagerly, and twice with the iterations after the first
    replayed from a captured graph, in the form of test_step_gpu.py::test_graph_replay_equals_eager_and_is_deterministic."""
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine

    rng = np.random.default_rng(1)
    N, P, B = 1024, 20, 6
    cano = rng.uniform(-0.3, 0.3, (N, 3)).astype(np.float32)
    pcs = (cano[None] + rng.normal(0, 0.02, (B, N, 3))).astype(np.float32)
    refs = [rng.uniform(-0.3, 0.3, (700 + 10 * i, 3)).astype(np.float32) for i in range(B)]
    flows = [rng.normal(0, 0.02, r.shape).astype(np.float32) for r in refs]
    src, tgt = torch.from_numpy(rng.permutation(N)[:256]), torch.from_numpy(np.stack([rng.permutation(N)[:256] for _ in range(B)]))
    results = []
    for mode in ("eager", "graph", "graph"):
        torch.manual_seed(0)
        model = BaseModel(num_parts=P, pose_len=B).to(dev)
        eng = RelaxEngine(t(cano, dev), t(pcs, dev), model, 3, [t(r, dev) for r in refs], [t(f, dev) for f in flows],
                          n_iter=100, seed=5, recon_with_assign=True)
        eng.set_assignment(src, tgt, LAM)
        done = eng.capture() if mode == "graph" else 0
        eng.step(4 - done)
        assert eng.graph_replays == (3 if mode == "graph" else 0)
        it, log = eng.loss_log()
        assert it == 4
        results.append(_state(eng, model))
    for r in results[1:]:
        _same_state(results[0], r)
    assert np.isfinite(results[0][0]).all() and (results[0][1] > 0).all()


@pytest.mark.parametrize("flow", [True, False])
def test_shared_launches(dev, flow):
    """Three combined engines of one shape (N = 300) in one RelaxBatch, eager and replayed, end in the bits of their own
    runs; a batch that mixes a combined and a plain engine is refused."""
    from reart_amd.relax import RelaxBatch

    K = 3
    clouds = [_synthetic(dev, flow, cano_idx=k) for k in range(K)]
    N, B = clouds[0][0].shape[0], clouds[0][1].shape[0]
    assert N == 300
    rng = np.random.default_rng(7)
    pairs = [(torch.from_numpy(rng.permutation(N)[:64]), torch.from_numpy(np.stack([rng.permutation(N)[:64] for _ in range(B)])))
             for _ in range(K)]

    def build():
        out = [_engine(dev, clouds[k], cano_idx=k, seed=100 + k, model_seed=10 + k) for k in range(K)]
        for (e, _), (s_, t_) in zip(out, pairs):
            e.set_assignment(s_, t_, LAM)
        return out

    solo = build()
    for e, _ in solo:
        e.step(7)
    batched = build()
    batch = RelaxBatch([e for e, _ in batched])
    batch.step(2)                        # eager
    batch.capture(steps_per_graph=2)     # +1 (warm-up)
    batch.step(4)                        # 2 replays
    assert batch.graph_replays == 2
    torch.cuda.synchronize()
    for (e0, m0), (e1, m1) in zip(solo, batched):
        a = _state(e0, m0)
        assert np.isfinite(a[0]).all() and (a[1] > 0).all()
        _same_state(a, _state(e1, m1))
    with pytest.raises(RuntimeError):
        mixed = [_engine(dev, clouds[0], cano_idx=0)[0], _engine(dev, clouds[0], cano_idx=0, both=False)[0]]
        RelaxBatch(mixed).step()


def test_through_the_assignment_phase(dev):
    """AssignmentPhase from iteration 0 on a combined engine (N = 512, B = 3, downsample 4, assign_gap 5, 12 iterations: the
    mode switch, the captured graph between refreshes, the device-side refresh).  The Chamfer term is still there:
    row[0] - last_assign_loss() is the Chamfer distance both ways round of the last pc_trans, and last_assign_loss() is
    lambda * sum |.|^2 over the pairs of the engine's map."""
    from reart_amd.run_robot import AssignmentPhase
    from reart_amd.synthetic import make_sequence, split_canonical
    from reart_amd.utils.chamfer import ChamferDistance

    seq = make_sequence(T=4, n_parts=4, pts_per_part=128, seed=6, n_ref=200, with_flow=True)
    cano, pcs = split_canonical(seq["complete"], 1)
    cano, pcs = t(cano, dev), t(pcs, dev)
    assert tuple(pcs.shape) == (3, 512, 3)
    eng, model = _engine(dev, (cano, pcs, ([t(r, dev) for r in seq["ref_loc"]], [t(f, dev) for f in seq["ref_flow"]])), cano_idx=1)
    phase = AssignmentPhase(eng, cano, pcs, 4, 5, LAM)
    assert phase.run(0, 12) == 12
    assert phase.refreshes == 3 and phase.fallbacks == 0
    assert eng.graph_replays > 0
    for p in model.parameters():
        assert torch.isfinite(p).all()
    row = eng.last_losses().cpu().numpy().astype(np.float64)
    ass = float(eng.last_assign_loss().cpu())
    x = eng.pc_trans
    cd = float(ChamferDistance()(x, pcs, bidirectional=True).double().sum())
    print("row", row.tolist(), "ass", ass, "chamfer", cd)
    _close(row[0] - ass, cd, "chamfer term")
    # the pairs as the engine holds them (storage order) against its own stored clouds
    amap = eng._assign_map.long()
    assert int((amap >= 0).sum()) == 3 * (512 // 4)
    want = 0.0
    for b in range(3):
        i = (amap[b] >= 0).nonzero()[:, 0]
        want += float(((eng._pc_trans[b, i].double() - eng.pc_list[b, amap[b, i]].double()) ** 2).sum())
    _close(ass, float(np.float32(LAM)) * want, "assignment term")
    assert ass > 0.0


def test_the_host_loop_adds_both_losses(dev):
    """OperatorLoop with --recon_with_assign: an iteration at i >= assign_iter returns the Chamfer loss and the assignment
    loss, and the total is their sum plus the flow loss; without the flag the dictionary is the former one."""
    from reart_amd import run_robot as rr
    from reart_amd.networks.model import BaseModel
    from reart_amd.synthetic import make_sequence, split_canonical
    from reart_amd.utils.model_utils import tau_cosine

    seq = make_sequence(T=4, n_parts=4, pts_per_part=128, with_flow=True)
    cano, pcs = split_canonical(seq["complete"].astype(np.float32), 2)
    keys = {}
    for flag in (True, False):
        a = rr.build_parser().parse_args(["--model", "base", "--use_flow_loss", "--use_assign_loss", "--assign_iter", "0", "--cano_idx", "2"]
                                         + (["--recon_with_assign"] if flag else []))
        assert a.recon_with_assign is flag
        torch.manual_seed(4)
        model = BaseModel(num_parts=a.num_parts, pose_len=pcs.shape[0]).to(dev)
        tau = functools.partial(tau_cosine, max_iter=a.n_iter, end_temp=a.end_tau, start_temp=a.start_tau)
        loop = rr.OperatorLoop(a, model, t(cano, dev), t(pcs, dev), [t(r.astype(np.float32), dev) for r in seq["ref_loc"]],
                               [t(f.astype(np.float32), dev) for f in seq["ref_flow"]], tau)
        losses = loop.iteration(0)
        keys[flag] = list(losses)
        if flag:
            total = losses["recon Loss"] + losses["opt assignment loss"] + losses["flow Loss"]
            assert torch.allclose(losses["total Loss"].detach(), total.detach())
            assert float(losses["recon Loss"].detach()) > 0 and float(losses["opt assignment loss"].detach()) > 0
    assert sorted(keys[True]) == ["flow Loss", "opt assignment loss", "recon Loss", "total Loss"]
    assert keys[False] == ["opt assignment loss", "flow Loss", "total Loss"]
    # --model kinematic with the flag goes through the operator loop (the kinematic engine has no such mode)
    # (the loop's constructor asks a model for its parameters only, so the base model can stand in here)
    a = rr.build_parser().parse_args(["--model", "kinematic", "--recon_with_assign"])
    assert isinstance(rr.make_projection_loop(a, model, t(cano, dev), t(pcs, dev)), rr.OperatorLoop)


def test_refusals_and_workspace_size():
    """Both flags without an assign_map: REART_ERR_INVALID_ARG.  The workspace grows by the assignment partials alone --
    8 * B * ceil(N / 1024) bytes, rounded to the plan's 256-byte granule -- and without the flag it does not depend on
    use_assign."""
    from reart_amd import relax

    def case(**over):
        cfg = relax.RelaxConfig(N=256, P=4, B=3, H=16, cano_idx=1, use_flow=1, flow_k=3, M_max=64, M_total=192, n_iter=100, ring=8,
                                lambda_flow=1.0, trans_lr=1e-2, seg_lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, start_tau=1.0,
                                end_tau=0.1, use_boxes=1, lambda_assign=1.0)
        for k, v in over.items():
            setattr(cfg, k, v)
        bufs = relax.RelaxBuffers(**{n: 4096 for n, _ in relax.RelaxBuffers._fields_ if n not in ("aux_stream", "ev_fork", "ev_join")})
        return cfg, bufs, relax._lib_fns().reart_relax_workspace_bytes(ctypes.byref(cfg))

    L = relax._lib_fns()
    cfg, bufs, nbytes = case(use_assign=1, recon_with_assign=1)
    bufs.assign_map = None
    assert L.reart_relax_step(ctypes.byref(cfg), ctypes.byref(bufs), 4096, nbytes, None) == -1
    for N, B in ((256, 3), (1100, 3), (5000, 40), (70000, 33)):
        plain = case(N=N, B=B)[2]
        assert plain > 0
        assert case(N=N, B=B, use_assign=1)[2] == plain
        assert case(N=N, B=B, recon_with_assign=1)[2] == case(N=N, B=B, use_assign=1, recon_with_assign=1)[2]
        extra = 8 * B * -(-N // 1024)
        assert case(N=N, B=B, recon_with_assign=1)[2] - plain == -(-extra // 256) * 256, (N, B)
