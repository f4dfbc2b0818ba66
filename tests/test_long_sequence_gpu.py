"""GPU: the relaxation model and the fused step on sequences whose pose table does not fit in LDS (csrc/model_long.hip),
pose_len 59 .. 1024.  Yardsticks: the reference's own BaseModel (tests/golden/base_model_long_{a,b}.npz), the C oracle,
and the float64 restatement tests/relax_grad_ref.py -- with the bounds the in-LDS kernels are held to
(tests/test_model_gpu.py, tests/test_step_grad_gpu.py).  reart_base_path says which kernels a shape runs; the tests assert
through it that the shapes meant for the long path take it and that their neighbours do not."""
import os

import numpy as np
import pytest
import torch

from tests import relax_grad_ref as rg
from tests.relax_grad_ref import PARAMS, TOL, check_grads, gumbel, kernel_grads, make_case, random_params, relax_grad_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _model(dev, params):
    from reart_amd.networks.model import BaseModel

    B, P = params["p6d"].shape[:2]
    m = BaseModel(num_parts=P, pose_len=B).to(dev)
    with torch.no_grad():
        m.seg_head.model[0].weight.copy_(t(params["W1"], dev)[:, :, None])
        m.seg_head.model[0].bias.copy_(t(params["b1"], dev))
        m.seg_head.model[2].weight.copy_(t(params["W2"], dev)[:, :, None])
        m.proposal_6d.copy_(t(params["p6d"], dev))
        m.proposal_t.copy_(t(params["pt"], dev))
    return m


def _params(model):
    f = lambda x: x.detach().cpu().numpy().copy()
    c1, c2 = model.seg_head.model[0], model.seg_head.model[2]
    return dict(W1=f(c1.weight)[:, :, 0], b1=f(c1.bias), W2=f(c2.weight)[:, :, 0], p6d=f(model.proposal_6d),
                pt=f(model.proposal_t))


def _path(P, B, backward, H=128):
    from reart_amd import _lib

    return _lib.lib().reart_base_path(P, B, H, backward)


def _close(x, y, rel, what=""):
    np.testing.assert_allclose(x.detach().cpu().numpy(), y, rtol=0, atol=rel * np.abs(y).max(), err_msg=what)


def _model_grads(m):
    return dict(g6d=m.proposal_6d.grad, gt=m.proposal_t.grad, gW1=m.seg_head.model[0].weight.grad[:, :, 0],
                gb1=m.seg_head.model[0].bias.grad, gW2=m.seg_head.model[2].weight.grad[:, :, 0])


# ------------------------------------------------------------------------------------------ 1. reference golden
@pytest.mark.parametrize("tag", ["a", "b"])
def test_long_base_model_matches_the_reference(oracle, dev, tag):
    """pose_len 150 (20 parts) and 60 (32 parts) through BaseModel and .backward(): the tolerances of
    test_base_model_forward_backward."""
    g = np.load(os.path.join(GOLD, f"base_model_long_{tag}.npz"))
    p = {k: g[f"{k}_{tag}"] for k in ("W1", "b1", "W2", "p6d", "pt")}
    B, P = p["p6d"].shape[:2]
    assert _path(P, B, 0) == 1 and _path(P, B, 1) == 1
    tau, cano, noise, G = float(g[f"tau_{tag}"]), g[f"cano_{tag}"], g[f"noise_{tag}"], g[f"G_{tag}"]
    m = _model(dev, p)
    out, seg, trans = m(t(cano, dev), tau=tau, gumbel=t(noise, dev))
    np.testing.assert_array_equal(seg.cpu().numpy(), g[f"seg_{tag}"])
    np.testing.assert_allclose(trans.detach().cpu().numpy(), g[f"trans_{tag}"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(out.detach().cpu().numpy(), g[f"out_{tag}"], rtol=0, atol=1e-6)
    f = oracle.base_forward(cano, p["W1"], p["b1"], p["W2"], p["p6d"], p["pt"], noise, tau)
    np.testing.assert_allclose(out.detach().cpu().numpy(), f["out"], rtol=0, atol=2e-7)
    (out * t(G, dev)).sum().backward()
    ref = oracle.base_backward(cano, p["W1"], p["b1"], p["W2"], p["p6d"], p["pt"], f["y_soft"], f["hard_idx"], tau, G)
    got = _model_grads(m)
    for k in got:
        _close(got[k], ref[k], 2e-5, k)                 # oracle accumulates in double, kernels in fp32 chunks
        _close(got[k], g[f"{k}_{tag}"], 2e-4, k)        # the reference's autograd


# ------------------------------------------------------------------------------------------ 2. boundaries
# (P, largest pose_len the in-LDS backward takes at H = 128): every instantiation (20, 10, 8, generic at 32 and 5)
_BWD_LAST = {20: 58, 10: 88, 8: 97, 32: 38, 5: 87}
_BOUNDARY = [(P, B + d, N) for (P, B), N in zip(sorted(_BWD_LAST.items()), (333, 70, 1000, 333, 70)) for d in (0, 1)] + \
            [(20, 90, 70), (20, 91, 70),          # the forward's own switch at 20 parts
             (20, 1024, 333)]


@pytest.mark.parametrize("P,B,N", _BOUNDARY)
def test_long_base_model_boundaries_match_the_oracle(oracle, dev, P, B, N):
    """The last pose_len the in-LDS kernels take and the first one they do not, per instantiation, and the largest
    pose_len there is; N not a multiple of 16 / 32 / 64.  Bounds of test_base_model_forward_backward."""
    last = _BWD_LAST.get(P)
    if last is not None and B in (last, last + 1):
        assert _path(P, B, 1) == (1 if B == last + 1 else 0)
    if (P, B) in ((20, 90), (20, 91)):
        assert _path(P, B, 0) == (1 if B == 91 else 0) and _path(P, B, 1) == 1
    if B == 1024:
        assert _path(P, B, 0) == 1 and _path(P, B, 1) == 1
    rng = np.random.default_rng([P, B, N])
    H, tau = 128, 2.0
    cano = rng.uniform(-0.3, 0.3, (N, 3)).astype(np.float32)
    p = dict(W1=rng.normal(0, 0.5, (H, 3)).astype(np.float32), b1=rng.normal(0, 0.1, H).astype(np.float32),
             W2=rng.normal(0, 0.3, (P, H)).astype(np.float32),
             p6d=(np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), (B, P, 1)) + rng.normal(0, 0.3, (B, P, 6))).astype(np.float32),
             pt=rng.normal(0, 0.05, (B, P, 3)).astype(np.float32))
    noise = gumbel(rng, N, P)
    G = rng.normal(size=(B, N, 3)).astype(np.float32)
    f = oracle.base_forward(cano, p["W1"], p["b1"], p["W2"], p["p6d"], p["pt"], noise, tau)
    ref = oracle.base_backward(cano, p["W1"], p["b1"], p["W2"], p["p6d"], p["pt"], f["y_soft"], f["hard_idx"], tau, G)
    runs = []
    for _ in range(2):
        m = _model(dev, p)
        out, seg, trans = m(t(cano, dev), tau=tau, gumbel=t(noise, dev))
        (out * t(G, dev)).sum().backward()
        runs.append([out.detach().cpu().numpy(), seg.cpu().numpy(), trans.detach().cpu().numpy()] +
                    [v.detach().cpu().numpy().copy() for v in _model_grads(m).values()])
        if len(runs) == 1:
            np.testing.assert_array_equal(runs[0][1], f["seg_part"])
            np.testing.assert_allclose(runs[0][2], f["trans_list"], rtol=0, atol=1e-6)
            np.testing.assert_allclose(runs[0][0], f["out"], rtol=0, atol=2e-7)
            for k, v in _model_grads(m).items():
                _close(v, ref[k], 2e-5, k)
    for x, y in zip(*runs):          # no atomics anywhere: reruns are bit-identical
        np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------------------------------ 3. fused step vs float64
LONG_CASES = {
    "long_B59_N321": dict(B=59, N=321, P=20, cano_idx=30),
    "long_B91_N321_cano0": dict(B=91, N=321, P=20, cano_idx=0),
    "long_B200_N257_canoB": dict(B=200, N=257, P=20, cano_idx=200),
    "long_B39_N130_P32": dict(B=39, N=130, P=32, cano_idx=7),
    "long_B600_N130_P8_chamfer": dict(B=600, N=130, P=8, cano_idx=300, flow=False),
    "long_B1024_N96": dict(B=1024, N=96, P=20, cano_idx=512),
    "long_B96_assign": dict(B=96, N=200, P=20, cano_idx=40, assign=0.3),
}


def _make(name, spec):
    """make_case of tests/relax_grad_ref.py for a shape that is not in its CASES (random_params, uniform canonical cloud
    +- 0.3, frames at sigma 0.02, lambda_flow 0.7)."""
    rg.CASES[name] = spec
    try:
        return make_case(name)
    finally:
        del rg.CASES[name]


def _engine(dev, case, model, n_iter=50, tuning=None):
    from reart_amd.relax import RelaxEngine

    refs = None if case["refs"] is None else [t(r, dev) for r in case["refs"]]
    flows = None if case["flows"] is None else [t(f, dev) for f in case["flows"]]
    tn = dict(case.get("tuning") or {})
    tn.update(tuning or {})
    eng = RelaxEngine(t(case["cano"], dev), t(case["pcs"], dev), model, case["cano_idx"], refs, flows, n_iter=n_iter,
                      tuning=tn, **case["engine_kw"])
    if case.get("assign") is not None:
        src, tgt, lam = case["assign"]
        eng.set_assignment(torch.from_numpy(src), torch.from_numpy(tgt), lam)
    return eng


@pytest.mark.parametrize("name", list(LONG_CASES))
def test_long_fused_step_gradients_match_float64(oracle, dev, name):
    """Three steps like test_fused_step_gradients_match_float64: gradients within TOL of the float64 iteration, recon and
    flow loss within 1e-5, seg_part equal to the fp32 oracle's."""
    from oracle.step import RelaxOracle

    assert TOL == 2e-4
    spec = LONG_CASES[name]
    assert _path(spec["P"], spec["B"], 1) == 1
    case = _make(name, spec)
    model = _model(dev, case["params"])
    eng = _engine(dev, case, model)
    p = case["params"]
    orc = RelaxOracle(case["cano"], case["pcs"], p["W1"], p["b1"], p["W2"], p["p6d"], p["pt"], case["cano_idx"],
                      case["refs"], case["flows"], n_iter=50, **case["kw"])
    rng = np.random.default_rng(3)
    N, P = case["cano"].shape[0], p["W2"].shape[0]
    for s in range(3):
        noise = gumbel(rng, N, P)
        params = _params(model)
        tau = float(eng.tau.item())
        eng.adam_m.zero_()
        eng.set_gumbel(t(noise, dev))
        ref = relax_grad_ref(case["cano"], case["pcs"], params, noise, tau, case["cano_idx"], case["refs"], case["flows"],
                             assign=case.get("assign"), **case["kw"])
        orc.params = {k: v.copy() for k, v in params.items()}
        out = orc.step(noise, tau=tau, assign=case.get("assign"))
        eng.step()
        what = f"{name} step {s}"
        got = kernel_grads(eng.adam_m.cpu().numpy(), {k: v.shape for k, v in params.items()})
        sp = check_grads(got, ref["grads"], what=what)
        print(f"\n[{what}] kernel vs float64, max|dg|/max|g|: " + "  ".join(f"{k} {sp[k]:.1e}" for k in PARAMS))
        row = eng.last_losses().cpu().numpy()
        assert abs(row[0] - ref["recon"]) <= 1e-5 * abs(ref["recon"]), (what, row, ref["recon"])
        assert abs(row[1] - ref["flow"]) <= 1e-5 * abs(ref["flow"]) + 1e-9, (what, row, ref["flow"])
        assert row[3] == np.float32(tau)
        np.testing.assert_array_equal(eng.seg_part.cpu().numpy(), ref["fw"]["seg_part"], err_msg=what)
        np.testing.assert_array_equal(eng.seg_part.cpu().numpy(), out["seg_part"], err_msg=what)


# ------------------------------------------------------------------------------------------ 4. both paths, one shape
_AB = {
    "headline_small": (dict(B=19, N=1024, P=20, cano_idx=10), None),
    "P32_N63": (None, None),
    "bwd16": (None, None),
    "bwd64_fwd64": (dict(B=4, N=577, P=20, cano_idx=2), {"tune_bwd_pts": 64, "tune_fwd_pts": 64}),
}


@pytest.mark.parametrize("name", list(_AB))
def test_long_path_equals_lds_path_on_one_shape(dev, name):
    """tune_long = 0 and 1 from one state with the same injected noise, one step: the forward and the searches are the
    same arithmetic (pc_trans, seg_part, recon and flow loss bit-equal); the gradients within 2e-5 of max|g| of each other,
    the bound both backward kernels are held to against the oracle."""
    spec, tuning = _AB[name]
    case = make_case(name) if spec is None else _make(name, spec)
    P, B = case["params"]["W2"].shape[0], case["params"]["p6d"].shape[0]
    assert _path(P, B, 0) == 0 and _path(P, B, 1) == 0           # by fit this shape runs the in-LDS kernels
    N = case["cano"].shape[0]
    noise = gumbel(np.random.default_rng(8), N, P)
    res = []
    for long_ in (0, 1):
        model = _model(dev, case["params"])
        eng = _engine(dev, case, model, tuning=dict(tuning or {}, tune_long=long_))
        assert eng.cfg.tune_long == long_
        eng.set_gumbel(t(noise, dev))
        eng.step()
        shapes = {k: v.shape for k, v in case["params"].items()}
        res.append(dict(pc=eng.pc_trans.cpu().numpy(), seg=eng.seg_part.cpu().numpy(), row=eng.last_losses().cpu().numpy(),
                        trans=eng.trans_list.cpu().numpy(), g=kernel_grads(eng.adam_m.cpu().numpy(), shapes)))
    a, b = res
    np.testing.assert_array_equal(a["pc"], b["pc"])
    np.testing.assert_array_equal(a["seg"], b["seg"])
    np.testing.assert_array_equal(a["trans"], b["trans"])
    assert a["row"][0] == b["row"][0] and a["row"][1] == b["row"][1], (a["row"], b["row"])
    assert np.isfinite(a["row"]).all() and a["row"][0] > 0
    for k in PARAMS:
        d = np.abs(a["g"][k].astype(np.float64) - b["g"][k]).max()
        assert d <= 2e-5 * np.abs(a["g"][k]).max(), (k, d, np.abs(a["g"][k]).max())


# ------------------------------------------------------------------------------------------ 5. determinism, graph replay
def test_long_graph_replay_equals_eager_and_is_deterministic(dev):
    """pose_len 128, N = 1024: eager, graph replay and a second graph replay leave the same bits after 12 steps."""
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine

    rng = np.random.default_rng(1)
    N, P, B = 1024, 20, 128
    assert _path(P, B, 0) == 1 and _path(P, B, 1) == 1
    cano = rng.uniform(-0.3, 0.3, (N, 3)).astype(np.float32)
    pcs = (cano[None] + rng.normal(0, 0.02, (B, N, 3))).astype(np.float32)
    refs = [rng.uniform(-0.3, 0.3, (700 + i, 3)).astype(np.float32) for i in range(B)]
    flows = [rng.normal(0, 0.02, r.shape).astype(np.float32) for r in refs]
    results = []
    for mode in ("eager", "graph", "graph"):
        torch.manual_seed(0)
        model = BaseModel(num_parts=P, pose_len=B).to(dev)
        eng = RelaxEngine(t(cano, dev), t(pcs, dev), model, 60, [t(r, dev) for r in refs], [t(f, dev) for f in flows],
                          n_iter=100, seed=5)
        done = eng.capture() if mode == "graph" else 0
        eng.step(12 - done)
        it, log = eng.loss_log()
        assert it == 12
        results.append((log.cpu().numpy(), model.proposal_t.detach().cpu().numpy().copy(),
                        model.proposal_6d.detach().cpu().numpy().copy(),
                        model.seg_head.model[2].weight.detach().cpu().numpy().copy(), eng.pc_trans.cpu().numpy()))
    for r in results[1:]:
        for x, y in zip(results[0], r):
            np.testing.assert_array_equal(x, y)
    assert np.isfinite(results[0][0]).all()


# ------------------------------------------------------------------------------------------ 6. instances
def test_long_batched_instances_equal_separate_engines(dev):
    """RelaxBatch of three engines at pose_len 96 (eager, then replayed from one graph) equals three solo engines."""
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxBatch, RelaxEngine
    from reart_amd.synthetic import make_sequence, split_canonical

    K, B = 3, 96
    assert _path(12, B, 1) == 1
    seq = make_sequence(T=B + 1, n_parts=4, pts_per_part=150, seed=5, n_ref=400, with_flow=True)

    def build():
        out = []
        for k in range(K):
            ci = (0, 40, B)[k]
            cano, pcs = split_canonical(seq["complete"], ci)
            torch.manual_seed(10 + k)
            model = BaseModel(num_parts=12, pose_len=B).to(dev)
            refs = [t(r, dev) for r in seq["ref_loc"]], [t(f, dev) for f in seq["ref_flow"]]
            out.append((RelaxEngine(t(cano, dev), t(pcs, dev), model, ci, refs[0], refs[1], n_iter=200, seed=100 + k), model))
        return out

    def state(eng, model):
        it, log = eng.loss_log()
        return (log.cpu().numpy(), model.proposal_6d.detach().cpu().numpy().copy(), model.proposal_t.detach().cpu().numpy().copy(),
                model.seg_head.model[2].weight.detach().cpu().numpy().copy(), eng.pc_trans.cpu().numpy(), eng.seg_part.cpu().numpy())

    solo = build()
    for eng, _ in solo:
        eng.step(16)
    batched = build()
    batch = RelaxBatch([e for e, _ in batched])
    batch.step(5)                        # eager
    batch.capture(steps_per_graph=2)     # +1 (warm-up)
    batch.step(10)                       # 5 replays
    assert batch.graph_replays == 5 and batch.eager_steps == 5
    torch.cuda.synchronize()
    for (e0, m0), (e1, m1) in zip(solo, batched):
        a, b = state(e0, m0), state(e1, m1)
        assert np.isfinite(a[0]).all() and a[0].shape == b[0].shape
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    assert not np.array_equal(state(*solo[0])[1], state(*solo[1])[1])


# ------------------------------------------------------------------------------------------ 7. it optimises
def test_long_sequence_optimises(dev):
    """129 frames, N = 1024, 20 parts, Chamfer + flow, 300 iterations: finite, and the mean total loss of the last 50
    below 0.6 x that of the first 50 (the condition of test_long_trajectory_stays_finite)."""
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine
    from reart_amd.synthetic import make_sequence, split_canonical

    seq = make_sequence(T=129, n_parts=4, pts_per_part=256, seed=4, n_ref=600)
    cano, pcs = split_canonical(seq["complete"], 64)
    torch.manual_seed(2)
    model = BaseModel(num_parts=20, pose_len=128).to(dev)
    eng = RelaxEngine(t(cano, dev), t(pcs, dev), model, 64, [t(r, dev) for r in seq["ref_loc"]],
                      [t(f, dev) for f in seq["ref_flow"]], n_iter=300, ring=1024)
    done = eng.capture()
    eng.step(300 - done)
    it, log = eng.loss_log()
    log = log.cpu().numpy()
    print(f"\n[long optimise] first 50: {log[:50, 2].mean():.6g}  last 50: {log[-50:, 2].mean():.6g}")
    assert it == 300 and np.isfinite(log).all()
    assert log[-50:, 2].mean() < 0.6 * log[:50, 2].mean()
    for p in model.parameters():
        assert torch.isfinite(p).all()


# ------------------------------------------------------------------------------------------ 8. the stated limit
def test_pose_len_above_the_limit_is_refused_up_front(dev):
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine

    B, N, P = 1025, 64, 4
    model = BaseModel(num_parts=P, pose_len=B).to(dev)
    cano = torch.zeros((N, 3), device=dev)
    with pytest.raises(NotImplementedError, match="REART_MAX_POSE_LEN"):
        model(cano, tau=1.0)
    with pytest.raises(NotImplementedError, match="REART_MAX_POSE_LEN"):
        RelaxEngine(cano, torch.zeros((B, N, 3), device=dev), model, 0)
