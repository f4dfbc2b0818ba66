"""GPU: the gradients the fused relaxation step reduces (reart_relax_step / reart_relax_step_batch: csrc/step.hip and the
backward of csrc/model.hip), read from RelaxEngine.adam_m after one step from m = 0, against the float64 restatement
tests/relax_grad_ref.py on the same inputs and injected noise: per tensor within TOL of max|g|, at the first step and at
two states Adam has moved.  Adam's first step sees only the sign of each entry, and no step sees a constant factor per
tensor, so the parameter comparisons of test_step_gpu.py cannot see a dropped 1/tau or a lambda applied twice; this one
does (tests/test_relax_grad_ref_cpu.py shows it rejects each)."""
import numpy as np
import pytest
import torch

from tests.relax_grad_ref import (CASES, PARAMS, check_grads, gumbel, kernel_grads, make_case, random_params,
                                  relax_grad_ref)

pytestmark = pytest.mark.gpu


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


def _engine(dev, case, model, n_iter=50):
    from reart_amd.relax import RelaxEngine

    refs = None if case["refs"] is None else [t(r, dev) for r in case["refs"]]
    flows = None if case["flows"] is None else [t(f, dev) for f in case["flows"]]
    eng = RelaxEngine(t(case["cano"], dev), t(case["pcs"], dev), model, case["cano_idx"], refs, flows, n_iter=n_iter,
                      tuning=case.get("tuning"), **case["engine_kw"])
    if case.get("assign") is not None:
        src, tgt, lam = case["assign"]
        eng.set_assignment(torch.from_numpy(src), torch.from_numpy(tgt), lam)
    return eng


def _prepare(eng, model, case, noise):
    """Before a measured step: m = 0, the injected noise, and the float64 iteration at the engine's own state."""
    params = _params(model)
    tau = float(eng.tau.item())                 # the temperature the coming step uses
    eng.adam_m.zero_()
    eng.set_gumbel(t(noise, eng.device))
    ref = relax_grad_ref(case["cano"], case["pcs"], params, noise, tau, case["cano_idx"], case["refs"], case["flows"],
                         assign=case.get("assign"), **case["kw"])
    return dict(ref=ref, tau=tau, shapes={k: v.shape for k, v in params.items()}, params=params)


def _verify(eng, pre, what):
    ref = pre["ref"]
    got = kernel_grads(eng.adam_m.cpu().numpy(), pre["shapes"])
    sp = check_grads(got, ref["grads"], what=what)
    print(f"\n[{what}] kernel vs float64, max|dg|/max|g|: " + "  ".join(f"{k} {sp[k]:.1e}" for k in PARAMS))
    row = eng.last_losses().cpu().numpy()
    assert abs(row[0] - ref["recon"]) <= 1e-5 * abs(ref["recon"]), (what, row, ref["recon"])
    assert abs(row[1] - ref["flow"]) <= 1e-5 * abs(ref["flow"]) + 1e-9, (what, row, ref["flow"])
    assert row[3] == np.float32(pre["tau"])
    np.testing.assert_array_equal(eng.seg_part.cpu().numpy(), ref["fw"]["seg_part"], err_msg=what)
    return sp


@pytest.mark.parametrize("name", list(CASES))
def test_fused_step_gradients_match_float64(oracle, dev, name):
    """One edge of the fused step per case (tests/relax_grad_ref.py CASES): the first step, then twice: the engine's
    parameters as they are, m zeroed, the engine's own temperature."""
    from oracle.step import RelaxOracle

    case = make_case(name)
    model = _model(dev, case["params"])
    eng = _engine(dev, case, model)
    p = case["params"]
    orc = RelaxOracle(case["cano"], case["pcs"], p["W1"], p["b1"], p["W2"], p["p6d"], p["pt"], case["cano_idx"],
                      case["refs"], case["flows"], n_iter=50, **case["kw"])
    rng = np.random.default_rng(3)
    N, P = case["cano"].shape[0], p["W2"].shape[0]
    for s in range(3):
        noise = gumbel(rng, N, P)
        pre = _prepare(eng, model, case, noise)
        orc.params = {k: v.copy() for k, v in pre["params"].items()}
        out = orc.step(noise, tau=pre["tau"], assign=case.get("assign"))
        eng.step()
        _verify(eng, pre, f"{name} step {s}")
        np.testing.assert_array_equal(eng.seg_part.cpu().numpy(), out["seg_part"])
    st = pre["ref"]["stats"]
    if case["kw"]["robust"]:
        assert st["huber_frac"] >= 0.25, st
    if not case["kw"]["euclidean"]:
        assert st["smooth_frac"] >= 0.25, st


def test_fused_step_gradients_full_size_mid_run(oracle, dev):
    """BASELINE size (T = 20 x N = 4096, P = 20, Chamfer + flow, canonical frame 10): 300 iterations with the in-kernel
    noise, then one measured step at that state (one: the float64 iteration needs the C oracle's searches at this size)."""
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine
    from reart_amd.synthetic import make_sequence, split_canonical

    T, N, P, c = 20, 4096, 20, 10
    seq = make_sequence(T=T, n_parts=8, pts_per_part=N // 8, seed=2, n_ref=3000, with_flow=True)
    cano, pcs = split_canonical(seq["complete"], c)
    torch.manual_seed(2)
    model = BaseModel(num_parts=P, pose_len=T - 1).to(dev)
    prng = np.random.default_rng(7)
    with torch.no_grad():      # distinct part poses (see tests/test_parity2_gpu.py)
        model.proposal_6d.add_(t(prng.normal(0, 0.05, tuple(model.proposal_6d.shape)).astype(np.float32), dev))
        model.proposal_t.add_(t(prng.normal(0, 0.01, tuple(model.proposal_t.shape)).astype(np.float32), dev))
    eng = RelaxEngine(t(cano, dev), t(pcs, dev), model, c, [t(r, dev) for r in seq["ref_loc"]],
                      [t(f, dev) for f in seq["ref_flow"]], n_iter=15000)
    eng.step(300)
    case = dict(cano=cano, pcs=pcs, refs=seq["ref_loc"], flows=seq["ref_flow"], cano_idx=c,
                kw=dict(lambda_flow=1.0, robust=False, smooth_weight=1e-2, euclidean=True, weight_decay=0.0))
    pre = _prepare(eng, model, case, gumbel(np.random.default_rng(4), N, P))
    eng.step()
    _verify(eng, pre, "full size after 300 iterations")


def test_batched_step_gradients_match_float64(dev):
    """reart_relax_step_batch: three instances of one shape at canonical frames 0, 2 and B in shared launches, one step,
    each against its own float64 iteration."""
    from reart_amd.relax import RelaxBatch
    from reart_amd.synthetic import make_sequence, split_canonical

    B, P = 4, 16
    seq = make_sequence(T=B + 1, n_parts=4, pts_per_part=160, seed=5, n_ref=500, with_flow=True)
    N = seq["complete"].shape[1]
    rng = np.random.default_rng(11)
    runs = []
    for ci in (0, 2, B):
        cano, pcs = split_canonical(seq["complete"], ci)
        case = dict(cano=cano, pcs=pcs, refs=seq["ref_loc"], flows=seq["ref_flow"], cano_idx=ci, params=random_params(rng, B, P),
                    kw=dict(lambda_flow=0.7, robust=False, smooth_weight=1e-2, euclidean=True, weight_decay=0.0),
                    engine_kw=dict(lambda_flow=0.7))
        model = _model(dev, case["params"])
        eng = _engine(dev, case, model)
        runs.append((eng, _prepare(eng, model, case, gumbel(rng, N, P)), ci))
    RelaxBatch([e for e, _, _ in runs]).step(1)
    for eng, pre, ci in runs:
        _verify(eng, pre, f"batch instance at canonical frame {ci}")
