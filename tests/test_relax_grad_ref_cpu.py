"""CPU: the gradients of one relaxation iteration in the C oracle (oracle/step.py: fp32, point sums in double) against the
float64 restatement tests/relax_grad_ref.py, on every configuration of tests/test_step_grad_gpu.py, per tensor within TOL of
max|g| (the spread is printed: run with -s); and the comparison the GPU test uses rejects each of a set of injected errors,
among them the per-tensor scale errors (a dropped 1/tau, a lambda applied twice) that Adam's update cannot show."""
import numpy as np
import pytest

from tests.relax_grad_ref import (CASES, PARAMS, TOL, check_grads, gumbel, make_case, oracle_grads, relax_grad_ref)

N_ITER = 50


def _oracle(case):
    from oracle.step import RelaxOracle

    p = case["params"]
    return RelaxOracle(case["cano"], case["pcs"], p["W1"], p["b1"], p["W2"], p["p6d"], p["pt"], case["cano_idx"],
                       case["refs"], case["flows"], n_iter=N_ITER, **case["kw"])


def _step(orc, case, noise, mutate=None):
    """One oracle iteration and the float64 restatement at the oracle's state -> (oracle grads, restatement)."""
    from oracle.step import tau_cosine

    params = {k: v.copy() for k, v in orc.params.items()}
    tau = float(np.float32(tau_cosine(orc.it + 1, N_ITER, 1.0, 5.0)))
    ref = relax_grad_ref(case["cano"], case["pcs"], params, noise, tau, case["cano_idx"], case["refs"], case["flows"],
                         assign=case["assign"], mutate=mutate, **case["kw"])
    out = orc.step(noise, tau=tau, assign=case["assign"])
    return oracle_grads(out, params, case["kw"]["weight_decay"]), out, ref


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_gradients_match_float64(oracle, name):
    case = make_case(name)
    orc = _oracle(case)
    rng = np.random.default_rng(1)
    N, P = case["cano"].shape[0], case["params"]["W2"].shape[0]
    for s in range(2):          # the first step, then a state Adam has moved
        got, out, ref = _step(orc, case, gumbel(rng, N, P))
        sp = check_grads(got, ref["grads"], what=f"{name} step {s}")
        print(f"\n[{name} step {s}] oracle vs float64, max|dg|/max|g|: " + "  ".join(f"{k} {sp[k]:.1e}" for k in PARAMS))
        assert abs(out["recon"] - ref["recon"]) <= 1e-5 * abs(ref["recon"]), (s, out["recon"], ref["recon"])
        assert abs(out["flow"] - ref["flow"]) <= 1e-5 * abs(ref["flow"]), (s, out["flow"], ref["flow"])
        np.testing.assert_array_equal(out["seg_part"], ref["fw"]["seg_part"])
    st = ref["stats"]
    if case["kw"]["robust"]:            # Huber's linear branch carries most of the flow gradient
        assert st["huber_frac"] >= 0.25, st
    if not case["kw"]["euclidean"]:     # the smoothness branch of the mask (dmin > fmax and dmin > 0.05)
        assert st["smooth_frac"] >= 0.25, st


MUTATIONS = ([("flow_cano0_B4", ("scale", k)) for k in PARAMS] + [("assign_only", ("scale", "W2"))] +
             [("huber_linear", "huber_quadratic"),
              ("squared_smooth", "swap_weights"), ("flow_canoB_B4", "swap_weights"),
              ("flow_cano0_B4", "end_frame_shift"), ("flow_canoB_B4", "end_frame_shift"),
              ("B1_cano0", "end_frame_shift"), ("B1_cano1", "end_frame_shift"),
              ("flow_cano0_B4", "double_lambda"), ("assign_only", "double_lambda"),
              ("squared_smooth", "double_smooth"),
              ("chamfer_P20_B3_N1025", "drop_tau"), ("P2_N1088", "drop_tau")])


@pytest.mark.parametrize("name,mutate", MUTATIONS, ids=[f"{n}-{m if isinstance(m, str) else '_'.join(m)}" for n, m in MUTATIONS])
def test_comparison_rejects_injected_error(oracle, name, mutate):
    from oracle.step import tau_cosine

    case = make_case(name)
    orc = _oracle(case)
    noise = gumbel(np.random.default_rng(1), case["cano"].shape[0], case["params"]["W2"].shape[0])
    params = {k: v.copy() for k, v in orc.params.items()}
    got, _, ref = _step(orc, case, noise)
    check_grads(got, ref["grads"], what=name)
    tau = float(np.float32(tau_cosine(1, N_ITER, 1.0, 5.0)))
    bad = relax_grad_ref(case["cano"], case["pcs"], params, noise, tau, case["cano_idx"], case["refs"], case["flows"],
                         assign=case["assign"], mutate=mutate, **case["kw"])
    with pytest.raises(AssertionError, match="gradient spread"):
        check_grads(got, bad["grads"], what=f"{name} with {mutate}")
