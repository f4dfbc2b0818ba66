"""tests/relax_both_ref.py against the oracle it restates: where the combined iteration overlaps with
``oracle.step.RelaxOracle.step`` the two agree in every bit, so the yardstick of the combined mode of the fused step
(tests/test_relax_both_gpu.py) is pinned to the oracle without a change to it."""
import numpy as np
import pytest

from tests import relax_both_ref as R

ARRAYS = ("pc_trans", "G", "seg_part", "hard_idx")
SCALARS = ("recon", "flow", "total", "tau")


def _pair(oracle, flow=True):
    from oracle.step import RelaxOracle

    pb = R.problem()
    refs, flows = (pb["refs"], pb["flows"]) if flow else (None, None)
    mk = lambda: RelaxOracle(pb["cano"], pb["pcs"], pb["W1"], pb["b1"], pb["W2"], pb["p6d"], pb["pt"], 2, refs, flows,
                             lambda_flow=0.7, n_iter=50)
    return pb, mk(), mk()


def _same(a, b, orc_a, orc_b, msg):
    for k in ARRAYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{msg} {k}")
    for k, v in a["grads"].items():
        np.testing.assert_array_equal(v, b["grads"][k], err_msg=f"{msg} grads {k}")
    for k in orc_a.params:
        np.testing.assert_array_equal(orc_a.params[k], orc_b.params[k], err_msg=f"{msg} param {k}")
        np.testing.assert_array_equal(orc_a.m[k], orc_b.m[k], err_msg=f"{msg} m {k}")
        np.testing.assert_array_equal(orc_a.v[k], orc_b.v[k], err_msg=f"{msg} v {k}")


def _pairs(rng, N, B, n=64):
    return rng.permutation(N)[:n], np.stack([rng.permutation(N)[:n] for _ in range(B)])


@pytest.mark.parametrize("flow", [True, False])
def test_without_pairs_it_is_the_oracle_step(oracle, flow):
    pb, a, b = _pair(oracle, flow)
    for i in range(3):
        noise = R.gumbel(pb["rng"], pb["N"], pb["P"])
        ra, rb = a.step(noise), R.step_both(b, noise)
        _same(ra, rb, a, b, f"iter {i}")
        for k in SCALARS:
            assert ra[k] == rb[k], (i, k)
        assert rb["ass"] == 0.0 and a.it == b.it


@pytest.mark.parametrize("flow", [True, False])
def test_without_chamfer_it_is_the_oracle_assignment_step(oracle, flow):
    pb, a, b = _pair(oracle, flow)
    for i in range(3):
        noise = R.gumbel(pb["rng"], pb["N"], pb["P"])
        src, tgt = _pairs(pb["rng"], pb["N"], pb["B"])
        ra, rb = a.step(noise, assign=(src, tgt, 0.3)), R.step_both(b, noise, assign=(src, tgt, 0.3), chamfer=False)
        _same(ra, rb, a, b, f"iter {i}")
        # the oracle reports the assignment term as its `recon`; the restatement keeps the terms apart
        assert ra["recon"] == rb["ass"] and rb["recon"] == 0.0 and ra["flow"] == rb["flow"] and ra["total"] == rb["total"]
        assert ra["tau"] == rb["tau"]


def test_combined_gradient_is_the_float32_sum_of_the_pure_forms(oracle):
    """On one state, without the flow loss: G(both) = fl(G(Chamfer) + G(assignment)) element by element.  With it, both
    pure forms carry the flow term G_f, so the sum is taken of the pure forms WITHOUT flow and G_f is added to it last:
    G(both) = fl(fl(G_c + G_a) + G_f).  G_f is read off exactly where no pair sits (there G(assignment, flow) is G_f alone);
    at the paired points it is G(Chamfer, flow) - G_c up to one rounding.  The three loss terms come back separately."""
    import copy

    for flow in (False, True):
        pb, a, _ = _pair(oracle, flow)
        noise = R.gumbel(pb["rng"], pb["N"], pb["P"])
        a.step(noise)        # leave the initial state: Adam moments are no longer zero
        noise = R.gumbel(pb["rng"], pb["N"], pb["P"])
        src, tgt = _pairs(pb["rng"], pb["N"], pb["B"])
        asg = (src, tgt, 0.3)
        rc = copy.deepcopy(a).step(noise)
        ra = copy.deepcopy(a).step(noise, assign=asg)
        both = copy.deepcopy(a)
        rb = R.step_both(both, noise, assign=asg)
        np.testing.assert_array_equal(rb["pc_trans"], rc["pc_trans"])
        assert rb["G"].dtype == np.float32
        if not flow:
            np.testing.assert_array_equal(rb["G"], rc["G"] + ra["G"])
        else:
            # the pure forms without the flow term, on the same state
            nf = copy.deepcopy(a)
            nf.refs = nf.ref_flows = None
            gc = copy.deepcopy(nf).step(noise)["G"]
            ga = copy.deepcopy(nf).step(noise, assign=asg)["G"]
            gf = ra["G"].copy()
            un = np.ones(ra["G"].shape[:2], bool)
            un[:, src] = False
            np.testing.assert_array_equal(ga[un], 0.0)          # there G(assignment, flow) IS the flow term
            np.testing.assert_array_equal(rb["G"][un], (gc + ga)[un] + gf[un])
            np.testing.assert_array_equal(rc["G"][un], gc[un] + gf[un])
            np.testing.assert_allclose(rb["G"], (gc + ga) + (rc["G"] - gc), rtol=0, atol=2e-7 * np.abs(rc["G"]).max())
        assert rb["recon"] == rc["recon"] and rb["ass"] == ra["recon"] and rb["flow"] == rc["flow"] == ra["flow"]
        assert rb["total"] == rb["recon"] + rb["ass"] + rb["flow"]
        assert rb["ass"] > 0.0 and rb["recon"] > 0.0
        assert both.it == a.it + 1


def test_the_flag_is_off_by_default_and_the_structs_keep_their_layout():
    """--recon_with_assign on run_robot and the sweep; the config field sits in the padding in front of `seed`, so every
    older field keeps its offset and the struct its 176 bytes; the buffers grow by one pointer at the end."""
    import ctypes

    from reart_amd import relax, run_robot, sweep

    assert run_robot.build_parser().parse_args([]).recon_with_assign is False
    assert run_robot.build_parser().parse_args(["--recon_with_assign"]).recon_with_assign is True
    assert sweep.build_cli().parse_args([]).recon_with_assign is False
    C, Bf = relax.RelaxConfig, relax.RelaxBuffers
    assert (C.fixed_tau.offset, C.recon_with_assign.offset, C.seed.offset, C.tune_long.offset, ctypes.sizeof(C)) == (88, 92, 96, 168, 176)
    assert Bf._fields_[-1][0] == "losses_assign" and Bf.losses_assign.offset == Bf.assign_map.offset + 8
    assert ctypes.sizeof(Bf) == 8 * len(Bf._fields_)
    assert "recon_with_assign" in relax.RelaxBatch.SAME
    assert relax.RelaxConfig().recon_with_assign == 0
