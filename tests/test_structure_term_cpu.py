"""What of the structure term can be checked without a device: the argument and limit statuses of reart_structure_term /
reart_rel_trans_backward (decided before any launch), the float64 restatement of tests/structure_loss_ref.py against the
reference's own float32 values (tests/golden/loss_terms.npz), the float32 restatement against the float64 one within the
bounds the GPU test uses, the planted errors rejected by that comparison, every GPU case clear of the decision thresholds, and
the errors of the Python interface."""
import numpy as np
import pytest
import torch

from tests import structure_loss_ref as slr
from tests.structure_loss_ref import GOLDEN_CASES, golden_case, golden_ref

INVALID_ARG, UNSUPPORTED = -1, -2


def test_statuses_without_a_launch():
    from reart_amd import _lib

    L = _lib.lib()
    d = 4096                                                            # a non-null dummy address: refused before it is read
    big = 1 << 40
    term = lambda trans=d, T=9, P=10, pairs=d, E=9, loss=d, ws=d, nbytes=big: L.reart_structure_term(
        trans, T, P, pairs, E, 1.0, loss, None, None, d, ws, nbytes, None)
    assert term(trans=None) == INVALID_ARG and term(loss=None) == INVALID_ARG
    assert term(T=0) == INVALID_ARG and term(P=0) == INVALID_ARG and term(E=-1) == INVALID_ARG
    assert term(ws=None) == INVALID_ARG
    assert term(nbytes=L.reart_structure_term_workspace_bytes(9, 10, 9) - 1) == INVALID_ARG
    rel = lambda trans=d, T=9, P=10, pairs=d, E=9, g=d, out=d, ws=d, nbytes=big: L.reart_rel_trans_backward(
        trans, T, P, pairs, E, g, out, ws, nbytes, None)
    assert rel(trans=None) == INVALID_ARG and rel(out=None) == INVALID_ARG and rel(pairs=None) == INVALID_ARG
    assert rel(g=None) == INVALID_ARG and rel(T=0) == INVALID_ARG and rel(P=-1) == INVALID_ARG and rel(E=-1) == INVALID_ARG
    assert rel(ws=None) == INVALID_ARG
    assert rel(nbytes=L.reart_rel_trans_backward_workspace_bytes(9, 10, 9) - 1) == INVALID_ARG
    for nbytes in (L.reart_structure_term_workspace_bytes, L.reart_rel_trans_backward_workspace_bytes):
        assert nbytes(9, 10, 9) > 0 and nbytes(1024, 64, 4096) > 0 and nbytes(9, 10, 0) > 0
        assert nbytes(1024, 64, 4096) >= 1024 * 4096 * 24 * 4
        for T, P, E in ((1025, 10, 9), (9, 65, 9), (9, 10, 4097), (0, 10, 9), (9, 0, 9), (9, 10, -1)):
            assert nbytes(T, P, E) == 0, (T, P, E)
    for T, P, E in ((1025, 10, 9), (9, 65, 9), (9, 10, 4097)):           # bytes 0 exactly where UNSUPPORTED
        assert term(T=T, P=P, E=E) == UNSUPPORTED and rel(T=T, P=P, E=E) == UNSUPPORTED
    assert L.reart_structure_term(d, 1025, 1, None, 9, 1.0, d, None, None, None, d, big, None) == UNSUPPORTED   # relative-motion form


@pytest.mark.parametrize("tag", GOLDEN_CASES)
def test_float64_restatement_against_the_reference(tag):
    trans, pairs, _ = golden_case(tag)
    got = slr.structure_term(trans, pairs)
    sp = slr.compare(dict(got, edge_cost=None), golden_ref(tag), tag)
    print(f"\n[{tag}] float64 restatement vs the reference's float32: " + "  ".join(f"{k} {v:.1e}" for k, v in sp.items()))


@pytest.mark.parametrize("name", list(slr.CASES))
def test_float32_restatement_within_the_gpu_bounds(name):
    c = slr.case(name)
    slr.assert_clear_of_thresholds(c["trans"], c["pairs"])
    got = slr.structure_term(c["trans"], c["pairs"], dtype=torch.float32)
    sp = slr.compare(got, slr.case_ref(name), name)
    print(f"\n[{name}] float32 vs float64: " + "  ".join(f"{k} {v:.1e}" for k, v in sp.items()))


@pytest.mark.parametrize("tag", ("synA", "synB"))
def test_golden_synthetic_cases_are_clear_of_thresholds(tag):
    trans, pairs, _ = golden_case(tag)
    slr.assert_clear_of_thresholds(trans, pairs)


@pytest.mark.parametrize("tag", ("raw", "new"))
def test_fixture_decisions_agree_in_float32_and_float64(tag):
    trans, pairs, _ = golden_case(tag)
    d32 = slr.decisions(trans, pairs)
    d64 = slr.structure_term(trans, pairs, dec="own")["dec"]
    assert slr._same(d32, d64)


# mutation -> a case on which it must show
MUTATIONS = {"target_not_detached": "T9_P10_E9_mixed", "cost_rule": "E2_masked_mean_helical", "drop_src": "T9_P10_E9_mixed",
             "ignore_e1": "E1_plain_mean", ("scale", 1.001): "T2_E2"}


@pytest.mark.parametrize("mutation", list(MUTATIONS), ids=str)
def test_planted_errors_are_rejected(mutation):
    name = MUTATIONS[mutation]
    c = slr.case(name)
    bad = slr.structure_term(c["trans"], c["pairs"], mutate=mutation)
    with pytest.raises(AssertionError):
        slr.compare(bad, slr.case_ref(name), name)


def test_rel_trans_backward_restatement_ignores_row_3():
    c = slr.case("T2_E2")
    up = np.random.default_rng(5).normal(size=(2, 2, 4, 4)).astype(np.float32)
    g = slr.rel_trans_backward(c["trans"], c["pairs"], up)
    up2 = up.copy()
    up2[..., 3, :] = 7.0
    assert np.array_equal(g, slr.rel_trans_backward(c["trans"], c["pairs"], up2)) and not g[..., 3, :].any() and g.any()


def test_interface_errors():
    from reart_amd.networks.loss import StructureTerm, compute_connection_loss, structure_loss
    from reart_amd.utils.graph_utils import compute_relative_trans

    tl = torch.eye(4).repeat(3, 4, 1, 1)
    edges = torch.tensor([[0, 1], [1, 2], [2, 3]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        StructureTerm(edges)(tl)
    with pytest.raises(TypeError):
        StructureTerm(edges)(tl.double())
    with pytest.raises(ValueError):
        StructureTerm(torch.tensor([[0, 4]]))(tl)
    with pytest.raises(ValueError):
        StructureTerm(torch.tensor([[-1, 2]]))(tl)
    rel = torch.eye(4).repeat(3, 4, 4, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        structure_loss(rel, None, None, None, None, edges)
    with pytest.raises(TypeError):
        structure_loss(rel.double(), None, None, None, None, edges)
    with pytest.raises(ValueError):
        structure_loss(rel, None, None, None, None, torch.tensor([[0, 4]]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_relative_trans(tl.requires_grad_(True), return_trans=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_connection_loss(torch.zeros(8, 3), torch.zeros(8, dtype=torch.long), edges[:1], torch.zeros(2, 8, 3), None)
