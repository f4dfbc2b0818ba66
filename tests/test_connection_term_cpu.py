"""What of the connection term can be checked without a device: the restatement of tests/connection_term_ref.py against the
reference's own run (tests/golden/loss_terms.npz: selection exact, value and gradient within the bounds of the GPU test), its
tie rules on exact coordinates, every case meant for the composition tie-free, the limits of the workspace queries, the
argument statuses of the two entry points (decided before any launch) and the errors of the Python interface."""
import numpy as np
import pytest
import torch

from tests import connection_term_ref as ctr

INVALID_ARG, UNSUPPORTED = -1, -2


def test_restatement_reproduces_the_reference():
    c, g = ctr.golden_case()
    gaps = ctr.assert_tie_free(c["cano"], c["seg"], c["pairs"], c["P"], c["k"])
    print(f"\n[golden] smallest gap to a second neighbour {gaps[0]:.1e}, to the (k+1)-th source {gaps[1]:.1e}")
    ref = ctr.connection_term(c["cano"], c["seg"], c["pairs"], c["P"], c["pc"], c["k"])
    assert ref["valid"].all()
    assert np.array_equal(ref["src"], g["src"]) and np.array_equal(ref["tgt"], g["tgt"])      # topk's order: ascending distance
    lv = abs(ref["loss"] - float(g["loss"])) / float(g["loss"])
    rows = g["rows"]
    assert not np.delete(ref["grad"], rows, axis=1).any()                   # the selected points, and only they
    top = float(np.abs(g["grad_rows"]).max())
    gv = float(np.abs(ref["grad"][:, rows] - g["grad_rows"]).max()) / top
    print(f"[golden] float64 restatement vs the reference's float32: loss {lv:.1e}  grad {gv:.1e}")
    assert lv <= ctr.VALUE_TOL and gv <= ctr.GRAD_TOL


def test_tie_rules():
    c, expect = ctr.tie_case()
    got = ctr.select(c["cano"], c["seg"], c["pairs"], c["P"], c["k"])
    for key in ("src", "tgt", "dist", "valid"):
        assert np.array_equal(got[key], expect[key]), key
    ref = ctr.term(c["pc"], got["src"], got["tgt"], got["valid"], c["k"])
    assert ref["edge_cost"][1] == 0.0 and ref["edge_cost"][0] > 0.0        # the self edge costs nothing
    assert ref["grad"][:, 1].any() and not ref["grad"][:, [3, 4, 6, 7]].any()


@pytest.mark.parametrize("name", list(ctr.CASES))
def test_cases_are_what_they_claim(name):
    c = ctr.case(name)                                                      # asserts tie-free where compose is set
    ref = ctr.case_ref(name)
    if ctr.CASES[name][1]:
        assert ref["valid"].all()
    if name == "invalid_edges":
        assert ref["valid"].tolist() == [False, False, True, False, False, True, True]
        assert not ref["edge_cost"][~ref["valid"]].any()
    if name == "E0":
        assert ref["loss"] == 0.0 and not ref["grad"].any()
    if name == "star_twice_both_self":
        assert np.array_equal(ref["src"][4], ref["src"][5]) and np.array_equal(ref["src"][8], ref["tgt"][8])
    members = [set(np.flatnonzero(c["seg"] == p).tolist()) for p in range(c["P"])]
    for e in np.flatnonzero(ref["valid"]):
        a, b = c["pairs"][e]
        assert set(ref["src"][e].tolist()) <= members[a] and set(ref["tgt"][e].tolist()) <= members[b]
        assert len(set(ref["src"][e].tolist())) == c["k"]


def test_workspace_queries_know_the_limits():
    from reart_amd import _lib

    L = _lib.lib()
    sel, term = L.reart_connection_select_workspace_bytes, L.reart_connection_term_workspace_bytes
    assert _lib.CONN_MAX_N == 65536 and _lib.CONN_MAX_K == 64
    assert sel(4096, 20, 19, 10) > 0 and sel(65536, 64, 4096, 64) > 0 and sel(1, 1, 0, 1) > 0
    for N, P, E, k in ((65537, 64, 9, 10), (4096, 65, 9, 10), (4096, 20, 4097, 10), (4096, 20, 9, 65), (4096, 20, 9, 0),
                       (0, 20, 9, 10), (4096, 0, 9, 10), (4096, 20, -1, 10)):
        assert sel(N, P, E, k) == 0, (N, P, E, k)
    assert term(19, 4096, 19, 10) > 0 and term(1024, 65536, 4096, 64) > 0 and term(1, 1, 0, 1) > 0
    assert term(1024, 65536, 4096, 64) >= 2 * 4096 * 64 * 4 + 65537 * 4
    for T, N, E, k in ((1025, 4096, 9, 10), (9, 65537, 9, 10), (9, 4096, 4097, 10), (9, 4096, 9, 65), (9, 4096, 9, 0),
                       (0, 4096, 9, 10), (9, 0, 9, 10), (9, 4096, -1, 10)):
        assert term(T, N, E, k) == 0, (T, N, E, k)


def test_statuses_without_a_launch():
    from reart_amd import _lib

    L = _lib.lib()
    d, big = 4096, 1 << 40                                                  # a non-null dummy address: refused before it is read
    sel = lambda cano=d, seg=d, N=512, P=6, pairs=d, E=7, k=10, src=d, tgt=d, valid=d, ws=d, nbytes=big: \
        L.reart_connection_select(cano, seg, N, P, pairs, E, k, src, tgt, None, valid, ws, nbytes, None)
    for bad in (dict(cano=None), dict(seg=None), dict(pairs=None), dict(src=None), dict(tgt=None), dict(valid=None), dict(N=0),
                dict(P=0), dict(E=-1), dict(k=0), dict(ws=None),
                dict(nbytes=L.reart_connection_select_workspace_bytes(512, 6, 7, 10) - 1)):
        assert sel(**bad) == INVALID_ARG, bad
    for over in (dict(N=65537), dict(P=65), dict(E=4097), dict(k=65)):
        assert sel(**over) == UNSUPPORTED, over
    assert sel(E=0, pairs=None, src=None, tgt=None, valid=None) == 0        # nothing to select, nothing launched
    term = lambda pc=d, src=d, tgt=d, valid=d, T=9, N=512, E=7, k=10, loss=d, ws=d, nbytes=big: \
        L.reart_connection_term(pc, src, tgt, valid, T, N, E, k, 1.0, loss, None, None, ws, nbytes, None)
    for bad in (dict(pc=None), dict(src=None), dict(tgt=None), dict(valid=None), dict(loss=None), dict(T=0), dict(N=0),
                dict(E=-1), dict(k=0), dict(ws=None), dict(nbytes=L.reart_connection_term_workspace_bytes(9, 512, 7, 10) - 1)):
        assert term(**bad) == INVALID_ARG, bad
    for over in (dict(T=1025), dict(N=65537), dict(E=4097), dict(k=65)):
        assert term(**over) == UNSUPPORTED, over


def test_interface_errors():
    from reart_amd.networks.loss import ConnectionTerm

    cano, seg, pc = torch.zeros(8, 3), torch.zeros(8, dtype=torch.long), torch.zeros(2, 8, 3)
    edges = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(TypeError):
        ConnectionTerm(edges)(cano.double(), seg, pc)
    with pytest.raises(TypeError):
        ConnectionTerm(edges)(cano, seg, pc.double())
    with pytest.raises(TypeError):
        ConnectionTerm(edges)(cano, seg.float(), pc)
    for bad in ((cano[:, :2], seg, pc), (cano, seg[:7], pc), (cano, seg, pc[:, :7]), (cano, seg, pc[0])):
        with pytest.raises(ValueError):
            ConnectionTerm(edges)(*bad)
    with pytest.raises(ValueError):
        ConnectionTerm(torch.tensor([[-1, 2]]))(cano, seg, pc)
    with pytest.raises(ValueError):
        ConnectionTerm(edges, num_parts=2)(cano, seg, pc)
    with pytest.raises(ValueError):
        ConnectionTerm(edges, num_parts=2).select(cano, seg)
    # the limits come before anything is launched, hence before the device is asked for
    with pytest.raises(NotImplementedError, match="64"):
        ConnectionTerm(torch.tensor([[0, 64]]))(cano, seg, pc)
    with pytest.raises(NotImplementedError, match="4096"):
        ConnectionTerm(torch.tensor([[0, 1]] * 4097))(cano, seg, pc)
    with pytest.raises(NotImplementedError, match="k = 65"):
        ConnectionTerm(edges, k=65)(cano, seg, pc)
    with pytest.raises(NotImplementedError, match="k = 0"):
        ConnectionTerm(edges, k=0)(cano, seg, pc)
    with pytest.raises(NotImplementedError, match="1024"):
        ConnectionTerm(edges)(cano, seg, torch.zeros(1025, 8, 3))
    with pytest.raises(NotImplementedError, match="65536"):
        ConnectionTerm(edges)(torch.zeros(65537, 3), torch.zeros(65537, dtype=torch.long), torch.zeros(1, 65537, 3))
    with pytest.raises(NotImplementedError, match="65536"):
        ConnectionTerm(edges).select(torch.zeros(65537, 3), torch.zeros(65537, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ConnectionTerm(edges)(cano, seg, pc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ConnectionTerm(edges)(cano, seg.int(), pc)                          # labels of another integer dtype are cast
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ConnectionTerm(edges).select(cano, seg)
    with pytest.raises(RuntimeError, match="select"):
        ConnectionTerm(edges)(pc)                                           # no kept tables
    assert ConnectionTerm(edges).last is None and ConnectionTerm([]).num_parts == 1 and ConnectionTerm(edges).num_parts == 3
