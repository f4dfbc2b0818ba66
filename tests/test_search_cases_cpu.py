"""The hostile cases of tests/search_cases.py do what their table says, and the claim the pruned searches rest on --
``lower_bound(q, box) <= distance(q, t)`` in float32 for every target t of the box (csrc/prune.hip, "Exactness") -- holds
on exactly the numbers that could break it: ties, zero extents, 1e22, quantised coordinates, denormal squares.  No GPU."""
import numpy as np
import pytest

from tests import search_cases as sc

TIED = ("lattice", "tiny70", "offset")


def _big(name):
    return sc.case(name)[1].shape[0] >= 1000


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("name", sc.NAMES)
def test_the_two_references_agree(oracle, name, K):
    """oracle.knn_points (C) and brute (numpy, stable sort) give the same distances and indices at these inputs."""
    q, t = sc.case(name)
    d_ref, i_ref = oracle.knn_points(q[None], t[None], K=K)
    d, i = sc.brute(q, t, K)
    np.testing.assert_array_equal(i, i_ref[0])
    np.testing.assert_array_equal(d, d_ref[0])


@pytest.mark.parametrize("name", sc.NAMES)
def test_the_bound_never_exceeds_a_distance(name):
    """Zero (query, box, target) triples with lower_bound > distance, both ways round (every entry searches both)."""
    q, t = sc.case(name)
    v = sc.violations(q, t), sc.violations(t, q)
    print(f"{name}: P1 {q.shape[0]} P2 {t.shape[0]} violations of lb <= d: {v[0]} (x -> y), {v[1]} (y -> x)")
    assert v == (0, 0)


@pytest.mark.parametrize("name", sc.NAMES)
def test_the_case_is_what_its_row_says(name):
    q, t = sc.case(name)
    tie = {K: sc.tie_fraction(q, t, K) for K in (1, 3)}
    pr = {K: sc.prunable(q, t, K) for K in (1, 3)}
    print(f"{name}: P1 {q.shape[0]} P2 {t.shape[0]} tie share {tie[1]:.3f} (K=1) {tie[3]:.3f} (K=3), "
          f"prunable share {pr[1]:.3f} (K=1) {pr[3]:.3f} (K=3)")
    if name in TIED:
        assert tie[1] >= 0.4 and tie[3] >= 0.8
    if name == "coincident":
        assert tie[1] == 1.0 and tie[3] == 1.0 and pr[1] == 0.0 and pr[3] == 0.0
    elif _big(name):
        assert pr[1] >= 0.7 and pr[3] >= 0.7


def test_sizes_sit_on_the_structural_edges():
    """What the table promises about the sizes: no case beyond 4112 points, the first four cases' sizes, one past the
    multiples, a second coarse round of exactly one box at S = 4, and both clouds in k-d leaf order already."""
    import torch

    from reart_amd.relax import kd_order

    shapes = {n: (sc.case(n)[0].shape[0], sc.case(n)[1].shape[0]) for n in sc.NAMES}
    assert max(max(s) for s in shapes.values()) == 4112
    assert shapes["lattice"] == (922, 1728) and shapes["sphere"] == (650, 3000) and shapes["cluster"] == (800, 2100)
    assert shapes["sheet"] == (700, 2500) and shapes["line"] == (513, 1025) and shapes["coincident"] == (130, 300)
    assert shapes["jump"] == (1000, 4112) and (4112 + 15) // 16 == 4 * 64 + 1
    assert sorted(s[1] for n, s in shapes.items() if n.startswith("small_")) == [1, 2, 3, 8, 9, 16, 17, 63, 129, 193]
    assert {s[0] for n, s in shapes.items() if n.startswith("small_")} == {1, 3, 64, 65}
    for n in sc.NAMES:
        for c in sc.case(n):
            assert c.dtype == np.float32 and np.isfinite(c).all()
            np.testing.assert_array_equal(c[kd_order(torch.tensor(c)).numpy()], c, err_msg=n)
    q, t = sc.case("sheet")
    assert not t[:, 2].any()
    q, t = sc.case("line")
    assert not t[:, 1:].any()
    q, t = sc.case("coincident")
    assert (t == t[0]).all()
    q, t = sc.case("tiny70")
    d = sc.sqdist(q, t)
    assert d.max() < 1024 * np.float32(2.0 ** -149)          # denormal squares: fewer than 1024 values for 10^6 pairs
    q, t = sc.case("tiny60")
    assert np.median(sc.sqdist(q, t)) > np.finfo(np.float32).tiny
    q, t = sc.case("big")
    assert 1e21 < np.median(sc.sqdist(q, t)) < 1e24
    assert not np.array_equal(sc.case("jump", seed=1)[1], sc.case("jump")[1])
