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


# ---- the large cases (search_cases.LARGE) -----------------------------------------------------------------------------
def _sampled(name, swapped=False):
    """(the sampled rows, those queries, all targets) of one large case, one way round."""
    q, t = sc.large_case(name)[::-1] if swapped else sc.large_case(name)
    rows = sc.sample(q.shape[0])
    assert rows.shape[0] * t.shape[0] <= sc.MAX_ENTRIES
    return rows, q[rows], t


@pytest.mark.parametrize("name", sc.LARGE_NAMES)
def test_large_the_two_references_agree(oracle, name):
    """On 512 sampled queries of every large case, both ways round: oracle.knn_points equals a stable sort of the float32
    distance rows (`brute`), and so does the chunked form (`brute_chunked`), K = 1 and 3."""
    for swapped in (False, True):
        rows, q, t = _sampled(name, swapped)
        sorted3, chunked3 = sc.brute(q, t, 3), sc.brute_chunked(q, t, 3)      # K = 1 is the first column of the same sort
        for K in (1, 3):
            d_ref, i_ref = oracle.knn_points(q[None], t[None], K=K)
            n = min(K, t.shape[0])
            for d, i in (sorted3, chunked3):
                np.testing.assert_array_equal(i[:, :n], i_ref[0][:, :n])
                np.testing.assert_array_equal(d[:, :n], d_ref[0][:, :n])


@pytest.mark.parametrize("name", sc.LARGE_NAMES)
def test_large_the_bound_never_exceeds_a_distance(name):
    """Zero (query, box, target) triples with lower_bound > distance on the sampled queries, both ways round."""
    v = []
    for swapped in (False, True):
        rows, q, t = _sampled(name, swapped)
        v.append(sc.violations(q, t))
        assert sc.violations_chunked(q, t) == v[-1]
    print(f"{name}: violations of lb <= d on the sample: {v[0]} (x -> y), {v[1]} (y -> x)")
    assert v == [0, 0]


def test_large_cases_are_what_their_rows_say(oracle):
    """Sizes, storage order, coarse rounds, ties where the row promises them and none at all in `scan70k`."""
    import torch

    from reart_amd.relax import kd_order

    shapes = {n: (sc.large_case(n)[0].shape[0], sc.large_case(n)[1].shape[0]) for n in sc.LARGE_NAMES}
    assert shapes == {"round3": (1000, 8208), "coincident8k": (130, 8208), "lattice27k": (6313, 27000),
                      "scan70k": (70000, 70000), "fanin70k": (70000, 8)}
    assert sc.NAMES == tuple(n for n in sc.NAMES if n not in sc.LARGE) and len(sc.NAMES) == 21
    for n in sc.LARGE_NAMES:
        for c in sc.large_case(n):
            assert c.dtype == np.float32 and np.isfinite(c).all() and not c.flags.writeable
            np.testing.assert_array_equal(c[kd_order(torch.tensor(c)).numpy()], c, err_msg=n)
    # boxes and coarse rounds of 64 S boxes
    for n in sc.ROUNDS3:
        (nbox, r1), (_, r4) = (sc.coarse_rounds(shapes[n][1], S) for S in (1, 4))
        print(f"{n}: {nbox} boxes, {r1} coarse rounds at S = 1, {r4} at S = 4")
        assert r1 >= 3 and r4 >= 3
    assert sc.coarse_rounds(8208, 4) == (2 * 256 + 1, 3) and sc.coarse_rounds(8208, 1) == (513, 9)
    assert sc.coarse_rounds(27000, 4) == (1688, 7) and sc.coarse_rounds(70000, 4) == (4375, 18)
    assert sc.coarse_rounds(70000, 4)[0] > 4096 and 70000 > 65536
    # a cold wave evaluates every target for its 64 queries: more than 2^20 evaluations from 16 384 targets per slice on
    assert 64 * (70000 // 4) > 2 ** 20 and 64 * 70000 > 2 ** 20 and 64 * (8208 // 1) < 2 ** 20
    assert sc.coarse_rounds(12304, 3) == (769, 5) and sc.coarse_rounds(12304, 1) == (769, 13)
    # ties
    q, t = sc.large_case("coincident8k")
    assert (t == t[0]).all()
    for n, K in (("lattice27k", 1), ("lattice27k", 3), ("coincident8k", 1), ("coincident8k", 3)):
        rows, q, t = _sampled(n)
        share = sc.tie_fraction_chunked(q, t, K)
        assert share == sc.tie_fraction(q, t, K)
        print(f"{n}: share of the sampled queries with a tied K-th distance, K = {K}: {share:.3f}")
        assert share == 1.0 if n == "coincident8k" else share > 0.3
    # scan70k: every query of both directions has four different nearest distances, so an exact search returns the
    # oracle's indices in every slot, whatever its storage order
    q, t = sc.large_case("scan70k")
    for a, b in ((q, t), (t, q)):
        d, i = oracle.knn_points(a[None], b[None], K=4)
        assert (d[0][:, 1:] > d[0][:, :-1]).all()
        assert i.min() >= 0 and i.max() > 65535
    # fanin70k: every one of the 70 000 points has the same nearest target
    q, t = sc.large_case("fanin70k")
    assert len(set(oracle.knn_points(q[None], t[None], K=1)[1].ravel().tolist())) == 1
    for a, b in zip(sc.large_case("scan70k", seed=1), sc.large_case("scan70k")):      # another seed, another instance
        assert a.shape == b.shape and not np.array_equal(a, b)


def _search_cloud_lds(Ppad, waves, wave_bytes):
    """csrc/prune.hip, search_cloud_lds: bytes of the cloud-resident form (the SoA cloud, 8 floats per box of 16, the waves'
    own space, 256) or 0 when they exceed 152 KiB."""
    need = (3 * Ppad + 8 * (Ppad // sc.BOX)) * 4 + waves * wave_bytes + 256
    return need if need <= 152 * 1024 else 0


def test_plan_arithmetic_of_the_cloud_resident_form():
    """The resident form takes 14 Ppad + 57 600 bytes (16 waves of 3584 bytes and 256): 6992 targets are the last size that
    fits 152 KiB, 7008 (the next multiple of 16) the first that does not -- the two sizes, beside 6704 and 6720, at which
    tests/test_search_large_gpu.py runs the engine.  The constants are read from the source, so that a change there shows
    here."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reart_amd", "csrc", "prune.hip")).read()
    waves = int(re.search(r"#define PC_WAVES (\d+)", src).group(1))
    qcap = int(re.search(r"#define PC_QCAP (\d+)", src).group(1))
    assert int(re.search(r"need <= (\d+) \* 1024", src).group(1)) == 152
    wave_bytes = 64 * 16 + 3 * 64 * 8 + qcap * 4          # a wave's queries | result slots | queue (PC_WAVE_BYTES)
    assert waves * wave_bytes + 256 == 57600
    for Ppad in (6704, 6720, 6992):
        assert _search_cloud_lds(Ppad, waves, wave_bytes) == 14 * Ppad + 57600 <= 152 * 1024
    assert _search_cloud_lds(6992, waves, wave_bytes) == 155488
    assert _search_cloud_lds(7008, waves, wave_bytes) == 0 and 14 * 7008 + 57600 > 152 * 1024
