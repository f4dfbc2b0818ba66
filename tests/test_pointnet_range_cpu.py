"""The case tables of tests/pointnet_range_ref.py hold what tests/test_pointnet_range_gpu.py relies on (no GPU): the
restated kernel choice is the launcher's, the layer table reaches every kernel instantiation, sub-path and input form, the
derived bound separates an honest float32 layer from three planted errors, and the ball, 3-NN and matching inputs are
well defined in float32.  Removing a case from a table fails a coverage assertion here."""
import numpy as np
import pytest
import torch

from tests import pointnet_range_ref as R


def test_pick_is_the_launchers_choice():
    from reart_amd import _lib

    L = _lib.lib()
    for Cin in (1, 3, 7, 8, 9, 15, 16, 17, 131, 515):
        for Cout in list(range(1, 260)) + [511, 512]:
            for pool_k in (0, 1, 2, 16, 24, 31, 32, 33, 64, 100, 128, 129, 130, 384, 1000):
                NB, BK, ANY = R.pick(Cin, Cout, pool_k)
                assert L.reart_mlp_layer_kernel(Cin, Cout, pool_k) == NB | (BK << 8) | (int(ANY) << 16), (Cin, Cout, pool_k)
    assert L.reart_mlp_layer_kernel(0, 8, 0) == 0 and L.reart_mlp_layer_kernel(8, 0, 0) == 0 and L.reart_mlp_layer_kernel(8, 8, -1) == 0
    assert {R.pick(ci, co, pk) for ci in (8, 9) for co in (32, 64, 96, 224, 256) for pk in (0, 24)} == set(R.TRIPLES)


def test_layer_table_coverage():
    cases = R.LAYER_CASES
    assert len(cases) <= 70 and all(c.rows <= 4000 for c in cases)
    picks = [R.pick(c.Cin, c.Cout, c.pool_k) for c in cases]
    assert set(picks) == set(R.TRIPLES) and len(R.TRIPLES) == 16
    for nb in (1, 2, 3, 7):
        pools = {c.pool_k for c, p in zip(cases, picks) if p[0] == nb and p[2]}
        small, large = {k for k in pools if k <= 128}, {k for k in pools if k > 128}
        assert 2 in small and any(128 % k for k in small), (nb, pools)            # whole groups inside a tile
        assert any(k % 128 and (k % 128) % 16 for k in large), (nb, pools)        # a short last chunk, no multiple of 16
    assert {24, 100, 2, 130, 200, 1000, 384} <= {c.pool_k for c in cases}
    assert {32, 64, 128, 1} <= {c.pool_k for c in cases}
    assert {1, 127, 128, 129, 300} <= {c.rows for c in cases if c.pool_k == 0}
    assert {1, 3, 8, 9, 16, 17, 131} <= {c.Cin for c in cases}
    assert {1, 32, 33, 64, 65, 96, 100, 193, 224, 225, 256} <= {c.Cout for c in cases}
    assert any(not c.relu and c.pool_k > 1 and p[2] and c.pool_k <= 128 for c, p in zip(cases, picks))
    assert any(not c.relu and c.pool_k > 128 for c in cases) and any(not c.relu and c.pool_k in (32, 64, 128) for c in cases)
    for c in cases:
        if c.pool_k > 1:
            assert c.rows % c.pool_k == 0
    # every input form at both K steps
    assert {(c.form, p[1]) for c, p in zip(cases, picks)} == {(f, bk) for f in ("plain", "strided", "gather_fx", "gather_xf")
                                                              for bk in (8, 16)}
    strided = [c for c in cases if c.form == "strided"]
    assert {c.opt["off"] for c in strided} == {0, 1, 2, 3} and any(c.opt["ldx"] % 2 for c in strided)
    assert all(c.opt["ldx"] > c.Cin for c in strided) and any(not c.opt["bias"] for c in strided)
    for c in strided:
        if c.opt["ldx"] % 2:                                                   # aligned and unaligned rows in one call
            al = {(c.opt["off"] + r * c.opt["ldx"]) % 4 == 0 for r in range(c.rows)}
            assert al == {True, False}
    for form in ("gather_fx", "gather_xf"):
        g = [c for c in cases if c.form == form]
        assert {c.opt["D"] for c in g} == {0, 1, 4, 5, 12, 131}, form
        assert {c.opt["centres"] for c in g} == {True, False}, form
        assert all(c.pool_k > 1 and c.rows == c.opt["B"] * c.opt["S"] * c.pool_k and c.Cin == c.opt["D"] + 3 for c in g)
        assert any(c.opt["B"] > 1 and c.opt["S"] > 1 for c in g)
    # relu off with pooling: the maxima it is there for are negative
    for i, c in enumerate(cases):
        if not c.relu and c.pool_k > 1 and R.layer_data(i)["b"] is not None:
            assert (R.layer_ref(i)[0] < 0).any(), i


def test_bound_separates_honest_float32_from_planted_errors():
    caught = {f: [] for f in R.FAULTS}
    for i, c in enumerate(R.LAYER_CASES):
        ref, bound = R.layer_ref(i)
        assert ref.shape == bound.shape == (R.out_rows(c), c.Cout) and (bound >= 0).all()
        assert R.layer_ratio(i, R.layer_emulate(i)) <= 1.0, (i, c)            # np.float32 matmul: inside on every case
        for f in R.FAULTS:
            if R.layer_ratio(i, R.layer_emulate(i, f)) > 1.0:
                caught[f].append(R.pick(c.Cin, c.Cout, c.pool_k))
    assert {p[0] for p in caught["bias32"]} == {2, 3, 7}                      # every NB that has an accumulator n >= 1
    assert {p[1] for p in caught["drop_k"]} == {8, 16}
    assert {p[0] for p in caught["live128"]} == {1, 2, 3, 7}                  # the large-group path of every NB


def test_ball_cases_are_well_defined_and_cover_the_exits(oracle):
    assert {c.N for c in R.BALL_CASES} == {1, 63, 64, 65, 129, 700}
    assert {c.nsample for c in R.BALL_CASES} == {1, 2, 64, 65, 200} and {c.S for c in R.BALL_CASES} == {1, 3, 5, 130}
    assert any(c.nsample > c.N for c in R.BALL_CASES) and any(c.nsample == c.N for c in R.BALL_CASES)
    seen = np.zeros(3, int)
    for i, c in enumerate(R.BALL_CASES):
        xyz, ctr = R.ball_data(i)
        count, empty, over, exact, rel = R.ball_classes(i)
        assert rel > 0.15, (c, rel)
        for cuda_mode in (False, True):                                        # the margin in each rule set's own float32 distance
            _, mg = oracle.ball_query(R.BALL_RADIUS, c.nsample, xyz, ctr, cuda_mode=cuda_mode, want_margin=True)
            assert mg.min() > R.BALL_MARGIN, (c, cuda_mode, mg.min())
        assert empty.any(), c
        assert exact.any() == (R.ball_step_index(c.nsample) < c.N), c         # wherever the cloud is long enough
        assert over.any() == (c.N > c.nsample), c                              # wherever the cloud has more points than slots
        assert ((count > 0) & (count < c.nsample)).any() == (c.nsample > 1 and (c.N > c.nsample + 2 or c.N < c.nsample)), c
        seen += [empty.any(), exact.any(), over.any()]
    assert (seen >= [len(R.BALL_CASES), 8, 8]).all(), seen                    # each kind in at least half of the cases


def test_tnn_cases_hold_their_structure(oracle):
    assert {c.S2 for c in R.TNN_CASES} == {3, 4, 1023, 1024, 1025, 2048, 2049} and {c.N for c in R.TNN_CASES} == {1, 255, 256, 257}
    assert {c.D for c in R.TNN_CASES} == {1, 256, 257} and {c.B for c in R.TNN_CASES} == {1, 3}
    negative = 0
    for i, c in enumerate(R.TNN_CASES):
        fine, coarse, pts = R.tnn_data(i)
        assert fine.shape == (c.B, c.N, 3) and coarse.shape == (c.B, c.S2, 3) and pts.shape == (c.B, c.S2, c.D)
        d, idx = oracle.three_nn_expanded(fine, coarse)
        for b in range(c.B):
            small, large = (coarse[b], fine[b]) if c.N >= c.S2 else (fine[b], coarse[b])
            assert all((large == p).all(1).any() for p in small)              # a subset, coordinate for coordinate
            uniq, cnt = np.unique(coarse[b], axis=0, return_counts=True)
            assert (cnt == 2).sum() == 1 and cnt.max() == 2                    # one coarse point stored twice
            twice = uniq[cnt == 2][0]
            q = np.nonzero((fine[b] == twice).all(1))[0]
            assert len(q) >= 1                                                 # ... and it is a fine point: a tie of two "zeros"
            copies = np.nonzero((coarse[b] == twice).all(1))[0]
            assert list(idx[b, q[0], :2]) == list(copies) and d[b, q[0], 0] == d[b, q[0], 1]
        assert np.abs(d[..., 0]).max() < 1e-5 if c.N <= c.S2 else np.abs(d[..., 0]).min() < 1e-5
        negative += int((d < 0).any())
    assert negative >= 3                                                       # the "zero" distances come out negative too


def test_smnn_cases_are_admitted_and_planted():
    assert {(c.N1, c.N2) for c in R.SMNN_CASES} == {(2, 2), (63, 65), (64, 64), (65, 130), (300, 77)}
    assert {c.E for c in R.SMNN_CASES} == {1, 3} and {c.th for c in R.SMNN_CASES} == {0.9, 0.5, -1.0} and len(R.SMNN_CASES) == 30
    for i, c in enumerate(R.SMNN_CASES):
        d1, d2, plants, keep, tgt, margin = R.smnn_data(i)
        assert margin >= R.SMNN_MARGIN, (c, margin)
        assert d1.shape == (c.E, c.N1, 64) and d2.shape == (c.E, c.N2, 64)
        for e, (p, i2, j, j2) in enumerate(plants):
            assert (d2[e, j] == d2[e, j2]).all() and j != j2 and (d1[e, i2] == d2[e, j]).all() and i2 != p
            assert tgt[e, p] == min(j, j2) and tgt[e, i2] == min(j, j2)       # the tie goes to the lower index
            assert not keep[e, p]                                              # ratio 1 fails a test; mutual goes to i2
            assert keep[e, i2] == (c.th < 0)                                   # 0 / 0: rejected under a ratio test only
        if c.N1 >= 63:
            assert keep.sum() >= c.E * 10, (c, keep.sum())                     # the correlated rows do match
    # the same answer from the oracle's matcher where both apply (E = 1 slices, ratio tests)
    import oracle as O

    for i, c in enumerate(R.SMNN_CASES):
        if c.th > 0 and c.N1 == 300:
            d1, d2, _, keep, tgt, _ = R.smnn_data(i)
            pairs = O.match_smnn(d1[0], d2[0], c.th)[0]
            rows = np.nonzero(keep[0])[0]
            np.testing.assert_array_equal(pairs, np.stack([rows, tgt[0][rows]], 1))


WRAPPER_ARGS = {
    # name -> (leading ints, tensors as (kind, shape)); kind f = float32, i = int32 index
    "furthest_point_sampling_wrapper": ((2, 50, 8), [("f", (2, 50, 3)), ("f", (2, 50)), ("i", (2, 8))]),
    "ball_query_wrapper": ((2, 50, 8, 0.3, 4), [("f", (2, 8, 3)), ("f", (2, 50, 3)), ("i", (2, 8, 4))]),
    "three_nn_wrapper": ((2, 50, 8), [("f", (2, 50, 3)), ("f", (2, 8, 3)), ("f", (2, 50, 3)), ("i", (2, 50, 3))]),
    "knn_wrapper": ((2, 50, 8, 4), [("f", (2, 50, 3)), ("f", (2, 8, 3)), ("f", (2, 50, 4)), ("i", (2, 50, 4))]),
    "gather_points_wrapper": ((2, 5, 50, 8), [("f", (2, 5, 50)), ("i", (2, 8)), ("f", (2, 5, 8))]),
    "gather_points_grad_wrapper": ((2, 5, 50, 8), [("f", (2, 5, 8)), ("i", (2, 8)), ("f", (2, 5, 50))]),
    "group_points_wrapper": ((2, 5, 50, 8, 4), [("f", (2, 5, 50)), ("i", (2, 8, 4)), ("f", (2, 5, 8, 4))]),
    "group_points_grad_wrapper": ((2, 5, 50, 8, 4), [("f", (2, 5, 8, 4)), ("i", (2, 8, 4)), ("f", (2, 5, 50))]),
    "three_interpolate_wrapper": ((2, 5, 8, 50), [("f", (2, 5, 8)), ("i", (2, 50, 3)), ("f", (2, 50, 3)), ("f", (2, 5, 50))]),
    "three_interpolate_grad_wrapper": ((2, 5, 50, 8), [("f", (2, 5, 50)), ("i", (2, 50, 3)), ("f", (2, 50, 3)), ("f", (2, 5, 8))]),
}


def _wrapper_tensors(spec, wrong=None, how=None):
    out = []
    for n, (kind, shape) in enumerate(spec):
        t_ = torch.zeros(shape, dtype=torch.float32 if kind == "f" else torch.int32)
        if n == wrong:
            if how == "dtype":
                t_ = t_.to(torch.int64 if kind == "i" else torch.float64)
            else:
                t_ = torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=t_.dtype)[..., ::2]
        out.append(t_)
    return out


@pytest.mark.parametrize("name", sorted(WRAPPER_ARGS))
def test_pointnet2_cuda_wrappers_refuse_before_any_launch(name):
    """Every wrapper refuses a wrong dtype (an int64 index tensor first of all) and a strided tensor with RuntimeError, as the
    reference's CHECK_INPUT does, before the device is looked at: host tensors get that far and no further, so nothing
    here can reach a kernel.  Well-formed host tensors are refused for their device."""
    from reart_amd import _lib
    from reart_amd import pointnet2_cuda as pc

    ints, spec = WRAPPER_ARGS[name]
    fn = getattr(pc, name)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        fn(*ints, *_wrapper_tensors(spec))
    for n, (kind, shape) in enumerate(spec):
        with pytest.raises(RuntimeError, match="int32" if kind == "i" else "float32"):
            fn(*ints, *_wrapper_tensors(spec, n, "dtype"))
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(*ints, *_wrapper_tensors(spec, n, "stride"))
    if name == "furthest_point_sampling_wrapper":                              # the path above the LDS limit checks ``temp`` too
        n_big = _lib.FPS_MAX_N_LDS + 1
        spec_big = [("f", (1, n_big, 3)), ("f", (1, n_big)), ("i", (1, 8))]
        for n, (kind, _) in enumerate(spec_big):
            with pytest.raises(RuntimeError, match="int32" if kind == "i" else "float32"):
                fn(1, n_big, 8, *_wrapper_tensors(spec_big, n, "dtype"))
            with pytest.raises(RuntimeError, match="contiguous"):
                fn(1, n_big, 8, *_wrapper_tensors(spec_big, n, "stride"))
