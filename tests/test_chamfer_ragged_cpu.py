"""The reference statements the GPU tests of the ragged warm Chamfer operators lean on (tests/chamfer_ragged_ref.py), held
to the brute-force contract with lengths (oracle.knn_points) and to the reference's own compute_chamfer_list on lists of
frames of differing lengths (tests/golden/chamfer_ragged.npz).  Host only."""
import importlib.util
import os

import numpy as np
import pytest

from tests import chamfer_ragged_ref as rref

HERE = os.path.dirname(os.path.abspath(__file__))


def _maker():
    spec = importlib.util.spec_from_file_location("make_golden_chamfer_ragged",
                                                  os.path.join(HERE, "golden", "make_golden_chamfer_ragged.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MAKER = _maker()
GOLDEN = np.load(os.path.join(HERE, "golden", "chamfer_ragged.npz"))


@pytest.mark.parametrize("fill", [0.0, np.nan])
@pytest.mark.parametrize("name", sorted(rref.CASES))
def test_helper_equals_the_contract_with_lengths(oracle, name, fill):
    """Distances and indices of both directions, live and padding rows, bit for bit -- whatever the padding rows hold."""
    x, y, lx, ly = rref.make_case(name, fill)
    for a, b, la, lb in ((x, y, lx, ly), (y, x, ly, lx)):
        d, i = rref.knn_ragged(a, b, la, lb)
        dw, iw = oracle.knn_points(a, b, np.array(la), np.array(lb), K=1)
        np.testing.assert_array_equal(i, iw[..., 0])
        np.testing.assert_array_equal(d, dw[..., 0])
        for n in range(a.shape[0]):      # padding rows, and every row against an empty cloud
            assert not d[n, la[n]:].any() and not i[n, la[n]:].any()
            if lb[n] == 0:
                assert not d[n].any() and not i[n].any()


def test_fixture_is_the_scripts():
    """The stored frames are the ones the script draws, with lengths between 1 and 300 that differ inside every list."""
    assert int(GOLDEN["n_lists"]) == len(MAKER.LISTS) >= 3
    for k in range(int(GOLDEN["n_lists"])):
        a, b = MAKER.frames(GOLDEN, k)
        wa, wb = MAKER.make_list(k)
        assert len(a) == len(wa) and len(b) == len(wb) == len(a)
        for got, want in zip(a + b, wa + wb):
            np.testing.assert_array_equal(got, want)
        for frames in (a, b):
            lens = [f.shape[0] for f in frames]
            assert min(lens) >= 1 and max(lens) <= 300 and len(set(lens)) > 1


@pytest.mark.parametrize("reduction", ["sum", "mean", "none"])
def test_frame_formula_equals_the_reference(reduction):
    """float64 brute force against the reference's float64 KD-tree: 1e-9 relative."""
    for k in range(int(GOLDEN["n_lists"])):
        a, b = MAKER.frames(GOLDEN, k)
        got = rref.frame_formula(a, b, reduction)
        want = GOLDEN[f"L{k}_{reduction}"]
        assert np.shape(got) == want.shape
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)


def test_trimmed_gradients_land_in_the_live_rows():
    """The per-element gradient helper: live rows are the dense reference on the trimmed clouds, everything else is zero."""
    from tests import chamfer_loss_ref

    x, y, lx, ly = rref.make_case("A")
    d_xy, i_xy = rref.knn_ragged(x, y, lx, ly)
    d_yx, i_yx = rref.knn_ragged(y, x, ly, lx)
    g = rref.gradients(x, y, lx, ly, i_xy, i_yx)
    for n in range(x.shape[0]):
        assert not g["x"]["grad"][n, lx[n]:].any() and not g["y"]["grad"][n, ly[n]:].any()
        if lx[n] == 0 or ly[n] == 0:
            assert not g["x"]["grad"][n].any() and not g["y"]["grad"][n].any()
            continue
        want = chamfer_loss_ref.gradients(x[n:n + 1, :lx[n]], y[n:n + 1, :ly[n]], i_xy[n:n + 1, :lx[n]], i_yx[n:n + 1, :ly[n]])
        np.testing.assert_array_equal(g["x"]["grad"][n, :lx[n]], want["x"]["grad"][0])
        np.testing.assert_array_equal(g["y"]["cnt"][n, :ly[n]], want["y"]["cnt"][0])
    assert rref.loss(d_xy, d_yx, lx, ly) == np.float32(np.float64(d_xy.astype(np.float64).sum()) + d_yx.astype(np.float64).sum())
