"""GPU: the PointNet++ layer kernel, ball query, 3-NN interpolation and the descriptor matching over the tables of
tests/pointnet_range_ref.py -- the layer inside its derived float64 bound on every element, the other three equal to their
references in every element.  ``-s`` shows the worst error / bound of the layer cases per kernel instantiation."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from tests import pointnet_range_ref as R

pytestmark = pytest.mark.gpu

CANARY = -7.0
RATIOS = {}          # (NB, BK, ANY) -> worst |kernel - f64| / bound seen


def t(a, dev):
    return None if a is None else torch.tensor(np.asarray(a), device=dev)     # a copy: the shared inputs are read-only


def _run_layer(i, dev):
    """Case i into columns 3 .. 3 + Cout of a canary-filled matrix that is two rows longer and five columns wider."""
    from reart_amd import _lib
    from reart_amd.networks.feature_extractor import mlp_layer

    c, d = R.LAYER_CASES[i], R.layer_data(i)
    out = torch.full((R.out_rows(c) + 2, c.Cout + 5), CANARY, device=dev)
    W, b = t(d["W"], dev), t(d["b"], dev)
    if c.form == "plain":
        mlp_layer(t(d["X"], dev), W, b, relu=c.relu, pool_k=c.pool_k, out=out, out_col=3)
    elif c.form == "strided":
        buf = t(d["buf"], dev)
        assert buf.data_ptr() % 16 == 0
        rc = _lib.lib().reart_mlp_layer(c_void_p(buf.data_ptr() + 4 * c.opt["off"]), c.opt["ldx"], None, 0, 0, 0, None, 0, None, None,
                                        0, _lib.ptr(W), _lib.ptr(b), c.rows, c.Cin, c.Cout, int(c.relu), c.pool_k,
                                        _lib.ptr(out), out.shape[1], 3, _lib.stream())
        _lib.check(rc, "reart_mlp_layer")
        torch.cuda.synchronize()                                               # ``buf`` stays alive until the kernel is done
    else:
        gather = dict(idx=t(d["idx"], dev), F=t(d["F"], dev), Q=t(d["Q"], dev), C=t(d["C"], dev), Npts=c.opt["Npts"],
                      xyz_first=int(c.form == "gather_xf"))
        mlp_layer(None, W, b, relu=c.relu, pool_k=c.pool_k, out=out, out_col=3, gather=gather)
    return out.cpu().numpy()


@pytest.mark.parametrize("i", range(len(R.LAYER_CASES)), ids=lambda i: "%d-%dx%dx%d-k%d-%s" % ((i,) + tuple(R.LAYER_CASES[i][:4]) + (R.LAYER_CASES[i].form,)))
def test_layer_inside_the_derived_bound(dev, i):
    c = R.LAYER_CASES[i]
    ref, bound = R.layer_ref(i)
    full = _run_layer(i, dev)
    n, got = R.out_rows(c), full[:R.out_rows(c), 3:3 + c.Cout]
    assert (full[:, :3] == CANARY).all() and (full[:, 3 + c.Cout:] == CANARY).all() and (full[n:] == CANARY).all()
    ratio = R.layer_ratio(i, got)
    key = R.pick(c.Cin, c.Cout, c.pool_k)
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print("layer case %d %s %s: worst |kernel - f64| / bound = %.4f" % (i, tuple(c[:6]), key, ratio))
    bad = np.argwhere(np.abs(got.astype(np.float64) - ref) > bound)
    assert len(bad) == 0, (c, key, ratio, bad[:5])
    assert np.array_equal(_run_layer(i, dev).view(np.uint32), full.view(np.uint32))          # two runs, the same bits


def test_layer_ratio_report(dev):
    """The figures of the README's table: worst error / bound per (NB, BK, ANY) over the cases that ran before this one."""
    for key in sorted(RATIOS):
        print("mlp_gemm_kernel<%d, %d, %s>: worst |kernel - f64| / bound = %.4f" % (key[0], key[1], str(key[2]).lower(), RATIOS[key]))
    assert not RATIOS or max(RATIOS.values()) <= 1.0


@pytest.mark.parametrize("cuda_mode", [False, True])
@pytest.mark.parametrize("i", range(len(R.BALL_CASES)), ids=lambda i: "N%d-k%d-S%d" % tuple(R.BALL_CASES[i]))
def test_ball_query_every_element(oracle, dev, i, cuda_mode):
    from reart_amd.networks.pointnet2_utils import query_ball_point

    c = R.BALL_CASES[i]
    xyz, ctr = R.ball_data(i)
    ref = oracle.ball_query(R.BALL_RADIUS, c.nsample, xyz, ctr, cuda_mode=cuda_mode)
    got = query_ball_point(R.BALL_RADIUS, c.nsample, t(xyz, dev), t(ctr, dev), cuda_mode=cuda_mode)
    np.testing.assert_array_equal(got.cpu().numpy(), ref)


@pytest.mark.parametrize("i", range(len(R.TNN_CASES)), ids=lambda i: "B%d-N%d-S%d-D%d" % tuple(R.TNN_CASES[i]))
def test_three_nn_interpolation_every_bit(oracle, dev, i):
    from reart_amd import _lib
    from reart_amd.networks.feature_extractor import three_interpolate

    c = R.TNN_CASES[i]
    fine, coarse, pts = R.tnn_data(i)
    x1, x2 = t(fine, dev), t(coarse, dev)
    dist = torch.full((c.B, c.N, 3), CANARY, device=dev)
    idx = torch.full((c.B, c.N, 3), -1, dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().reart_three_nn(_lib.ptr(x1), _lib.ptr(x2), c.B, c.N, c.S2, _lib.ptr(dist), _lib.ptr(idx), _lib.stream()),
               "reart_three_nn")
    rd, ri = oracle.three_nn_expanded(fine, coarse)
    np.testing.assert_array_equal(idx.cpu().numpy(), ri)
    np.testing.assert_array_equal(dist.cpu().numpy().view(np.uint32), rd.view(np.uint32))
    out = torch.full((c.B * c.N + 2, c.D + 7), CANARY, device=dev)
    three_interpolate(x1, x2, t(pts, dev), out, 4)
    full = out.cpu().numpy()
    ref = oracle.three_interpolate(fine, coarse, pts).reshape(c.B * c.N, c.D)
    np.testing.assert_array_equal(full[:c.B * c.N, 4:4 + c.D].view(np.uint32), ref.view(np.uint32))
    assert (full[:, :4] == CANARY).all() and (full[:, 4 + c.D:] == CANARY).all() and (full[c.B * c.N:] == CANARY).all()


@pytest.mark.parametrize("i", range(len(R.SMNN_CASES)), ids=lambda i: "%dx%d-E%d-th%g" % tuple(R.SMNN_CASES[i]))
def test_match_smnn_every_element(dev, i):
    from reart_amd.utils.flow_utils import _smnn_batched, match_smnn

    c = R.SMNN_CASES[i]
    d1, d2, _, keep_ref, tgt_ref, _ = R.smnn_data(i)
    keep, tgt = _smnn_batched(t(d1, dev), t(d2, dev), c.th)                   # the form compute_corr_list_filter launches
    assert keep.dtype == torch.bool and tgt.dtype == torch.int64 and keep.shape == tgt.shape == (c.E, c.N1)
    np.testing.assert_array_equal(keep.cpu().numpy(), keep_ref)
    np.testing.assert_array_equal(tgt.cpu().numpy(), tgt_ref)                 # the nearest row of every row, kept or not
    if c.E == 1 and c.th >= 0:
        _, pairs = match_smnn(t(d1[0], dev), t(d2[0], dev), c.th)
        rows = np.nonzero(keep_ref[0])[0]
        np.testing.assert_array_equal(pairs.cpu().numpy(), np.stack([rows, tgt_ref[0][rows]], 1))


def test_pointnet2_cuda_wrappers_refuse_int64_indices_on_the_device(dev):
    """An int64 index tensor on the device (torch's default) is refused by every wrapper: only the raise is asserted, nothing
    is launched (tests/test_pointnet_range_cpu.py goes through every tensor of every wrapper on the host)."""
    from reart_amd import pointnet2_cuda as pc
    from tests.test_pointnet_range_cpu import WRAPPER_ARGS

    for name, (ints, spec) in sorted(WRAPPER_ARGS.items()):
        tensors = [torch.zeros(shape, dtype=torch.float32 if kind == "f" else torch.int64, device=dev) for kind, shape in spec]
        with pytest.raises(RuntimeError, match="int32"):
            getattr(pc, name)(*ints, *tensors)
