"""GPU: the first-order backward of the PointNet++ front end -- ``reart_mlp_layer_backward`` and
``reart_three_interpolate_backward`` over the tables of tests/pointnet_grad_ref.py, every element inside its derived float64
bound (decisions from the float32 activation the kernel itself is given), and the ``grad=True`` switch of the layer classes and
the extractor: the same bits as ``grad=False``, gradients against the reference's own (tests/golden/pointnet_grad.npz) within
2e-4 of each tensor's largest entry.  ``torch.autograd.gradcheck`` is not used: float32.  ``-s`` shows worst error / bound."""
import itertools
import os
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from tests import pointnet_grad_ref as G
from tests import pointnet_range_ref as R
from tests.golden import make_golden_pointnet_grad as M

pytestmark = pytest.mark.gpu

CANARY = -7.0
PAD = 64                 # canary floats in front of and behind every flat output
RATIOS = {}              # output name -> worst |kernel - f64| / bound seen
HERE = os.path.dirname(os.path.abspath(__file__))


def t(a, dev):
    return None if a is None else torch.tensor(np.asarray(a), device=dev)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Layer:
    """Case i on the device: operands, the un-pooled activation A (from reart_mlp_layer itself) and the backward call."""

    def __init__(self, i, dev, idx=None, dY=None):
        from reart_amd import _lib
        from reart_amd.networks.feature_extractor import mlp_layer

        self.i, self.dev, self.c, self.d = i, dev, G.GRAD_CASES[i].c, G.grad_data(i)
        c, d = self.c, self.d
        self.W, self.b = t(d["W"], dev), t(d["b"], dev)
        self.keep = []
        if c.form == "plain":
            self.X = t(d["X"], dev)
            self.args = (_lib.ptr(self.X), c.Cin, None, 0, 0, 0, None, 0, None, None, 0)
            self.B = self.Npts = self.D = 0
        elif c.form == "strided":
            self.buf = t(d["buf"], dev)
            self.args = (c_void_p(self.buf.data_ptr() + 4 * c.opt["off"]), c.opt["ldx"], None, 0, 0, 0, None, 0, None, None, 0)
            self.B = self.Npts = self.D = 0
        else:
            self.idx = t(d["idx"] if idx is None else idx, dev)
            self.F, self.Q, self.C = t(d["F"], dev), t(d["Q"], dev), t(d["C"], dev)
            self.B, self.Npts, self.D = c.opt["B"], c.opt["Npts"], c.opt["D"]
            self.args = (None, 0, _lib.ptr(self.idx), c.pool_k, c.opt["S"], self.Npts, _lib.ptr(self.F), self.D, _lib.ptr(self.Q),
                         _lib.ptr(self.C), int(c.form == "gather_xf"))
        # the un-pooled activation, from the valid indices of the case
        A = torch.empty((c.rows, c.Cout), device=dev)
        fargs = self.args
        if idx is not None:
            self.idx0 = t(d["idx"], dev)
            fargs = self.args[:2] + (_lib.ptr(self.idx0),) + self.args[3:]
        rc = _lib.lib().reart_mlp_layer(*fargs, _lib.ptr(self.W), _lib.ptr(self.b), c.rows, c.Cin, c.Cout, int(c.relu), 0,
                                        _lib.ptr(A), c.Cout, 0, _lib.stream())
        _lib.check(rc, "reart_mlp_layer")
        self.A = A
        # dY: columns 3 .. 3 + Cout of a wider, longer tensor of large values
        n = R.out_rows(c)
        wide = torch.full((n + 2, c.Cout + 5), 1.0e6, device=dev)
        wide[:n, 3:3 + c.Cout] = t(d["dY"] if dY is None else dY, dev)
        self.dY = wide
        self.gathered = c.form.startswith("gather")
        self.names = ("dWt", "dbias") + ((("dF",) if self.D else ()) if self.gathered else ("dX",))

    def shape(self, name):
        c = self.c
        return {"dWt": (c.Cin, c.Cout), "dbias": (c.Cout,), "dX": (c.rows + 2, c.Cin + 5), "dF": (self.B * self.Npts, self.D)}[name]

    def run(self, want=None):
        """-> {name: numpy result} for the wanted outputs; canaries around every output are checked here."""
        from reart_amd import _lib

        c = self.c
        want = self.names if want is None else want
        flat = {k: torch.full((int(np.prod(self.shape(k))) + 2 * PAD,), CANARY, device=self.dev) for k in self.names}
        p = {k: (c_void_p(flat[k].data_ptr() + 4 * PAD) if k in want else None) for k in ("dWt", "dbias", "dX", "dF")
             if k in self.names}
        L = _lib.lib()
        ws = _lib.workspace(L.reart_mlp_layer_backward_scratch_bytes(c.rows, c.Cin, c.Cout, self.B, self.Npts, self.D), self.dev)
        rc = L.reart_mlp_layer_backward(*self.args, _lib.ptr(self.W), c.rows, c.Cin, c.Cout, int(c.relu), c.pool_k, _lib.ptr(self.A),
                                        _lib.ptr(self.dY), self.dY.shape[1], 3, p.get("dWt"), p.get("dbias"), p.get("dX"), c.Cin + 5,
                                        p.get("dF"), _lib.ptr(ws), ws.numel(), _lib.stream())
        _lib.check(rc, "reart_mlp_layer_backward")
        out = {}
        for k in self.names:
            full = flat[k].cpu().numpy()
            assert (full[:PAD] == CANARY).all() and (full[-PAD:] == CANARY).all(), k
            body = full[PAD:-PAD].reshape(self.shape(k))
            if k not in want:
                assert (body == CANARY).all(), k
                continue
            if k == "dX":
                assert (body[c.rows:] == CANARY).all() and (body[:, c.Cin:] == CANARY).all()
                body = body[:c.rows, :c.Cin]
            out[k] = np.ascontiguousarray(body)
        return out


@pytest.mark.parametrize("i", range(len(G.GRAD_CASES)), ids=G.case_id)
def test_layer_backward_inside_the_derived_bounds(dev, i):
    lay = Layer(i, dev)
    got = lay.run()
    A = lay.A.cpu().numpy()
    ref = G.grad_ref(i, A)
    for k, v in got.items():
        val, bound = ref[k]
        r = G.ratio(v, val, bound)
        RATIOS[k] = max(RATIOS.get(k, 0.0), r)
        print("grad case %s %s: worst |kernel - f64| / bound = %.4f" % (G.case_id(i), k, r))
        bad = np.argwhere(np.abs(v.astype(np.float64) - val) > bound)
        assert len(bad) == 0, (G.case_id(i), k, r, bad[:5])
    again = lay.run()
    for k in got:                                             # two runs, the same bits
        assert np.array_equal(bits(again[k]), bits(got[k])), k


def test_layer_backward_ratio_report(dev):
    """The figures of the README: worst error / bound per output over the cases that ran before this one."""
    for k in sorted(RATIOS):
        print("reart_mlp_layer_backward %s: worst |kernel - f64| / bound = %.4f" % (k, RATIOS[k]))
    assert not RATIOS or max(RATIOS.values()) <= 1.0


def _case(name):
    return [g.name for g in G.GRAD_CASES].index(name)


@pytest.mark.parametrize("name", ["2chunk+1", "padded", "everywhere-nowhere", "2chunk+1-pooled"])
def test_every_combination_of_wanted_outputs(dev, name):
    lay = Layer(_case(name), dev)
    full = lay.run()
    for n in range(len(lay.names)):
        for want in itertools.combinations(lay.names, n):
            got = lay.run(want)                               # the unwanted outputs keep their canaries (checked in run)
            assert set(got) == set(want)
            for k in want:
                assert np.array_equal(bits(got[k]), bits(full[k])), (want, k)


def test_a_tie_selects_the_lower_row(dev):
    """A diagonal weight: dX[r, k] = dZ[r, k] W[k, k], so dX shows dZ's pattern -- exactly one non-zero row per (group, column),
    the lowest row that holds the maximum.  Row 5 of every group is stored again at row pool_k - 3."""
    from reart_amd import _lib
    from reart_amd.networks.feature_extractor import mlp_layer

    rows, C, K = 96, 20, 24
    rng = np.random.default_rng(11)
    X = rng.normal(size=(rows, C)).astype(np.float32)
    X3 = X.reshape(-1, K, C)
    X3[:, K - 3] = X3[:, 5]
    X3[:, 5, ::2] = 9.0                                       # in every other column the stored-twice row IS the maximum
    X3[:, K - 3, ::2] = 9.0
    W = np.diag(np.arange(1, C + 1)).astype(np.float32)
    dY = rng.uniform(1.0, 2.0, (rows // K, C)).astype(np.float32)
    Xd, Wd, dYd = t(X, dev), t(W, dev), t(dY, dev)
    A = mlp_layer(Xd, Wd, None, relu=False)
    dX = torch.full((rows, C), CANARY, device=dev)
    L = _lib.lib()
    ws = _lib.workspace(L.reart_mlp_layer_backward_scratch_bytes(rows, C, C, 0, 0, 0), dev)
    rc = L.reart_mlp_layer_backward(_lib.ptr(Xd), C, None, 0, 0, 0, None, 0, None, None, 0, _lib.ptr(Wd), rows, C, C, 0, K, _lib.ptr(A),
                                    _lib.ptr(dYd), C, 0, None, None, _lib.ptr(dX), C, None, _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "reart_mlp_layer_backward")
    g = dX.cpu().numpy().reshape(-1, K, C)
    assert ((g != 0).sum(axis=1) == 1).all()                  # one non-zero row per (group, column)
    first = np.argmax(X3 * np.diag(W)[None, None, :], axis=1)
    assert np.array_equal(np.argmax(g != 0, axis=1), first)
    assert (first[:, ::2] == 5).all() and (g[:, K - 3, ::2] == 0).all() and (g[:, 5, ::2] != 0).all()


def test_a_dead_group_gets_exact_zeros(dev):
    i = _case("dead-group")
    lay = Layer(i, dev)
    K = lay.c.pool_k
    assert (lay.A.cpu().numpy()[K:2 * K] == 0).all()          # every pre-activation of group 1 is negative
    dX = lay.run()["dX"]
    assert (dX[K:2 * K] == 0).all() and (dX[:K] != 0).any() and (dX[2 * K:] != 0).any()


def test_a_point_in_no_group_gets_an_exact_zero_row(dev):
    i = _case("everywhere-nowhere")
    lay = Layer(i, dev)
    dF = lay.run()["dF"].reshape(lay.B, lay.Npts, lay.D)
    assert (dF[:, 1] == 0).all() and (dF[:, 0] != 0).all()


@pytest.mark.parametrize("name", ["2chunk+1", "padded", "tie-relu"])
def test_zero_upstream_gives_zero_outputs(dev, name):
    i = _case(name)
    lay = Layer(i, dev, dY=np.zeros_like(G.grad_data(i)["dY"]))
    for k, v in lay.run().items():
        assert (v == 0).all(), k


def test_an_index_out_of_range_is_skipped(dev):
    """Records whose index lies outside [0, Npts) count for dbias (their dZ is what it is) but neither for dWt (their operand
    row is a zero row) nor for dF (they are in no point's list).  The activation is handed in with those records as their
    groups' maxima, so that every one of them is selected."""
    i = _case("padded")
    c, d = G.GRAD_CASES[i].c, G.grad_data(i)
    idx = d["idx"].copy()
    bad_rows = np.array([1, 30, 55, c.rows - 1])                  # one per group
    idx.reshape(-1)[bad_rows] = [-1, c.opt["Npts"], 1 << 40, -(1 << 35)]
    lay = Layer(i, dev, idx=idx)                                # A from the valid indices
    lay.A[torch.tensor(bad_rows, device=dev)] = 1.0e9
    got = lay.run()
    A = lay.A.cpu().numpy()
    dZ = G.dz_of(c, A, d["dY"]).astype(np.float64)
    assert (dZ[bad_rows] != 0).all()
    X = d["Xop"].astype(np.float64)
    X[bad_rows] = 0.0
    ref = G.grad_ref(i, A)
    assert np.all(np.abs(got["dWt"] - X.T @ dZ) <= ref["dWt"][1])
    assert np.all(np.abs(got["dbias"] - ref["dbias"][0]) <= ref["dbias"][1])
    dX = ref["dX"][0].copy()
    dX[bad_rows] = 0.0
    keep = d["idx"].copy()                                      # the valid index of a bad record: its row is zero here
    val, _ = G.scatter_rows(c, keep, dX[:, G.feature_columns(c)])
    assert np.all(np.abs(got["dF"] - val) <= ref["dF"][1])
    assert not np.all(np.abs(got["dF"] - ref["dF"][0]) <= ref["dF"][1])      # and the records do matter


# ---------------------------------------------------------------------------------------------------------------------
# interpolation backward
# ---------------------------------------------------------------------------------------------------------------------
def _interp_backward(x1, x2, dOut, c, S2, dev):
    from reart_amd import _lib

    L = _lib.lib()
    dP = torch.full((c.B * S2 * c.D + 2 * PAD,), CANARY, device=dev)
    W = torch.full((c.B * c.N * 3 + 2 * PAD,), CANARY, device=dev)
    ws = _lib.workspace(L.reart_three_interpolate_backward_scratch_bytes(c.B, c.N, S2), dev)
    rc = L.reart_three_interpolate_backward(_lib.ptr(x1), _lib.ptr(x2), _lib.ptr(dOut), dOut.shape[1], G.INTERP_COL0, c.B, c.N, S2, c.D,
                                            c_void_p(dP.data_ptr() + 4 * PAD), c_void_p(W.data_ptr() + 4 * PAD), _lib.ptr(ws),
                                            ws.numel(), _lib.stream())
    _lib.check(rc, "reart_three_interpolate_backward")
    dP, W = dP.cpu().numpy(), W.cpu().numpy()
    for a in (dP, W):
        assert (a[:PAD] == CANARY).all() and (a[-PAD:] == CANARY).all()
    return dP[PAD:-PAD].reshape(c.B, S2, c.D), W[PAD:-PAD].reshape(c.B, c.N, 3)


@pytest.mark.parametrize("i", range(len(G.TNN_CASES)), ids=lambda i: "B%d-N%d-S%d-D%d" % tuple(G.TNN_CASES[i]))
def test_interpolation_backward_inside_the_derived_bound(dev, i):
    from reart_amd import _lib
    from reart_amd.networks.feature_extractor import three_interpolate

    c = G.TNN_CASES[i]
    fine, coarse, dOut = G.interp_data(i)
    S2 = coarse.shape[1]
    x1, x2, dO = t(fine, dev), t(coarse, dev), t(dOut, dev)
    dist = torch.empty((c.B, c.N, 3), device=dev)
    idx = torch.empty((c.B, c.N, 3), dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().reart_three_nn(_lib.ptr(x1), _lib.ptr(x2), c.B, c.N, S2, _lib.ptr(dist), _lib.ptr(idx), _lib.stream()),
               "reart_three_nn")
    dP, W = _interp_backward(x1, x2, dO, c, S2, dev)
    idx3, w = idx.cpu().numpy(), G.interp_weights(dist.cpu().numpy())
    # the backward's weights are the float32 expression of the forward, and the forward's output is made of the same weights
    assert np.array_equal(bits(W), bits(w))
    pts = np.random.default_rng(9500 + i).normal(size=(c.B, S2, c.D)).astype(np.float32)
    out = torch.empty((c.B * c.N, c.D), device=dev)
    three_interpolate(x1, x2, t(pts, dev), out, 0)
    bb = np.arange(c.B)[:, None]
    fwd = (pts[bb, idx3[:, :, 0]] * w[:, :, 0:1] + pts[bb, idx3[:, :, 1]] * w[:, :, 1:2]) + pts[bb, idx3[:, :, 2]] * w[:, :, 2:3]
    assert np.array_equal(bits(out.cpu().numpy()), bits(fwd.reshape(c.B * c.N, c.D).astype(np.float32)))
    val, bound, cnt = G.interp_ref(idx3, w, dOut[:, G.INTERP_COL0:G.INTERP_COL0 + c.D], S2)
    r = G.ratio(dP, val, bound)
    RATIOS["dpoints2"] = max(RATIOS.get("dpoints2", 0.0), r)
    print("interpolation case %s: worst |kernel - f64| / bound = %.4f" % (tuple(c), r))
    assert np.all(np.abs(dP.astype(np.float64) - val) <= bound), r
    assert (dP[cnt == 0] == 0).all()
    if i == len(G.TNN_CASES) - 1:
        assert (cnt[:, G.FAR_INDEX] == 0).all() and (dP[:, G.FAR_INDEX] == 0).all()
    again, _ = _interp_backward(x1, x2, dO, c, S2, dev)
    assert np.array_equal(bits(again), bits(dP))


def test_interpolation_ratio_report(dev):
    if "dpoints2" in RATIOS:
        print("reart_three_interpolate_backward: worst |kernel - f64| / bound = %.4f" % RATIOS["dpoints2"])
        assert RATIOS["dpoints2"] <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the grad=True switch of the modules
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return M, np.load(os.path.join(HERE, "golden", "pointnet_grad.npz"))


def _close(name, got, want):
    """The project's rule for gradients against the reference's own float32 results: within 2e-4 of the largest entry."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print("%s: max |ours - reference| = %.3e = %.3e of the largest entry %.3e" % (name, err, err / scale if scale else 0.0, scale))
    assert err <= 2e-4 * scale, (name, err, scale)


@pytest.mark.parametrize("name", M.LAYERS)
def test_layer_gradients_equal_the_references(dev, cpu_rules, golden, name):
    """Every stored gradient of a layer configuration -- parameters and incoming features -- and the outputs' bits with and
    without the graph."""
    M, z = golden
    mod, inputs, starts = M.build_ours(name, z, dev)
    for k, v in inputs.items():
        if v is not None and k.startswith("points"):
            v.requires_grad_(True)
    kw = dict(fps_start=starts, cuda_mode=False)
    plain = mod(*inputs.values(), **kw)
    out = mod(*inputs.values(), **kw, grad=True)
    feats = out[1] if isinstance(out, tuple) else out
    if isinstance(out, tuple):
        assert out[0].grad_fn is None and not out[0].requires_grad        # new_xyz carries no graph
        assert np.array_equal(bits(out[0].cpu().numpy()), bits(plain[0].cpu().numpy()))
        plain = plain[1]
    assert plain.grad_fn is None and not plain.requires_grad
    assert feats.grad_fn is not None
    assert np.array_equal(bits(feats.detach().cpu().numpy()), bits(plain.cpu().numpy()))
    U = t(M.upstream(name, tuple(feats.shape)), dev)
    (feats * U).sum().backward()
    stored = [k for k in z.files if k.startswith(name + "/grad/")]
    assert stored
    for k in stored:
        what = k[len(name) + 6:]
        if what in inputs:
            _close(k, inputs[what].grad.cpu().numpy(), z[k])
        else:
            _close(k, dict(mod.named_parameters())[what].grad.cpu().numpy(), z[k])


def test_extractor_gradients_equal_the_references(dev, cpu_rules, golden):
    M, z = golden
    net, xyz, starts = M.build_ours("extractor", z, dev)
    plain = net(xyz, fps_start=starts, cuda_mode=False)
    out = net(xyz, fps_start=starts, cuda_mode=False, grad=True)
    assert plain.grad_fn is None and out.grad_fn is not None
    assert np.array_equal(bits(out.detach().cpu().numpy()), bits(plain.cpu().numpy()))
    (out * t(M.upstream("extractor", tuple(out.shape)), dev)).sum().backward()
    params = dict(net.named_parameters())
    for k in M.EXTRACTOR_GRADS:
        _close(k, params[k].grad.cpu().numpy(), z["extractor/grad/" + k])
    g1 = {k: p.grad.clone() for k, p in params.items()}
    net.zero_grad(set_to_none=True)
    out2 = net(xyz, fps_start=starts, cuda_mode=False, grad=True)
    (out2 * t(M.upstream("extractor", tuple(out.shape)), dev)).sum().backward()
    for k, p in params.items():                                 # two runs agree in every bit
        assert torch.equal(p.grad, g1[k]), k


def _small_msg(dev):
    from reart_amd.networks.pointnet2_utils import PointNetSetAbstractionMsg
    from reart_amd.synthetic import extractor_state

    torch.manual_seed(5)
    mod = PointNetSetAbstractionMsg(16, [0.2, 0.4], [16, 24], 5, [[8, 8, 16], [16, 12, 20]]).to(dev).eval()
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)
    rng = np.random.default_rng(3)
    xyz = t(rng.uniform(-0.5, 0.5, (2, 3, 200)).astype(np.float32), dev)
    pts = t(rng.normal(size=(2, 5, 200)).astype(np.float32), dev)
    return mod, xyz, pts


def test_a_frozen_module_gives_feature_gradients_only(dev):
    from reart_amd.networks import feature_extractor as fe

    mod, xyz, pts = _small_msg(dev)
    for p in mod.parameters():
        p.requires_grad_(False)
    pts.requires_grad_(True)
    xyz.requires_grad_(True)                                    # ignored: coordinates get no gradient
    before = dict(fe.GRAD_CALLS)
    _, out = mod(xyz, pts, grad=True)
    out.sum().backward()
    assert fe.GRAD_CALLS["parameter"] == before["parameter"] and fe.GRAD_CALLS["feature"] > before["feature"]
    assert pts.grad is not None and (pts.grad != 0).any() and xyz.grad is None
    assert all(p.grad is None for p in mod.parameters())
    # the other way round: trainable parameters, constant features
    for p in mod.parameters():
        p.requires_grad_(True)
    before = dict(fe.GRAD_CALLS)
    _, out = mod(xyz.detach(), pts.detach(), grad=True)
    out.sum().backward()
    assert fe.GRAD_CALLS["parameter"] > before["parameter"]
    assert all(p.grad is not None for p in mod.parameters())


def test_training_mode_and_no_grad_still_raise(dev):
    from reart_amd.networks.feature_extractor import PointNet2Msg2

    mod, xyz, pts = _small_msg(dev)
    mod.train()
    for g in (False, True):
        with pytest.raises(RuntimeError, match=r"PointNetSetAbstractionMsg is inference-only here \(call \.eval\(\)\)"):
            mod(xyz, pts, grad=g)
    mod.eval()
    with torch.no_grad():
        mod(xyz, pts)
        with pytest.raises(RuntimeError, match="grad=True needs autograd enabled"):
            mod(xyz, pts, grad=True)
    net = PointNet2Msg2(64).to(dev)
    net.train()
    with pytest.raises(RuntimeError, match="PointNet2Msg2 is inference-only here"):
        net(xyz, grad=True)
    net.eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="grad=True needs autograd enabled"):
        net(xyz, grad=True)


def test_strided_and_non_float32_operands_are_refused(dev):
    from reart_amd.networks.feature_extractor import mlp_layer, three_interpolate

    X = torch.randn(40, 8, device=dev)
    W = torch.randn(8, 16, device=dev, requires_grad=True)
    b = torch.zeros(16, device=dev)
    with pytest.raises(ValueError, match="contiguous"):
        mlp_layer(X.t().contiguous().t(), W, b, grad=True)
    with pytest.raises(TypeError, match="float32"):
        mlp_layer(X.double(), W, b, grad=True)
    with pytest.raises(ValueError, match="out must be None"):
        mlp_layer(X, W, b, out=torch.empty(40, 16, device=dev), grad=True)
    x1, x2, p2 = torch.randn(1, 9, 3, device=dev), torch.randn(1, 4, 3, device=dev), torch.randn(1, 4, 6, device=dev)
    with pytest.raises(TypeError, match="float32"):
        three_interpolate(x1, x2, p2.double(), None, 0, grad=True)
    with pytest.raises(ValueError, match="contiguous"):
        three_interpolate(x1, x2, p2.transpose(1, 2).contiguous().transpose(1, 2), None, 0, grad=True)
