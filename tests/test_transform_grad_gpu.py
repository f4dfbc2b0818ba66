"""The gradients through the transforms on the device (csrc/transform_grad.hip and the autograd functions over it) against
the float64 restatements of tests/transform_grad_ref.py: rotation_6d_to_matrix, compute_pc_transform, fk and
KinematicModel.forward, BaseModel.forward, each with an upstream on trans_list, on pc_trans or on both, and the gradient of
the input cloud.  Per tensor max |g - g_ref| <= 2e-4 max |g_ref| (tests/test_transform_grad_cpu.py holds the reference itself
against that bound).  Every case runs twice and must give the same bits; one case runs captured in a graph."""
import functools

import numpy as np
import pytest
import torch

from tests import kin_ref as kr
from tests import transform_grad_ref as tr

pytestmark = pytest.mark.gpu


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(g, like):
    return np.zeros(tuple(like.shape), np.float32) if g is None else g.detach().cpu().numpy()


def _twice(run, ref, what):
    """Two runs: the first within the bound of `ref`, the second equal to the first bit for bit -> the first run's gradients."""
    fw1, g1 = run()
    fw2, g2 = run()
    sp = tr.check(g1, ref, what=what)
    print(f"\n[{what}] kernel vs float64: " + "  ".join(f"{k} {v:.1e}" for k, v in sp.items()))
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), (what, k)
    for k in fw1:
        assert (fw1[k] is None and fw2[k] is None) or np.array_equal(fw1[k], fw2[k]), (what, k)
    return fw1, g1


def _close(got, ref, what):
    scale = max(1.0, float(np.abs(ref).max())) if ref.size else 1.0
    assert got.shape == ref.shape and (not ref.size or np.abs(got - ref).max() <= kr.FK_FWD_TOL * scale), what


# ------------------------------------------------------------------------------------------- rotation_6d_to_matrix
@pytest.mark.parametrize("shape", tr.R6D_SHAPES, ids=str)
def test_rotation_6d_to_matrix(dev, shape):
    from reart_amd.screw_se3 import rotation_6d_to_matrix

    c = tr.make_r6d_case(shape)
    fw_ref, ref = tr.r6d_grads(c)

    def run():
        d6 = t(c["d6"], dev).requires_grad_(True)
        R = rotation_6d_to_matrix(d6)
        assert R.requires_grad and R.shape == shape[:-1] + (3, 3)
        (R * t(c["W"], dev)).sum().backward()
        return dict(R=R.detach().cpu().numpy()), dict(d6=_np(d6.grad, d6))

    fw, _ = _twice(run, ref, f"r6d {shape}")
    _close(fw["R"], fw_ref["R"], shape)
    assert not rotation_6d_to_matrix(t(c["d6"], dev)).requires_grad


# -------------------------------------------------------------------------------------------- compute_pc_transform
@pytest.mark.parametrize("wrt", ("both", "cano", "pose"))
@pytest.mark.parametrize("shape", tr.PCT_SHAPES, ids=str)
def test_compute_pc_transform(dev, shape, wrt):
    from reart_amd.utils.model_utils import compute_pc_transform

    c = tr.make_pct_case(*shape)
    fw_ref, ref = tr.pct_grads(c)
    ref = {k: v for k, v in ref.items() if wrt in ("both", k)}

    def run():
        x = t(c["cano"], dev).requires_grad_(wrt != "pose")
        pose = t(c["pose"], dev).requires_grad_(wrt != "cano")
        out = compute_pc_transform(x, pose, t(c["part"], dev))
        (out * t(c["A"], dev)).sum().backward()
        assert (x.grad is None) == (wrt == "pose") and (pose.grad is None) == (wrt == "cano")
        return dict(out=out.detach().cpu().numpy()), {k: _np(v.grad, v) for k, v in (("cano", x), ("pose", pose)) if k in ref}

    fw, g = _twice(run, ref, f"pc_transform {shape} wrt {wrt}")
    _close(fw["out"], fw_ref["out"], shape)
    if "pose" in g:
        assert (g["pose"][:, :, 3, :] == 0).all()                 # row 3 is a constant of the apply: exactly zero
        assert (g["pose"][:, c["empty"]] == 0).all()              # a part without points
    out = compute_pc_transform(t(c["cano"], dev), t(c["pose"], dev), t(c["part"], dev))
    assert not out.requires_grad and np.array_equal(out.cpu().numpy(), fw["out"])      # the plain call


# ------------------------------------------------------------------------------------- fk and KinematicModel.forward
def _tree_dicts(c):
    edge_index = {f"{p}_{int(c['parent'][p])}": int(c["edge_of"][p]) for p in range(len(c["parent"])) if c["parent"][p] >= 0}
    return edge_index, [int(v) for v in c["order"]]


def _types(c):
    return None if c["prismatic"] is None else ["prismatic" if b else "revolute" for b in c["prismatic"]]


def _kin_model(c, dev):
    from reart_amd.knn_cuda import KNN
    from reart_amd.networks.model import KinematicModel

    edge_index, topo = _tree_dicts(c)
    kw = dict(edge_index=edge_index, paths_to_base=None, reverse_topo=topo, axis_list=t(c["axis"], dev), moment_list=t(c["moment"], dev),
              theta_list=t(c["theta"], dev), joint_type_list=_types(c))
    if c["distance"] is not None:
        kw["distance_list"] = t(c["distance"], dev)
    if c["root_6d"] is not None:
        kw["load_root_trans"] = True
    model = KinematicModel(pose_len=c["theta"].shape[0], seg_part=t(c["part"], dev), cano_pc=t(c["x"], dev),
                           knn=KNN(k=1, transpose_mode=True), **kw).to(dev)
    if c["root_6d"] is not None:
        with torch.no_grad():
            model.root_6d.copy_(t(c["root_6d"], dev))
            model.root_t.copy_(t(c["root_t"], dev))
    return model


KIN_NAMES = dict(axis="axis_list", moment="moment_list", theta="theta_list", distance="distance_list", root_6d="root_6d", root_t="root_t")


def _run_kin_model(c, dev, use, W=None):
    model = _kin_model(c, dev)
    x = t(c["x"], dev).requires_grad_(True)
    plain = model(x)[2]
    assert not plain.requires_grad                                # as before: a tensor callers hand to numpy as it is
    out, seg, trans = model(x, trans_grad=True)
    assert torch.equal(seg, t(c["part"], dev)) and torch.equal(plain, trans.detach())
    loss = torch.zeros((), device=dev)
    if use != "trans":
        loss = loss + (out * t(c["A"], dev)).sum()
    if use != "out":
        loss = loss + (trans * t(c["W"] if W is None else W, dev)).sum()
    if loss.requires_grad:
        loss.backward()
    grads = {k: _np(getattr(model, n).grad, getattr(model, n)) for k, n in KIN_NAMES.items() if hasattr(model, n)}
    grads["x"] = _np(x.grad, x)
    return dict(out=out.detach().cpu().numpy(), trans=trans.detach().cpu().numpy()), grads


@functools.lru_cache(maxsize=None)
def _kin_ref(name, use):
    return tr.kin_grads(tr.make_kin_case(name), use)


@pytest.mark.parametrize("use", tr.USES)
@pytest.mark.parametrize("name", list(tr.KIN_CASES))
def test_kinematic_model(dev, name, use):
    c = tr.make_kin_case(name)
    fw_ref, ref = _kin_ref(name, use)
    fw, g = _twice(lambda: _run_kin_model(c, dev, use), ref, f"{name}/{use}")
    _close(fw["out"], fw_ref["out"], name)
    _close(fw["trans"], fw_ref["trans"], name)
    if use == "trans":
        assert not g["x"].any()
    if c["prismatic"] is not None:                                # the placeholders of utils/kinematic_utils.py:174-186
        pris = c["prismatic"]
        assert (g["theta"][:, pris] == 0).all() and (g["distance"][:, ~pris] == 0).all()


@pytest.mark.parametrize("name", ("star_P6_distance", "random_P64_root_motion_distance"))
def test_row3_of_the_upstream_is_ignored(dev, name):
    """trans_list's row 3 is constant: another upstream there changes no gradient by a bit."""
    c = tr.make_kin_case(name)
    W2 = c["W"].copy()
    W2[:, :, 3, :] = 1e3 * (1.0 + np.abs(W2[:, :, 3, :]))
    _, g = _run_kin_model(c, dev, "both")
    _, g2 = _run_kin_model(c, dev, "both", W=W2)
    for k in g:
        assert np.array_equal(g[k], g2[k]), k


@pytest.mark.parametrize("name", [n for n, v in tr.KIN_CASES.items() if not v[4]])
def test_fk_alone(dev, name):
    from reart_amd.utils.kinematic_utils import fk

    c = tr.make_kin_case(name)
    fw_ref, ref = tr.kin_grads(c, "trans", cloud=False)
    edge_index, topo = _tree_dicts(c)

    def run():
        leaves = {k: t(c[k], dev).requires_grad_(True) for k in ("axis", "moment", "theta", "distance") if c[k] is not None}
        trans = fk(None, topo, edge_index, leaves["axis"], leaves["moment"], leaves["theta"], leaves.get("distance"), _types(c))
        assert trans.requires_grad
        (trans * t(c["W"], dev)).sum().backward()
        return dict(trans=trans.detach().cpu().numpy()), {k: _np(v.grad, v) for k, v in leaves.items()}

    fw, _ = _twice(run, ref, f"fk {name}")
    _close(fw["trans"], fw_ref["trans"], name)


def _fk_args(c, dev):
    E = c["axis"].shape[0]
    assert c["prismatic"] is None and E > 0
    return (t(c["x"], dev), t(c["part"], dev), t(c["axis"], dev), t(c["moment"], dev), t(c["theta"], dev),
            None if c["distance"] is None else t(c["distance"], dev), t(c["parent"], dev), t(c["edge_of"], dev), t(c["order"], dev))


def test_without_the_new_arguments_fk_backward_trans_is_fk_backward(dev):
    """reart_fk_backward_trans with g_trans = g_x = NULL leaves reart_fk_backward's four joint gradients, bit for bit."""
    from reart_amd import _lib
    from reart_amd.utils.kinematic_utils import _FK

    c = tr.make_kin_case("chain_P64_distance")
    x, part, axis, moment, theta, dist, parent, edge_of, order = _fk_args(c, dev)
    with torch.no_grad():
        _, trans = _FK.apply(x, part, axis, moment, theta, dist, parent, edge_of, order)
    (B, E), P, N = theta.shape, parent.shape[0], x.shape[0]
    G = t(c["A"], dev)
    L = _lib.lib()
    ws = _lib.workspace(L.reart_fk_backward_workspace_bytes(P, B, E), dev)
    got = []
    for new in (False, True):
        g = [torch.full_like(v, float("nan")) for v in (axis, moment, theta, dist)]
        head = (_lib.ptr(x), _lib.ptr(part), _lib.ptr(G), N, _lib.ptr(parent), _lib.ptr(edge_of), _lib.ptr(order), P, _lib.ptr(axis),
                _lib.ptr(moment), _lib.ptr(theta), _lib.ptr(dist), B, E, _lib.ptr(trans))
        outs = tuple(_lib.ptr(v) for v in g)
        tail = (_lib.ptr(ws), ws.numel(), _lib.stream())
        if new:
            _lib.check(L.reart_fk_backward_trans(*head, None, *outs, None, *tail), "reart_fk_backward_trans")
        else:
            _lib.check(L.reart_fk_backward(*head, *outs, *tail), "reart_fk_backward")
        got.append(g)
    for a, b in zip(*got):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_fk_and_the_trans_upstream_captured_in_a_graph(dev):
    """_FK forward and its backward from an upstream on both outputs, captured on a single stream and replayed on other joint
    angles: the bits of the eager calls.  The eager calls run on the stream of the capture, so the backward's scratch buffer of
    that stream (_lib.workspace) exists before the capture opens: the backward runs on autograd's thread, and the capture
    should not have that thread grow the allocator's pool."""
    from reart_amd.utils.kinematic_utils import _FK

    c = tr.make_kin_case("star_P6_distance")
    x, part, axis, moment, theta, dist, parent, edge_of, order = _fk_args(c, dev)
    A, W = t(c["A"], dev), t(c["W"], dev)
    other = (theta * 0.5).contiguous()

    def step(th):
        leaves = [v.requires_grad_(True) for v in (x, axis, moment, th, dist)]
        out, trans = _FK.apply(leaves[0], part, leaves[1], leaves[2], leaves[3], leaves[4], parent, edge_of, order, True)
        return (out, trans) + torch.autograd.grad((out * A).sum() + (trans * W).sum(), leaves)

    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eager = [[v.clone() for v in step(th.clone())] for th in (theta, other)]
    torch.cuda.synchronize()
    static = theta.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        outs = step(static)
    for want, th in ((eager[1], other), (eager[0], theta)):
        static.detach().copy_(th)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, want):
            assert torch.equal(a, b)
    assert not torch.equal(eager[0][5], eager[1][5])


# ----------------------------------------------------------------------------------------------- BaseModel.forward
def _base_model(c, dev):
    from reart_amd.networks.model import BaseModel

    p = c["params"]
    B, P = p["p6d"].shape[:2]
    model = BaseModel(num_parts=P, pose_len=B).to(dev)
    W1, b1, W2 = model._weights()
    with torch.no_grad():
        W1.copy_(t(p["W1"], dev)[:, :, None])
        b1.copy_(t(p["b1"], dev))
        W2.copy_(t(p["W2"], dev)[:, :, None])
        model.proposal_6d.copy_(t(p["p6d"], dev))
        model.proposal_t.copy_(t(p["pt"], dev))
    return model


def _run_base(c, dev, use, cano_grad=True):
    model = _base_model(c, dev)
    x = t(c["cano"], dev).requires_grad_(cano_grad)
    out, seg, trans = model(x, tau=c["tau"], gumbel=t(c["gumbel"], dev))
    loss = torch.zeros((), device=dev)
    if use != "trans":
        loss = loss + (out * t(c["A"], dev)).sum()
    if use != "out":
        loss = loss + (trans * t(c["W"], dev)).sum()
    loss.backward()
    W1, b1, W2 = model._weights()
    leaves = dict(W1=W1, b1=b1, W2=W2, p6d=model.proposal_6d, pt=model.proposal_t, cano=x)
    like = dict(c["params"], cano=c["cano"])                      # the conv weights carry a trailing axis of one
    grads = {k: _np(v.grad, v).reshape(like[k].shape) for k, v in leaves.items() if k != "cano" or cano_grad}
    if use != "trans" and cano_grad:
        assert x.grad is not None
    return dict(out=out.detach().cpu().numpy(), trans=trans.detach().cpu().numpy()), grads


@functools.lru_cache(maxsize=None)
def _base_ref(name, use):
    return tr.base_grads(tr.make_base_case(name), use)


@pytest.mark.parametrize("use", tr.USES)
@pytest.mark.parametrize("name", list(tr.BASE_CASES))
def test_base_model(dev, name, use):
    from reart_amd import _lib

    c = tr.make_base_case(name)
    N, P, B = tr.BASE_CASES[name][:3]
    long_path = _lib.lib().reart_base_path(P, B, 128, 0) == 1 and _lib.lib().reart_base_path(P, B, 128, 1) == 1
    assert long_path == name.endswith("long_path")
    fw_ref, ref = _base_ref(name, use)
    fw, g = _twice(lambda: _run_base(c, dev, use), ref, f"{name}/{use}")
    np.testing.assert_allclose(fw["out"], fw_ref["out"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(fw["trans"], fw_ref["trans"], rtol=0, atol=1e-6)
    if use == "trans":
        assert not any(g[k].any() for k in ("W1", "b1", "W2", "cano"))


@pytest.mark.parametrize("name", ("N200_P20_B3_tau5_unassigned_part", "N100_P20_B100_tau5_long_path"))
def test_parameter_gradients_on_the_existing_path_are_those_of_reart_base_backward(dev, name):
    """Parameters only, upstream on pc_trans only: the five gradients are a direct reart_base_backward call's on the tensors the
    forward saves, bit for bit; with the cloud's gradient and the trans_list upstream asked for as well, W1 | b1 | W2 still
    are (the new terms touch the poses and the cloud only)."""
    from reart_amd import _lib

    c = tr.make_base_case(name)
    p = c["params"]
    (B, P), N, H = p["p6d"].shape[:2], c["cano"].shape[0], p["W1"].shape[0]
    cano, W1, b1, W2, p6d, pt, noise, G = (t(a, dev) for a in (c["cano"], p["W1"], p["b1"], p["W2"], p["p6d"], p["pt"], c["gumbel"], c["A"]))
    e = lambda *s, dtype=torch.float32: torch.empty(s, dtype=dtype, device=dev)
    out, yT, hT, hard = e(B, N, 3), e(P, N), e(H, N), e(N, dtype=torch.int32)
    L = _lib.lib()
    _lib.check(L.reart_base_forward(_lib.ptr(cano), N, P, B, _lib.ptr(W1), _lib.ptr(b1), _lib.ptr(W2), H, _lib.ptr(p6d), _lib.ptr(pt),
                                    _lib.ptr(noise), c["tau"], _lib.ptr(out), None, None, _lib.ptr(yT), _lib.ptr(hT), _lib.ptr(hard),
                                    _lib.stream()), "reart_base_forward")
    direct = dict(W1=e(H, 3), b1=e(H), W2=e(P, H), p6d=e(B, P, 6), pt=e(B, P, 3))
    ws = _lib.workspace(L.reart_base_backward_workspace_bytes(N, P, B, H), dev)
    _lib.check(L.reart_base_backward(_lib.ptr(cano), N, P, B, _lib.ptr(W1), _lib.ptr(b1), _lib.ptr(W2), H, _lib.ptr(p6d), _lib.ptr(pt),
                                     _lib.ptr(yT), _lib.ptr(hT), _lib.ptr(hard), c["tau"], _lib.ptr(G), *(_lib.ptr(direct[k]) for k in
                                                                                                         ("W1", "b1", "W2", "p6d", "pt")),
                                     _lib.ptr(ws), ws.numel(), _lib.stream()), "reart_base_backward")
    direct = {k: v.cpu().numpy() for k, v in direct.items()}
    assert np.array_equal(hard.cpu().numpy(), c["hard"])          # the device's decisions are the oracle's
    _, plain = _run_base(c, dev, "out", cano_grad=False)
    for k in direct:
        assert np.array_equal(plain[k], direct[k]), k
    _, full = _run_base(c, dev, "both", cano_grad=True)
    for k in ("W1", "b1", "W2"):
        assert np.array_equal(full[k], direct[k]), k
    assert not np.array_equal(full["p6d"], direct["p6d"])
