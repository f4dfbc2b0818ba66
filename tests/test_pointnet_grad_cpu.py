"""No GPU: the yardstick of tests/test_pointnet_grad_gpu.py measures.  The float64 restatement of
tests/pointnet_grad_ref.py equals torch's float64 autograd of the same layer written as tensor expressions; an honest float32
backward stays inside every derived bound on every case; each of four planted errors leaves them on every case it can touch;
the tables hold the cases they must; and the reference's gradients of tests/golden/pointnet_grad.npz lie within 1e-4 of their
largest entry of the float64 restatement of the modules (so the reference alone stays inside the GPU test's 2e-4)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import pointnet_grad_ref as G
from tests import pointnet_range_ref as R
from tests.golden import make_golden_pointnet_grad as M

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = range(len(G.GRAD_CASES))


def test_the_tables_hold_their_cases():
    from reart_amd import _lib

    n = len(R.LAYER_CASES)
    assert n == 57 and [g.c for g in G.GRAD_CASES[:n]] == list(R.LAYER_CASES) and all(g.name is None for g in G.GRAD_CASES[:n])
    assert tuple(g.name for g in G.GRAD_CASES[n:]) == G.NEW_NAMES and len(G.NEW_NAMES) == 11
    header = open(os.path.join(HERE, "..", "include", "reart_hip.h")).read()
    assert int(re.search(r"#define REART_MLP_GRAD_ROW_CHUNK (\d+)", header).group(1)) == _lib.MLP_GRAD_ROW_CHUNK == G.ROW_CHUNK
    rows = {g.c.rows for g in G.GRAD_CASES[n:]}
    assert {G.ROW_CHUNK - 1, G.ROW_CHUNK, G.ROW_CHUNK + 1, 2 * G.ROW_CHUNK + 1} <= rows
    assert G.TNN_CASES[:len(R.TNN_CASES)] == list(R.TNN_CASES) and len(R.TNN_CASES) == 10 and G.TNN_CASES[-1] == G.FAR_CASE
    for name in ("reart_mlp_layer_backward", "reart_mlp_layer_backward_scratch_bytes", "reart_three_interpolate_backward",
                 "reart_three_interpolate_backward_scratch_bytes"):
        assert name in _lib.PROTOTYPES and re.search(r"\b%s\(" % name, header)


def test_the_new_cases_are_what_they_claim():
    by = {g.name: i for i, g in enumerate(G.GRAD_CASES) if g.name}
    for name in ("tie-relu", "tie-linear"):                       # one row twice per group, and it decides somewhere
        i = by[name]
        c, A = G.GRAD_CASES[i].c, G.forward_A(i)
        A3 = A.reshape(-1, c.pool_k, c.Cout)
        assert np.array_equal(A3[:, 5], A3[:, c.pool_k - 3])
        assert (G.dz_of(c, A, G.grad_data(i)["dY"], last_tie=True) != G.dz_of(c, A, G.grad_data(i)["dY"])).any()
    i = by["dead-group"]
    c, d = G.GRAD_CASES[i].c, G.grad_data(i)
    pre = d["Xop"].astype(np.float64) @ d["W"].astype(np.float64) + d["b"]
    assert (pre[c.pool_k:2 * c.pool_k] < 0).all() and (pre[:c.pool_k].max(axis=0) > 0).any()
    assert (G.grad_ref(i, G.forward_A(i))["dX"][0][c.pool_k:2 * c.pool_k] == 0).all()
    i = by["everywhere-nowhere"]
    idx = G.grad_data(i)["idx"]
    assert (idx == 0).any(axis=2).all() and not (idx == 1).any()
    assert (G.grad_ref(i, G.forward_A(i))["dF"][0].reshape(2, 30, 5)[:, 1] == 0).all()
    for name in ("padded", "padded-fx"):                          # an index repeated inside a group
        idx = G.grad_data(by[name])["idx"]
        assert all(len(np.unique(row)) < len(row) for row in idx.reshape(-1, idx.shape[2]))


def _torch_grads(i, A):
    """The layer as float64 tensor expressions with the decisions of ``A``; gradients by autograd."""
    c, d = G.GRAD_CASES[i].c, G.grad_data(i)
    f64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    W = f64(d["W"]).requires_grad_(True)
    b = f64(np.zeros(c.Cout) if d["b"] is None else d["b"]).requires_grad_(True)
    F = None
    if c.form.startswith("gather") and c.opt["D"]:
        B, Npts = c.opt["B"], c.opt["Npts"]
        F = f64(d["F"]).requires_grad_(True)
        gp = torch.from_numpy((np.arange(B)[:, None, None] * Npts + d["idx"]).reshape(-1))
        cols = G.feature_columns(c)
        xyz = f64(np.delete(d["Xop"], np.r_[cols], axis=1))          # the float32 Q - C the kernel forms
        X = torch.cat([F[gp], xyz] if c.form == "gather_fx" else [xyz, F[gp]], dim=1)
    else:
        X = f64(d["Xop"]).requires_grad_(True)
    X.retain_grad()
    act = X @ W + b
    if c.relu:
        act = act * torch.from_numpy(A > 0)
    if c.pool_k > 1:
        sel = torch.from_numpy(np.argmax(A.reshape(-1, c.pool_k, c.Cout), axis=1))
        act = torch.gather(act.reshape(-1, c.pool_k, c.Cout), 1, sel[:, None, :])[:, 0]
    (act * f64(d["dY"])).sum().backward()
    out = {"dWt": W.grad, "dbias": b.grad, "dX": X.grad}
    if F is not None:
        out["dF"] = F.grad
    return {k: v.numpy() for k, v in out.items()}


@pytest.mark.parametrize("i", CASES, ids=G.case_id)
def test_restatement_equals_float64_autograd_and_float32_stays_inside(i):
    A = G.forward_A(i)
    ref = G.grad_ref(i, A)
    for k, v in _torch_grads(i, A).items():
        scale = max(1.0, np.abs(ref[k][0]).max())
        assert np.abs(v - ref[k][0]).max() <= 1e-12 * scale, (k, np.abs(v - ref[k][0]).max())
    got = G.grad_emulate(i, A)
    for k, v in got.items():                                      # an honest float32 backward, every output
        assert np.all(np.abs(v.astype(np.float64) - ref[k][0]) <= ref[k][1]), (k, G.ratio(v, *ref[k]))


def _family(fault):
    """The cases a planted error can touch: its float64 effect on an OUTPUT is not exactly nothing."""
    fam = []
    for i in CASES:
        c, d = G.GRAD_CASES[i].c, G.grad_data(i)
        A = G.forward_A(i)
        gathered = c.form.startswith("gather")
        dZ = G.dz_of(c, A, d["dY"])
        if fault in ("last_tie", "mask_ge"):
            other = G.dz_of(c, A, d["dY"], **{fault: True})
            # a tie between two copies of ONE gathered point is the same row twice: either choice gives the same outputs
            if (other != dZ).any() and not (fault == "last_tie" and gathered):
                fam.append(i)
        elif fault == "drop_chunk":
            keep = (-(-c.rows // G.ROW_CHUNK) - 1) * G.ROW_CHUNK
            if (d["Xop"][keep:].astype(np.float64).T @ dZ[keep:].astype(np.float64) != 0).any():
                fam.append(i)
        elif gathered and c.opt["D"] and (dZ != 0).any():
            fam.append(i)
    return fam


@pytest.mark.parametrize("fault", G.FAULTS)
def test_a_planted_error_leaves_the_bounds(fault):
    fam = _family(fault)
    names = {G.GRAD_CASES[i].name for i in fam}
    need = {"last_tie": {"tie-relu", "tie-linear"}, "mask_ge": {"dead-group", "chunk", "2chunk+1"},
            "drop_chunk": set(G.NEW_NAMES), "skip_first": {"everywhere-nowhere", "padded", "padded-fx"}}[fault]
    assert need <= names, (fault, need - names)
    floor = {"last_tie": 2, "mask_ge": 30, "drop_chunk": len(G.GRAD_CASES) - 3, "skip_first": 14}[fault]
    assert len(fam) >= floor, (fault, len(fam))
    for i in fam:
        A = G.forward_A(i)
        assert G.worst_ratio(i, A, G.grad_emulate(i, A, fault)) > 1.0, (fault, G.case_id(i))


@pytest.mark.parametrize("i", range(len(G.TNN_CASES)), ids=lambda i: "B%d-N%d-S%d-D%d" % tuple(G.TNN_CASES[i]))
def test_interpolation_yardstick(oracle, i):
    c = G.TNN_CASES[i]
    fine, coarse, dOut = G.interp_data(i)
    dist3, idx3 = oracle.three_nn_expanded(fine, coarse)
    w = G.interp_weights(dist3)
    g = dOut[:, G.INTERP_COL0:G.INTERP_COL0 + c.D]
    val, bound, cnt = G.interp_ref(idx3, w, g, c.S2)
    honest, _, _ = G.interp_ref(idx3, w, g, c.S2, dtype=np.float32)
    assert np.all(np.abs(honest.astype(np.float64) - val) <= bound)
    skipped, _, _ = G.interp_ref(idx3, w, g, c.S2, skip_first=True, dtype=np.float32)
    assert G.ratio(skipped, val, bound) > 1.0
    assert (val[cnt == 0] == 0).all() and ((cnt == 0).any() or c.S2 <= 4)      # coarse points no fine point selects
    if c == G.FAR_CASE:
        assert (cnt[:, G.FAR_INDEX] == 0).all()
    # the restatement is the float64 autograd of the forward's expression
    P = torch.zeros((c.B, c.S2, c.D), dtype=torch.float64, requires_grad=True)
    bb = torch.arange(c.B)[:, None]
    wd, ti = torch.from_numpy(w).double(), torch.from_numpy(idx3)
    out = sum(P[bb, ti[:, :, j]] * wd[:, :, j:j + 1] for j in range(3))
    (out.reshape(c.B * c.N, c.D) * torch.tensor(g).double()).sum().backward()
    assert np.abs(P.grad.numpy() - val).max() <= 1e-12 * max(1.0, np.abs(val).max())


# ---------------------------------------------------------------------------------------------------------------------
# the module fixture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "pointnet_grad.npz"))


def _within(name, got, want, tol=1e-4):
    scale = np.abs(want).max()
    err = np.abs(np.asarray(got, np.float64) - want).max()
    assert err <= tol * scale, (name, err, scale)


@pytest.mark.parametrize("name", M.LAYERS)
def test_the_reference_stays_inside_half_the_margin_layers(oracle, golden, name):
    z = golden
    assert float(z[name + "/margin"]) >= M.MARGIN
    start = z[name + "/start"] if name + "/start" in z.files else None
    rs, y, leaves = M.restate(name, int(z[name + "/seed"]), start)
    assert rs.margin == float(z[name + "/margin"])
    (y * torch.from_numpy(M.upstream(name, tuple(y.shape))).double()).sum().backward()
    stored = [k for k in z.files if k.startswith(name + "/grad/")]
    assert len(stored) >= 8
    for k in stored:
        what = k[len(name) + 6:]
        if what in leaves:
            _within(k, leaves[what].grad.permute(0, 2, 1).numpy(), z[k])
        else:
            _within(k, rs.p64[what].grad.reshape(z[k].shape).numpy(), z[k])
    assert {k[len(name) + 6:] for k in stored} >= {k for k in leaves}


def test_the_reference_stays_inside_half_the_margin_extractor(oracle, golden):
    from reart_amd.networks.feature_extractor import PointNet2Msg2
    from reart_amd.synthetic import extractor_state

    z = golden
    net = PointNet2Msg2(64)
    rs = G.Restatement({k: v.numpy() for k, v in extractor_state(net, seed=M.EXTRACTOR["weight_seed"]).items()})
    pts = M.cloud(np.random.default_rng(int(z["extractor/seed"])), M.EXTRACTOR["N"])
    _, y = rs.extractor(pts, (z["extractor/start1"], z["extractor/start2"]))
    U = torch.from_numpy(M.upstream("extractor", (M.B, 64, M.EXTRACTOR["N"]))).double()
    (y.permute(0, 2, 1) * U).sum().backward()
    assert sorted(k[len("extractor/grad/"):] for k in z.files if k.startswith("extractor/grad/")) == sorted(M.EXTRACTOR_GRADS)
    for k in M.EXTRACTOR_GRADS:
        _within(k, rs.p64[k].grad.reshape(z["extractor/grad/" + k].shape).numpy(), z["extractor/grad/" + k])


def test_the_fixture_is_small():
    biggest = max(os.path.getsize(os.path.join(HERE, "golden", f)) for f in os.listdir(os.path.join(HERE, "golden")) if f != "pointnet_grad.npz"
                  and os.path.isfile(os.path.join(HERE, "golden", f)))
    assert os.path.getsize(os.path.join(HERE, "golden", "pointnet_grad.npz")) < biggest / 4
