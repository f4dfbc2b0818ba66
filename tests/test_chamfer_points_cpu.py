"""CPU-side checks of the ChamferPoints operator: the boundary (header, ctypes mirror, exports), argument checks of both
entries before any device work, the host mirrors' refusals, the adapter's validation, the dispatch of
compute_chamfer_list, and the float64 restatement the GPU tests use."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG = 0, -1
A = 4096        # a non-null dummy address: good for calls that are refused before anything is launched


def _fwd(L, x=A, y=A, N=2, P1=8, P2=8, dirs=3, sxy=A, syx=A, same=0, dxy=A, ixy=A, dyx=A, iyx=A, ws=A, nbytes=None):
    if nbytes is None:
        nbytes = L.reart_chamfer_loss_workspace_bytes(N, P1, P2)
    return L.reart_chamfer_points(x, y, N, P1, P2, dirs, sxy, syx, same, dxy, ixy, dyx, iyx, ws, nbytes, None)


def _bwd(L, x=A, y=A, N=2, P1=8, P2=8, ixy=A, iyx=A, dxy=A, dyx=A, gxy=A, gyx=A, gx=A, gy=A, bits=A):
    return L.reart_chamfer_points_backward(x, y, N, P1, P2, ixy, iyx, dxy, dyx, gxy, gyx, gx, gy, bits, None)


def test_header_mirror_and_exports_agree():
    from reart_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "reart_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _lib.lib()
    for name in ("reart_chamfer_points", "reart_chamfer_points_backward"):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, f"{name} is not declared in include/reart_hip.h"
        assert hasattr(L, name)
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.c_int
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == len(args)
        for p, a in zip(params, args):
            want = _lib.c_void_p if "*" in p else (_lib.c_size_t if p.startswith("size_t") else _lib.c_int)
            assert a is want, (name, p)


def test_entries_check_their_arguments_before_any_device_work():
    from reart_amd import _lib

    L = _lib.lib()
    need = L.reart_chamfer_loss_workspace_bytes(2, 8, 8)
    assert need > 0
    # forward: what every searched direction needs, the workspace, the sizes, the mask
    for null in ("x", "y", "sxy", "syx", "dxy", "ixy", "dyx", "iyx", "ws"):
        assert _fwd(L, **{null: None}) == INVALID_ARG, null
    for null in ("x", "y", "sxy", "dxy", "ixy", "ws"):
        assert _fwd(L, dirs=1, syx=None, dyx=None, iyx=None, **{null: None}) == INVALID_ARG, null
    for null in ("x", "y", "syx", "dyx", "iyx", "ws"):
        assert _fwd(L, dirs=2, sxy=None, dxy=None, ixy=None, **{null: None}) == INVALID_ARG, null
    assert _fwd(L, nbytes=need - 1) == INVALID_ARG
    assert _fwd(L, nbytes=0) == INVALID_ARG
    for neg in (dict(N=-1), dict(P1=-1), dict(P2=-1), dict(N=65536), dict(N=4, P1=1 << 29)):
        assert _fwd(L, nbytes=1 << 20, **neg) == INVALID_ARG, neg
    for dirs in (0, 4, -1, 7):
        assert _fwd(L, dirs=dirs) == INVALID_ARG, dirs
    # backward: the clouds and the outputs always, indices and distances with their upstream
    for null in ("x", "y", "gx", "bits"):
        assert _bwd(L, **{null: None}) == INVALID_ARG, null
    for null in ("ixy", "dxy", "iyx", "dyx"):
        assert _bwd(L, **{null: None}) == INVALID_ARG, null
    for neg in (dict(N=-1), dict(P1=-1), dict(P2=-1), dict(N=65536), dict(N=4, P1=1 << 29)):
        assert _bwd(L, **neg) == INVALID_ARG, neg
    # empty problems: fine, nothing is launched (no device here) and nothing is dereferenced
    none_f = dict(x=None, y=None, sxy=None, syx=None, dxy=None, ixy=None, dyx=None, iyx=None, ws=None, nbytes=0)
    none_b = dict(x=None, y=None, ixy=None, iyx=None, dxy=None, dyx=None, gxy=None, gyx=None, gx=None, gy=None, bits=None)
    for empty in (dict(N=0), dict(P1=0), dict(P2=0)):
        assert _fwd(L, **none_f, **empty) == OK, empty
        assert _bwd(L, **none_b, **empty) == OK, empty
        assert _fwd(L, dirs=5, **none_f, **empty) == INVALID_ARG, empty


def test_host_tensors_have_no_cpu_fallback():
    from reart_amd.networks.loss import recon_loss
    from reart_amd.utils.chamfer import ChamferPoints, WarmChamferDistance

    a = torch.zeros(1, 8, 3)
    mod = ChamferPoints()
    for call in (lambda: mod(a, a), lambda: mod(a.double(), a.double()), lambda: mod(a, a, "xy"), lambda: mod(a, a, "nonsense"),
                 lambda: mod.seed(a, a), lambda: WarmChamferDistance()(a, a), lambda: WarmChamferDistance()(a, a, reverse=True),
                 lambda: recon_loss(a, a, WarmChamferDistance())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError):
        mod([1], a)


def test_adapter_refuses_what_chamfer_distance_refuses():
    """Every invalid input of test_boundary_cpu.py: the same exception type and the same message from both classes, and
    the same warning."""
    from reart_amd.utils.chamfer import ChamferDistance, WarmChamferDistance

    a = torch.zeros(2, 8, 3)
    cases = [(([1, 2], a), {}), ((a, torch.zeros(3, 8, 3)), {}), ((a, torch.zeros(2, 8, 2)), {}), ((a, a), dict(reduction="max")),
             ((a[:1], a[:1]), {}), ((a, a), dict(bidirectional=True, reverse=True))]
    for args, kw in cases:
        seen = []
        for cls in (ChamferDistance, WarmChamferDistance):
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                with pytest.raises((TypeError, ValueError, RuntimeError)) as e:
                    cls()(*args, **kw)
            seen.append((e.type, str(e.value), [str(x.message) for x in w]))
        assert seen[0] == seen[1], (args, kw)
    assert seen[0][2] == ["Both bidirectional and reverse set to True. bidirectional behavior takes precedence."]


def test_compute_chamfer_list_dispatch(monkeypatch):
    """Without ``chamfer`` the two ChamferDistance searches of today; a ChamferPoints is called once, for both directions.
    Patched: nothing here runs a GPU."""
    from reart_amd.utils import chamfer
    from reart_amd.utils.eval_utils import compute_chamfer_list

    a, b = torch.zeros(2, 8, 3), torch.ones(2, 8, 3)
    calls = []

    def fake_cd(self, src, tgt, **kw):
        calls.append(("cd", src is a, tgt is b, kw))
        return torch.full((2, 8), 0.5)

    def fake_cp(self, x, y, directions="both"):
        calls.append(("cp", x is a, y is b, directions))
        return torch.full((2, 8), 0.25), torch.full((2, 8), 1.0)

    monkeypatch.setattr(chamfer.ChamferDistance, "forward", fake_cd)
    monkeypatch.setattr(chamfer.ChamferPoints, "forward", fake_cp)
    assert compute_chamfer_list(a, b) == 16.0
    assert compute_chamfer_list(a, b, chamfer=None, reduction="mean") == 1.0
    assert calls == [("cd", True, True, {}), ("cd", False, False, {})] * 2
    del calls[:]
    mod = chamfer.ChamferPoints()
    assert compute_chamfer_list(a, b, chamfer=mod) == 20.0
    assert compute_chamfer_list(a, b, reduction="mean", chamfer=mod) == 1.25
    np.testing.assert_array_equal(compute_chamfer_list(a, b, reduction="none", chamfer=mod), [10.0, 10.0])
    assert calls == [("cp", True, True, "both")] * 3


def test_reference_restatement():
    """The float64 restatement on the hand case of test_chamfer_loss_cpu.py with per-point upstreams, with one direction
    dropped, and against central differences of sum_i w_i d_xy[i] + sum_j v_j d_yx[j]."""
    from tests import chamfer_points_ref as ref

    x = np.array([[[0.0, 0, 0], [10.0, 0, 0]]], np.float32)
    y = np.array([[[1.0, 0, 0], [2.0, 0, 0], [9.0, 0, 0]]], np.float32)
    i_xy, i_yx = ref.nearest(x, y)[1], ref.nearest(y, x)[1]
    assert i_xy.tolist() == [[0, 2]] and i_yx.tolist() == [[0, 0, 1]]
    g_xy, g_yx = np.array([[3.0, -1.0]]), np.array([[0.5, 2.0, -4.0]])
    g = ref.gradients(x, y, i_xy, i_yx, g_xy, g_yx)
    assert g["x"]["grad"][0, :, 0].tolist() == [2 * 3 * (0 - 1) + 2 * (0.5 * (0 - 1) + 2 * (0 - 2)), 2 * -1 * (10 - 9) + 2 * -4 * (10 - 9)]
    assert g["y"]["grad"][0, :, 0].tolist() == [2 * 0.5 * (1 - 0) + 2 * 3 * (1 - 0), 2 * 2 * (2 - 0), 2 * -4 * (9 - 10) + 2 * -1 * (9 - 10)]
    assert g["x"]["grad"][0, :, 0].tolist() == [-15.0, -10.0] and g["y"]["grad"][0, :, 0].tolist() == [7.0, 8.0, 10.0]
    assert g["x"]["cnt"].tolist() == [[2, 1]] and g["y"]["cnt"].tolist() == [[1, 0, 1]]
    assert g["x"]["mag"][0, :, 0].tolist() == [1.0 + 8.0, 8.0] and g["y"]["mag"][0, :, 0].tolist() == [6.0, 0.0, 2.0]
    assert not g["x"]["grad"][..., 1:].any() and not g["y"]["grad"][..., 1:].any()
    # only d_xy used: x keeps its own term, y only what the x points send; the y -> x indices are not read
    h = ref.gradients(x, y, i_xy, None, g_xy, None)
    assert h["x"]["grad"][0, :, 0].tolist() == [-6.0, -2.0] and h["y"]["grad"][0, :, 0].tolist() == [6.0, 0.0, 2.0]
    assert h["x"]["cnt"].tolist() == [[0, 0]] and h["y"]["cnt"].tolist() == [[1, 0, 1]]
    # g = 1 everywhere is the restatement of the Chamfer sum
    from tests import chamfer_loss_ref

    one = ref.gradients(x, y, i_xy, i_yx, np.ones((1, 2)), np.ones((1, 3)))
    for name in ("x", "y"):
        for k in ("grad", "own", "scat", "mag", "cnt"):
            np.testing.assert_array_equal(one[name][k], chamfer_loss_ref.gradients(x, y, i_xy, i_yx)[name][k])
    # central differences of the weighted float64 sum (away from ties the neighbours are locally constant)
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (1, 6, 3)); y = rng.uniform(-1, 1, (1, 9, 3))
    w, v = rng.normal(0, 1, (1, 6)), rng.normal(0, 1, (1, 9))
    w[0, 1] = v[0, 4] = 0.0
    g = ref.gradients(x, y, ref.nearest(x, y)[1], ref.nearest(y, x)[1], w, v)
    for name, c in (("x", x), ("y", y)):
        for p in range(c.shape[1]):
            for k in range(3):
                e = np.zeros_like(c); e[0, p, k] = 1e-6
                fd = ((ref.value(x + e, y, w, v) - ref.value(x - e, y, w, v)) if name == "x"
                      else (ref.value(x, y + e, w, v) - ref.value(x, y - e, w, v))) / 2e-6
                assert abs(fd - g[name]["grad"][0, p, k]) < 1e-6
