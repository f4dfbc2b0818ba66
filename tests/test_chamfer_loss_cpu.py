"""CPU-side checks of the ChamferLoss operator: the boundary (header, ctypes mirror, exports), argument checks of both
entries before any device work, the host mirror's refusals and dispatch, and the float64 restatement the GPU tests use."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG = 0, -1


def _call(L, x=4096, y=4096, N=2, P1=8, P2=8, sxy=4096, syx=4096, same=0, loss=4096, gx=4096, gy=None, bits=4096, ws=4096,
          nbytes=None):
    if nbytes is None:
        nbytes = L.reart_chamfer_loss_workspace_bytes(N, P1, P2)
    return L.reart_chamfer_loss(x, y, N, P1, P2, sxy, syx, same, None, None, None, None, loss, gx, gy, bits, ws, nbytes, None)


def test_header_mirror_and_exports_agree():
    from reart_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "reart_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _lib.lib()
    for name in ("reart_chamfer_loss_workspace_bytes", "reart_chamfer_loss"):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, f"{name} is not declared in include/reart_hip.h"
        assert hasattr(L, name)
        res, args = _lib.PROTOTYPES[name]
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
    assert L.reart_chamfer_loss_workspace_bytes(3, 100, 257) > L.reart_chamfer_loss_workspace_bytes(3, 100, 130) > need
    for shape in ((-1, 8, 8), (2, -1, 8), (2, 8, -1), (0, 8, 8), (2, 0, 8), (2, 8, 0), (65536, 8, 8), (4, 1 << 29, 8)):
        assert L.reart_chamfer_loss_workspace_bytes(*shape) == 0, shape
    for null in ("x", "y", "sxy", "syx", "loss", "gx", "bits", "ws"):
        assert _call(L, **{null: None}) == INVALID_ARG, null
    assert _call(L, nbytes=need - 1) == INVALID_ARG
    assert _call(L, nbytes=0) == INVALID_ARG
    for neg in (dict(N=-1), dict(P1=-1), dict(P2=-1)):
        assert _call(L, nbytes=1 << 20, **neg) == INVALID_ARG, neg
    # empty problems: fine, nothing is launched (no device here) and nothing is dereferenced
    for empty in (dict(N=0), dict(P1=0), dict(P2=0)):
        assert _call(L, x=None, y=None, sxy=None, syx=None, loss=None, gx=None, bits=None, ws=None, nbytes=0, **empty) == OK, empty


def test_host_tensors_have_no_cpu_fallback():
    from reart_amd.networks.loss import recon_loss
    from reart_amd.utils.chamfer import ChamferLoss
    from reart_amd.utils.flow_utils import blend_anchor_motion_batch
    from reart_amd.knn_cuda import KNN

    a = torch.zeros(1, 8, 3)
    mod = ChamferLoss()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mod(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mod(a.double(), a.double())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        recon_loss(a, a, mod)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mod.seed(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        blend_anchor_motion_batch(a, a, a, None, KNN(k=3, transpose_mode=True))
    with pytest.raises(TypeError):
        mod([1], a)


def test_recon_loss_dispatch(monkeypatch):
    """A ChamferDistance still goes through the per-point path and torch.sum; a ChamferLoss is called and its scalar
    returned as it is.  Patched: nothing here runs a GPU."""
    from reart_amd.networks import loss as loss_mod
    from reart_amd.utils import chamfer

    a, b = torch.zeros(2, 8, 3), torch.ones(2, 8, 3)
    calls = []

    def fake_cd(self, src, tgt, bidirectional=False, **kw):
        calls.append(("cd", bidirectional, src is a, tgt is b))
        return torch.full((2, 8), 0.5)

    def fake_cl(self, x, y, bidirectional=True):
        calls.append(("cl", x is a, y is b))
        return torch.tensor(7.0)

    monkeypatch.setattr(chamfer.ChamferDistance, "forward", fake_cd)
    monkeypatch.setattr(chamfer.ChamferLoss, "forward", fake_cl)
    assert float(loss_mod.recon_loss(a, b, chamfer.ChamferDistance())) == 8.0
    assert calls == [("cd", True, True, True)]
    assert float(loss_mod.recon_loss(a, b, chamfer.ChamferLoss())) == 7.0
    assert calls[1:] == [("cl", True, True)]


def test_run_robot_has_the_flag_off_by_default():
    from reart_amd import run_robot as rr

    p = rr.build_parser()
    assert p.parse_args([]).fused_losses is False
    assert p.parse_args(["--fused_losses"]).fused_losses is True


def test_reference_restatement_and_the_cluster_case():
    """The float64 restatement on a case small enough to do by hand, and the degenerate construction of the GPU test:
    all 1000 y points have one and the same nearest x point."""
    from tests import chamfer_loss_ref as ref

    x = np.array([[[0.0, 0, 0], [10.0, 0, 0]]], np.float32)
    y = np.array([[[1.0, 0, 0], [2.0, 0, 0], [9.0, 0, 0]]], np.float32)
    d_xy, i_xy = ref.nearest(x, y)
    d_yx, i_yx = ref.nearest(y, x)
    assert i_xy.tolist() == [[0, 2]] and i_yx.tolist() == [[0, 0, 1]]
    assert d_xy.tolist() == [[1.0, 1.0]] and d_yx.tolist() == [[1.0, 4.0, 1.0]]
    g = ref.gradients(x, y, i_xy, i_yx)
    assert g["x"]["grad"][0, :, 0].tolist() == [2 * (0 - 1) + 2 * ((0 - 1) + (0 - 2)), 2 * (10 - 9) + 2 * (10 - 9)]
    assert g["y"]["grad"][0, :, 0].tolist() == [2 * (1 - 0) + 2 * (1 - 0), 2 * (2 - 0), 2 * (9 - 10) + 2 * (9 - 10)]
    assert g["x"]["cnt"].tolist() == [[2, 1]] and g["y"]["cnt"].tolist() == [[1, 0, 1]]
    assert float(ref.loss(d_xy, d_yx)) == 8.0
    # central differences of the float64 loss agree with the formulas (away from ties the neighbours are locally constant)
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (1, 6, 3)); y = rng.uniform(-1, 1, (1, 9, 3))
    f = lambda x_, y_: ref.nearest(x_, y_)[0].sum() + ref.nearest(y_, x_)[0].sum()
    g = ref.gradients(x, y, ref.nearest(x, y)[1], ref.nearest(y, x)[1])
    for name, c in (("x", x), ("y", y)):
        for k in range(3):
            e = np.zeros_like(c); e[0, 2, k] = 1e-6
            fd = (f(x + e, y) - f(x - e, y)) / 2e-6 if name == "x" else (f(x, y + e) - f(x, y - e)) / 2e-6
            assert abs(fd - g[name]["grad"][0, 2, k]) < 1e-6
    xc, yc = ref.cluster_case()
    assert yc.shape[1] == 1000
    cnt = ref.counts(ref.nearest(yc, xc)[1], xc.shape[1])
    assert cnt[0, 0] == 1000 and cnt[0, 1:].sum() == 0
