"""CPU-side checks of the FlowTerm operator: the boundary (header, ctypes mirror, exports), the limits and argument checks of
its entries before any device work, the host mirror's refusals, and the float64 restatement the GPU tests use, held to the
golden vectors the reference produced."""
import os
import re

import numpy as np
import pytest
import torch

from tests.flow_term_ref import flow_term

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2
NAMES = ("reart_flow_term_workspace_bytes", "reart_flow_term_prepare", "reart_flow_term")


def test_header_mirror_and_exports_agree():
    from reart_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "reart_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _lib.lib()
    for name in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert m, f"{name} is not declared in include/reart_hip.h"
        assert hasattr(L, name)
        res, args = _lib.PROTOTYPES[name]
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == len(args)
        for p, a in zip(params, args):
            want = _lib.c_void_p if "*" in p else (_lib.c_size_t if p.startswith("size_t") else (_lib.c_float if p.startswith("float") else _lib.c_int))
            assert a is want, (name, p)


def test_workspace_is_zero_beyond_the_limits():
    from reart_amd import _lib

    L = _lib.lib()
    size = L.reart_flow_term_workspace_bytes
    assert size(3, 100, 130) > 0 and size(_lib.MAX_POSE_LEN, 64, 64) > 0
    for shape in ((0, 100, 130), (3, 0, 130), (3, 100, 2), (-1, 100, 130), (_lib.MAX_POSE_LEN + 1, 64, 64), (3, (1 << 20) + 1, 130),
                  (3, 100, (1 << 20) + 1), (1024, 1 << 20, 64), (1024, 64, 1 << 20)):
        assert size(*shape) == 0, shape
    # the size is how a call learns nr_max: it must separate every padded reference length, whatever B and N
    for B, N in ((1, 1), (3, 100), (19, 4096)):
        sizes = [size(B, N, nr) for nr in (3, 16, 17, 32, 33, 130, 144, 145, 4096)]
        assert sizes[0] == sizes[1] and sizes[2] == sizes[3] and sizes[5] == sizes[6]        # same padded length
        distinct = [sizes[0], sizes[2], sizes[4], sizes[5], sizes[7], sizes[8]]
        assert all(a < b for a, b in zip(distinct, distinct[1:])), (B, N, sizes)


def test_entries_check_their_arguments_before_any_device_work():
    from reart_amd import _lib

    L = _lib.lib()
    need = L.reart_flow_term_workspace_bytes(3, 100, 130)
    d = 4096     # a non-null dummy address: these calls are refused before anything is launched

    def prepare(ref=d, flo=d, B=3, nr=130, ws=d, nbytes=need):
        return L.reart_flow_term_prepare(ref, flo, None, B, nr, ws, nbytes, None)

    def term(x=d, cano=d, B=3, N=100, c=1, seed=d, G=d, ws=d, nbytes=need):
        return L.reart_flow_term(x, cano, None, B, N, c, 1, 0, 1e-2, 1.0, seed, None, None, None, None, None, G, 0, ws, nbytes, None)

    for null in ("ref", "flo", "ws"):
        assert prepare(**{null: None}) == INVALID_ARG, null
    assert prepare(B=0) == INVALID_ARG and prepare(nr=2) == INVALID_ARG
    assert prepare(nbytes=1024) == INVALID_ARG
    assert prepare(B=_lib.MAX_POSE_LEN + 1) == UNSUPPORTED and prepare(nr=(1 << 20) + 1) == UNSUPPORTED
    for null in ("x", "cano", "seed", "G", "ws"):
        assert term(**{null: None}) == INVALID_ARG, null
    for bad in (dict(B=0), dict(N=0), dict(c=-1), dict(c=4)):
        assert term(**bad) == INVALID_ARG, bad
    assert term(B=_lib.MAX_POSE_LEN + 1, c=0) == UNSUPPORTED and term(N=(1 << 20) + 1) == UNSUPPORTED
    # a size reart_flow_term_workspace_bytes(B, N, .) does not return names no reference length
    for nbytes in (need - 1, need + 1, need + 256, 0):
        assert term(nbytes=nbytes) == INVALID_ARG, nbytes


def test_host_tensors_have_no_cpu_fallback():
    from reart_amd.utils.flow_utils import FlowTerm

    ref, flo = [torch.zeros(4, 3)] * 2, [torch.zeros(4, 3)] * 2
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FlowTerm(ref, flo, cano_idx=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FlowTerm.forward(FlowTerm.__new__(FlowTerm), torch.zeros(2, 8, 3), torch.zeros(8, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FlowTerm.seed(FlowTerm.__new__(FlowTerm), torch.zeros(8, 3))


def test_float64_restatement_matches_the_golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "flow_term.npz"))
    refs, flows = [g[f"ref{f}"] for f in range(3)], [g[f"flow{f}"] for f in range(3)]
    assert [r.shape[0] for r in refs] == [3, 17, 130] and g["pc_trans"].shape == (3, 100, 3)
    for c in (0, 1, 3):
        for robust in (0, 1):
            tag = f"c{c}_r{robust}"
            r = flow_term(g["pc_trans"], g["cano"], refs, flows, c, robust=bool(robust))
            np.testing.assert_array_equal(r["idx"], g[f"idx_{tag}"])
            np.testing.assert_array_equal(r["mask"], g[f"mask_{tag}"])
            assert 0.05 <= r["mask"].mean() <= 0.95
            np.testing.assert_allclose(r["gt"], g[f"gt_{tag}"], rtol=0, atol=1e-5 * np.abs(g[f"gt_{tag}"]).max())
            assert abs(r["loss"] - float(g[f"loss_{tag}"])) <= 1e-5 * abs(float(g[f"loss_{tag}"]))
            np.testing.assert_allclose(r["grad"], g[f"grad_{tag}"], rtol=0, atol=1e-5 * np.abs(g[f"grad_{tag}"]).max())
        if c == 1:      # Huber's linear branch is taken, and the quadratic one
            gt, pred = r["gt"], np.diff(np.concatenate((g["pc_trans"][:c], g["cano"][None], g["pc_trans"][c:])), axis=0)
            big = np.abs(pred - gt)[r["mask"]] > 1.0
            assert big.any() and not big.all()
