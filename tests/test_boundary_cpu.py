"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol
include/reart_hip.h declares, and the host mirror raises the reference's errors.  No compute."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "reart_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(reart_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from reart_amd import _lib

    L = _lib.lib()
    names = _declared_symbols()
    assert len(names) >= 8
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/reart_hip.h but not exported"
        assert n in _lib.PROTOTYPES, f"{n} has no ctypes prototype in reart_amd/_lib.py"
    assert set(_lib.PROTOTYPES) == set(names)
    assert L.reart_version() >= 100
    assert L.reart_status_string(-2) == b"unsupported configuration"


def test_no_cpu_fallback():
    from reart_amd.utils.chamfer import ChamferDistance, knn_points
    from reart_amd.knn_cuda import KNN

    a = torch.zeros(1, 8, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        knn_points(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ChamferDistance()(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KNN(k=1, transpose_mode=True)(a, a)


def test_chamfer_argument_errors_match_reference():
    """Same exception types as utils/chamfer.py:34-76,261-264."""
    from reart_amd.utils.chamfer import ChamferDistance, knn_points

    cd = ChamferDistance()
    a = torch.zeros(2, 8, 3)
    with pytest.raises(TypeError):
        cd([1, 2], a)
    with pytest.raises(ValueError, match="same batchsize"):
        cd(a, torch.zeros(3, 8, 3))
    with pytest.raises(ValueError, match="same dimensionality"):
        cd(a, torch.zeros(2, 8, 2))
    with pytest.raises(ValueError, match="Reduction"):
        cd(a, a, reduction="max")
    with pytest.raises(ValueError, match="same batch dimension"):
        knn_points(a, torch.zeros(3, 8, 3))
    with pytest.raises(ValueError, match="same point dimension"):
        knn_points(a, torch.zeros(2, 8, 4))


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under reart_amd/ may reference it."""
    pkg = os.path.join(ROOT, "reart_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", src, flags=re.M), f
                assert "liboracle" not in src, f


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    """Argument checks come before any device work: status codes, never exit() (SURVEY.md 8b error convention)."""
    from reart_amd import _lib

    L = _lib.lib()
    bad = -1   # REART_ERR_INVALID_ARG
    assert L.reart_screw_fit(None, 3, 2, None, 4, 0, None, None, None, None, None, None, None, 0, None) == bad
    assert L.reart_part_fps(None, None, 10, None, 2, 20, 0, None, None, None) == bad
    assert L.reart_part_pair_cost(None, None, 0, 3, 20, None, None, None, None) == bad
    assert L.reart_group_temporal_err(None, 2, 10, None, None, 3, None, None, None) == bad
    assert L.reart_cdist(None, None, 1, 4, 4, None, None) == bad
    assert L.reart_cdist(None, None, 1, 70000, 4, None, None) == bad
    assert L.reart_lap_auction(None, 1, 5000, None, None, None, None, None, 0, None) == bad      # n above 4096
    assert L.reart_lap_workspace_bytes(3, 4096) > L.reart_lap_workspace_bytes(3, 2048) > 0
    assert L.reart_lap_workspace_bytes(3, 4097) == 0
    assert L.reart_screw_fit_workspace_bytes(19, 400) == 400 * 6 * 4
    # the measurement aid of the headline's roofline: shapes are validated before anything is launched
    import ctypes
    shape = (ctypes.c_int * 5)(128, 320, 4096, 1, 6)
    assert L.reart_relax_step_floor(None, 1, 1, 1, 1 << 20, None) == bad
    assert L.reart_relax_step_floor(shape, 1, 1, None, 1 << 20, None) == bad
    assert L.reart_relax_step_floor(shape, 9, 1, 1, 1 << 20, None) == bad                    # at most eight launches per iteration
    assert L.reart_relax_step_floor(shape, 1, 1, 1, 1024, None) == bad                       # workspace below 64 KB
    shape[1] = 2048
    assert L.reart_relax_step_floor(shape, 1, 1, 1, 1 << 20, None) == bad                    # block size above 1024
    # empty problems are fine
    assert L.reart_part_fps(1, 1, 10, 1, 0, 20, 0, 1, 1, None) == 0
    assert L.reart_cdist(None, None, 0, 4, 4, None, None) == 0


INVALID_ARG, UNSUPPORTED = -1, -2   # REART_ERR_INVALID_ARG, REART_ERR_UNSUPPORTED (include/reart_hip.h)


def _relax_case(**over):
    """(cfg, bufs, workspace bytes) of a small fused-step problem whose buffers are a non-null dummy address: good for
    calls that are refused before anything is launched."""
    import ctypes

    from reart_amd import relax

    cfg = relax.RelaxConfig(N=256, P=4, B=3, H=16, cano_idx=1, use_flow=1, flow_k=3, M_max=64, M_total=192, n_iter=100, ring=8,
                            lambda_flow=1.0, trans_lr=1e-2, seg_lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, start_tau=1.0,
                            end_tau=0.1, use_boxes=1, lambda_assign=1.0)
    for k, v in over.items():
        setattr(cfg, k, v)
    dummy = 4096
    bufs = relax.RelaxBuffers(**{n: dummy for n, _ in relax.RelaxBuffers._fields_ if n not in ("aux_stream", "ev_fork", "ev_join")})
    return cfg, bufs, relax._lib_fns().reart_relax_workspace_bytes(ctypes.byref(cfg))


def _step(cfg, bufs, nbytes, workspace=4096):
    import ctypes

    from reart_amd import relax

    return relax._lib_fns().reart_relax_step(ctypes.byref(cfg) if cfg is not None else None,
                                             ctypes.byref(bufs) if bufs is not None else None, workspace, nbytes, None)


def _step_batch(cases, K=None):
    import ctypes

    from reart_amd import relax

    n = max(len(cases), 1)
    cfgs = (relax.RelaxConfig * n)(*[c[0] for c in cases])
    bufs = (relax.RelaxBuffers * n)(*[c[1] for c in cases])
    ws = (ctypes.c_void_p * n)(*[4096] * n)
    nbytes = max([c[2] for c in cases], default=0)
    return relax._lib_fns().reart_relax_step_batch(cfgs, bufs, ws, nbytes, len(cases) if K is None else K, None)


def test_step_entries_refuse_before_they_launch():
    """Every refusal of reart_relax_step / reart_relax_step_batch is decided from the configuration and the buffer
    addresses alone, before the first launch, so each is checked here without a device and with dummy addresses.  Left
    out: what can only be decided after a launch (a kernel the runtime refuses: REART_ERR_LAUNCH) and the instances of a
    batch that agree in geometry but differ in a tuning switch, which the launchers of the kernels turn down."""
    good = _relax_case()
    assert good[2] > 0
    # reart_relax_step
    assert _step(None, good[1], good[2]) == INVALID_ARG
    assert _step(good[0], None, good[2]) == INVALID_ARG
    assert _step(*good, workspace=None) == INVALID_ARG
    assert _step(good[0], good[1], good[2] - 1) == INVALID_ARG
    cfg, bufs, nbytes = _relax_case()
    bufs.W1 = None
    assert _step(cfg, bufs, nbytes) == INVALID_ARG
    assert _step(_relax_case(P=33)[0], good[1], good[2]) == INVALID_ARG
    assert _step(_relax_case(flow_k=2)[0], good[1], good[2]) == UNSUPPORTED
    # reart_relax_step_batch: the instance count, then what no batch takes -- also not a batch of one
    assert _step_batch([good], K=0) == INVALID_ARG
    assert _step_batch([good] * 7) == INVALID_ARG
    for over in (dict(use_grid=1), dict(search_mode=1), dict(use_boxes=0), dict(tune_cloud=1)):
        assert _step_batch([_relax_case(**over)]) == UNSUPPORTED, over
    assign = dict(use_assign=1, use_flow=0)
    assert _step_batch([_relax_case(**assign), _relax_case(N=512, **assign)]) == INVALID_ARG
    cfg, bufs, nbytes = _relax_case(**assign)
    bufs.assign_map = None
    assert _step_batch([(cfg, bufs, nbytes)]) == INVALID_ARG


def test_step_refusals_need_no_call_of_the_runtime():
    """Refusals that must not depend on the runtime's state (no device here; on a device, an earlier failed launch of
    somebody else must not be reported in their place): Chamfer-mode instances that cannot share their launches, and a
    single step with the assignment loss and no assign_map, which is refused before its forward is launched."""
    cfg, bufs, nbytes = _relax_case(use_assign=1)
    bufs.assign_map = None
    assert _step(cfg, bufs, nbytes) == INVALID_ARG
    good = _relax_case()
    for over in (dict(N=512), dict(B=4), dict(use_flow=0), dict(use_assign=1)):
        assert _step_batch([good, _relax_case(**over)]) == INVALID_ARG, over


def test_structure_wrappers_have_no_cpu_fallback():
    from reart_amd.utils import graph_utils as gu
    from reart_amd.utils.lap import cdist
    from reart_amd.utils.model_utils import compute_ass_err, compute_group_temporal_err

    t = torch.eye(4).repeat(2, 3, 1, 1)
    for call in (lambda: gu.screw_fit(t), lambda: gu.fps_sample_cano(torch.zeros(8, 3), torch.zeros(8, dtype=torch.long), torch.zeros(1, dtype=torch.long)),
                 lambda: gu.compute_spatial_cost(torch.zeros(2, 4, 3)), lambda: cdist(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3)),
                 lambda: compute_ass_err(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3)),
                 lambda: compute_group_temporal_err(torch.zeros(2, 4, 3), torch.zeros(4, dtype=torch.long))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_relax_config_struct_matches_the_header():
    """The ctypes mirror of reart_relax_config lists the header's fields in the header's order with the header's types
    (a silent mismatch would shift every tuning field)."""
    import ctypes
    import re

    from reart_amd.relax import RelaxConfig

    hdr = open(os.path.join(ROOT, "include", "reart_hip.h")).read()
    body = hdr[hdr.index("typedef struct reart_relax_config {"):hdr.index("} reart_relax_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"\b(int|float|uint64_t)\s+([a-zA-Z_0-9,\s]+);", body):
        for nm in names.split(","):
            fields.append((nm.strip(), typ))
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64}
    assert [(n, ctype[t]) for n, t in fields] == list(RelaxConfig._fields_)
