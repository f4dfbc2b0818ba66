"""CPU side of the gradients through the transforms (tests/transform_grad_ref.py): the float64 restatements that
tests/test_transform_grad_gpu.py compares the kernels with are held against themselves here --
  * evaluated in float32 they stay inside the bound on every case the GPU test runs, so a correct float32 implementation
    passes on rounding alone, and
  * a restatement with one planted error is rejected by the same comparison;
and every new entry point of csrc/transform_grad.hip refuses NULL pointers and a part count above its limit before it
launches anything (no device here)."""
import functools

import numpy as np
import pytest
import torch

from tests import transform_grad_ref as tr

F32, F64 = torch.float32, torch.float64


@functools.lru_cache(maxsize=None)
def _kin64(name, use):
    return tr.kin_grads(tr.make_kin_case(name), use)[1]


@functools.lru_cache(maxsize=None)
def _base64(name, use):
    return tr.base_grads(tr.make_base_case(name), use)[1]


# ------------------------------------------------------------------------------------ float32 stays inside the bound
@pytest.mark.parametrize("shape", tr.R6D_SHAPES, ids=str)
def test_r6d_float32_is_inside_the_bound(shape):
    c = tr.make_r6d_case(shape)
    sp = tr.check(tr.r6d_grads(c, F32)[1], tr.r6d_grads(c)[1], what=str(shape))
    print(f"\n[r6d {shape}] float32 vs float64: {sp}")
    a1, a2 = c["d6"].reshape(-1, 6)[0, :3].astype(np.float64), c["d6"].reshape(-1, 6)[0, 3:].astype(np.float64)
    b1 = a1 / np.linalg.norm(a1)
    rest = np.linalg.norm(a2 - (b1 @ a2) * b1)
    assert 1e-12 * 1e6 < rest < 2 * tr.R6D_STEP * np.linalg.norm(a2) / 1.7   # near-parallel, and nowhere near eps


@pytest.mark.parametrize("shape", tr.PCT_SHAPES, ids=str)
def test_pc_transform_float32_is_inside_the_bound(shape):
    c = tr.make_pct_case(*shape)
    ref = tr.pct_grads(c)[1]
    sp = tr.check(tr.pct_grads(c, F32)[1], ref, what=str(shape))
    print(f"\n[pc_transform {shape}] float32 vs float64: {sp}")
    assert (ref["pose"][:, :, 3, :] == 0).all() and (ref["pose"][:, c["empty"]] == 0).all()
    assert bool(c["empty"]) == (shape[1] >= 3)


@pytest.mark.parametrize("use", tr.USES)
@pytest.mark.parametrize("name", list(tr.KIN_CASES))
def test_kinematic_float32_is_inside_the_bound(name, use):
    c = tr.make_kin_case(name)
    sp = tr.check(tr.kin_grads(c, use, F32)[1], _kin64(name, use), what=f"{name}/{use}")
    print(f"\n[{name}/{use}] float32 vs float64: {sp}")


@pytest.mark.parametrize("name", [n for n, v in tr.KIN_CASES.items() if not v[4]])
def test_fk_alone_float32_is_inside_the_bound(name):
    c = tr.make_kin_case(name)
    ref = tr.kin_grads(c, "trans", cloud=False)[1]
    tr.check(tr.kin_grads(c, "trans", F32, cloud=False)[1], ref, what=name)
    with_cloud = _kin64(name, "trans")                             # the cloud takes no part in a loss on trans_list
    assert all(np.array_equal(ref[k], with_cloud[k]) for k in ref) and not with_cloud["x"].any()


def test_prismatic_placeholders_take_no_gradient():
    c = tr.make_kin_case("random_P6_mixed_joint_types")
    g = _kin64("random_P6_mixed_joint_types", "both")
    pris = c["prismatic"]
    assert pris.any() and not pris.all()
    assert (g["theta"][:, pris] == 0).all() and (g["distance"][:, ~pris] == 0).all()
    assert (g["theta"][:, ~pris] != 0).all() and (g["distance"][:, pris] != 0).all()


@pytest.mark.parametrize("use", tr.USES)
@pytest.mark.parametrize("name", list(tr.BASE_CASES))
def test_base_float32_is_inside_the_bound(name, use):
    c = tr.make_base_case(name)
    sp = tr.check(tr.base_grads(c, use, F32)[1], _base64(name, use), what=f"{name}/{use}")
    print(f"\n[{name}/{use}] float32 vs float64: {sp}")
    if use == "trans":                                             # trans_list depends on the poses alone
        assert not any(_base64(name, use)[k].any() for k in ("W1", "b1", "W2", "cano"))


# ----------------------------------------------------------------------------------- a planted error is rejected
def _rejected(got, ref, what):
    with pytest.raises(AssertionError, match="gradient spread above"):
        tr.check(got, ref, what=what)


def test_a_scaled_tensor_is_rejected():
    c = tr.make_r6d_case((257, 6))
    _rejected(tr.r6d_grads(c, mutate=("scale", "d6"))[1], tr.r6d_grads(c)[1], "d6")
    c = tr.make_pct_case(3, 20, 300)
    for k in ("cano", "pose"):
        _rejected(tr.pct_grads(c, mutate=("scale", k))[1], tr.pct_grads(c)[1], k)
    for name in ("star_P6_distance", "random_P64_root_motion_distance"):
        ref = _kin64(name, "both")
        for k in ref:
            _rejected(tr.kin_grads(tr.make_kin_case(name), "both", mutate=("scale", k))[1], ref, f"{name}/{k}")
    for name in ("N200_P5_B3_tau1", "N100_P20_B100_tau5_long_path"):
        ref = _base64(name, "both")
        for k in tr.BASE_PARAMS:
            _rejected(tr.base_grads(tr.make_base_case(name), "both", mutate=("scale", k))[1], ref, f"{name}/{k}")


@pytest.mark.parametrize("use", ("both", "trans"))
def test_a_row3_upstream_that_is_not_ignored_is_rejected(use):
    for name in tr.KIN_CASES:
        if name != "P1_no_edges":                                  # a single part: trans_list is the constant identity
            _rejected(tr.kin_grads(tr.make_kin_case(name), use, mutate="row3")[1], _kin64(name, use), name)
    for name in tr.BASE_CASES:
        _rejected(tr.base_grads(tr.make_base_case(name), use, mutate="row3")[1], _base64(name, use), name)


def test_a_dropped_inverse_temperature_on_the_cano_path_is_rejected():
    for name, (_, _, _, tau, _) in tr.BASE_CASES.items():
        c = tr.make_base_case(name)
        got = tr.base_grads(c, "both", mutate="drop_tau_cano")[1]
        ref = _base64(name, "both")
        if tau == 1.0:                                             # nothing to drop
            tr.check(got, ref, what=name)
            continue
        assert all(np.array_equal(got[k], ref[k]) for k in tr.rg.PARAMS), name       # the parameters' paths keep theirs
        sp = tr.spread(got, ref)
        assert sp["cano"] > tr.TOL, (name, sp)
        _rejected(got, ref, name)


# ------------------------------------------------------------------------------------------- refusals, no device
def test_new_entries_refuse_null_pointers_and_too_many_parts():
    from reart_amd import _lib

    L = _lib.lib()
    bad, a = -1, 4096          # REART_ERR_INVALID_ARG; a non-null dummy address: these calls are refused before any launch
    assert L.reart_rotation_6d_to_matrix_backward(None, a, 4, a, None) == bad
    assert L.reart_rotation_6d_to_matrix_backward(a, None, 4, a, None) == bad
    assert L.reart_rotation_6d_to_matrix_backward(a, a, 4, None, None) == bad
    assert L.reart_rotation_6d_to_matrix_backward(a, a, -1, a, None) == bad
    assert L.reart_rotation_6d_to_matrix_backward(None, None, 0, None, None) == 0

    assert L.reart_pose_trans_backward(None, a, 6, a, a, 0, None) == bad
    assert L.reart_pose_trans_backward(a, None, 6, a, a, 0, None) == bad
    assert L.reart_pose_trans_backward(a, a, 6, None, a, 1, None) == bad
    assert L.reart_pose_trans_backward(a, a, 6, a, None, 1, None) == bad
    assert L.reart_pose_trans_backward(None, None, 0, None, None, 0, None) == 0

    ws = L.reart_compute_pc_transform_backward_workspace_bytes(70, 3, 2)
    assert ws > 0 and L.reart_compute_pc_transform_backward_workspace_bytes(70, 1025, 2) == 0
    assert _lib.PC_GRAD_MAX_P == 1024
    for i in range(4):         # cano, pose, part, G
        ptrs = [a] * 4
        ptrs[i] = None
        assert L.reart_compute_pc_transform_backward(*ptrs, 70, 3, 2, a, a, a, ws, None) == bad, i
    assert L.reart_compute_pc_transform_backward(a, a, a, a, 70, 3, 2, a, a, None, ws, None) == bad      # g_pose needs the workspace
    assert L.reart_compute_pc_transform_backward(a, a, a, a, 70, 3, 2, a, a, a, ws - 1, None) == bad
    assert L.reart_compute_pc_transform_backward(a, a, a, a, 70, 1025, 2, a, a, a, 1 << 30, None) == bad
    assert L.reart_compute_pc_transform_backward(a, a, a, a, 70, 0, 2, a, a, a, ws, None) == bad

    P, B, E, N = 6, 3, 5, 150
    ws = L.reart_fk_backward_workspace_bytes(P, B, E)

    def fk_bt(N=N, P=P, E=E, nul=(), ws_bytes=ws):
        # x part G | parent edge order | axis moment theta distance | trans g_trans | g_axis g_moment g_theta g_dist g_x | ws
        p = {k: a for k in ("x", "part", "G", "parent", "edge", "order", "axis", "moment", "theta", "dist", "trans", "g_trans",
                            "g_axis", "g_moment", "g_theta", "g_dist", "g_x", "ws")}
        p.update({k: None for k in nul})
        return L.reart_fk_backward_trans(p["x"], p["part"], p["G"], N, p["parent"], p["edge"], p["order"], P, p["axis"], p["moment"],
                                         p["theta"], p["dist"], B, E, p["trans"], p["g_trans"], p["g_axis"], p["g_moment"],
                                         p["g_theta"], p["g_dist"], p["g_x"], p["ws"], ws_bytes, None)

    for k in ("x", "part", "G", "parent", "edge", "order", "axis", "moment", "theta", "trans", "g_axis", "g_moment", "g_theta", "ws"):
        assert fk_bt(nul=(k,)) == bad, k
    assert fk_bt(P=65, E=64, ws_bytes=1 << 30) == bad               # P above 64, as reart_fk_backward
    assert fk_bt(ws_bytes=ws - 1) == bad
    assert fk_bt(N=0, nul=("x", "part", "G", "parent")) == bad      # an empty cloud excuses x, part and G only

    N, P, B, H = 200, 5, 3, 128
    ws = L.reart_base_backward_cano_workspace_bytes(P, B)
    assert ws >= 4 * 12 * B * P
    assert L.reart_base_backward_cano_workspace_bytes(33, B) == 0 and L.reart_base_backward_cano_workspace_bytes(P, 1025) == 0

    def cano_bw(P=P, B=B, H=H, tau=1.0, nul=(), ws_bytes=ws):
        p = {k: a for k in ("cano", "W1", "b1", "W2", "p6d", "pt", "yT", "hT", "hard", "G", "g_cano", "ws")}
        p.update({k: None for k in nul})
        return L.reart_base_backward_cano(p["cano"], N, P, B, p["W1"], p["b1"], p["W2"], H, p["p6d"], p["pt"], p["yT"], p["hT"],
                                          p["hard"], tau, p["G"], p["g_cano"], p["ws"], ws_bytes, None)

    for k in ("cano", "W1", "W2", "p6d", "pt", "yT", "hT", "hard", "G", "g_cano", "ws"):
        assert cano_bw(nul=(k,)) == bad, k
    assert cano_bw(P=33, ws_bytes=1 << 30) == bad                   # P above 32, as reart_base_forward
    assert cano_bw(B=1025, ws_bytes=1 << 30) == bad                 # B above REART_MAX_POSE_LEN
    assert cano_bw(ws_bytes=ws - 1) == bad
    assert cano_bw(tau=0.0) == bad
    assert cano_bw(H=257) == -2                                      # REART_ERR_UNSUPPORTED: the weights would not fit in LDS


def test_wrappers_have_no_cpu_fallback():
    from reart_amd.screw_se3 import rotation_6d_to_matrix
    from reart_amd.utils.kinematic_utils import fk
    from reart_amd.utils.model_utils import compute_pc_transform

    for call in (lambda: rotation_6d_to_matrix(torch.zeros(2, 6, requires_grad=True)),
                 lambda: compute_pc_transform(torch.zeros(4, 3, requires_grad=True), torch.eye(4).repeat(1, 2, 1, 1),
                                              torch.zeros(4, dtype=torch.long)),
                 lambda: fk({}, [0, 1], {"1_0": 0}, torch.zeros(1, 3, requires_grad=True), torch.zeros(1, 3), torch.zeros(2, 1))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
