"""CPU: the float64 restatement tests/kin_ref.py of the kinematic projection's pieces, before tests/test_kinematic_long_gpu.py
holds the kernels to it.
 (a) fk_ref with autograd reproduces the reference's own forward and autograd gradients (tests/golden/kinematic.npz, and the
     variant with prismatic joints and distances of kinematic_root.npz) within the bounds tests/test_oracle_golden_cpu.py and
     tests/test_kinematic_root_gpu.py hold the oracle and the kernels to.
 (b) a prismatic joint, theta = float32(1e-6), translates by d l: the branch is decided in float32.
 (c) the comparisons of the GPU test (check_fk, check_post) reject each of a set of planted errors, given a correct float32
     evaluation in the kernel's place; and that float32 evaluation itself passes them with room to spare (printed: -s).
Measured here: float32 FK within 6.2e-7 of max(1, max|out|) and 1.6e-6 of max|g| over FK_CASES (7.7e-6 for theta at B = 1, N = 5,
whose one joint is the small rotation under the clamp); bounds 5e-6 / 2e-4.  The float32 kin_post is within 1.48e-7 of max|G| over
the 27 cases of the GPU test, so reart_kin_post is allowed 1.18e-6."""
import os

import numpy as np
import pytest
import torch

from tests import kin_ref as kr

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
t64 = kr._t64


def test_fk_ref_reproduces_the_reference_golden():
    k = np.load(os.path.join(G, "kinematic.npz"))
    axis, moment, theta = (t64(k[n]).requires_grad_(True) for n in ("axis", "moment", "theta"))
    # (the checkpoint's own joint values: one of them has |theta| |l| = 0.0093, next to the clamp; the decision is the float32 one
    # on both sides here, so the inputs' distance from the thresholds is not asked for)
    trans = kr.fk_ref(k["parent"], k["edge_of_part"], k["order"], axis, moment, theta, check=False)
    np.testing.assert_allclose(trans.detach().numpy(), k["trans"], rtol=0, atol=1e-6)
    out = kr.apply_parts(t64(k["input_pc"]), trans, k["seg"])
    np.testing.assert_allclose(out.detach().numpy(), k["out"], rtol=0, atol=1e-6)
    (out * t64(k["G"])).sum().backward()
    for got, name in ((axis.grad, "g_axis"), (moment.grad, "g_moment"), (theta.grad, "g_theta")):
        np.testing.assert_allclose(got.numpy(), k[name], rtol=0, atol=2e-5 * np.abs(k[name]).max(), err_msg=name)


def test_fk_ref_reproduces_the_golden_with_prismatic_joints():
    """kinematic_root.npz: joint types, distances and a per-frame root motion (composed here as a constant)."""
    g = np.load(os.path.join(G, "kinematic_root.npz"))
    assert g["prismatic"].any() and not g["prismatic"].all()
    P = int(g["reverse_topo"].shape[0])
    parent, edge_of = np.full(P, -1, np.int32), np.full(P, -1, np.int32)
    for e, (c, p) in enumerate(zip(g["edge_child"].tolist(), g["edge_parent"].tolist())):
        parent[c], edge_of[c] = p, e
    axis, moment, theta, dist = (t64(g[n]).requires_grad_(True) for n in ("axis", "moment", "theta", "distance"))
    th, d = kr.effective_joint_values(theta, dist, g["prismatic"])
    trans = t64(g["root_trans"])[:, None] @ kr.fk_ref(parent, edge_of, g["reverse_topo"], axis, moment, th, d, check=False)
    np.testing.assert_allclose(trans.detach().numpy(), g["trans"], rtol=0, atol=2e-6)
    out = kr.apply_parts(t64(g["input_pc"]), trans, g["seg"])
    np.testing.assert_allclose(out.detach().numpy(), g["out"], rtol=0, atol=2e-6)
    (out * t64(g["G"])).sum().backward()
    for got, key in ((axis.grad, "g_axis"), (moment.grad, "g_moment"), (theta.grad, "g_theta"), (dist.grad, "g_distance")):
        assert np.abs(got.numpy() - g[key]).max() <= 2e-4 * max(1.0, np.abs(g[key]).max()), key
    pris = g["prismatic"]
    assert (theta.grad.numpy()[:, pris] == 0).all() and (dist.grad.numpy()[:, ~pris] == 0).all()     # masked entries take no gradient


def test_prismatic_placeholder_takes_the_float32_branch():
    """theta = float32(1e-6), d = 0.05: NOT the no-rotation branch (in float32 |theta| < 1e-6 is false) -> a translation of d l.
    Decided on the doubles, 9.99999997e-7 < 1e-6 holds and the joint would move by theta l = 1e-6 l."""
    l = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8]], np.float32)
    m = np.array([[0.02, -0.01, 0.0], [0.0, 0.03, 0.0]], np.float32)
    theta = np.full((1, 2), 1e-6, np.float32)
    assert float(theta[0, 0]) < 1e-6 and not (theta[0, 0] < np.float32(1e-6))                        # the trap itself
    no_rot, clamped = kr.fk_decisions(l, theta)
    assert not no_rot.any() and clamped.all()
    parent, edge_of, order = np.array([-1, 0, 1], np.int32), np.array([-1, 0, 1], np.int32), np.arange(3, dtype=np.int32)
    T = kr.fk_ref(parent, edge_of, order, t64(l), t64(m), t64(theta), t64(np.full((1, 2), 0.05, np.float32)))[0].numpy()
    np.testing.assert_allclose(T[1, :3, 3], 0.05 * l[0].astype(np.float64), rtol=0, atol=2e-7)
    np.testing.assert_allclose(T[1, :3, :3], np.eye(3), rtol=0, atol=2e-6)
    np.testing.assert_allclose(T[2, :3, 3], 0.05 * (l[0].astype(np.float64) + l[1]), rtol=0, atol=4e-7)


def test_inputs_next_to_a_threshold_are_refused():
    l = np.array([[0.0, 0.0, 1.0]], np.float32)
    for bad in (0.01, 0.0085, 5e-5, np.pi - 5e-4):
        with pytest.raises(AssertionError, match="threshold"):
            kr.assert_clear_of_thresholds(l, np.array([[0.5], [bad]], np.float32))
    kr.assert_clear_of_thresholds(l, np.array([[3e-3], [1e-6], [-2.4], [0.02]], np.float32))


@pytest.mark.parametrize("kind,P", [("chain", 64), ("star", 64), ("random", 33), ("random", 2)])
def test_random_tree_is_a_tree_in_a_shuffled_numbering(kind, P):
    rng = np.random.default_rng(P)
    parent, edge_of, order, owners = kr.random_tree(rng, P, kind, empty=P // 3)
    assert sorted(order.tolist()) == list(range(P)) and (parent < 0).sum() == 1 and parent[order[0]] == -1
    seen = set()
    for c in order:                                             # parents precede their children
        assert parent[c] < 0 or int(parent[c]) in seen
        seen.add(int(c))
    assert sorted(edge_of[edge_of >= 0].tolist()) == list(range(P - 1)) and edge_of[order[0]] == -1
    assert len(owners) == P - P // 3
    depth = {int(order[0]): 0}
    for c in order[1:]:
        depth[int(c)] = depth[int(parent[c])] + 1
    assert max(depth.values()) == {"chain": P - 1, "star": 1}.get(kind, max(depth.values()))
    if P > 2:
        assert not np.array_equal(order, np.arange(P))


@pytest.mark.parametrize("name", list(kr.FK_CASES))
def test_float32_fk_fits_the_bounds(name):
    """A correct float32 evaluation on every shape of the GPU test: within the bounds with room to spare, so that a kernel
    outside them is wrong and not merely rounded."""
    c = kr.make_fk_case(name)
    ref = kr.fk_case_ref(c)
    out, grads = kr.fk_case_f32(c)
    sp = kr.check_fk(out, grads, ref, what=name)
    print(f"\n[{name}] float32 CPU vs float64: " + "  ".join(f"{k} {v:.1e}" for k, v in sp.items()))
    assert sp["out"] <= 0.2 * kr.FK_FWD_TOL and max(v for k, v in sp.items() if k != "out") <= 0.1 * kr.FK_GRAD_TOL, sp
    if c["prismatic"] is not None:
        assert (ref["grads"]["theta"][:, c["prismatic"]] == 0).all() and (ref["grads"]["distance"][:, ~c["prismatic"]] == 0).all()
        assert np.abs(ref["grads"]["distance"][:, c["prismatic"]]).min() > 0


def test_check_fk_rejects_a_frame_left_out_of_the_axis_sum():
    """Frame 64 is the one live lane of the second workgroup at B = 65."""
    c = kr.make_fk_case("second_workgroup_one_lane")
    out, grads = kr.fk_case_f32(c)
    kr.check_fk(out, grads, kr.fk_case_ref(c))
    with pytest.raises(AssertionError, match="gradient spread"):
        kr.check_fk(out, grads, kr.fk_case_ref(c, mutate=("skip_axis_frame", 64)), what="frame 64 skipped")


def test_float32_kin_post_spread(oracle):
    sp = kr.post_f32_spread()
    print(f"\nfloat32 kin_post vs float64 over {len(kr.POST_SHAPES) * len(kr.POST_VARIANTS)} cases: {sp:.2e} of max|G| -> bound {kr.post_g_tol():.2e}")
    assert 1e-9 < sp < 5e-7, sp                 # a handful of float32 roundings: neither exact nor more
    for B, c in kr.POST_SHAPES:
        case = kr.make_post_case(B, c)
        assert case["margin"] >= kr.MASK_MARGIN and min(case["lens"]) == 3 and (B == 1 or max(case["lens"]) == 200)


# (at B = 1 with the canonical frame first, comp[:-1] IS the canonical frame, which takes no gradient: nothing to flip there)
PLANTED = [(B, c, m) for B, c in kr.POST_SHAPES for m in ("drop_last_frame", "flip_prev_sign", "cano_shift", "single_lambda")
           if (B, c, m) != (1, 0, "flip_prev_sign")]


@pytest.mark.parametrize("B,c,mutate", PLANTED, ids=[f"B{B}-c{c}-{m}" for B, c, m in PLANTED])
def test_check_post_rejects_planted_errors(oracle, B, c, mutate):
    case = kr.make_post_case(B, c)
    for _, flow, robust in kr.POST_VARIANTS[1:]:
        a, kw = kr.post_args(case, flow, robust)
        ref = kr.kin_post_ref(*a, **kw)
        got = kr.kin_post_f32(*a, **kw)
        kr.check_post(got, ref["matched"], ref["losses"].astype(np.float32), ref, kr.post_g_tol(), what="unplanted")
        bad = kr.kin_post_ref(*a, mutate=mutate, **kw)
        with pytest.raises(AssertionError, match="dL/d pc_trans off"):
            kr.check_post(got, ref["matched"], ref["losses"].astype(np.float32), bad, kr.post_g_tol(), what=mutate)


def test_check_post_rejects_wrong_matches_and_losses(oracle):
    case = kr.make_post_case(2, 1)
    a, kw = kr.post_args(case, True, False)
    ref = kr.kin_post_ref(*a, **kw)
    got = kr.kin_post_f32(*a, **kw)
    m = ref["matched"].copy()
    m[1, 5] = np.nextafter(m[1, 5], np.float32(1))
    with pytest.raises(AssertionError, match="matched"):
        kr.check_post(got, m, ref["losses"], ref, kr.post_g_tol())
    for i in range(3):
        l = ref["losses"].copy()
        l[i] *= 1.0 + 3e-6
        with pytest.raises(AssertionError, match="loss"):
            kr.check_post(got, ref["matched"], l, ref, kr.post_g_tol())
