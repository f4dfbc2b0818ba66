"""GPU: the kinematic projection beyond pose_len 9 and at the ends of the sequence, against the float64 restatement
tests/kin_ref.py (tests/test_kin_ref_cpu.py pins it to the reference's goldens and shows that the comparisons used here reject
planted errors) and against the host loop oracle/kinematic_step.py.

 a. csrc/kinematic.hip through utils.kinematic_utils._FK: forward and the gradients of a random functional on trees whose
    `order` is not the identity, at the sizes where the launch shape changes (kin_ref.FK_CASES: B = 64 / 65 / 130 / 1024, P = 64,
    N < 21, N % 21 != 0, parts without points, the dynamic-LDS path of pose_grad_kernel, both joint types); two backward runs
    bit-identical; P = 65 refused by the host check of both entry points.
    Bounds: forward 5e-6 max(1, max|out|), gradients 2e-4 max|g| per tensor (a float32 CPU evaluation: 6.2e-7 / 7.7e-6).
    The kernel's ratios are printed per case (run with -s); no measured figure is recorded here yet.
 b. csrc/kinpost.hip (reart_kin_post, called as KinematicEngine._post calls it) at B in {1, 2, 70} with the canonical frame at
    0, 1, B - 1, B: G = dL/d pc_trans, the matched targets (bit-equal) and the three losses (1e-6) against kin_post_ref; the
    batched blend under it against the C oracle's per-frame blend at B = 70 (masks equal, every point at least 1e-5 off the
    mask's threshold; flows rtol 2e-6).
    Bound of G: 8 x the deviation of the float32 restatement kin_post_f32 from float64 over the same cases = 8 x 1.48e-7 =
    1.18e-6 of max|G|.  The kernel's ratio is printed per case; none is recorded here yet (see a.).
 c. KinematicEngine.iteration against oracle.kinematic_step.KinematicOracle (torch-CPU FK, C-oracle FPS / cdist / blend, scipy's
    assignment) at B = 130 / 70 / 300 with the canonical frame at 0 / B / the middle: the solver sizes of utils/lap.py at
    256 // B = 1, 3 and 0.
 d. Six iterations with and without the captured graphs at B = 70, n = 512: bit-identical.
"""
import numpy as np
import pytest
import torch

from tests import kin_ref as kr

pytestmark = pytest.mark.gpu


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------------------ a. FK
def _run_fk(dev, c):
    from reart_amd.utils.kinematic_utils import _FK, _effective_joint_values

    leaves = {k: t(c[k], dev).requires_grad_(True) for k in ("axis", "moment", "theta")}
    if c["distance"] is not None:
        leaves["distance"] = t(c["distance"], dev).requires_grad_(True)
    th, d = leaves["theta"], leaves.get("distance")
    if c["prismatic"] is not None:
        th, d = _effective_joint_values(th, d, ["prismatic" if p else "revolute" for p in c["prismatic"]])
    out, trans = _FK.apply(t(c["x"], dev), t(c["part"], dev), leaves["axis"], leaves["moment"], th, d, t(c["parent"], dev),
                           t(c["edge_of"], dev), t(c["order"], dev))
    (out * t(c["Gw"], dev)).sum().backward()
    return out.detach(), trans, {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize("name", list(kr.FK_CASES))
def test_fk_forward_backward_match_float64(dev, name):
    c = kr.make_fk_case(name)
    ref = kr.fk_case_ref(c)
    out, trans, grads = _run_fk(dev, c)
    out2, trans2, grads2 = _run_fk(dev, c)
    sp = kr.check_fk(out.cpu().numpy(), {k: g.cpu().numpy() for k, g in grads.items()}, ref, what=name)
    print(f"\n[{name}] kernel vs float64: " + "  ".join(f"{k} {v:.1e}" for k, v in sp.items()))
    scale = max(1.0, float(np.abs(ref["trans"]).max()))
    assert np.abs(trans.cpu().numpy() - ref["trans"]).max() <= kr.FK_FWD_TOL * scale, name
    assert torch.equal(out, out2) and torch.equal(trans, trans2)
    for k in grads:                                             # ordered reductions, no atomics: the same bits every run
        assert torch.equal(grads[k], grads2[k]), (name, k)
    if c["prismatic"] is not None:                              # torch.where's backward: the masked entries take no gradient
        pris = t(c["prismatic"], dev)
        assert (grads["theta"][:, pris] == 0).all() and (grads["distance"][:, ~pris] == 0).all()
        assert (grads["distance"][:, pris] != 0).all()


def test_more_than_64_parts_are_refused_on_the_host(dev):
    """P = 65: both entry points return the library's invalid-argument status from their host-side checks, before any launch --
    the forward too, so that a model is refused at its first forward and not at its first backward."""
    from reart_amd import _lib
    from reart_amd.utils.kinematic_utils import _FK

    rng = np.random.default_rng(65)
    P, B, N = 65, 2, 10
    parent, edge_of, order, _ = kr.random_tree(rng, P, "chain")
    E = P - 1
    axis = rng.normal(size=(E, 3)).astype(np.float32)
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    args = (z(N, 3), torch.zeros(N, dtype=torch.long, device=dev), t(axis, dev), z(E, 3), z(B, E) + 0.5, None, t(parent, dev),
            t(edge_of, dev), t(order, dev))
    with pytest.raises(_lib.ReartHipError, match="reart_fk_forward failed") as e_fwd:
        _FK.apply(*args)
    L = _lib.lib()
    ws = torch.empty((max(int(L.reart_fk_backward_workspace_bytes(P, B, E)), 256),), dtype=torch.uint8, device=dev)
    rc = L.reart_fk_backward(_lib.ptr(args[0]), _lib.ptr(args[1]), _lib.ptr(z(B, N, 3)), N, _lib.ptr(args[6]), _lib.ptr(args[7]),
                             _lib.ptr(args[8]), P, _lib.ptr(args[2]), _lib.ptr(args[3]), _lib.ptr(args[4]), None, B, E,
                             _lib.ptr(z(B, P, 4, 4)), _lib.ptr(z(E, 3)), _lib.ptr(z(E, 3)), _lib.ptr(z(B, E)), None, _lib.ptr(ws),
                             ws.numel(), _lib.stream())
    with pytest.raises(_lib.ReartHipError, match="reart_fk_backward failed") as e_bwd:
        _lib.check(rc, "reart_fk_backward")
    assert str(e_fwd.value).split("failed:")[1] == str(e_bwd.value).split("failed:")[1]              # the same status
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ b. kin_post
def _padded_refs(dev, case):
    B, lens = case["B"], case["lens"]
    nr = max(lens)
    rp, fp = torch.zeros((B, nr, 3), device=dev), torch.zeros((B, nr, 3), device=dev)
    for f in range(B):
        rp[f, :lens[f]], fp[f, :lens[f]] = t(case["refs"][f], dev), t(case["flows"][f], dev)
    ln = torch.tensor(lens, dtype=torch.int64, device=dev) if min(lens) != nr else None       # as KinematicEngine passes them
    return rp, fp, ln, nr


def _kin_post(dev, case, flow, robust, want_matched):
    from reart_amd import _lib

    L = _lib.lib()
    B, N, n = case["B"], case["N"], case["n"]
    rp = fp = ln = None
    nr = 0
    if flow:
        rp, fp, ln, nr = _padded_refs(dev, case)
    ws = torch.empty((max(int(L.reart_kin_post_workspace_bytes(B, N, nr, 3)), 256),), dtype=torch.uint8, device=dev)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    G, matched, losses = nan(B, N, 3), (nan(B, n, 3) if want_matched else None), nan(3)
    keep = [t(case[k], dev) for k in ("pc_trans", "cano", "pc_src", "tgt", "cols", "slot")]
    rc = L.reart_kin_post(_lib.ptr(keep[0]), _lib.ptr(keep[1]), B, N, case["c"], _lib.ptr(keep[2]), _lib.ptr(keep[3]), _lib.ptr(keep[4]),
                          _lib.ptr(keep[5]), n, kr.POST_LAM_A, _lib.ptr(rp), _lib.ptr(fp), _lib.ptr(ln), nr, 3, 1, kr.POST_LAM_F,
                          int(robust), kr.POST_SMOOTH, _lib.ptr(G), _lib.ptr(matched), _lib.ptr(losses), _lib.ptr(ws), ws.numel(),
                          _lib.stream())
    _lib.check(rc, "reart_kin_post")
    torch.cuda.synchronize()
    return G.cpu().numpy(), None if matched is None else matched.cpu().numpy(), losses.cpu().numpy()


@pytest.mark.parametrize("B,c", kr.POST_SHAPES, ids=[f"B{B}-c{c}" for B, c in kr.POST_SHAPES])
def test_kin_post_matches_float64(oracle, dev, B, c):
    case = kr.make_post_case(B, c)
    assert case["margin"] >= kr.MASK_MARGIN                     # no point of the oracle's masks sits on the threshold
    tol = kr.post_g_tol()
    for i, (tag, flow, robust) in enumerate(kr.POST_VARIANTS):
        a, kw = kr.post_args(case, flow, robust)
        ref = kr.kin_post_ref(*a, **kw)
        G, matched, losses = _kin_post(dev, case, flow, robust, want_matched=True)
        sp = kr.check_post(G, matched, losses, ref, tol, what=f"B {B} cano {c} {tag}")
        print(f"\n[B {B} cano {c} {tag}] kernel vs float64: G {sp:.2e} of max|G| (bound {tol:.2e})")
        if not flow:
            assert losses[1] == 0.0 and losses[2] == losses[0]
        if i == c % len(kr.POST_VARIANTS):                      # the matched targets not asked for: everything else unchanged
            G0, m0, l0 = _kin_post(dev, case, flow, robust, want_matched=False)
            assert m0 is None and np.array_equal(G0, G) and np.array_equal(l0, losses)


def test_batched_blend_at_70_frames_equals_the_oracle(oracle, dev):
    """The mask and the blended flow reart_kin_post keeps in its workspace: reart_blend_anchor_motion_batch on the same ragged
    reference sets (3 ... 200 points) against oracle.blend_anchor_motion frame by frame."""
    from reart_amd import _lib

    case = kr.make_post_case(70, 1)
    B, N = case["B"], case["N"]
    assert case["margin"] >= kr.MASK_MARGIN and min(case["lens"]) == 3 and max(case["lens"]) == 200
    f, p = B // 2, 17                                           # the exact hit: the d < 1e-10 clamp
    assert (case["refs"][f] == case["comp"][f][p]).all(axis=1).any()
    rp, fp, ln, nr = _padded_refs(dev, case)
    q = t(case["comp"][:B], dev)
    flow = torch.full((B, N, 3), float("nan"), device=dev)
    mask = torch.full((B, N), 2, dtype=torch.uint8, device=dev)
    L = _lib.lib()
    ws = torch.empty((int(L.reart_blend_anchor_motion_batch_workspace_bytes(B, N, nr, 3)),), dtype=torch.uint8, device=dev)
    _lib.check(L.reart_blend_anchor_motion_batch(_lib.ptr(q), _lib.ptr(rp), _lib.ptr(fp), _lib.ptr(ln), B, N, nr, 3, 1, _lib.ptr(flow),
                                                 _lib.ptr(mask), _lib.ptr(ws), ws.numel(), _lib.stream()), "reart_blend_anchor_motion_batch")
    np.testing.assert_array_equal(mask.cpu().numpy(), case["mask"].astype(np.uint8))
    np.testing.assert_allclose(flow.cpu().numpy(), case["gt"], rtol=2e-6, atol=1e-9)


# -------------------------------------------------------------------------------------------------- c, d. the engine
def _model(dev, s, theta):
    from reart_amd.knn_cuda import KNN
    from reart_amd.networks.model import KinematicModel

    P = len(s["parent"])
    edge_index = {f"{c}_{int(s['parent'][c])}": int(s["edge_of"][c]) for c in range(P) if s["parent"][c] >= 0}
    return KinematicModel(pose_len=theta.shape[0], seg_part=t(s["seg"], dev), cano_pc=t(s["cano"], dev), knn=KNN(k=1, transpose_mode=True),
                          edge_index=edge_index, paths_to_base=None, reverse_topo=[int(v) for v in s["order"]],
                          axis_list=t(s["axis"], dev), moment_list=t(s["moment"], dev), theta_list=t(theta, dev)).to(dev)


def _sequence(dev, B, N, c, with_flow, seed):
    """A 6-part model on a random tree; frames = its forward at perturbed joint angles + N(0, 0.004) noise, the points of every
    frame permuted; flow references from the spliced sequence (before the permutation), ragged."""
    rng = np.random.default_rng(seed)
    P = 6
    parent, edge_of, order, _ = kr.random_tree(rng, P, "random")
    cano = rng.uniform(-0.3, 0.3, (N, 3)).astype(np.float32)
    seg = rng.integers(0, P, N)
    seg[:P] = np.arange(P)
    axis = rng.normal(size=(P - 1, 3))
    axis = (axis / np.linalg.norm(axis, axis=1, keepdims=True)).astype(np.float32)
    moment = rng.normal(0, 0.1, (P - 1, 3)).astype(np.float32)
    phase, turns = rng.uniform(0, 2 * np.pi, P - 1), rng.integers(1, 4, P - 1)
    theta = (0.6 + 0.35 * np.sin(2 * np.pi * turns[None] * np.arange(B)[:, None] / B + phase[None])).astype(np.float32)    # 0.25 ... 0.95
    s = dict(parent=parent, edge_of=edge_of, order=order, cano=cano, seg=seg.astype(np.int64), axis=axis, moment=moment, theta=theta)
    kr.assert_clear_of_thresholds(axis, theta)
    with torch.no_grad():
        moved = _model(dev, s, theta + rng.normal(0, 0.02, theta.shape).astype(np.float32))(t(cano, dev))[0].cpu().numpy()
    moved = (moved + rng.normal(0, 0.004, moved.shape)).astype(np.float32)
    s["pcs"] = np.stack([f[rng.permutation(N)] for f in moved])
    s["refs"] = s["flows"] = None
    if with_flow:
        comp = np.concatenate((moved[:c], cano[None], moved[c:]), axis=0)
        sel = [rng.permutation(N)[:N // 6 + (7 * f) % (N // 2)] for f in range(B)]
        s["refs"] = [comp[f][x] for f, x in enumerate(sel)]
        s["flows"] = [((comp[f + 1][x] - comp[f][x]) * 0.5).astype(np.float32) for f, x in enumerate(sel)]
    return s


def _engine(dev, s, c):
    from reart_amd.kinematic_engine import KinematicEngine

    model = _model(dev, s, s["theta"])
    refs = None if s["refs"] is None else [t(r, dev) for r in s["refs"]]
    flows = None if s["flows"] is None else [t(f, dev) for f in s["flows"]]
    return model, KinematicEngine(model, t(s["cano"], dev), t(s["pcs"], dev), c, refs, flows, assign_iter=0, assign_gap=1, downsample=2)


ENGINE_CASES = {          # B, N, cano_idx, flow: the re-solve's form at n = N / 2 and 256 // B
    "B130_n128_cano0_flow": (130, 256, 0, True),          # one-launch form, a single racer
    "B70_n512_canoB_flow": (70, 1024, 70, True),          # chain form, 256 // 70 = 3 racers, in-place re-solve
    "B300_n64_cano150": (300, 128, 150, False),           # 256 // B = 0
}


@pytest.mark.parametrize("name", list(ENGINE_CASES))
def test_engine_equals_the_oracle_loop(oracle, dev, name):
    """Two iterations; the assertions and bounds of test_config5_literal_against_the_oracle_loop."""
    from oracle.kinematic_step import KinematicOracle

    B, N, c, with_flow = ENGINE_CASES[name]
    s = _sequence(dev, B, N, c, with_flow, seed=B)
    orc = KinematicOracle(s["cano"], s["pcs"], s["seg"], s["parent"], s["edge_of"], s["order"], s["axis"], s["moment"], s["theta"], c,
                          s["refs"], s["flows"], downsample=2, assign_gap=1, nproc=1)
    model, eng = _engine(dev, s, c)
    assert eng.B == B and eng.src_idx.numel() == N // 2
    np.testing.assert_array_equal(eng.part.cpu().numpy(), s["seg"])
    np.testing.assert_array_equal(eng.src_idx.cpu().numpy().ravel(), orc.src_idx.numpy())
    order = eng.tgt_order.cpu().numpy()
    np.testing.assert_array_equal(np.sort(order, axis=1), np.tile(np.arange(order.shape[1]), (order.shape[0], 1)))
    np.testing.assert_array_equal(eng.tgt_pts.cpu().numpy(), np.take_along_axis(orc.tgt_pts.numpy(), order[..., None], axis=1))
    for i in range(2):
        lo, pc_o = orc.iteration(i)
        le = eng.iteration(i)
        np.testing.assert_allclose(eng.pc_trans.cpu().numpy(), pc_o, rtol=0, atol=2e-6, err_msg=f"iteration {i} forward")
        np.testing.assert_array_equal(eng.matched.cpu().numpy(), orc.matched.numpy(), err_msg=f"iteration {i} assignment")
        assert set(le) == set(lo)
        for key in lo:
            assert abs(float(le[key]) - lo[key]) <= 1e-4 * abs(lo[key]), (i, key, float(le[key]), lo[key])
        for j, pname in enumerate(("axis_list", "moment_list", "theta_list")):
            g_o = orc.grads[j]
            g_e = eng.grads[id(getattr(model, pname))].cpu().numpy()
            print(f"\n[{name} iteration {i}] d/d{pname}: {np.abs(g_e - g_o).max() / np.abs(g_o).max():.1e} of max|g|")
            np.testing.assert_allclose(g_e, g_o, rtol=0, atol=1e-4 * np.abs(g_o).max(), err_msg=f"iteration {i} d/d{pname}")
    assert eng.lap_solves == orc.lap_solves == 2
    assert eng.lap_fallbacks == 0


def test_graph_replays_equal_the_eager_iterations_at_70_frames(dev):
    """B = 70, n = 512, the canonical frame last, flow loss: six iterations with and without the captured graphs (from the third
    iteration on, with the in-place re-solve between them) end in the same parameters, losses and assignments, bit for bit."""
    B, N, c, _ = ENGINE_CASES["B70_n512_canoB_flow"]
    s = _sequence(dev, B, N, c, True, seed=B)
    outs = []
    for graphs in (True, False):
        model, eng = _engine(dev, s, c)
        eng.GRAPHS = graphs
        for i in range(6):
            losses = eng.iteration(i)
        assert eng.lap_solves == 6 and eng.lap_fallbacks == 0
        assert (eng._g_pre is not None and eng._g_post is not None) == graphs
        assert eng._inplace is not None
        outs.append([getattr(model, n_).detach().clone() for n_ in ("axis_list", "moment_list", "theta_list")]
                    + [eng.lap_state["cols"].clone(), eng.matched.clone()] + [losses[key].clone() for key in sorted(losses)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
