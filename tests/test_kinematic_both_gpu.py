"""KinematicEngine(recon_with_assign=True): the Chamfer loss in every iteration and the assignment loss on top of it from
assign_iter on (the objective of the reference's run_real.py:175-203 / run_sapien.py:174-203), without autograd.

 1. reart_kin_post_recon (csrc/kinpost.hip) against tensor expressions that round as it does, without any search.
 2. The engine's Chamfer term is ChamferLoss's: gradient and fixed-point bits equal, the loss to one ulp, the gradient inside the
    float64 bound of tests/test_chamfer_loss_gpu.py.
 3. Seeds never matter.
 4. / 5. Against OperatorLoop --recon_with_assign (autograd, ChamferDistance, torch.optim.Adam), also with root motion and mixed
    joint types.
 6. Graph replays equal the eager iterations.   7. warm_flow.   8. Routing, defaults and the refused shapes.

Every test that constructs the mode fails without it: the keyword and the C entry do not exist there."""
import numpy as np
import pytest
import torch

from tests import chamfer_loss_ref as cref
from tests import kinematic_both_ref as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
NAMES = ("axis_list", "moment_list", "theta_list")


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _call(dev, case, inv_x="case", entry="reart_kin_post_recon", **over):
    """One call on canary-framed outputs -> (rc, G, matched, losses, canaries untouched)."""
    from reart_amd import _lib

    L = _lib.lib()
    B, N, n, c = case["B"], case["N"], case["n"], case["c"]
    rp, fp, ln, nr = R.padded_refs(case, dev)
    ws = torch.empty((max(int(L.reart_kin_post_workspace_bytes(B, N, nr, 3)), 256),), dtype=torch.uint8, device=dev)
    Gb = torch.full((B + 2, N, 3), -77.0, dtype=torch.float32, device=dev)
    Mb = torch.full((B + 2, max(n, 1), 3), -77.0, dtype=torch.float32, device=dev)
    losses = torch.full((6,), -77.0, dtype=torch.float32, device=dev)
    inv = case["inv_x"] if isinstance(inv_x, str) else inv_x
    a = {"pc_trans": case["pc_trans"], "cano": case["cano"], "B": B, "N": N, "c": c, "pc_src": case["pc_src"], "tgt": case["tgt"],
         "cols": case["cols"], "slot": case["slot"], "n": n, "g_recon": case["g_recon"], "inv_x": inv, "loss_recon": case["loss_recon"],
         "G": Gb[1:B + 1], "matched": Mb[1:B + 1] if n else None, "losses": losses[1:5], "ws": ws, "ws_bytes": ws.numel()}
    a.update(over)
    p = _lib.ptr
    head = (p(a["pc_trans"]), p(a["cano"]), a["B"], a["N"], a["c"], p(a["pc_src"]), p(a["tgt"]), p(a["cols"]), p(a["slot"]), a["n"], R.LAM_A,
            p(rp), p(fp), p(ln), nr, 3, 1, R.LAM_F, 0, R.SMOOTH)
    tail = (p(a["G"]), p(a["matched"]), p(a["losses"]), p(a["ws"]), a["ws_bytes"], _lib.stream())
    if entry == "reart_kin_post":
        rc = L.reart_kin_post(*head, *tail)
    else:
        rc = L.reart_kin_post_recon(*head, p(a["g_recon"]), p(a["inv_x"]), p(a["loss_recon"]), *tail)
    torch.cuda.synchronize()
    clean = bool((Gb[0] == -77.0).all() and (Gb[B + 1] == -77.0).all() and (Mb[0] == -77.0).all() and (Mb[B + 1] == -77.0).all()
                 and losses[0] == -77.0 and losses[5] == -77.0)
    return rc, Gb[1:B + 1].clone(), (Mb[1:B + 1].clone() if n else None), losses[1:5].clone(), clean


@pytest.mark.parametrize("B,N,n", [(1, 1, 1), (3, 300, 75), (4, 257, 64), (2, 513, 0)])
@pytest.mark.parametrize("flow", [False, True])
@pytest.mark.parametrize("perm", [False, True])
def test_kernel_equals_the_tensor_expressions(dev, B, N, n, flow, perm):
    """G and the matched targets bit for bit, the four losses to 1e-6 relative + 1e-9 (the tolerance of
    test_fused_post_equals_the_tensor_expressions: a double sum here, torch's fp32 tree sum there); canary rows around the
    outputs untouched; two runs equal; losses[2] is the input, losses[3] = fl(fl(l0 + l2) + l1) of the call's own terms."""
    for c in sorted({0, B // 2, B}):
        case = R.kernel_case(dev, B, N, n, c, flow, perm)
        if n and N > 1:
            assert int((case["slot"] < 0).sum()) == N - n > 0
        Gx, Mx, lx = R.expressions(case)
        rc, G, M, l, clean = _call(dev, case)
        assert rc == 0 and clean, (c, rc, clean)
        assert torch.equal(G, Gx), f"cano_idx {c}: G differs at {int((G != Gx).sum())} entries"
        if n:
            assert torch.equal(M, Mx), f"cano_idx {c}: matched"
        got = [float(v) for v in l]
        print(f"[B {B} N {N} n {n} c {c} flow {flow} perm {perm}] losses {got} expressions {lx}")
        for a_, b_ in zip(got, lx):
            assert abs(a_ - b_) <= 1e-6 * abs(b_) + 1e-9, (c, got, lx)
        assert got[2] == float(case["loss_recon"])
        assert np.float32(got[3]) == np.float32(np.float32(np.float32(got[0]) + np.float32(got[2])) + np.float32(got[1]))
        if n == 0:
            assert got[0] == 0.0
        if not flow:
            assert got[1] == 0.0
        rc2, G2, M2, l2, _ = _call(dev, case)
        assert rc2 == 0 and torch.equal(G2, G) and torch.equal(l2, l) and (M is None or torch.equal(M2, M))


@pytest.mark.parametrize("flow", [False, True])
def test_kernel_range_checks_the_stored_rows(dev, flow):
    """One inv_x entry = N and one = -1: those two points take no Chamfer gradient, nothing else changes."""
    B, N, n = 3, 300, 75
    case = R.kernel_case(dev, B, N, n, 1, flow, True)
    _, G0, M0, l0, _ = _call(dev, case)
    bad = case["inv_x"].clone()
    p_hi, p_lo = int(case["src"][3]), int((case["slot"] < 0).nonzero()[5])        # a sampled point and one outside the sample
    bad[p_hi], bad[p_lo] = N, -1
    rc, G, M, l, clean = _call(dev, case, inv_x=bad)
    assert rc == 0 and clean
    Gx, _, _ = R.expressions(case, inv_x=bad)
    assert torch.equal(G, Gx)
    rest = torch.ones(N, dtype=torch.bool, device=dev)
    rest[[p_hi, p_lo]] = False
    assert torch.equal(G[:, rest], G0[:, rest]) and torch.equal(M, M0) and torch.equal(l, l0)
    assert not torch.equal(G[:, p_hi], G0[:, p_hi]) and not torch.equal(G[:, p_lo], G0[:, p_lo])
    if not flow:
        assert (G[:, p_lo] == 0).all()


def test_kernel_refusals(dev):
    """NULL g_recon / loss_recon: REART_ERR_INVALID_ARG (the code reart_kin_post returns for its own refusals, which are kept)."""
    case = R.kernel_case(dev, 3, 300, 75, 1, True, True)
    invalid = _call(dev, case, entry="reart_kin_post", B=0)[0]
    assert invalid != 0
    assert _call(dev, case)[0] == 0
    for over in ({"g_recon": None}, {"loss_recon": None}, {"B": 0}, {"N": 0}, {"n": -1}, {"c": -1}, {"c": 4}, {"pc_trans": None},
                 {"cano": None}, {"G": None}, {"losses": None}, {"ws": None}, {"ws_bytes": 16}, {"cols": None}, {"slot": None},
                 {"pc_src": None}, {"tgt": None}):
        rc, G, _, l, clean = _call(dev, case, **over)
        assert rc == invalid and clean, over
        if "G" not in over:
            assert (G == -77.0).all() and (l == -77.0).all(), over       # a refused call writes nothing
    assert _call(dev, case, inv_x=None)[0] == 0 and _call(dev, case, matched=None)[0] == 0


def test_the_existing_entry_is_unchanged_by_its_sibling(dev):
    """reart_kin_post on the same inputs: its G is the expressions' without the Chamfer input, its three losses as before."""
    case = R.kernel_case(dev, 4, 257, 64, 2, True, False)
    zero = dict(case, g_recon=torch.zeros_like(case["g_recon"]), loss_recon=torch.zeros_like(case["loss_recon"]))
    Gx, Mx, lx = R.expressions(zero)
    rc, G, M, l, clean = _call(dev, case, entry="reart_kin_post")
    assert rc == 0 and clean and torch.equal(M, Mx)
    assert torch.equal(G, Gx)
    assert float(l[3]) == -77.0 and float(l[2]) == float(np.float32(float(l[0])) + np.float32(float(l[1])))


# ------------------------------------------------------------------------------------------------ the engine
def _engine(dev, pb, gap=1, wd=0.0, assign_iter=0, downsample=4, **kw):
    from reart_amd.kinematic_engine import KinematicEngine

    k, cano, seg, pcs, refs, flows, make = pb
    m = make()
    return m, KinematicEngine(m, cano, pcs, 2, refs, flows, weight_decay=wd, assign_iter=assign_iter, assign_gap=gap,
                              downsample=downsample, recon_with_assign=True, **kw)


def test_the_chamfer_term_is_chamfer_loss(dev):
    """After forward() and the term, on the engine's own pc_trans: recon_grad() and last_fx_bits equal those of
    ChamferLoss(spatial_sort=False) in every bit (the scatter sums are integer sums: the storage order cannot change them), the
    loss to one float32 ulp (the double sum runs in another order), the gradient inside the per-component float64 bound of
    tests/test_chamfer_loss_gpu.py.  Precondition, asserted: no query of either direction has two equidistant nearest targets."""
    from reart_amd.utils.chamfer import ChamferLoss, knn_points

    pb = R.golden_problem(dev, 3, False, N=4096)
    pcs = pb[3]
    m, eng = _engine(dev, pb)
    assert eng.last_fx_bits is not None and eng._cham_calls == 0
    for call in range(2):                       # cold (y_unchanged = 0) and warm
        x = eng.forward().clone()
        eng._recon_term()
        for a_, b_ in ((x, pcs), (pcs, x)):
            d = knn_points(a_, b_, K=2).dists
            assert bool((d[..., 0] != d[..., 1]).all()), "a tie between two nearest targets: the clouds do not serve this test"
        mod = ChamferLoss(spatial_sort=False)
        xr = x.clone().requires_grad_(True)
        want = mod(xr, pcs)
        want.backward()
        got_g = eng.recon_grad()
        assert torch.equal(got_g, xr.grad), f"call {call}: {int((got_g != xr.grad).sum())} entries differ"
        assert torch.equal(eng.last_fx_bits, mod.fx_bits)
        got, want = np.float32(float(eng._loss_recon)), np.float32(float(want.detach()))
        print(f"call {call}: loss {got!r} ChamferLoss {want!r} ulp {np.spacing(want)!r} bits {eng.last_fx_bits.tolist()}")
        assert abs(np.float64(got) - np.float64(want)) <= np.float64(np.spacing(want))
        _, i_xy, _, i_yx = (v.cpu().numpy() for v in mod.last)
        r = cref.gradients(x.cpu().numpy(), pcs.cpu().numpy(), i_xy, i_yx)["x"]
        quantum = np.exp2(-eng.last_fx_bits.cpu().numpy().astype(np.float64))[:, None, None]
        bound = (U * (np.abs(r["own"]) + r["mag"] + np.abs(r["scat"]) + np.abs(r["grad"])) + 2.0 * r["cnt"][..., None] * quantum) * (1.0 + 2.0 ** -20)
        err = np.abs(got_g.cpu().numpy().astype(np.float64) - r["grad"])
        print(f"call {call}: gradient max err {err.max():.3e}, err/bound max {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert (err <= bound).all()


def _params(m, names=NAMES):
    return [getattr(m, n_).detach().clone() for n_ in names]


def test_seeds_never_matter(dev):
    """Both seed arrays overwritten with garbage (out of range, repeats, -1) between iterations: three iterations equal three of
    an undisturbed engine in every parameter bit."""
    pb = R.golden_problem(dev, 4, True)
    outs = []
    for disturb in (False, True):
        m, eng = _engine(dev, pb, assign_iter=1)
        rng = np.random.default_rng(9)
        for i in range(3):
            if disturb:
                junk = rng.integers(-5, eng.N + 50, (2, eng.B, eng.N)).astype(np.int32)
                junk[0, :, ::3], junk[1, :, ::2] = -1, 7
                junk[0, 0], junk[1, -1] = 2 ** 31 - 1, -2 ** 31
                eng._seed_xy.copy_(R.t(junk[0], dev))
                eng._seed_yx.copy_(R.t(junk[1], dev))
            losses = eng.iteration(i)
        outs.append(_params(m) + [eng.G.clone(), eng.recon_grad()] + [losses[key].clone() for key in losses])
    for a_, b_ in zip(*outs):
        assert torch.equal(a_, b_)


def test_the_recon_loss_is_current_in_every_iteration(dev):
    """Eight iterations beside an OperatorLoop in the same process, every loss read in every iteration, graphs on: the engine's
    recon Loss is ChamferLoss's on the engine's own pc_trans to one ulp, and its Chamfer gradient equal in every bit, every time.
    (With the Chamfer call captured in the first graph this scenario returned the loss of iteration 4 from iteration 5 on.)"""
    from reart_amd import run_robot as rr
    from reart_amd.utils.chamfer import ChamferLoss

    k, cano, seg, pcs, refs, flows, make = R.golden_problem(dev, 3, True, N=4096)
    argv = ["--model", "kinematic", "--use_assign_loss", "--recon_with_assign", "--assign_iter", "0", "--downsample", "4", "--assign_gap", "1",
            "--cano_idx", "2", "--use_flow_loss"]
    loop = rr.make_projection_loop(rr.build_parser().parse_args(argv), make(), cano, pcs, refs, flows)
    eng = rr.make_projection_loop(rr.build_parser().parse_args(argv + ["--fused_recon"]), make(), cano, pcs, refs, flows)
    for i in range(8):
        l_ref = {key: float(v.detach()) for key, v in loop.iteration(i).items()}
        l_eng = {key: float(v) for key, v in eng.iteration(i).items()}
        x = eng.pc_trans.clone().requires_grad_(True)
        want = ChamferLoss(spatial_sort=False)(x, pcs)
        want.backward()
        want = np.float32(float(want.detach()))
        print(f"iteration {i}: engine {l_eng['recon Loss']!r} ChamferLoss {want!r} loop {l_ref['recon Loss']!r}")
        assert abs(np.float64(np.float32(l_eng["recon Loss"])) - np.float64(want)) <= np.float64(np.spacing(want)), i
        assert torch.equal(eng.recon_grad(), x.grad), i
        assert np.float32(l_eng["total Loss"]) == np.float32(np.float32(np.float32(l_eng["opt assignment loss"]) + np.float32(l_eng["recon Loss"]))
                                                             + np.float32(l_eng["flow Loss"])), i
    assert eng._g_pre is not None and eng._g_post is not None


def _against_the_loop(dev, loop, eng, m_ref, m_eng, names, keys_of):
    """Six iterations side by side at the tolerances tests/test_kinematic_engine_gpu.py uses for its Chamfer-branch rows (the
    Chamfer term is in every iteration here): losses 2e-5 relative + 1e-7, gradients 1e-4 of their largest entry over the first
    three iterations, parameters atol 1e-4."""
    for i in range(6):
        l_ref, l_eng = loop.iteration(i), eng.iteration(i)
        assert list(l_ref) == list(l_eng) == keys_of(i), (i, list(l_ref), list(l_eng))
        for key in l_ref:
            a_, b_ = float(l_ref[key].detach()), float(l_eng[key].detach())
            print(f"iteration {i} {key}: loop {a_!r} engine {b_!r}")
            assert abs(a_ - b_) <= 2e-5 * abs(a_) + 1e-7, (i, key, a_, b_)
        for name in names:
            if i < 3:
                g_ref = getattr(m_ref, name).grad.detach().cpu().numpy()
                g_eng = eng.grads[id(getattr(m_eng, name))].cpu().numpy()
                np.testing.assert_allclose(g_eng, g_ref, rtol=0, atol=1e-4 * np.abs(g_ref).max(), err_msg=f"iteration {i} d/d{name}")
            np.testing.assert_allclose(getattr(m_eng, name).detach().cpu().numpy(), getattr(m_ref, name).detach().cpu().numpy(),
                                       rtol=0, atol=1e-4, err_msg=f"iteration {i} {name}")
    assert eng.lap_solves == loop.lap_solves
    assert eng.lap_fallbacks == 0 and loop.lap_fallbacks == 0


def _keys(with_flow, assign_iter):
    return lambda i: ((["opt assignment loss"] if i >= assign_iter else []) + ["recon Loss"] + (["flow Loss"] if with_flow else [])
                      + ["total Loss"])


@pytest.mark.parametrize("with_flow,gap,wd,assign_iter", [(True, 1, 0.0, 0), (False, 2, 0.0, 0), (True, 2, 0.01, 0), (True, 1, 0.0, 3)])
def test_engine_equals_the_autograd_loop(dev, with_flow, gap, wd, assign_iter):
    """The set-up of tests/test_kinematic_engine_gpu.py::test_engine_equals_the_autograd_loop (golden kinematic.npz, cloud and
    labels at their full 4096 points) under --recon_with_assign: OperatorLoop with ChamferDistance and torch.optim.Adam against
    make_projection_loop's engine under --fused_recon.

    The Chamfer gradient is discontinuous where a point has two nearest neighbours: the engine stays inside these bounds because
    in this mode it computes the cloud and the Adam step in the bits of the loop's (the model's own root-motion expression,
    reart_amd.optim.Adam).  Measured on the MI355X: gradients <= 1.1e-5 of their largest entry, parameters <= 2.2e-7, losses
    <= 2.4e-7 relative in all four rows (with reart_adam_step_multi's last-bit-different step the row (False, 2, 0, 0) left the
    loop's trajectory in iteration 4, when ONE point took another nearest neighbour on the two sides: losses 2.24e-5)."""
    from reart_amd import run_robot as rr
    from reart_amd.kinematic_engine import KinematicEngine

    k, cano, seg, pcs, refs, flows, make = R.golden_problem(dev, 3, with_flow, N=4096)
    argv = ["--model", "kinematic", "--use_assign_loss", "--recon_with_assign", "--assign_iter", str(assign_iter), "--downsample", "4",
            "--assign_gap", str(gap), "--cano_idx", "2", "--weight_decay", str(wd)] + (["--use_flow_loss"] if with_flow else [])
    m_ref, m_eng = make(), make()
    loop = rr.make_projection_loop(rr.build_parser().parse_args(argv), m_ref, cano, pcs, refs, flows)
    eng = rr.make_projection_loop(rr.build_parser().parse_args(argv + ["--fused_recon"]), m_eng, cano, pcs, refs, flows)
    assert isinstance(loop, rr.OperatorLoop) and isinstance(eng, KinematicEngine) and eng.recon_with_assign
    _against_the_loop(dev, loop, eng, m_ref, m_eng, NAMES, _keys(with_flow, assign_iter))


@pytest.mark.parametrize("with_flow", [True, False])
def test_real_scan_model_equals_the_autograd_loop(dev, with_flow):
    """Root motion and mixed joint types (tests/golden/kinematic_root.npz, the set-up of
    test_engine_with_root_motion_equals_the_autograd_loop) with the flag.

    The engine applies the root motion with the model's own expression (a matrix product, then an addition) in this mode: as
    one baddbmm two thirds of the points differed from the loop's in their last bit after the first step, and in iteration 1 ONE
    point took another nearest neighbour on the two sides (d/d theta_list 6.7e-4 against the bound 3.1e-4, measured)."""
    from reart_amd import run_robot as rr
    from reart_amd.kinematic_engine import KinematicEngine
    from tests.test_kinematic_engine_gpu import _root_model

    g, m_eng = _root_model(dev)
    _, m_ref = _root_model(dev)
    cano = R.t(g["cano_pc"], dev)
    rng = np.random.default_rng(5)
    B, N = 9, cano.shape[0]
    with torch.no_grad():
        pcs = m_ref(cano)[0]
    pcs = (pcs + R.t(rng.normal(0, 0.004, (B, N, 3)).astype(np.float32), dev)).contiguous()
    pcs = torch.stack([p[torch.from_numpy(rng.permutation(N)).to(dev)] for p in pcs])
    refs = flows = None
    if with_flow:
        comp = torch.cat((pcs[:2], cano[None], pcs[2:]), dim=0)
        sel = [torch.from_numpy(rng.permutation(N)[:300 + 7 * f]).to(dev) for f in range(B)]
        refs = [comp[f][s] for f, s in enumerate(sel)]
        flows = [(comp[f + 1][s] - comp[f][s]) * 0.5 for f, s in enumerate(sel)]
    argv = ["--model", "kinematic", "--use_assign_loss", "--recon_with_assign", "--assign_iter", "0", "--downsample", "4", "--assign_gap", "1",
            "--cano_idx", "2"] + (["--use_flow_loss"] if with_flow else [])
    loop = rr.make_projection_loop(rr.build_parser().parse_args(argv), m_ref, cano, pcs, refs, flows)
    eng = rr.make_projection_loop(rr.build_parser().parse_args(argv + ["--fused_recon"]), m_eng, cano, pcs, refs, flows)
    assert isinstance(loop, rr.OperatorLoop) and isinstance(eng, KinematicEngine) and eng.root and eng._pris is not None
    _against_the_loop(dev, loop, eng, m_ref, m_eng, NAMES + ("distance_list", "root_6d", "root_t"), _keys(with_flow, 0))


def test_graph_replays_equal_the_eager_iterations(dev):
    """Ten iterations (downsample 2, assign_gap 1, flow loss) with and without the two captured graphs (the Chamfer term is queued
    eagerly between them), one cold re-solve in between (it resets the post graph, which is then captured again): the same
    parameters, losses, assignments and Chamfer gradient, bit for bit."""
    pb = R.golden_problem(dev, 5, True)
    outs = []
    for graphs in (True, False):
        m, eng = _engine(dev, pb, downsample=2)
        eng.GRAPHS = graphs
        for i in range(10):
            if i == 5:
                assert (eng._g_post is not None) == graphs
                eng.lap_state.clear()               # the next solve is a cold one
            losses = eng.iteration(i)
        assert eng.lap_solves == 10 and eng.lap_fallbacks == 0
        assert (eng._g_pre is not None and eng._g_post is not None) == graphs
        outs.append(_params(m) + [eng.lap_state["cols"].clone(), eng.matched.clone(), eng.G.clone(), eng.recon_grad(), eng.last_fx_bits.clone()]
                    + [losses[key].clone() for key in losses])
    for a_, b_ in zip(*outs):
        assert torch.equal(a_, b_)


def test_fused_post_equals_the_expression_fallback(dev):
    """FUSED_POST off (_post_expressions in the new mode) against reart_kin_post_recon inside the engine, before and after
    assign_iter: G, matched targets and parameters bit for bit, losses to 1e-6."""
    pb = R.golden_problem(dev, 11, True)
    out = {}
    for fused in (True, False):
        m, eng = _engine(dev, pb, assign_iter=2)
        eng.FUSED_POST, eng.GRAPHS = fused, False
        rec = []
        for i in range(5):
            losses = eng.iteration(i)
            rec.append((eng.G.clone(), None if i < 2 else eng.matched.clone(), {key: float(v) for key, v in losses.items()}))
        out[fused] = (rec, torch.cat([p.reshape(-1) for p in _params(m)]))
    for i, ((g1, m1, l1), (g0, m0, l0)) in enumerate(zip(out[True][0], out[False][0])):
        assert torch.equal(g1, g0), f"iteration {i}: dL/d pc_trans"
        assert m1 is None and m0 is None or torch.equal(m1, m0)
        assert list(l1) == list(l0)
        for key in l1:
            assert abs(l1[key] - l0[key]) <= 1e-6 * abs(l0[key]) + 1e-9, (i, key, l1[key], l0[key])
    assert torch.equal(out[True][1], out[False][1])


def test_warm_flow_in_the_new_mode(dev):
    """warm_flow on and off (tests/test_flow_term_gpu.py::test_kinematic_engine_with_warm_flow's tolerances): the same
    parameters, assignments and gradient bit for bit, assignment and Chamfer loss equal, flow and total loss to one ulp."""
    pb = R.golden_problem(dev, 5, True)
    outs = []
    for warm in (True, False):
        m, eng = _engine(dev, pb, downsample=2, warm_flow=warm)
        assert (eng._flow_term is not None) == warm
        rows = []
        for i in range(6):
            losses = eng.iteration(i)
            rows.append({key: float(v) for key, v in losses.items()})
        assert eng._g_post is not None and eng.lap_fallbacks == 0
        outs.append((_params(m) + [eng.lap_state["cols"].clone(), eng.matched.clone(), eng.G.clone()], rows))
    for a_, b_ in zip(outs[0][0], outs[1][0]):
        assert torch.equal(a_, b_)
    for i, (on, off) in enumerate(zip(outs[0][1], outs[1][1])):
        print(f"iteration {i}: warm {on} | plain {off}")
        assert list(on) == list(off) == ["opt assignment loss", "recon Loss", "flow Loss", "total Loss"]
        assert on["opt assignment loss"] == off["opt assignment loss"] and on["recon Loss"] == off["recon Loss"]
        for key in ("flow Loss", "total Loss"):
            assert abs(on[key] - off[key]) <= float(np.spacing(np.float32(off[key]))), (i, key, on, off)


# ------------------------------------------------------------------------------------------------ 8. routing and defaults
def test_routing_and_defaults(dev):
    from reart_amd import run_robot as rr
    from reart_amd.kinematic_engine import KinematicEngine

    k, cano, seg, pcs, refs, flows, make = R.golden_problem(dev, 2, False, N=256, B=3)
    base = ["--model", "kinematic", "--use_assign_loss", "--assign_iter", "0", "--cano_idx", "2"]
    parse = lambda extra: rr.build_parser().parse_args(base + extra)
    plain = rr.make_projection_loop(parse([]), make(), cano, pcs)
    assert isinstance(plain, KinematicEngine) and plain.recon_with_assign is False
    for name in ("_order_x", "_inv_x", "_ys", "_seed_xy", "_seed_yx", "_fx_bits", "_cham_ws", "_xs", "_g_recon", "_loss_recon", "_loss4",
                 "last_fx_bits"):
        assert getattr(plain, name) is None, name
    assert isinstance(rr.make_projection_loop(parse(["--recon_with_assign"]), make(), cano, pcs), rr.OperatorLoop)
    eng = rr.make_projection_loop(parse(["--recon_with_assign", "--fused_recon"]), make(), cano, pcs)
    assert isinstance(eng, KinematicEngine) and eng.recon_with_assign
    assert eng._seed_xy.shape == eng._seed_yx.shape == (3, 256) and bool((eng._seed_xy == -1).all()) and eng._fx_bits.shape == (3,)
    assert torch.equal(eng._order_x.long()[eng._inv_x.long()], torch.arange(256, device=dev))
    with pytest.raises(ValueError, match="fused_recon"):
        rr.make_projection_loop(parse(["--fused_recon"]), make(), cano, pcs)


@pytest.mark.parametrize("B,N", [(65536, 16), (1024, 1 << 20)])
def test_constructor_refuses_what_the_warm_call_does_not_take(dev, B, N):
    """More than 65535 frames, frames x (points + 512) >= 2^30: NotImplementedError before anything is launched or allocated per
    frame (the frames here are one expanded row, the model is None: any step past the check would fail otherwise)."""
    from reart_amd.kinematic_engine import KinematicEngine

    cano = torch.zeros((N, 3), dtype=torch.float32, device=dev)
    with pytest.raises(NotImplementedError, match="reart_chamfer_loss"):
        KinematicEngine(None, cano, cano[None].expand(B, N, 3), 0, recon_with_assign=True)
