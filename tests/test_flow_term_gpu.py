"""FlowTerm / reart_flow_term against the composition it replaces on the same device: blend_anchor_motion_batch + flow_loss +
autograd through ``cat`` and the subtraction (itself held to the reference by tests/golden/flow.npz).  Neighbours, distances,
blended flow, mask and gradient are compared bit for bit; the loss with float32(sum of the float64 per-point terms), one ulp."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#         B, N, reference lengths, clustered
SHAPES = [(1, 1, (3,), False), (2, 15, (3, 17), False), (3, 100, (3, 17, 130), False), (2, 513, (40, 600), False),
          (3, 700, (257, 1000, 64), True), (2, 1500, (1000, 1500), False)]
IDS = ["1x1", "2x15", "3x100", "2x513", "3x700c", "2x1500"]


@functools.lru_cache(maxsize=None)
def _inputs(B, N, lens, clustered, seed=0):
    """complete frames [B+1,N,3], reference sets and flows: queries are reference points plus N(0, 0.01); every tenth is
    shifted by +1 in x (masked out: the flows have size 0.02); every tenth reference carries a flow of size 3 (Huber's linear
    branch); every 16th query sits exactly on a reference point (the 1e-10 clamp)."""
    rng = np.random.default_rng(100 + seed)
    refs, flows, frames = [], [], []
    for n in lens:
        if clustered:
            centres = rng.uniform(-0.3, 0.3, (4, 3))
            r = centres[rng.integers(0, 4, n)] + rng.normal(0, 0.02, (n, 3))
        else:
            r = rng.uniform(-0.3, 0.3, (n, 3))
        d = rng.normal(size=(n, 3))
        fl = 0.02 * d / np.linalg.norm(d, axis=1, keepdims=True)
        fl[5::10] *= 150.0
        r = r.astype(np.float32)
        q = r[rng.integers(0, n, N)].astype(np.float64) + rng.normal(0, 0.01, (N, 3))
        q[3::10, 0] += 1.0
        q = q.astype(np.float32)
        q[::16] = r[rng.integers(0, n, q[::16].shape[0])]
        refs.append(r); flows.append(fl.astype(np.float32)); frames.append(q)
    frames.append((frames[-1] + rng.normal(0, 0.01, (N, 3))).astype(np.float32))
    return np.stack(frames), refs, flows


def _split(complete, c, dev):
    pc = np.concatenate((complete[:c], complete[c + 1:]), axis=0)
    return torch.from_numpy(pc).to(dev), torch.from_numpy(np.ascontiguousarray(complete[c])).to(dev)


def _t(arrs, dev):
    return [torch.from_numpy(a).to(dev) for a in arrs]


def _yardstick(pc, cano, refs, flows, c, squared, robust, weight=1.0):
    """The parent's composition: (outputs dict, float32(sum of the float64 per-point terms))."""
    from reart_amd.knn_cuda import KNN
    from reart_amd.networks.loss import flow_loss
    from reart_amd.utils.flow_utils import blend_anchor_motion_batch, pad_reference_sets

    knn = KNN(k=3, transpose_mode=True, squared=squared)
    x = pc.clone().requires_grad_(True)
    with torch.no_grad():
        comp = torch.cat((x[:c], cano[None], x[c:]), dim=0)
        gt, mask = blend_anchor_motion_batch(comp[:-1], *pad_reference_sets(refs, flows), knn, return_mask=True)
        di = [knn(r[None], q[None]) for q, r in zip(comp[:-1], refs)]
        dists, idx = torch.stack([d[0][0] for d in di]), torch.stack([d[1][0] for d in di])
    comp = torch.cat((x[:c], cano[None], x[c:]), dim=0)
    pred = comp[1:] - comp[:-1]
    loss = weight * flow_loss(gt, pred, flow_mask_list=mask, robust=robust)
    (G,) = torch.autograd.grad(loss, x)
    with torch.no_grad():       # the per-point terms with flow_loss_kernel's float32 expressions, added in double
        p, d = pred.detach(), pred.detach() - gt
        if robust:
            e = torch.where(d.abs() <= 1.0, 0.5 * d * d, d.abs() - 0.5)
        else:
            e = d * d
        f = (e[..., 0] + e[..., 1]) + e[..., 2]
        sm = ((p * p)[..., 0] + (p * p)[..., 1]) + (p * p)[..., 2]
        terms = torch.where(mask, f, 1e-2 * sm)
        total = np.float32(terms.double().sum().item())
    return dict(gt=gt, mask=mask, dists=dists, idx=idx, G=G, loss=loss.detach()), total


def _run(mod, pc, cano, upstream=None):
    x = pc.clone().requires_grad_(True)
    loss = mod(x, cano)
    (G,) = torch.autograd.grad(loss if upstream is None else loss * upstream, x)
    gt, mask, dists, idx = mod.last
    return dict(gt=gt, mask=mask, dists=dists, idx=idx, G=G, loss=loss.detach())


def _same(got, want, keys=("idx", "dists", "gt", "mask", "G"), what=""):
    for k in keys:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (what, k, (got[k] != want[k]).sum().item())


def _loss_ok(got, total, weight=1.0, what=""):
    want = np.float32(weight) * total
    ulp = float(np.spacing(np.abs(want)))
    print(f"{what}: loss {float(got['loss'])!r}, float32(double sum) {float(want)!r}, diff/ulp {abs(float(got['loss']) - float(want)) / ulp:.2f}")
    assert abs(float(got["loss"]) - float(want)) <= ulp, what


def _garbage(mod, N, cano, lens, rng):
    """Seeds from -5 to nr + 5 with repeats, written where the native call reads them."""
    st = mod._get_state(N, cano)
    g = np.stack([rng.integers(-5, n + 6, (N, 3)) for n in lens])
    g[:, ::3, 1] = g[:, ::3, 0]
    st["seed"].copy_(torch.from_numpy(g.astype(np.int32)))


@pytest.mark.parametrize("spatial_sort", [False, True])
@pytest.mark.parametrize("B,N,lens,clustered", SHAPES, ids=IDS)
def test_exact_for_any_seed(dev, B, N, lens, clustered, spatial_sort):
    """Every cano_idx in {0, middle, B}, euclidean and squared distances, plain and robust loss; cold seeds, random valid seeds
    and garbage seeds.  Upstream 1, then 0.37 on the warm module."""
    from reart_amd.utils.flow_utils import FlowTerm

    complete, refs, flows = _inputs(B, N, lens, clustered)
    refs, flows = _t(refs, dev), _t(flows, dev)
    rng = np.random.default_rng(5)
    frac = []
    for c in sorted({0, B // 2, B}):
        pc, cano = _split(complete, c, dev)
        for squared in (False, True):
            for robust in (False, True):
                what = f"c={c} squared={squared} robust={robust}"
                want, total = _yardstick(pc, cano, refs, flows, c, squared, robust)
                frac.append(want["mask"].float().mean().item())
                mod = FlowTerm(refs, flows, c, robust=robust, knn_squared=squared, spatial_sort=spatial_sort)
                got = _run(mod, pc, cano)                                    # cold
                _same(got, want, what=what + " cold")
                _loss_ok(got, total, what=what + " cold")
                valid = torch.from_numpy(np.stack([rng.integers(0, n, (N, 3)) for n in lens])).to(dev)
                mod.seed(cano, valid)
                got = _run(mod, pc, cano)
                _same(got, want, what=what + " random seeds")
                _loss_ok(got, total, what=what + " random seeds")
                _garbage(mod, N, cano, lens, rng)
                got = _run(mod, pc, cano)
                _same(got, want, what=what + " garbage seeds")
                _loss_ok(got, total, what=what + " garbage seeds")
                up = _run(mod, pc, cano, upstream=0.37)                      # warm, upstream scalar
                assert torch.equal(up["G"], got["G"] * 0.37), what
    print("masked in:", [round(f, 3) for f in frac])
    if N >= 15:     # (a single point cannot be on both sides)
        assert all(0.05 <= f <= 0.95 for f in frac), frac


def test_weight_scales_the_gradient_and_the_loss(dev):
    from reart_amd.utils.flow_utils import FlowTerm

    B, N, lens, clustered = SHAPES[2]
    complete, refs, flows = _inputs(B, N, lens, clustered)
    refs, flows = _t(refs, dev), _t(flows, dev)
    pc, cano = _split(complete, 1, dev)
    for robust in (False, True):
        want, total = _yardstick(pc, cano, refs, flows, 1, False, robust, weight=0.3)
        got = _run(FlowTerm(refs, flows, 1, weight=0.3, robust=robust), pc, cano)
        _same(got, want, what=f"weight robust={robust}")
        _loss_ok(got, total, weight=0.3, what=f"weight robust={robust}")


def test_ties_go_to_the_lowest_index(dev):
    """Every reference point stored three times: the three neighbours are the three copies of the nearest point in index order,
    whatever the seeds name."""
    from reart_amd.utils.flow_utils import FlowTerm

    B, N, lens, clustered = SHAPES[3]
    complete, refs, flows = _inputs(B, N, lens, clustered)
    refs3, flows3 = _t([np.tile(r, (3, 1)) for r in refs], dev), _t([np.tile(f, (3, 1)) for f in flows], dev)
    pc, cano = _split(complete, 1, dev)
    want, total = _yardstick(pc, cano, refs3, flows3, 1, False, False)
    n = torch.tensor(lens, device=dev)[:, None]
    assert (want["idx"][..., 0] < n).all() and torch.equal(want["idx"][..., 1], want["idx"][..., 0] + n)
    assert torch.equal(want["idx"][..., 2], want["idx"][..., 0] + 2 * n)
    mod = FlowTerm(refs3, flows3, 1, spatial_sort=False)
    _same(_run(mod, pc, cano), want, what="cold")
    later = want["idx"][..., :1] + 2 * n[..., None]
    for seeds in (later.expand(-1, -1, 3), torch.cat((later, later - n[..., None], later), dim=2), want["idx"].flip(2)):
        mod.seed(cano, seeds.contiguous())
        _same(_run(mod, pc, cano), want, what="seeded with later copies")


def test_warm_state_never_changes_a_result(dev):
    """Queries moving by 1e-3, 1e-1 and a jump: every call of the warm module equals a fresh module's; so does the call after
    reset(), and a module on other reference sets owes nothing to the first."""
    from reart_amd.utils.flow_utils import FlowTerm

    B, N, lens, clustered = SHAPES[4]
    complete, refs, flows = _inputs(B, N, lens, clustered)
    refs, flows = _t(refs, dev), _t(flows, dev)
    rng = np.random.default_rng(8)
    moves = [complete, complete + rng.normal(0, 1e-3, complete.shape).astype(np.float32),
             complete + rng.normal(0, 1e-1, complete.shape).astype(np.float32), complete[:, rng.permutation(N)] + np.float32(0.2)]
    for spatial_sort in (False, True):
        warm = FlowTerm(refs, flows, 1, robust=True, spatial_sort=spatial_sort)
        for k, m in enumerate(moves):
            pc, cano = _split(np.ascontiguousarray(m.astype(np.float32)), 1, dev)
            got = _run(warm, pc, cano)
            fresh = _run(FlowTerm(refs, flows, 1, robust=True, spatial_sort=spatial_sort), pc, cano)
            _same(got, fresh, keys=("idx", "dists", "gt", "mask", "G", "loss"), what=f"move {k}")
        warm.reset()
        assert warm.last is None
        _same(_run(warm, pc, cano), fresh, keys=("idx", "dists", "gt", "mask", "G", "loss"), what="after reset")
    complete2, refs2, flows2 = _inputs(B, N, lens, clustered, seed=1)
    refs2, flows2 = _t(refs2, dev), _t(flows2, dev)
    want, _ = _yardstick(pc, cano, refs2, flows2, 1, False, True)
    _same(_run(FlowTerm(refs2, flows2, 1, robust=True), pc, cano), want, what="other references")


def test_captured_calls_equal_eager_calls(dev):
    from reart_amd.utils.flow_utils import FlowTerm

    B, N, lens, clustered = SHAPES[3]
    complete, refs, flows = _inputs(B, N, lens, clustered)
    refs, flows = _t(refs, dev), _t(flows, dev)
    rng = np.random.default_rng(3)
    clouds = [_split((complete + rng.normal(0, 1e-3 * k, complete.shape)).astype(np.float32), 1, dev) for k in range(3)]
    eager_mod, graph_mod = FlowTerm(refs, flows, 1), FlowTerm(refs, flows, 1)
    eager = [_run(eager_mod, pc, cano) for pc, cano in clouds]
    _same(_run(graph_mod, *clouds[0]), eager[0])
    xs = [pc.clone().requires_grad_(True) for pc, _ in clouds]
    graph, outs = torch.cuda.CUDAGraph(), []
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        for x, (_, cano) in list(zip(xs, clouds))[1:]:
            loss = graph_mod(x, cano)
            (G,) = torch.autograd.grad(loss, x)
            outs.append(dict(zip(("gt", "mask", "dists", "idx"), graph_mod.last), G=G, loss=loss.detach()))
    graph.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, eager[1:]):
        _same(o, e, keys=("idx", "dists", "gt", "mask", "G", "loss"), what="captured")


def test_accumulate_adds_onto_g(dev):
    from reart_amd import _lib
    from reart_amd.utils.flow_utils import FlowTerm

    B, N, lens, clustered = SHAPES[2]
    complete, refs, flows = _inputs(B, N, lens, clustered)
    refs, flows = _t(refs, dev), _t(flows, dev)
    for c in (0, 1, 3):
        pc, cano = _split(complete, c, dev)
        for spatial_sort in (False, True):
            mod = FlowTerm(refs, flows, c, weight=0.7, spatial_sort=spatial_sort)
            G = _run(mod, pc, cano)["G"]
            st = mod._get_state(N, cano)
            G0 = torch.randn_like(G)
            acc = G0.clone()
            rc = _lib.lib().reart_flow_term(_lib.ptr(pc), _lib.ptr(cano), _lib.ptr(st["order"]), B, N, c, 1, 0, 1e-2, 0.7, _lib.ptr(st["seed"]),
                                            None, None, None, None, None, _lib.ptr(acc), 1, _lib.ptr(st["ws"]), st["ws"].numel(), _lib.stream())
            assert rc == 0
            assert torch.equal(acc, G0 + G), (c, spatial_sort)


@pytest.mark.parametrize("spatial_sort", [False, True])
def test_golden(dev, spatial_sort):
    from reart_amd.utils.flow_utils import FlowTerm

    g = np.load(os.path.join(ROOT, "tests", "golden", "flow_term.npz"))
    refs, flows = _t([g[f"ref{f}"] for f in range(3)], dev), _t([g[f"flow{f}"] for f in range(3)], dev)
    pc, cano = torch.from_numpy(g["pc_trans"]).to(dev), torch.from_numpy(g["cano"]).to(dev)
    for c in (0, 1, 3):
        for robust in (0, 1):
            tag = f"c{c}_r{robust}"
            got = _run(FlowTerm(refs, flows, c, robust=bool(robust), spatial_sort=spatial_sort), pc, cano)
            np.testing.assert_array_equal(got["mask"].cpu().numpy(), g[f"mask_{tag}"])
            np.testing.assert_array_equal(got["idx"].cpu().numpy(), g[f"idx_{tag}"])
            np.testing.assert_allclose(got["gt"].cpu().numpy(), g[f"gt_{tag}"], rtol=0, atol=1e-5 * np.abs(g[f"gt_{tag}"]).max())
            assert abs(float(got["loss"]) - float(g[f"loss_{tag}"])) <= 1e-5 * abs(float(g[f"loss_{tag}"]))
            np.testing.assert_allclose(got["G"].cpu().numpy(), g[f"grad_{tag}"], rtol=0, atol=1e-5 * np.abs(g[f"grad_{tag}"]).max())


def test_what_the_native_call_does_not_serve_takes_the_composition(dev):
    from reart_amd.utils.flow_utils import FlowTerm

    B, N, lens, clustered = SHAPES[2]
    complete, refs, flows = _inputs(B, N, lens, clustered)
    refs, flows = _t(refs, dev), _t(flows, dev)
    pc, cano = _split(complete, 1, dev)
    want, _ = _yardstick(pc, cano, refs, flows, 1, False, False)
    mod = FlowTerm(refs, flows, 1)
    x = pc.double().requires_grad_(True)
    loss = mod(x, cano.double())
    (G,) = torch.autograd.grad(loss, x)
    assert mod.last[2] is None and torch.equal(mod.last[0], want["gt"]) and torch.equal(mod.last[1], want["mask"])
    assert torch.equal(loss.detach(), want["loss"]) and torch.equal(G.float(), want["G"])
    with pytest.raises(Exception):
        mod(pc[:2], cano)                                    # not [B,N,3]: the composition's own refusal


def _loop(dev, seq, composition, n_iter=6):
    from reart_amd import run_robot as rr
    from reart_amd.networks.model import BaseModel
    from reart_amd.synthetic import split_canonical
    from reart_amd.utils.model_utils import tau_cosine

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cano, pcs = split_canonical(seq["complete"].astype(np.float32), 2)
    a = rr.build_parser().parse_args(["--model", "base", "--use_flow_loss", "--cano_idx", "2", "--fused_losses", "--fused_flow"])
    torch.manual_seed(4)
    model = BaseModel(num_parts=a.num_parts, pose_len=pcs.shape[0]).to(dev)
    tau = functools.partial(tau_cosine, max_iter=a.n_iter, end_temp=a.end_tau, start_temp=a.start_tau)
    loop = rr.OperatorLoop(a, model, t(cano), t(pcs), [t(r.astype(np.float32)) for r in seq["ref_loc"]],
                           [t(f.astype(np.float32)) for f in seq["ref_flow"]], tau)
    assert loop.flow_term is not None and loop.flow_term.weight == a.lambda_flow
    if composition:
        loop.flow_term = None
    torch.manual_seed(9)                                         # the Gumbel draws of the model's forward
    rows = [{k: float(v.detach()) for k, v in loop.iteration(i).items()} for i in range(n_iter)]
    return rows, torch.cat([p.detach().flatten() for p in model.parameters()])


def test_operator_loop_with_the_flow_term(dev):
    """Six iterations of OperatorLoop --fused_losses --fused_flow at T = 4, N = 256 with FlowTerm and with the composition in its place: the
    gradients are bit for bit the same, so the parameters are."""
    from reart_amd.synthetic import make_sequence

    seq = make_sequence(T=4, n_parts=4, pts_per_part=64, with_flow=True)
    assert seq["complete"].shape[1] == 256
    rows_on, p_on = _loop(dev, seq, False)
    rows_off, p_off = _loop(dev, seq, True)
    for i, (on, off) in enumerate(zip(rows_on, rows_off)):
        print(f"iteration {i}: flow {on['flow Loss']!r} / {off['flow Loss']!r}, total {on['total Loss']!r} / {off['total Loss']!r}")
    assert torch.isfinite(p_on).all() and torch.equal(p_on, p_off)
    for on, off in zip(rows_on, rows_off):
        assert on["recon Loss"] == off["recon Loss"]
        assert abs(on["flow Loss"] - off["flow Loss"]) <= float(np.spacing(np.float32(off["flow Loss"])))


@pytest.mark.parametrize("N", [256, 1024])
def test_kinematic_engine_with_warm_flow(dev, N):
    """Six iterations of KinematicEngine at T = 4 with warm_flow on and off: the same parameters, assignments and gradient bit
    for bit, the losses to one ulp.  N = 256: every launch eager (128 sampled points are below the in-place re-solve's range).
    N = 1024, assign_gap 1: from the third iteration the post graph, with the pair reart_kin_post + reart_flow_term captured in
    it, is replayed around every re-solve."""
    from reart_amd.kinematic_engine import KinematicEngine
    from reart_amd.knn_cuda import KNN
    from reart_amd.networks.model import KinematicModel

    k = np.load(os.path.join(ROOT, "tests", "golden", "kinematic.npz"))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    B = 3
    cano = t(k["cano_pc"][:N])

    def model():
        edge_index = {f"{c}_{int(k['parent'][c])}": int(k["edge_of_part"][c]) for c in range(len(k["parent"])) if k["parent"][c] >= 0}
        return KinematicModel(pose_len=B, seg_part=t(k["seg_part"][:N]), cano_pc=cano, knn=KNN(k=1, transpose_mode=True),
                              edge_index=edge_index, paths_to_base=None, reverse_topo=[int(v) for v in k["order"]],
                              axis_list=t(k["axis"]), moment_list=t(k["moment"]), theta_list=t(k["theta"][:B])).to(dev)

    rng = np.random.default_rng(5)
    with torch.no_grad():
        pcs = model()(cano)[0]
    pcs = (pcs + t(rng.normal(0, 0.004, (B, N, 3)).astype(np.float32))).contiguous()
    pcs = torch.stack([p[torch.from_numpy(rng.permutation(N)).to(dev)] for p in pcs])
    comp = torch.cat((pcs[:2], cano[None], pcs[2:]), dim=0)
    sel = [torch.from_numpy(rng.permutation(N)[:100 + 7 * f]).to(dev) for f in range(B)]
    refs = [comp[f][s] for f, s in enumerate(sel)]
    flows = [(comp[f + 1][s] - comp[f][s]) * 0.5 for f, s in enumerate(sel)]
    outs = []
    for warm in (True, False):
        m = model()
        eng = KinematicEngine(m, cano, pcs, 2, refs, flows, assign_iter=0, assign_gap=1, downsample=2, warm_flow=warm)
        assert (eng._flow_term is not None) == warm
        rows = []
        for i in range(6):
            losses = eng.iteration(i)
            rows.append({key: float(v) for key, v in losses.items()})
        assert (eng._g_post is not None) == (N == 1024) and eng.lap_fallbacks == 0
        outs.append(([getattr(m, n_).detach().clone() for n_ in ("axis_list", "moment_list", "theta_list")]
                     + [eng.lap_state["cols"].clone(), eng.matched.clone(), eng.G.clone()], rows))
    for a, b in zip(outs[0][0], outs[1][0]):
        assert torch.equal(a, b)
    for i, (on, off) in enumerate(zip(outs[0][1], outs[1][1])):
        print(f"iteration {i}: warm {on} | plain {off}")
        assert sorted(on) == sorted(off) == ["flow Loss", "opt assignment loss", "total Loss"]
        assert on["opt assignment loss"] == off["opt assignment loss"]
        for key in ("flow Loss", "total Loss"):
            assert abs(on[key] - off[key]) <= float(np.spacing(np.float32(off[key]))), (i, key, on, off)


def test_headline_shape(dev):
    """T = 20, N = 4096 against 19 sets of 3000 points: sixteen columns of nineteen workgroups hand their gradients over inside the
    launch, on whichever XCDs they run.  Cold and warm."""
    from reart_amd.synthetic import make_sequence, split_canonical
    from reart_amd.utils.flow_utils import FlowTerm

    seq = make_sequence(T=20, n_parts=8, pts_per_part=512, seed=2, n_ref=3000, with_flow=True)
    cano, pcs = split_canonical(seq["complete"], 2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(dev)
    pc, cano = t(pcs), t(cano)
    refs, flows = [t(r) for r in seq["ref_loc"]], [t(f) for f in seq["ref_flow"]]
    want, total = _yardstick(pc, cano, refs, flows, 2, False, False)
    mod = FlowTerm(refs, flows, 2)
    for what in ("cold", "warm", "warm again"):
        got = _run(mod, pc, cano)
        _same(got, want, what=what)
        _loss_ok(got, total, what=what)
