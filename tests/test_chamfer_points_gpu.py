"""``ChamferPoints`` (reart_chamfer_points, reart_chamfer_points_backward) and ``WarmChamferDistance``: the per-point
distances of the warm-started search with a backward for per-point upstream gradients.  Neighbours and distances bit for
bit against the brute-force contract (oracle.knn_points) for any seeds, both storage settings and every choice of
directions; the gradients to a bound derived per component; bit for bit ``ChamferLoss`` when the upstream is 1; warm
state never changes a result."""
import numpy as np
import pytest
import torch

from tests import chamfer_points_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # half an ulp of a float32, relative

SHAPES = [(1, 1, 1), (1, 1, 3), (2, 15, 17), (2, 64, 64), (3, 100, 130), (2, 513, 40), (2, 300, 200), (3, 100, 257), (2, 1500, 1000)]


def _clouds(N, P1, P2):
    """The generator, ranges and seeds of test_chamfer_loss_gpu.py::test_exact_for_any_seed (no ties between distinct targets)."""
    rng = np.random.default_rng(1000 * N + 31 * P1 + P2)
    x = rng.uniform(-0.4, 0.4, (N, P1, 3)).astype(np.float32)
    y = rng.uniform(-0.4, 0.4, (N, P2, 3)).astype(np.float32)
    return rng, x, y


def _upstream(rng, shape, lo=-6.0, hi=3.0):
    """Random normal times 10^uniform(lo, hi), a third of the entries exactly 0, both signs present."""
    g = (rng.normal(0, 1, shape) * 10.0 ** rng.uniform(lo, hi, shape)).astype(np.float32)
    g[rng.uniform(0, 1, shape) < 1.0 / 3.0] = 0.0
    if g.size >= 2:
        flat = g.reshape(-1)
        flat[0], flat[-1] = abs(flat[0]) + np.float32(0.5), -abs(flat[-1]) - np.float32(0.5)
    return g


def _run(mod, x, y, dev, g_xy=None, g_yx=None, grad_y=True, directions="both"):
    """One forward, and a backward of sum(g_xy d_xy) + sum(g_yx d_yx) over the upstreams given (the upstream that arrives
    at the operator is then g itself: 1 * g is exact) -> numpy results in the caller's numbering."""
    tx = torch.from_numpy(x).to(dev).requires_grad_(True) if isinstance(x, np.ndarray) else x
    ty = torch.from_numpy(y).to(dev).requires_grad_(grad_y) if isinstance(y, np.ndarray) else y
    tx.grad = None
    if ty.requires_grad:
        ty.grad = None
    d_xy, d_yx = mod(tx, ty, directions)
    out = {"o_xy": None if d_xy is None else d_xy.detach().cpu().numpy(), "o_yx": None if d_yx is None else d_yx.detach().cpu().numpy()}
    total = None
    for d, g in ((d_xy, g_xy), (d_yx, g_yx)):
        if g is not None:
            term = (d * torch.from_numpy(g).to(dev)).sum()
            total = term if total is None else total + term
    if total is not None:
        total.backward()
    for k, v in zip(("d_xy", "i_xy", "d_yx", "i_yx"), mod.last):
        out[k] = None if v is None else v.cpu().numpy()
    out["gx"] = None if tx.grad is None else tx.grad.cpu().numpy()
    out["gy"] = None if ty.grad is None else ty.grad.cpu().numpy()
    out["bits"] = mod.fx_bits.cpu().numpy() if total is not None else None
    return out


def _same(a, b, keys=("d_xy", "i_xy", "d_yx", "i_yx", "gx", "gy")):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _exact(oracle, out, x, y, directions="both"):
    """d and i of the searched directions equal the brute-force contract bit for bit, as .last and as the returned
    distances; the other direction is None."""
    for name, q, t, want in (("xy", x, y, directions in ("both", "xy")), ("yx", y, x, directions in ("both", "yx"))):
        if not want:
            assert out["d_" + name] is None and out["i_" + name] is None and out["o_" + name] is None
            continue
        d, i = oracle.knn_points(q, t, K=1)
        np.testing.assert_array_equal(out["i_" + name], i[..., 0])
        np.testing.assert_array_equal(out["d_" + name], d[..., 0])
        np.testing.assert_array_equal(out["o_" + name], d[..., 0])


def _grad_ok(out, x, y, g_xy, g_yx, label=""):
    """Per component, against the float64 formulas evaluated on the float32 inputs and upstreams with the operator's own
    indices.  The kernel computes, in float32 unless said otherwise,

        grad = fl( fl(2 g_i) fl(x_i - y_nn(i)) )  +  fl( 2 * 2^-bits * sum_j trunc( fl( g_j fl(x_i - y_j) ) * 2^bits ) )

    - a float32 difference carries at most half an ulp, relative U = 2^-24; 2 g_i is exact; the product rounds once more.
      First term: 2 U |own| (to first order).  Every addend likewise carries the rounding of its difference and of its
      product: together 2 U mag, mag = sum_j |2 g_j (x_i - y_j)| (the doubling is exact);
    - every fixed-point addend is truncated toward zero by less than one quantum 2^-bits (bits of THIS output cloud, read
      back from the call), doubled: 2 cnt 2^-bits over the cnt addends (an addend with g_j = 0 is skipped by the kernel and
      is exactly 0 in the reference; counting it only loosens the bound by its quantum, which the kernel could also have
      spent); the integer sum itself is exact whatever the order;
    - the sum is converted to float32 once: U |scat|; the final addition rounds once: U |grad|.
    The magnitudes are the float64 reference's; the computed ones differ from them by the error terms themselves, a
    second-order effect (relative 2^-23 of the bound) covered by the factor 1 + 2^-20, as is the conversion of the
    64-bit sum to double (relative 2^-53)."""
    g = ref.gradients(x, y, out["i_xy"], out["i_yx"], g_xy, g_yx)
    for c, (name, got) in enumerate((("x", out["gx"]), ("y", out["gy"]))):
        if got is None:
            continue
        r = g[name]
        quantum = np.exp2(-out["bits"][:, c].astype(np.float64))[:, None, None]
        bound = (U * (2.0 * np.abs(r["own"]) + 2.0 * r["mag"] + np.abs(r["scat"]) + np.abs(r["grad"]))
                 + 2.0 * r["cnt"][..., None] * quantum) * (1.0 + 2.0 ** -20)
        err = np.abs(got.astype(np.float64) - r["grad"])
        worst = np.unravel_index(np.argmax(err - bound), err.shape)
        print(f"{label}grad_{name}: max err {err.max():.3e}, err/bound max {np.max(err / np.maximum(bound, 1e-300)):.3f}, "
              f"bits {out['bits'][:, c].tolist()}, worst {worst} err {err[worst]:.3e} bound {bound[worst]:.3e}")
        assert (out["bits"][:, c] >= 0).all() and (out["bits"][:, c] <= 39).all()
        assert (err <= bound).all(), (name, worst, err[worst], bound[worst])


@pytest.mark.parametrize("spatial_sort", [False, True])
@pytest.mark.parametrize("N,P1,P2", SHAPES)
def test_exact_for_any_seed(oracle, dev, N, P1, P2, spatial_sort):
    """Cold, random valid and garbage seeds (-5 .. P+5, repeated): neighbours and distances of both directions equal the
    brute-force contract bit for bit, also when only one direction is asked for (the other is None); later calls equal the
    first."""
    from reart_amd.utils.chamfer import ChamferPoints

    rng, x, y = _clouds(N, P1, P2)
    mod = ChamferPoints(spatial_sort=spatial_sort)
    tx, ty = torch.from_numpy(x).to(dev).requires_grad_(True), torch.from_numpy(y).to(dev).requires_grad_(True)
    garbage_xy, garbage_yx = rng.integers(-5, P2 + 5, (N, P1)), rng.integers(-5, P1 + 5, (N, P2))
    garbage_xy[:, ::3], garbage_yx[:, ::3] = 0, 0
    first = None
    for seeds in (None, (rng.integers(0, P2, (N, P1)), rng.integers(0, P1, (N, P2))), (garbage_xy, garbage_yx)):
        for directions in ("both", "xy", "yx"):
            if seeds is not None:
                mod.seed(tx, ty, torch.from_numpy(seeds[0]), torch.from_numpy(seeds[1]))
            out = _run(mod, tx, ty, dev, directions=directions)
            _exact(oracle, out, x, y, directions)
            if first is None:
                first = out
            elif directions == "both":
                _same(out, first)
    # single directions on a fresh module: no image of the other cloud was ever built
    for directions in ("yx", "xy"):
        _exact(oracle, _run(ChamferPoints(spatial_sort=spatial_sort), tx, ty, dev, directions=directions), x, y, directions)


@pytest.mark.parametrize("spatial_sort", [False, True])
@pytest.mark.parametrize("N,P1,P2", SHAPES)
def test_gradients_within_the_derived_bound(dev, N, P1, P2, spatial_sort):
    """Upstreams over nine decades with a third of exact zeros and both signs: both gradients hold the bound of
    ``_grad_ok``; so do the gradients when only one of the two outputs is used."""
    from reart_amd.utils.chamfer import ChamferPoints

    rng, x, y = _clouds(N, P1, P2)
    g_xy, g_yx = _upstream(rng, (N, P1)), _upstream(rng, (N, P2))
    mod = ChamferPoints(spatial_sort=spatial_sort)
    out = _run(mod, x, y, dev, g_xy, g_yx)
    assert out["gx"] is not None and out["gy"] is not None and out["bits"].shape == (N, 2)
    _grad_ok(out, x, y, g_xy, g_yx)
    _grad_ok(_run(mod, x, y, dev, g_xy, None), x, y, g_xy, None, "d_xy only: ")
    _grad_ok(_run(mod, x, y, dev, None, g_yx), x, y, None, g_yx, "d_yx only: ")


@pytest.mark.parametrize("spatial_sort", [False, True])
@pytest.mark.parametrize("N,P1,P2", SHAPES)
def test_sum_of_both_outputs_is_chamfer_loss(dev, N, P1, P2, spatial_sort):
    """(d_xy.sum() + d_yx.sum()).backward(): with g = 1 the arithmetic is chamfer_loss_kernel's, so whenever both report
    the same fractional bits -- 39 at these shapes and ranges -- x.grad and y.grad are ChamferLoss's bit for bit, and the
    distances are its ``.last``."""
    from reart_amd.utils.chamfer import ChamferLoss, ChamferPoints

    _, x, y = _clouds(N, P1, P2)
    tx, ty = torch.from_numpy(x).to(dev).requires_grad_(True), torch.from_numpy(y).to(dev).requires_grad_(True)
    loss_mod, mod = ChamferLoss(spatial_sort=spatial_sort), ChamferPoints(spatial_sort=spatial_sort)
    loss_mod(tx, ty).backward()
    want_x, want_y = tx.grad.clone(), ty.grad.clone()
    tx.grad = ty.grad = None
    d_xy, d_yx = mod(tx, ty)
    (d_xy.sum() + d_yx.sum()).backward()
    assert (loss_mod.fx_bits.cpu().numpy() == 39).all() and (mod.fx_bits.cpu().numpy() == 39).all()
    assert torch.equal(tx.grad, want_x) and torch.equal(ty.grad, want_y)
    for a, b in zip(mod.last, loss_mod.last):
        assert torch.equal(a, b)
    assert torch.equal(d_xy.detach(), loss_mod.last[0]) and torch.equal(d_yx.detach(), loss_mod.last[2])


@pytest.mark.parametrize("spatial_sort", [False, True])
def test_upstream_special_cases(dev, spatial_sort):
    from reart_amd.utils.chamfer import ChamferPoints

    N, P1, P2 = 2, 130, 90
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, (N, P1, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (N, P2, 3)).astype(np.float32)
    g_xy, g_yx = _upstream(rng, (N, P1), -2, 2), _upstream(rng, (N, P2), -2, 2)
    mod = ChamferPoints(spatial_sort=spatial_sort)
    # an all-zero upstream gives exact zeros
    z = _run(mod, x, y, dev, np.zeros_like(g_xy), np.zeros_like(g_yx))
    assert not z["gx"].any() and not z["gy"].any()
    # only d_xy used (its upstream arrives, the other is None) equals an explicit zero upstream for d_yx
    a = _run(mod, x, y, dev, g_xy, None)
    b = _run(mod, x, y, dev, g_xy, np.zeros_like(g_yx))
    _same(a, b)
    _grad_ok(a, x, y, g_xy, None)
    # y without grad: no y.grad, the same x.grad
    full = _run(mod, x, y, dev, g_xy, g_yx)
    nogy = _run(mod, x, y, dev, g_xy, g_yx, grad_y=False)
    assert nogy["gy"] is None and full["gy"].any()
    np.testing.assert_array_equal(nogy["gx"], full["gx"])
    assert (nogy["bits"][:, 1] == 0).all() and (nogy["bits"][:, 0] == full["bits"][:, 0]).all()
    # half the upstream gives exactly half.  Below the clamp at 39, halving every upstream halves m, lowers e by one and
    # raises bits by one: fl(g/2 * diff) * 2^(bits+1) is the same integer, so the sums are the same integers and every
    # step after them scales by the power of two exactly.  2^24 g puts bits (39 for the plain upstreams) below the clamp
    big_xy, big_yx = g_xy * np.float32(2.0 ** 24), g_yx * np.float32(2.0 ** 24)
    one = _run(mod, x, y, dev, big_xy, big_yx)
    half = _run(mod, x, y, dev, np.float32(0.5) * big_xy, np.float32(0.5) * big_yx)
    assert (one["bits"] < 39).all() and (half["bits"] == one["bits"] + 1).all(), (one["bits"], half["bits"])
    np.testing.assert_array_equal(half["gx"], np.float32(0.5) * one["gx"])
    np.testing.assert_array_equal(half["gy"], np.float32(0.5) * one["gy"])
    _grad_ok(one, x, y, big_xy, big_yx)
    # a mask: weight 0 on every second x point, only d_xy used.  Those points get no gradient at all, and y gets exactly
    # what the remaining points alone send: the same addends at the same bits, hence the same integers
    masked = g_xy.copy()
    masked[:, ::2] = 0.0
    m = _run(mod, x, y, dev, masked, None)
    assert not m["gx"][:, ::2].any() and m["gx"][:, 1::2].any()
    sub = _run(ChamferPoints(spatial_sort=spatial_sort), x[:, 1::2].copy(), y, dev, masked[:, 1::2].copy(), None)
    np.testing.assert_array_equal(m["bits"][:, 1], sub["bits"][:, 1])
    np.testing.assert_array_equal(m["gy"], sub["gy"])
    np.testing.assert_array_equal(m["gx"][:, 1::2], sub["gx"])
    _grad_ok(m, x, y, masked, None)


def test_cluster_on_one_target(dev):
    """1000 y points whose nearest x is one and the same point (chamfer_loss_ref.cluster_case, checked on the CPU in
    test_chamfer_loss_cpu.py): the longest fixed-point sum the shapes allow, with upstreams from 1e-3 to 1e3."""
    from reart_amd.utils.chamfer import ChamferPoints

    x, y = ref.cluster_case()
    rng = np.random.default_rng(4)
    g_xy = (rng.choice([-1.0, 1.0], x.shape[:2]) * 10.0 ** rng.uniform(-3, 3, x.shape[:2])).astype(np.float32)
    g_yx = (rng.choice([-1.0, 1.0], y.shape[:2]) * 10.0 ** rng.uniform(-3, 3, y.shape[:2])).astype(np.float32)
    out = _run(ChamferPoints(), x, y, dev, g_xy, g_yx)
    assert (out["i_yx"] == 0).all()
    assert ref.gradients(x, y, out["i_xy"], out["i_yx"], g_xy, g_yx)["x"]["cnt"][0, 0] == 1000
    print("fx_bits", out["bits"].tolist())
    _grad_ok(out, x, y, g_xy, g_yx)


@pytest.fixture(scope="module")
def moving():
    """The coherent moving clouds of test_chamfer_loss_gpu.py: x drifts a little more every call."""
    from reart_amd.synthetic import make_sequence

    frames = make_sequence(T=4, n_parts=4, pts_per_part=512, seed=5, with_flow=False)["complete"].astype(np.float32)
    rng = np.random.default_rng(1)
    xs = [(frames[0][None] + rng.normal(0, 2e-3 * (it + 1), frames[0][None].shape)).astype(np.float32) for it in range(4)]
    g_xy, g_yx = _upstream(rng, xs[0].shape[:2], -2, 2), _upstream(rng, frames[1][None].shape[:2], -2, 2)
    return xs, frames[1][None].copy(), frames[2][None].copy(), g_xy, g_yx


@pytest.mark.parametrize("spatial_sort", [False, True])
def test_warm_state_never_changes_a_result(oracle, dev, moving, spatial_sort):
    """Four calls with the seeds carried from call to call, then y replaced by another tensor, then y modified in place:
    every call equals a fresh module on the same inputs in distances, indices and gradients, bit for bit.  Two forwards
    followed by the backward of the FIRST give the first call's gradients: the backward reads no state of the module."""
    from reart_amd.utils.chamfer import ChamferPoints

    xs, y0, y1, g_xy, g_yx = moving
    mod = ChamferPoints(spatial_sort=spatial_sort)
    ty = torch.from_numpy(y0).to(dev).requires_grad_(True)

    def both(x, ty_):
        out = _run(mod, x, ty_, dev, g_xy, g_yx)
        _same(out, _run(ChamferPoints(spatial_sort=spatial_sort), x, ty_, dev, g_xy, g_yx))
        return out

    outs = [both(x, ty) for x in xs]
    _exact(oracle, outs[-1], xs[-1], y0)
    _same(_run(mod, xs[-1], ty, dev, g_xy, g_yx), outs[-1])    # same inputs, same state
    # a "yx" call in between leaves y's image alone, and the next call still finds it valid
    _exact(oracle, _run(mod, xs[2], ty, dev, directions="yx"), xs[2], y0, "yx")
    _same(_run(mod, xs[-1], ty, dev, g_xy, g_yx), outs[-1])
    # two forwards, then the backward of the first
    tx0, tx1 = (torch.from_numpy(x).to(dev).requires_grad_(True) for x in (xs[0], xs[3]))
    ty.grad = None
    d0 = mod(tx0, ty)
    mod(tx1, ty)
    ((d0[0] * torch.from_numpy(g_xy).to(dev)).sum() + (d0[1] * torch.from_numpy(g_yx).to(dev)).sum()).backward()
    np.testing.assert_array_equal(tx0.grad.cpu().numpy(), outs[0]["gx"])
    np.testing.assert_array_equal(ty.grad.cpu().numpy(), outs[0]["gy"])
    assert tx1.grad is None
    ty2 = torch.from_numpy(y1).to(dev).requires_grad_(True)    # another tensor
    out = both(xs[0], ty2)
    _exact(oracle, out, xs[0], y1)
    with torch.no_grad():                                      # the same tensor, modified in place
        ty2.copy_(torch.from_numpy(y0).to(dev))
    out = both(xs[1], ty2)
    _exact(oracle, out, xs[1], y0)
    _same(out, outs[1])


@pytest.mark.parametrize("spatial_sort", [False, True])
@pytest.mark.parametrize("N,P", [(N, P1) for N, P1, P2 in SHAPES if P1 == P2])
def test_adapter_equals_chamfer_distance(dev, N, P, spatial_sort):
    """WarmChamferDistance against ChamferDistance in the three modes: equal values and equal indices (the clouds have no
    ties between distinct targets).  The gradients of recon_loss through the adapter hold the bound of ``_grad_ok`` (g = 1
    in both directions) around the float64 restatement; the composition's own deviation is printed beside it."""
    from reart_amd.networks.loss import recon_loss
    from reart_amd.utils.chamfer import ChamferDistance, WarmChamferDistance

    _, x, y = _clouds(N, P, P)
    tx, ty = torch.from_numpy(x).to(dev).requires_grad_(True), torch.from_numpy(y).to(dev).requires_grad_(True)
    cold, warm = ChamferDistance(), WarmChamferDistance(spatial_sort=spatial_sort)
    for _ in range(2):                                          # the second round is warm
        for mode in (dict(), dict(reverse=True), dict(bidirectional=True)):
            want, got = cold(tx, ty, return_index=True, **mode), warm(tx, ty, return_index=True, **mode)
            assert len(want) == len(got) == (3 if mode.get("bidirectional") else 2)
            for a, b in zip(want, got):
                assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
            assert torch.equal(cold(tx, ty, **mode), warm(tx, ty, **mode))
    res = {}
    for name, cd in (("composition", cold), ("operator", warm)):
        tx.grad = ty.grad = None
        loss = recon_loss(tx, ty, cd)
        loss.backward()
        res[name] = (float(loss.detach()),tx.grad.cpu().numpy(), ty.grad.cpu().numpy())
    assert res["operator"][0] == res["composition"][0]
    d_xy, i_xy, d_yx, i_yx = (v.cpu().numpy() for v in warm.points.last)
    one_x, one_y = np.ones((N, P), np.float32), np.ones((N, P), np.float32)
    want = ref.gradients(x, y, i_xy, i_yx, one_x, one_y)
    for name, k in (("x", 1), ("y", 2)):
        print(f"composition grad_{name}: max deviation from float64 {np.abs(res['composition'][k] - want[name]['grad']).max():.3e}")
    out = {"i_xy": i_xy, "i_yx": i_yx, "gx": res["operator"][1], "gy": res["operator"][2], "bits": warm.points.fx_bits.cpu().numpy()}
    _grad_ok(out, x, y, one_x, one_y, "operator ")


def test_captured_calls_equal_eager_calls(dev, moving):
    """After one eager call, two forward + backward calls captured in a graph on a single stream and replayed equal their
    eager results."""
    from reart_amd.utils.chamfer import ChamferPoints

    xs, y0, _, g_xy, g_yx = moving
    ty = torch.from_numpy(y0).to(dev)
    w, v = torch.from_numpy(g_xy).to(dev), torch.from_numpy(g_yx).to(dev)
    eager_mod, graph_mod = ChamferPoints(), ChamferPoints()
    eager = [_run(eager_mod, x, ty, dev, g_xy, g_yx) for x in xs[:3]]
    txs = [torch.from_numpy(x).to(dev).requires_grad_(True) for x in xs[:3]]
    _same(_run(graph_mod, txs[0], ty, dev, g_xy, g_yx), eager[0])
    graph = torch.cuda.CUDAGraph()
    outs = []
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        for tx in txs[1:]:
            d_xy, d_yx = graph_mod(tx, ty)
            (gx,) = torch.autograd.grad((d_xy * w).sum() + (d_yx * v).sum(), tx)
            outs.append((gx,) + tuple(graph_mod.last))
    graph.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, eager[1:]):
        got = dict(zip(("gx", "d_xy", "i_xy", "d_yx", "i_yx"), (t.detach().cpu().numpy() for t in o)))
        got["gy"] = None
        _same(got, e)


def test_other_dimensions_and_float64_take_the_plain_path(dev):
    """D = 2 and float64: the values and gradients of knn_points; .last is filled; a direction not asked for is None."""
    from reart_amd.utils.chamfer import ChamferPoints, knn_points

    rng = np.random.default_rng(5)
    for x, y in ((rng.uniform(-1, 1, (2, 40, 2)).astype(np.float32), rng.uniform(-1, 1, (2, 30, 2)).astype(np.float32)),
                 (rng.uniform(-1, 1, (2, 40, 3)), rng.uniform(-1, 1, (2, 30, 3)))):
        tx, ty = torch.from_numpy(x).to(dev).requires_grad_(True), torch.from_numpy(y).to(dev).requires_grad_(True)
        w = torch.from_numpy(rng.normal(0, 1, (2, 40))).to(dev, tx.dtype)
        v = torch.from_numpy(rng.normal(0, 1, (2, 30))).to(dev, tx.dtype)
        fwd, bwd = knn_points(tx, ty, K=1), knn_points(ty, tx, K=1)
        ((fwd.dists[..., 0] * w).sum() + (bwd.dists[..., 0] * v).sum()).backward()
        want_x, want_y = tx.grad.clone(), ty.grad.clone()
        tx.grad = ty.grad = None
        mod = ChamferPoints()
        d_xy, d_yx = mod(tx, ty)
        ((d_xy * w).sum() + (d_yx * v).sum()).backward()
        assert d_xy.dtype == tx.dtype and torch.equal(d_xy, fwd.dists[..., 0]) and torch.equal(d_yx, bwd.dists[..., 0])
        assert torch.equal(tx.grad, want_x) and torch.equal(ty.grad, want_y)
        last = mod.last
        assert torch.equal(last[0], d_xy.detach()) and torch.equal(last[1], fwd.idx[..., 0])
        assert torch.equal(last[2], d_yx.detach()) and torch.equal(last[3], bwd.idx[..., 0])
        only, none = mod(tx, ty, "yx")[::-1]
        assert none is None and torch.equal(only, d_yx) and mod.last[0] is None and mod.last[1] is None
