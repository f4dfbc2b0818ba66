"""``ChamferLoss`` (reart_chamfer_loss): the bidirectional K = 1 Chamfer sum with its gradient as one warm-started call.
Neighbours and distances bit for bit against the brute-force contract (oracle.knn_points) for any seeds and both storage
settings; warm state never changes a result; the loss to one rounding; the gradients to a bound derived per component."""
import numpy as np
import pytest
import torch

from tests import chamfer_loss_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # half an ulp of a float32, relative


def _run(mod, x, y, dev, grad_y=False, upstream=None):
    """One forward + backward -> numpy results in the caller's numbering."""
    tx = torch.from_numpy(x).to(dev).requires_grad_(True) if isinstance(x, np.ndarray) else x
    ty = torch.from_numpy(y).to(dev).requires_grad_(grad_y) if isinstance(y, np.ndarray) else y
    tx.grad = None
    if ty.requires_grad:
        ty.grad = None
    loss = mod(tx, ty)
    (loss if upstream is None else loss * upstream).backward()
    d_xy, i_xy, d_yx, i_yx = (v.cpu().numpy() for v in mod.last)
    return {"loss": loss.detach().cpu().numpy(), "d_xy": d_xy, "i_xy": i_xy, "d_yx": d_yx, "i_yx": i_yx,
            "gx": tx.grad.cpu().numpy(), "gy": None if ty.grad is None else ty.grad.cpu().numpy(),
            "bits": mod.fx_bits.cpu().numpy()}


def _same(a, b, keys=("loss", "d_xy", "i_xy", "d_yx", "i_yx", "gx", "gy")):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _exact(oracle, out, x, y):
    d1, i1 = oracle.knn_points(x, y, K=1)
    d2, i2 = oracle.knn_points(y, x, K=1)
    np.testing.assert_array_equal(out["i_xy"], i1[..., 0])
    np.testing.assert_array_equal(out["d_xy"], d1[..., 0])
    np.testing.assert_array_equal(out["i_yx"], i2[..., 0])
    np.testing.assert_array_equal(out["d_yx"], d2[..., 0])


def _loss_ok(out):
    """One float32 ulp of float32(sum(float64(d))): the kernel adds at most 2^24 float32 terms in double (relative error
    far below 2^-24) and rounds once, so at most that final rounding may differ."""
    want = ref.loss(out["d_xy"], out["d_yx"])
    got = np.float32(out["loss"])
    print("loss", got, "reference", want, "ulp", np.spacing(want))
    assert abs(np.float64(got) - np.float64(want)) <= np.float64(np.spacing(want))


def _grad_ok(out, x, y, scale=1.0):
    """Per component, against the float64 formulas evaluated on the float32 inputs with the operator's own indices.
    The kernel computes, in float32 unless said otherwise,

        g = 2 fl(x_i - y_nn(i))  +  fl( 2 * 2^-bits * sum_j trunc( fl(x_i - y_j) * 2^bits ) )

    - every float32 difference carries at most half an ulp, relative U = 2^-24; doubling is exact.  First term: U |own|;
      the addends together: U * mag, mag = sum_j |2 (x_i - y_j)|;
    - every fixed-point addend is truncated toward zero by less than one quantum 2^-bits (bits read back from the call),
      doubled: 2 cnt 2^-bits over the cnt addends; the integer sum itself is exact whatever the order;
    - the sum is converted to float32 once: U |scat|; the final addition rounds once: U |grad|.
    The magnitudes are the float64 reference's; the computed ones differ from them by the error terms themselves, a
    second-order effect (relative 2^-24 of the bound) covered by the factor 1 + 2^-20, as is the conversion of the
    64-bit sum to double (relative 2^-53)."""
    g = ref.gradients(x, y, out["i_xy"], out["i_yx"])
    for name, got in (("x", out["gx"]), ("y", out["gy"])):
        if got is None:
            continue
        r = g[name]
        quantum = np.exp2(-out["bits"].astype(np.float64))[:, None, None]
        bound = (U * (np.abs(r["own"]) + r["mag"] + np.abs(r["scat"]) + np.abs(r["grad"]))
                 + 2.0 * r["cnt"][..., None] * quantum) * (1.0 + 2.0 ** -20)
        err = np.abs(got.astype(np.float64) / scale - r["grad"])
        worst = np.unravel_index(np.argmax(err - bound), err.shape)
        print(f"grad_{name}: max err {err.max():.3e}, err/bound max {np.max(err / np.maximum(bound, 1e-300)):.3f}, "
              f"bits {out['bits'].tolist()}, worst {worst} err {err[worst]:.3e} bound {bound[worst]:.3e}")
        assert (err <= bound).all(), (name, worst, err[worst], bound[worst])


SHAPES = [(1, 1, 1), (1, 1, 3), (2, 15, 17), (2, 64, 64), (3, 100, 130), (2, 513, 40), (2, 300, 200), (3, 100, 257), (2, 1500, 1000)]


@pytest.mark.parametrize("spatial_sort", [False, True])
@pytest.mark.parametrize("N,P1,P2", SHAPES)
def test_exact_for_any_seed(oracle, dev, N, P1, P2, spatial_sort):
    """Unsorted uniform clouds with cold, random valid and garbage seeds (-5 .. P+5, repeated): neighbours and distances
    of both directions equal the brute-force contract bit for bit; loss and gradients hold their bounds."""
    from reart_amd.utils.chamfer import ChamferLoss

    rng = np.random.default_rng(1000 * N + 31 * P1 + P2)
    x = rng.uniform(-0.4, 0.4, (N, P1, 3)).astype(np.float32)
    y = rng.uniform(-0.4, 0.4, (N, P2, 3)).astype(np.float32)
    mod = ChamferLoss(spatial_sort=spatial_sort)
    tx, ty = torch.from_numpy(x).to(dev).requires_grad_(True), torch.from_numpy(y).to(dev).requires_grad_(True)
    garbage_xy, garbage_yx = rng.integers(-5, P2 + 5, (N, P1)), rng.integers(-5, P1 + 5, (N, P2))
    garbage_xy[:, ::3], garbage_yx[:, ::3] = 0, 0
    first = None
    for seeds in (None, (rng.integers(0, P2, (N, P1)), rng.integers(0, P1, (N, P2))), (garbage_xy, garbage_yx)):
        if seeds is not None:
            mod.seed(tx, ty, torch.from_numpy(seeds[0]), torch.from_numpy(seeds[1]))
        out = _run(mod, tx, ty, dev)
        _exact(oracle, out, x, y)
        if first is None:
            first = out
            _loss_ok(out)
            _grad_ok(out, x, y)
        else:
            _same(out, first)


@pytest.mark.parametrize("spatial_sort", [False, True])
def test_ties_go_to_the_lowest_index(oracle, dev, spatial_sort):
    """Every point of one cloud appears three times (in different boxes and slices), in both directions: the lowest index
    wins, also when the seed points at a later copy."""
    from reart_amd.utils.chamfer import ChamferLoss

    rng = np.random.default_rng(7)
    base = rng.uniform(-1, 1, (1, 400, 3)).astype(np.float32)
    tripled = np.concatenate([base, base, base], axis=1)
    single = np.concatenate([rng.uniform(-1, 1, (1, 300, 3)).astype(np.float32), base[:, :200]], axis=1)  # exact hits too
    for x, y in ((single, tripled), (tripled, single)):
        mod = ChamferLoss(spatial_sort=spatial_sort)
        tx, ty = torch.from_numpy(x).to(dev).requires_grad_(True), torch.from_numpy(y).to(dev)
        out = _run(mod, tx, ty, dev)
        _exact(oracle, out, x, y)
        if y is tripled:
            later_xy, later_yx = np.minimum(out["i_xy"] + 800, 1199), out["i_yx"]
            assert (out["i_xy"] < 400).all()
        else:
            later_xy, later_yx = out["i_xy"], np.minimum(out["i_yx"] + 800, 1199)
            assert (out["i_yx"] < 400).all()
        mod.seed(tx, ty, torch.from_numpy(later_xy), torch.from_numpy(later_yx))
        again = _run(mod, tx, ty, dev)
        _exact(oracle, again, x, y)
        _same(again, out)


def test_identical_clouds_give_exact_zeros(dev):
    from reart_amd.utils.chamfer import ChamferLoss

    x = np.random.default_rng(2).uniform(-1, 1, (2, 333, 3)).astype(np.float32)
    out = _run(ChamferLoss(), x, x.copy(), dev, grad_y=True)
    assert out["loss"] == 0.0 and not out["gx"].any() and not out["gy"].any()
    assert not out["d_xy"].any() and not out["d_yx"].any()
    np.testing.assert_array_equal(out["i_xy"], np.arange(333)[None].repeat(2, 0))


@pytest.fixture(scope="module")
def moving():
    """The coherent moving clouds of test_warm_coherent_clouds_over_iterations: x drifts a little more every call."""
    from reart_amd.synthetic import make_sequence

    frames = make_sequence(T=4, n_parts=4, pts_per_part=512, seed=5, with_flow=False)["complete"].astype(np.float32)
    rng = np.random.default_rng(1)
    xs = [(frames[0][None] + rng.normal(0, 2e-3 * (it + 1), frames[0][None].shape)).astype(np.float32) for it in range(4)]
    return xs, frames[1][None].copy(), frames[2][None].copy()


@pytest.mark.parametrize("spatial_sort", [False, True])
def test_warm_state_never_changes_a_result(oracle, dev, moving, spatial_sort):
    """Four calls with the seeds carried from call to call, then y replaced by another tensor, then y modified in place:
    every call equals a fresh module on the same inputs in indices, distances, loss and gradients, bit for bit; a call
    repeated with the same inputs and state gives identical bits."""
    from reart_amd.utils.chamfer import ChamferLoss

    xs, y0, y1 = moving
    mod = ChamferLoss(spatial_sort=spatial_sort)
    ty = torch.from_numpy(y0).to(dev).requires_grad_(True)

    def both(x, ty_):
        out = _run(mod, x, ty_, dev)
        _same(out, _run(ChamferLoss(spatial_sort=spatial_sort), x, ty_, dev))
        return out

    for x in xs:
        out = both(x, ty)
    _exact(oracle, out, xs[-1], y0)
    _same(_run(mod, xs[-1], ty, dev), out)                     # same inputs, same state
    ty2 = torch.from_numpy(y1).to(dev).requires_grad_(True)    # another tensor
    out = both(xs[0], ty2)
    _exact(oracle, out, xs[0], y1)
    with torch.no_grad():                                      # the same tensor, modified in place
        ty2.copy_(torch.from_numpy(y0).to(dev))
    out = both(xs[1], ty2)
    _exact(oracle, out, xs[1], y0)


@pytest.mark.parametrize("spatial_sort", [False, True])
def test_seeding_never_marks_an_image_as_built(oracle, dev, moving, spatial_sort):
    """``seed()`` prepares the module's state for its clouds but builds nothing in the native workspace: seeds installed on
    a fresh module before its first forward, and seeds installed for a y that replaced the one of the earlier calls (another
    tensor, then the same tensor modified in place), are followed by a forward that builds y's image -- results against the
    oracle and equal to a fresh module's."""
    from reart_amd.utils.chamfer import ChamferLoss

    xs, y0, y1 = moving
    rng = np.random.default_rng(3)
    P1, P2 = xs[0].shape[1], y0.shape[1]
    seeds = lambda: (torch.from_numpy(rng.integers(-5, P2 + 5, (1, P1))), torch.from_numpy(rng.integers(-5, P1 + 5, (1, P2))))
    mod = ChamferLoss(spatial_sort=spatial_sort)
    tx = torch.from_numpy(xs[0]).to(dev).requires_grad_(True)
    ty = torch.from_numpy(y0).to(dev)
    mod.seed(tx, ty, *seeds())                                 # fresh module: no native call has happened yet
    out = _run(mod, tx, ty, dev)
    _exact(oracle, out, xs[0], y0)
    _loss_ok(out)
    _same(out, _run(ChamferLoss(spatial_sort=spatial_sort), tx, ty, dev))
    ty2 = torch.from_numpy(y1).to(dev)                         # another y, first seen by seed()
    mod.seed(tx, ty2, *seeds())
    out = _run(mod, tx, ty2, dev)
    _exact(oracle, out, xs[0], y1)
    _same(out, _run(ChamferLoss(spatial_sort=spatial_sort), tx, ty2, dev))
    ty2.copy_(torch.from_numpy(y0).to(dev))                    # modified in place, first seen by seed()
    mod.seed(tx, ty2, *seeds())
    out = _run(mod, tx, ty2, dev)
    _exact(oracle, out, xs[0], y0)
    _loss_ok(out)
    _same(out, _run(ChamferLoss(spatial_sort=spatial_sort), tx, ty2, dev))


def test_cluster_on_one_target(dev):
    """1000 y points whose nearest x is one and the same point, the other x points far away (the construction is checked
    on the CPU in test_chamfer_loss_cpu.py): the longest fixed-point sum the shapes allow."""
    from reart_amd.utils.chamfer import ChamferLoss

    x, y = ref.cluster_case()
    out = _run(ChamferLoss(), x, y, dev, grad_y=True)
    assert (out["i_yx"] == 0).all()
    assert ref.gradients(x, y, out["i_xy"], out["i_yx"])["x"]["cnt"][0, 0] == 1000
    _loss_ok(out)
    _grad_ok(out, x, y)


def test_backward_fills_the_gradients(dev):
    """x.grad always, y.grad only when y requires grad; an upstream factor 0.5 halves the gradient (exactly: a power of two)."""
    from reart_amd.utils.chamfer import ChamferLoss

    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, (2, 130, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (2, 90, 3)).astype(np.float32)
    mod = ChamferLoss()
    a = _run(mod, x, y, dev, grad_y=False)
    assert a["gy"] is None and a["gx"].any()
    b = _run(mod, x, y, dev, grad_y=True)
    assert b["gy"] is not None and b["gy"].any()
    np.testing.assert_array_equal(a["gx"], b["gx"])
    _grad_ok(b, x, y)
    h = _run(mod, x, y, dev, grad_y=True, upstream=0.5)
    np.testing.assert_array_equal(h["gx"], 0.5 * b["gx"])
    np.testing.assert_array_equal(h["gy"], 0.5 * b["gy"])
    # the value of recon_loss(x, y, ChamferDistance()) needs equal sizes: compare there
    from reart_amd.networks.loss import recon_loss
    from reart_amd.utils.chamfer import ChamferDistance

    tx, tz = torch.from_numpy(x).to(dev), torch.from_numpy(x[:, ::-1].copy() + np.float32(0.01)).to(dev)
    old = float(recon_loss(tx, tz, ChamferDistance()))
    new = float(recon_loss(tx, tz, mod))
    # the per-point path rounds d_xy + d_yx per point and adds its n = N * P float32 terms in an order of torch's choosing:
    # at most (n - 1) roundings on any path through the sum, n U sum in all; the operator's sum carries one rounding
    n = x.shape[0] * x.shape[1]
    assert abs(old - new) <= n * U * old * (1.0 + 2.0 ** -20) + np.spacing(np.float32(old)), (old, new)


def test_other_dimensions_and_float64_take_the_plain_path(dev):
    from reart_amd.utils.chamfer import ChamferDistance, ChamferLoss

    rng = np.random.default_rng(5)
    for x, y in ((rng.uniform(-1, 1, (2, 40, 2)).astype(np.float32), rng.uniform(-1, 1, (2, 40, 2)).astype(np.float32)),
                 (rng.uniform(-1, 1, (2, 40, 3)), rng.uniform(-1, 1, (2, 40, 3)))):
        tx, ty = torch.from_numpy(x).to(dev).requires_grad_(True), torch.from_numpy(y).to(dev)
        mod = ChamferLoss()
        loss = mod(tx, ty)
        loss.backward()
        want = torch.sum(ChamferDistance()(tx.detach(), ty, bidirectional=True))
        assert torch.allclose(loss.detach(), want, rtol=1e-6, atol=0)
        assert tx.grad is not None and mod.last[1].shape == (2, 40)


def test_captured_calls_equal_eager_calls(dev, moving):
    """After one eager call, two more calls captured in a graph on a single stream and replayed equal their eager results."""
    from reart_amd.utils.chamfer import ChamferLoss

    xs, y0, _ = moving
    ty = torch.from_numpy(y0).to(dev)
    eager_mod, graph_mod = ChamferLoss(), ChamferLoss()
    eager = [_run(eager_mod, x, ty, dev) for x in xs[:3]]
    txs = [torch.from_numpy(x).to(dev).requires_grad_(True) for x in xs[:3]]
    _same(_run(graph_mod, txs[0], ty, dev), eager[0])
    graph = torch.cuda.CUDAGraph()
    outs = []
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        for tx in txs[1:]:
            loss = graph_mod(tx, ty)
            (gx,) = torch.autograd.grad(loss, tx)
            outs.append((loss, gx) + tuple(graph_mod.last))
    graph.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, eager[1:]):
        got = dict(zip(("loss", "gx", "d_xy", "i_xy", "d_yx", "i_yx"), (v.detach().cpu().numpy() for v in o)))
        got["gy"] = None
        _same(got, e)


def _loop(dev, fused, seq, n_iter=3):
    from reart_amd import run_robot as rr
    from reart_amd.networks.model import BaseModel
    from reart_amd.synthetic import split_canonical
    from reart_amd.utils.model_utils import tau_cosine
    import functools

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cano, pcs = split_canonical(seq["complete"].astype(np.float32), 2)
    a = rr.build_parser().parse_args(["--model", "base", "--use_flow_loss", "--cano_idx", "2"] + (["--fused_losses"] if fused else []))
    torch.manual_seed(4)
    model = BaseModel(num_parts=a.num_parts, pose_len=pcs.shape[0]).to(dev)
    tau = functools.partial(tau_cosine, max_iter=a.n_iter, end_temp=a.end_tau, start_temp=a.start_tau)
    loop = rr.OperatorLoop(a, model, t(cano), t(pcs), [t(r.astype(np.float32)) for r in seq["ref_loc"]],
                           [t(f.astype(np.float32)) for f in seq["ref_flow"]], tau)
    torch.manual_seed(9)                                         # the Gumbel draws of the model's forward
    rows = []
    for i in range(n_iter):
        losses = loop.iteration(i)
        rows.append({k: float(v.detach()) for k, v in losses.items()})
    params = torch.cat([p.detach().flatten() for p in model.parameters()])
    return loop, rows, params


def test_operator_loop_with_fused_losses(dev):
    """Three iterations of OperatorLoop on a small sequence with --fused_losses and without it.  The batched blend is bit
    for bit the per-frame calls at the loop's shapes.  The Chamfer sums agree to the bound of the loss test -- one ulp
    for the single rounding of the fused sum -- plus one ulp per frame, because the per-point path adds its per-frame
    sums in float32: (1 + frames) ulps of the loss.  In the first iteration both runs hold the same parameters and the same
    Gumbel draws, and the batched blend is bit for bit the per-frame one, so the flow terms are EQUAL there; the total
    is float32(recon + flow), one more rounding: the recon bound plus one ulp of the total.  From the second iteration on
    the parameters may differ by what Adam makes of the last bits of the Chamfer gradients, for which no bound is derived
    here: the flow and total terms of those iterations are printed, not asserted.  Both runs end with finite parameters."""
    from reart_amd.synthetic import make_sequence
    from reart_amd.utils.flow_utils import blend_anchor_motion, blend_anchor_motion_batch

    seq = make_sequence(T=4, n_parts=4, pts_per_part=128, with_flow=True)
    loop_on, rows_on, p_on = _loop(dev, True, seq)
    loop_off, rows_off, p_off = _loop(dev, False, seq)
    assert loop_on.fused_losses and loop_on.ref_batch is not None and not loop_off.fused_losses
    assert torch.isfinite(p_on).all() and torch.isfinite(p_off).all()
    # the blends at the loop's shapes
    with torch.no_grad():
        comp = torch.from_numpy(seq["complete"].astype(np.float32)).to(dev)
        flow, mask = blend_anchor_motion_batch(comp[:-1], *loop_on.ref_batch, loop_on.knn_flow, return_mask=True)
        for b, (q, r, f) in enumerate(zip(comp[:-1], loop_off.pc_ref_list, loop_off.flow_ref_list)):
            fb, mb = blend_anchor_motion(q, r, f, loop_off.knn_flow, return_mask=True)
            assert torch.equal(flow[b], fb) and torch.equal(mask[b], mb)
    frames = seq["complete"].shape[0] - 1
    for i, (on, off) in enumerate(zip(rows_on, rows_off)):
        ulp = float(np.spacing(np.float32(off["recon Loss"])))
        print(f"iteration {i}: recon on {on['recon Loss']!r} off {off['recon Loss']!r} diff/ulp "
              f"{abs(on['recon Loss'] - off['recon Loss']) / ulp:.2f}; flow on {on['flow Loss']!r} off {off['flow Loss']!r}; "
              f"total on {on['total Loss']!r} off {off['total Loss']!r}")
    for i, (on, off) in enumerate(zip(rows_on, rows_off)):
        ulp = float(np.spacing(np.float32(off["recon Loss"])))
        assert abs(on["recon Loss"] - off["recon Loss"]) <= (1 + frames) * ulp, (i, on, off)
    on, off = rows_on[0], rows_off[0]
    assert on["flow Loss"] == off["flow Loss"], (on, off)
    bound = (1 + frames) * float(np.spacing(np.float32(off["recon Loss"]))) + float(np.spacing(np.float32(off["total Loss"])))
    assert abs(on["total Loss"] - off["total Loss"]) <= bound, (on, off)
