"""reart_infonce_forward / reart_infonce_backward (csrc/infonce.hip), networks.loss.DescriptorInfoNCE and
utils.flow_utils.correspondence_targets on the device, against the float64 restatement and inside the derived bounds of
tests/infonce_ref.py on every case of its table (`top` exact on the qualifying rows, `count` exact, unused rows and masked
columns exactly 0), with canaries around every output; every combination of wanted / NULL gradients, an upstream scalar other
than 1, two runs bit for bit, symmetric=True, the limits and validation errors, capture in a graph, and one extractor step
against the torch composition (every parameter gradient within 2e-4 of its largest entry, the project's rule).
``-s`` shows the worst error / bound per case."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import infonce_ref as nr

pytestmark = pytest.mark.gpu

PAD, CANARY = 64, 12345.0


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def restated():
    out = {}
    for c in nr.CASES:
        r = nr.restate(c, g=1.0)
        out[c["name"]] = (r, nr.bounds(c, r))
    return out


class Guarded:
    """A contiguous output between two runs of canary values."""

    def __init__(self, shape, dtype, dev):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float64, device=dev).to(dtype)
        self.view = self.buf[PAD:PAD + n].view(*shape)
        self.n = n

    def intact(self):
        ref = torch.tensor(CANARY, dtype=torch.float64).to(self.buf.dtype).item()
        return bool((self.buf[:PAD] == ref).all()) and bool((self.buf[PAD + self.n:] == ref).all())


def native(c, dev, g=None, want=(True, True), tensors=None):
    """Both entry points on case `c` -> numpy outputs (a gradient that is not wanted: None)."""
    from reart_amd import _lib

    L = _lib.lib()
    B, N1, N2, C = c["B"], c["N1"], c["N2"], c["C"]
    f1, f2, pos = tensors[:3] if tensors else (t(c["f1"], dev), t(c["f2"], dev), t(c["pos"], dev))
    mask = (tensors[3] if tensors else (None if c["mask"] is None else t(c["mask"], dev)))
    o = dict(loss=Guarded((1,), torch.float32, dev), row_loss=Guarded((B, N1), torch.float32, dev), lse=Guarded((B, N1), torch.float32, dev),
             top=Guarded((B, N1), torch.int64, dev), count=Guarded((1,), torch.int64, dev),
             dF1=Guarded((B, N1, C), torch.float32, dev) if want[0] else None,
             dF2=Guarded((B, N2, C), torch.float32, dev) if want[1] else None)
    nbytes = L.reart_infonce_scratch_bytes(B, N1, N2, C)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tau = float(c["tau"])
    rc = L.reart_infonce_forward(_lib.ptr(f1), _lib.ptr(f2), _lib.ptr(pos), _lib.ptr(mask), B, N1, N2, C, tau, _lib.ptr(o["loss"].view),
                                 _lib.ptr(o["row_loss"].view), _lib.ptr(o["lse"].view), _lib.ptr(o["top"].view), _lib.ptr(o["count"].view),
                                 _lib.ptr(ws), ws.numel(), _lib.stream())
    assert rc == 0
    ws.fill_(0xA5)                                    # the backward owes nothing to what the forward left in the workspace
    gt = None if g is None else torch.tensor([g], dtype=torch.float32, device=dev)
    rc = L.reart_infonce_backward(_lib.ptr(f1), _lib.ptr(f2), _lib.ptr(pos), _lib.ptr(mask), _lib.ptr(o["lse"].view), _lib.ptr(o["count"].view),
                                  _lib.ptr(gt), B, N1, N2, C, tau, _lib.ptr(o["dF1"].view) if want[0] else None,
                                  _lib.ptr(o["dF2"].view) if want[1] else None, _lib.ptr(ws), ws.numel(), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    for k, v in o.items():
        assert v is None or v.intact(), f"canary of {k}"
    out = {k: (None if v is None else v.view.cpu().numpy()) for k, v in o.items()}
    out["loss"], out["count"] = out["loss"][0], int(out["count"][0])
    return out


def exact_zeros(c, r, out):
    """Unused rows and masked columns: exactly 0 (and -1), not merely small."""
    u = r["used"]
    assert (out["row_loss"][~u] == 0).all() and (out["lse"][~u] == 0).all() and (out["top"][~u] == -1).all()
    if out.get("dF1") is not None:
        assert (out["dF1"][~u] == 0).all()
    if out.get("dF2") is not None:
        assert (out["dF2"][~r["live"]] == 0).all()
    if r["count"] == 0:
        assert out["loss"] == 0 and out["count"] == 0


@pytest.mark.parametrize("c", nr.CASES, ids=nr.CASE_IDS)
def test_native_calls_inside_the_bounds(c, dev, restated):
    r, b = restated[c["name"]]
    out = native(c, dev)
    w = nr.worst(out, r, b)
    print(c["name"], w)
    assert nr.inside(w), w
    exact_zeros(c, r, out)
    assert np.isfinite(out["loss"])


@pytest.mark.parametrize("c", nr.CASES, ids=nr.CASE_IDS)
def test_class_inside_the_bounds(c, dev, restated):
    from reart_amd.networks.loss import DescriptorInfoNCE

    r, b = restated[c["name"]]
    op = DescriptorInfoNCE(tau=c["tau"])
    f1, f2 = t(c["f1"], dev).requires_grad_(True), t(c["f2"], dev).requires_grad_(True)
    mask = None if c["mask"] is None else t(c["mask"], dev)
    if c["name"].endswith("mask_bool"):
        mask = mask.bool()
    pos = t(c["pos"], dev)
    loss = op(f1, f2, pos, mask)
    assert loss.shape == () and loss.requires_grad
    loss.backward()
    row_loss, top, count = op.last
    out = dict(loss=loss.item(), row_loss=row_loss.cpu().numpy(), top=top.cpu().numpy(), count=int(count), dF1=f1.grad.cpu().numpy(),
               dF2=f2.grad.cpu().numpy())
    w = nr.worst(out, r, b)
    assert nr.inside(w), w
    acc = op.accuracy()
    assert acc.shape == () and acc.is_cuda
    hits = int(((out["top"] == c["pos"]) & r["used"]).sum())
    assert abs(acc.item() - (hits / r["count"] if r["count"] else 0.0)) < 1e-6


WANTS = [(True, True), (True, False), (False, True), (False, False)]


@pytest.mark.parametrize("name", ["n32_m33_c63_unused", "n300_m1000_c64_masked", "many_clouds_unsplit"])
def test_wanted_and_null_gradients_and_an_upstream_scale(name, dev):
    c = next(c for c in nr.CASES if c["name"] == name)
    g = -2.5
    r = nr.restate(c, g=g)
    b = nr.bounds(c, r)
    full = None
    for want in WANTS:
        out = native(c, dev, g=g, want=want)
        w = nr.worst(out, r, b)
        assert nr.inside(w), (want, w)
        exact_zeros(c, r, out)
        if full is None:
            full = out
        for k, on in zip(("dF1", "dF2"), want):                     # a gradient does not depend on whether the other is computed
            assert (out[k] is None) == (not on)
            if on:
                assert out[k].tobytes() == full[k].tobytes()


@pytest.mark.parametrize("name", ["n33_m64_c64", "n129_m257_c256_shared", "huge_logits", "n300_m1000_c64_masked"])
def test_two_runs_agree_in_every_bit(name, dev):
    c = next(c for c in nr.CASES if c["name"] == name)
    a, b = native(c, dev, g=0.75), native(c, dev, g=0.75)
    for k in ("row_loss", "lse", "top", "dF1", "dF2"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.float32(a["loss"]).tobytes() == np.float32(b["loss"]).tobytes() and a["count"] == b["count"]


def test_class_computes_only_what_needs_a_gradient(dev):
    from reart_amd.networks.loss import DescriptorInfoNCE

    c = nr.CASES[3]
    op = DescriptorInfoNCE(tau=c["tau"])
    f1, f2, pos = t(c["f1"], dev), t(c["f2"], dev), t(c["pos"], dev)
    assert not op(f1, f2, pos).requires_grad
    f2r = f2.clone().requires_grad_(True)
    (3.0 * op(f1, f2r, pos)).backward()
    r = nr.restate(c, g=3.0)
    assert nr.inside(nr.worst(dict(dF2=f2r.grad.cpu().numpy()), r, nr.bounds(c, r)))
    # non-contiguous operands are made contiguous
    f1t = t(np.ascontiguousarray(c["f1"].transpose(0, 2, 1)), dev).transpose(1, 2).requires_grad_(True)
    assert not f1t.is_contiguous()
    op(f1t, f2, pos).backward()
    r = nr.restate(c)
    assert nr.inside(nr.worst(dict(dF1=f1t.grad.cpu().numpy()), r, nr.bounds(c, r)))


@pytest.mark.parametrize("name", ["n129_m257_c256_shared", "n300_m1000_c64_masked", "n32_m33_c63_unused"])
def test_symmetric_against_two_restated_calls(name, dev):
    from reart_amd.networks.loss import DescriptorInfoNCE

    c = next(c for c in nr.CASES if c["name"] == name)
    live, used, col = nr.used_rows(c)
    pos_t = np.full((c["B"], c["N2"]), -1, np.int64)                # the lowest used row naming each column
    for bb in range(c["B"]):
        for i in range(c["N1"] - 1, -1, -1):
            if used[bb, i]:
                pos_t[bb, col[bb, i]] = i
    ct = dict(c, N1=c["N2"], N2=c["N1"], f1=c["f2"], f2=c["f1"], pos=pos_t, mask=None)
    ra, rb = nr.restate(c, g=0.5), nr.restate(ct, g=0.5)
    ba, bb_ = nr.bounds(c, ra), nr.bounds(ct, rb)
    op = DescriptorInfoNCE(tau=c["tau"], symmetric=True)
    f1, f2 = t(c["f1"], dev).requires_grad_(True), t(c["f2"], dev).requires_grad_(True)
    loss = op(f1, f2, t(c["pos"], dev), None if c["mask"] is None else t(c["mask"], dev))
    loss.backward()
    ref = 0.5 * (ra["loss"] + rb["loss"])
    assert abs(loss.item() - ref) <= 0.5 * (ba["loss"] + bb_["loss"]) + 2.0 ** -23 * abs(ref)
    for got, x, y, bx, by in ((f1.grad, ra["dF1"], rb["dF2"], ba["dF1"], bb_["dF2"]), (f2.grad, ra["dF2"], rb["dF1"], ba["dF2"], bb_["dF1"])):
        refg = x + y
        err = np.abs(got.cpu().numpy() - refg)
        assert (err <= bx + by + 2.0 ** -23 * np.abs(refg)).all(), float((err - bx - by).max())


def test_limits_and_validation_before_any_launch(dev):
    from reart_amd import _lib
    from reart_amd.networks.loss import DescriptorInfoNCE

    L = _lib.lib()
    for shape in ((1, 8, 8, 257), (1, 65537, 8, 8), (1, 8, 65537, 8), (1025, 8, 8, 8), (1, 8, 8, 0)):
        assert L.reart_infonce_scratch_bytes(*shape) == 0
    f = torch.zeros(1, 8, 8, device=dev)
    pos = torch.zeros(1, 8, dtype=torch.int64, device=dev)
    o = [torch.full((64,), 7.0, device=dev) for _ in range(3)] + [torch.full((64,), 7, dtype=torch.int64, device=dev) for _ in range(2)]
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    p = _lib.ptr

    def fwd(f1=f, B=1, N1=8, N2=8, C=8, tau=1.0, loss=o[0], wsb=ws.numel()):
        return L.reart_infonce_forward(p(f1), p(f), p(pos), None, B, N1, N2, C, tau, p(loss), p(o[1]), p(o[2]), p(o[3]), p(o[4]), p(ws), wsb,
                                       _lib.stream())

    def bwd(C=8, tau=1.0, count=o[4], N1=8, B=1):
        return L.reart_infonce_backward(p(f), p(f), p(pos), None, p(o[2]), p(count), None, B, N1, 8, C, tau, p(o[0]), None, p(ws), ws.numel(),
                                        _lib.stream())

    assert fwd(C=257) == -2 and fwd(N1=65537) == -2 and fwd(N2=65537) == -2 and fwd(B=1025) == -2
    assert bwd(C=257) == -2 and bwd(N1=65537) == -2 and bwd(B=1025) == -2
    assert fwd(tau=0.0) == -1 and fwd(tau=-1.0) == -1 and fwd(tau=float("nan")) == -1 and fwd(f1=None) == -1 and fwd(loss=None) == -1
    assert fwd(C=0) == -1 and fwd(wsb=16) == -1 and bwd(tau=0.0) == -1 and bwd(count=None) == -1
    torch.cuda.synchronize()
    assert all(bool((x == 7).all()) for x in o)                      # nothing was launched
    assert fwd(B=0) == 0 and o[0][0].item() == 0 and o[4][0].item() == 0 and bwd(B=0) == 0
    o[0].fill_(7.0); o[4].fill_(7)
    assert fwd(N1=0) == 0 and o[0][0].item() == 0 and o[4][0].item() == 0
    assert fwd(N2=0) == 0 and o[0][0].item() == 0 and o[4][0].item() == 0 and bool((o[3][:8] == -1).all())
    # the class: the same errors on device tensors, and empty operands
    op = DescriptorInfoNCE()
    with pytest.raises(TypeError):
        op(f.double(), f, pos)
    with pytest.raises(ValueError):
        op(f, f[:, :, :4], pos)
    with pytest.raises(NotImplementedError):
        op(torch.zeros(1, 2, 257, device=dev), torch.zeros(1, 2, 257, device=dev), pos[:, :2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op(f.cpu(), f, pos)
    e = torch.zeros(1, 0, 8, device=dev, requires_grad=True)
    fr = f.clone().requires_grad_(True)
    loss = op(e, fr, pos[:, :0])
    loss.backward()
    assert loss.item() == 0 and bool((fr.grad == 0).all()) and tuple(e.grad.shape) == (1, 0, 8)


def test_capture_in_a_graph_and_replay_with_new_contents(dev):
    from reart_amd.networks.loss import DescriptorInfoNCE

    a = next(c for c in nr.CASES if c["name"] == "n33_m64_c64")
    rng = np.random.default_rng(77)
    b = dict(a, f1=(a["f1"] * 1.5).astype(np.float32), f2=rng.permutation(a["f2"], axis=1), pos=rng.integers(-1, 64, a["pos"].shape).astype(np.int64))
    op = DescriptorInfoNCE(tau=a["tau"])
    f1, f2, pos = t(a["f1"], dev).requires_grad_(True), t(a["f2"], dev).requires_grad_(True), t(a["pos"], dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(op(f1, f2, pos), (f1, f2))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = op(f1, f2, pos)
        d1, d2 = torch.autograd.grad(loss, (f1, f2))
    for c in (b, a):
        with torch.no_grad():
            f1.copy_(t(c["f1"], dev)); f2.copy_(t(c["f2"], dev)); pos.copy_(t(c["pos"], dev))
        graph.replay()
        torch.cuda.synchronize()
        r = nr.restate(c)
        w = nr.worst(dict(loss=loss.item(), dF1=d1.cpu().numpy(), dF2=d2.cpu().numpy(), top=op.last[1].cpu().numpy(), count=int(op.last[2])),
                     r, nr.bounds(c, r))
        assert nr.inside(w), w


def test_correspondence_targets_against_brute_force(dev):
    from reart_amd.utils.flow_utils import correspondence_targets

    rng = np.random.default_rng(5)
    pred = rng.uniform(-0.35, 0.35, (2, 300, 3)).astype(np.float32)
    obs = rng.uniform(-0.35, 0.35, (2, 280, 3)).astype(np.float32)
    d = ((pred.astype(np.float64)[:, :, None, :] - obs.astype(np.float64)[:, None, :, :]) ** 2).sum(3)
    near = d.min(2)
    max_dist = float(np.sqrt(np.median(near)))                       # cuts about half
    got = correspondence_targets(t(pred, dev), t(obs, dev), max_dist).cpu().numpy()
    assert got.dtype == np.int64 and got.shape == (2, 300)
    clear = np.abs(near - max_dist ** 2) > 1e-6 * max_dist ** 2          # away from the threshold by more than float32 round-off
    want = np.where(near > max_dist ** 2, -1, d.argmin(2))
    assert 0.3 < (want == -1).mean() < 0.7
    assert (got[clear] == want[clear]).all()
    kept = got >= 0
    assert (np.take_along_axis(d, np.where(kept, got, 0)[..., None], 2)[..., 0][kept] <= near[kept] * (1 + 1e-5)).all()


def test_one_extractor_step_against_the_torch_composition(dev):
    from reart_amd.networks.feature_extractor import PointNet2Msg2
    from reart_amd.networks.loss import DescriptorInfoNCE
    from reart_amd.synthetic import extractor_state, make_sequence
    from reart_amd.utils.flow_utils import correspondence_targets

    seq = make_sequence(T=20, n_parts=4, pts_per_part=256, seed=4, with_flow=False)
    A, Bc = t(seq["complete"][0:2], dev), t(seq["complete"][1:3], dev)          # B = 2 pairs of N = 1024 points
    net = PointNet2Msg2(64)
    net.load_state_dict(extractor_state(net))
    net = net.to(dev).eval()
    pos = correspondence_targets(A, Bc, 0.02)
    assert 0.2 < (pos >= 0).float().mean().item() <= 1.0
    xyz = torch.cat([A, Bc]).transpose(1, 2).contiguous()
    tau = 0.07

    def step(native):
        net.zero_grad(set_to_none=True)
        desc = F.normalize(net(xyz, grad=True).transpose(1, 2), dim=2)
        f1, f2 = desc[:2], desc[2:]
        if native:
            loss = DescriptorInfoNCE(tau=tau)(f1, f2, pos)
        else:
            logits = torch.bmm(f1, f2.transpose(1, 2)) / tau
            loss = F.cross_entropy(logits.reshape(-1, logits.shape[2]), pos.reshape(-1), ignore_index=-1)
        loss.backward()
        return loss.item(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}

    l1, g1 = step(True)
    l2, g2 = step(False)
    assert abs(l1 - l2) <= 1e-5 * abs(l2)
    assert g1.keys() == g2.keys() and len(g1) > 50
    for k in g1:
        scale = g2[k].abs().max().item()
        assert (g1[k] - g2[k]).abs().max().item() <= 2e-4 * scale, (k, scale)
