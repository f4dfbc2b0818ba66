"""reart_connection_select and reart_connection_term on the device (csrc/connection_term.hip; networks.loss.ConnectionTerm)
against the restatement of tests/connection_term_ref.py (selection exact, value and gradient in float64), the composition
compute_connection_loss(..., ChamferDistance(), k) on the tie-free cases, and the reference's own float32 values
(tests/golden/loss_terms.npz).

Bounds, the project's: value and edge costs within 1e-4 relative, the gradient tensor within GRAD_TOL of its largest reference
entry (tests/structure_loss_ref.py); index tables and `valid` exact.  Shapes: see connection_term_ref.CASES."""
import numpy as np
import pytest
import torch

from tests import connection_term_ref as ctr

pytestmark = pytest.mark.gpu


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run_term(c, dev, weight=1.0, grad=True, upstream=None, kept=False):
    from reart_amd.networks.loss import ConnectionTerm

    term = ConnectionTerm(c["pairs"], k=c["k"], weight=weight, num_parts=c["P"])
    x = t(c["pc"], dev).requires_grad_(grad)
    if kept:
        term.select(t(c["cano"], dev), t(c["seg"], dev))
        loss = term(x)
    else:
        loss = term(t(c["cano"], dev), t(c["seg"], dev), x)
    assert loss.shape == () and loss.requires_grad == grad
    if grad:
        (loss if upstream is None else loss * upstream).backward()
    cost, src, tgt, valid = term.last
    assert valid.dtype == torch.bool and src.dtype == torch.int32 and tuple(src.shape) == (len(c["pairs"]), c["k"])
    return dict(loss=float(loss.detach()), edge_cost=cost.cpu().numpy(), src=src.cpu().numpy(), tgt=tgt.cpu().numpy(),
                valid=valid.cpu().numpy(), grad=x.grad.cpu().numpy() if grad else None,
                bits=loss.detach().cpu().numpy().tobytes())


def same_bits(a, b):
    return a["bits"] == b["bits"] and all(np.array_equal(a[k], b[k]) for k in ("edge_cost", "src", "tgt", "valid")) and \
        (a["grad"] is None or b["grad"] is None or np.array_equal(a["grad"], b["grad"]))


@pytest.mark.parametrize("name", list(ctr.CASES))
def test_connection_term_against_float64(dev, name):
    c, ref = ctr.case(name), ctr.case_ref(name)
    got = run_term(c, dev)
    sp = ctr.compare(got, ref, name)
    print(f"\n[{name}] kernel vs float64: " + "  ".join(f"{k} {v:.1e}" for k, v in sp.items()))
    inv = ~ref["valid"]
    assert not got["edge_cost"][inv].any() and not got["src"][inv].any() and not got["tgt"][inv].any()
    named = np.zeros(c["pc"].shape[1], bool)
    named[got["src"][ref["valid"]].ravel()] = True
    named[got["tgt"][ref["valid"]].ravel()] = True
    assert not got["grad"][:, ~named].any()                                 # zeros wherever no pair arrives
    again = run_term(c, dev)
    assert same_bits(got, again)
    plain = run_term(c, dev, grad=False)                                    # no gradient asked for: the same value
    assert same_bits(got, plain) and plain["grad"] is None


def test_tie_rules_on_the_device(dev):
    c, expect = ctr.tie_case()
    got = run_term(c, dev)
    for key in ("src", "tgt", "valid"):
        assert np.array_equal(got[key], expect[key]), key
    ctr.compare(got, dict(ctr.term(c["pc"], expect["src"], expect["tgt"], expect["valid"], c["k"]), **expect), "ties")
    assert got["edge_cost"][1] == 0.0


def test_selected_distances(dev):
    """sel_dist, which the module does not ask for: the float32 distances of the restatement, bit for bit."""
    from reart_amd import _lib

    c, ref = ctr.case("k10_sizes"), ctr.case_ref("k10_sizes")
    N, E, k = len(c["cano"]), len(c["pairs"]), c["k"]
    src, tgt = (torch.full((E, k), -1, dtype=torch.int32, device=dev) for _ in range(2))
    dist, valid = torch.full((E, k), -1.0, device=dev), torch.full((E,), 7, dtype=torch.uint8, device=dev)
    L = _lib.lib()
    ws = _lib.workspace(L.reart_connection_select_workspace_bytes(N, c["P"], E, k), dev)
    cano, seg, pairs = t(c["cano"], dev), t(c["seg"], dev), t(c["pairs"], dev)
    _lib.check(L.reart_connection_select(_lib.ptr(cano), _lib.ptr(seg), N, c["P"], _lib.ptr(pairs), E, k, _lib.ptr(src),
                                         _lib.ptr(tgt), _lib.ptr(dist), _lib.ptr(valid), _lib.ptr(ws), ws.numel(), _lib.stream()),
               "reart_connection_select")
    assert np.array_equal(dist.cpu().numpy(), ref["dist"]) and np.array_equal(src.cpu().numpy(), ref["src"])
    assert np.array_equal(valid.cpu().numpy().astype(bool), ref["valid"])


@pytest.mark.parametrize("name", [n for n, (_, compose) in ctr.CASES.items() if compose] + ["golden"])
def test_against_the_composition(dev, name):
    from reart_amd.networks.loss import compute_connection_loss
    from reart_amd.utils.chamfer import ChamferDistance

    c = ctr.golden_case()[0] if name == "golden" else ctr.case(name)
    got = run_term(c, dev)
    assert got["valid"].all()
    cano, seg, x = t(c["cano"], dev), t(c["seg"], dev), t(c["pc"], dev).requires_grad_(True)
    cd = ChamferDistance()
    loss = compute_connection_loss(cano, seg, t(c["pairs"], dev), x, cd, k=c["k"])
    loss.backward()
    ref, g = float(loss.detach()), x.grad.cpu().numpy().astype(np.float64)
    lv, top = abs(got["loss"] - ref) / abs(ref), float(np.abs(g).max())
    gv = float(np.abs(got["grad"] - g).max()) / top
    print(f"\n[{name}] kernel vs the composition: loss {lv:.1e}  grad {gv:.1e}")
    assert lv <= ctr.VALUE_TOL and gv <= ctr.GRAD_TOL
    sets = ctr.pair_sets(got["src"], got["tgt"])
    for e, edge in enumerate(c["pairs"]):                                   # the selection itself, as sets per edge
        sm, tm = seg == int(edge[0]), seg == int(edge[1])
        d, nn = cd(cano[sm][None], cano[tm][None], return_index=True)
        _, si = torch.topk(d[0], k=c["k"], largest=False)
        src = torch.where(sm)[0][si].cpu().tolist()
        tgt = torch.where(tm)[0][nn[0][si].long()].cpu().tolist()
        assert sorted(zip(src, tgt)) == sets[e], e


def test_against_the_reference(dev):
    c, g = ctr.golden_case()
    got = run_term(c, dev)
    assert np.array_equal(got["src"], g["src"]) and np.array_equal(got["tgt"], g["tgt"]) and got["valid"].all()
    lv = abs(got["loss"] - float(g["loss"])) / float(g["loss"])
    rows = g["rows"]
    assert not np.delete(got["grad"], rows, axis=1).any()
    gv = float(np.abs(got["grad"][:, rows] - g["grad_rows"]).max()) / float(np.abs(g["grad_rows"]).max())
    print(f"\n[golden] kernel vs the reference's float32: loss {lv:.1e}  grad {gv:.1e}")
    assert lv <= ctr.VALUE_TOL and gv <= ctr.GRAD_TOL
    sp = ctr.compare(got, ctr.connection_term(c["cano"], c["seg"], c["pairs"], c["P"], c["pc"], c["k"]), "golden / float64")
    print("[golden] kernel vs float64: " + "  ".join(f"{k} {v:.1e}" for k, v in sp.items()))


def test_weight_and_upstream_scale(dev):
    c = ctr.case("k10_sizes")
    one = run_term(c, dev)
    w = run_term(c, dev, weight=0.37)
    ctr.compare(w, ctr.case_ref("k10_sizes", 0.37), "weight 0.37")
    assert np.array_equal(w["edge_cost"], one["edge_cost"])                 # the weight is on the sum
    up = run_term(c, dev, upstream=-2.5)
    assert up["bits"] == one["bits"]
    np.testing.assert_array_equal(up["grad"], one["grad"] * np.float32(-2.5))


def test_kept_tables(dev):
    from reart_amd.networks.loss import ConnectionTerm

    c = ctr.case("star_twice_both_self")
    assert same_bits(run_term(c, dev), run_term(c, dev, kept=True))
    term = ConnectionTerm(c["pairs"], k=c["k"], num_parts=c["P"])
    cano, seg, x = t(c["cano"], dev), t(c["seg"], dev), t(c["pc"], dev)
    first = term.select(cano, seg)(x)
    kept = [v.clone() for v in term.last[1:]]
    seg.copy_(torch.roll(seg, 1))                                           # the labels change: ignored until reset()
    assert torch.equal(term(x), first) and all(torch.equal(a, b) for a, b in zip(term.last[1:], kept))
    fresh = term(cano, seg, x)                                              # three arguments: selected anew, kept tables stay
    assert not torch.equal(term.last[1], kept[0]) and not torch.equal(fresh, first)
    assert torch.equal(term(x), first)
    term.reset()
    with pytest.raises(RuntimeError, match="select"):
        term(x)
    assert torch.equal(term.select(cano, seg)(x), fresh)


def test_end_to_end_through_base_model(dev):
    """d ConnectionTerm(model.joint_connection)(cano, seg_part, pc_trans_list) / d proposal_6d, proposal_t of a small BaseModel
    against the float64 chain.  A point moves with the part its noisy arg-max names (here n mod P, forced by the injected
    noise), X[t,n] = R[t,n mod P] x_n + t[t,n mod P]; the pairs are selected on seg_part, the noise-free labels."""
    from reart_amd.networks.loss import ConnectionTerm
    from reart_amd.networks.model import BaseModel
    from tests.relax_grad_ref import rotation_6d_to_matrix

    T, N, P, k = 3, 256, 4, 10
    rng = np.random.default_rng(11)
    model = BaseModel(num_parts=P, pose_len=T).to(dev)
    p6d = (np.tile(np.array([1.0, 0, 0, 0, 1, 0]), (T, P, 1)) + rng.normal(0, 0.2, (T, P, 6))).astype(np.float32)
    pt = rng.normal(0, 0.1, (T, P, 3)).astype(np.float32)
    with torch.no_grad():
        model.proposal_6d.copy_(t(p6d, dev))
        model.proposal_t.copy_(t(pt, dev))
    cano_np = rng.uniform(-0.3, 0.3, (N, 3)).astype(np.float32)
    gumbel = rng.gumbel(size=(N, P)).astype(np.float32)
    gumbel[np.arange(N), np.arange(N) % P] += 50.0                          # the part a point moves with: n mod P
    # a segmentation head whose noise-free labels (seg_part) fill parts 0, 1, 2 with 67, 21, 168 points and leave part 3
    # empty: two valid edges of the chain and one without a target; logits below 10, the two largest 0.015 apart at least
    W1, b1, W2 = rng.normal(0, 3, (128, 3)).astype(np.float32), rng.normal(0, 0.5, 128).astype(np.float32), \
        rng.normal(0, 0.3, (P, 128)).astype(np.float32)
    with torch.no_grad():
        c1, c2 = model.seg_head.model[0], model.seg_head.model[2]
        c1.weight.copy_(t(W1, dev).reshape(c1.weight.shape))
        c1.bias.copy_(t(b1, dev))
        c2.weight.copy_(t(W2, dev).reshape(c2.weight.shape))
    labels = (np.maximum(cano_np.astype(np.float64) @ W1.T + b1, 0) @ W2.T).argmax(1)
    cano = t(cano_np, dev)
    pc, seg, _ = model(cano, tau=1.0, gumbel=t(gumbel, dev))
    assert pc.requires_grad and np.array_equal(seg.cpu().numpy(), labels)
    term = ConnectionTerm(model.joint_connection, k=k, weight=0.5)
    loss = term(cano, seg, pc)
    loss.backward()
    cost, src, tgt, valid = term.last
    sel = ctr.select(cano_np, labels, model.joint_connection.cpu().numpy(), P, k)
    assert sel["valid"].tolist() == [True, True, False] and np.array_equal(valid.cpu().numpy(), sel["valid"])
    assert np.array_equal(src.cpu().numpy(), sel["src"]) and np.array_equal(tgt.cpu().numpy(), sel["tgt"])
    a, b = (torch.as_tensor(v, dtype=torch.float64).requires_grad_(True) for v in (p6d, pt))
    R, x, lab = rotation_6d_to_matrix(a), torch.as_tensor(cano_np, dtype=torch.float64), torch.as_tensor(np.arange(N) % P)
    X = torch.einsum("tnij,nj->tni", R[:, lab], x) + b[:, lab]
    s, g = torch.as_tensor(sel["src"][sel["valid"]]).long(), torch.as_tensor(sel["tgt"][sel["valid"]]).long()
    ref_loss = 0.5 * ((X[:, s] - X[:, g]) ** 2).sum(-1).mean(-1).sum()
    ref_loss.backward()
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= ctr.VALUE_TOL * abs(float(ref_loss.detach()))
    for name, got, ref in (("proposal_6d", model.proposal_6d.grad, a.grad), ("proposal_t", model.proposal_t.grad, b.grad)):
        sp = float((got.cpu().double() - ref).abs().max() / ref.abs().max())
        print(f"\n[end to end] {name}: {sp:.1e}")
        assert sp <= ctr.GRAD_TOL, name
