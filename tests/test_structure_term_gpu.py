"""reart_structure_term and reart_rel_trans_backward on the device (csrc/structure_term.hip; networks.loss.StructureTerm,
structure_loss, compute_connection_loss; utils.graph_utils.compute_relative_trans) against the float64 restatement of
tests/structure_loss_ref.py and the reference's own float32 values (tests/golden/loss_terms.npz).

Bounds, the project's: a value within 1e-4 relative (README, fp32 parity), a gradient tensor within 2e-4 of its largest reference
entry (transform_grad_ref.TOL); tests/test_structure_term_cpu.py holds the float32 restatement against the same bounds.
Shapes: T = 1, 2, 9, 65 (a wave and one frame), 257 (a 256-thread workgroup and one frame), 1024 (the limit); E = 1 (plain mean),
2, 36 = P^2 with the diagonal (self pairs; every part the end of 2 P edges), P = 64; prismatic and revolute edges mixed."""
import numpy as np
import pytest
import torch

from tests import relax_grad_ref as rg
from tests import structure_loss_ref as slr
from tests.structure_loss_ref import GOLD, GOLDEN_CASES, golden_case, golden_ref

pytestmark = pytest.mark.gpu


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run_term(trans, pairs, dev, weight=1.0, grad=True, upstream=None):
    from reart_amd.networks.loss import StructureTerm

    term = StructureTerm(pairs, weight=weight)
    x = t(trans, dev).requires_grad_(grad)
    loss = term(x)
    assert loss.shape == () and loss.requires_grad == grad
    if grad:
        (loss if upstream is None else loss * upstream).backward()
    cost, pris = term.last
    return dict(loss=float(loss.detach()), edge_cost=cost.cpu().numpy(), prismatic=pris.cpu().numpy(),
                grad=x.grad.cpu().numpy() if grad else None, bits=loss.detach().cpu().numpy().tobytes())


@pytest.mark.parametrize("name", list(slr.CASES))
def test_structure_term_against_float64(dev, name):
    c = slr.case(name)
    ref = slr.case_ref(name)
    got = run_term(c["trans"], c["pairs"], dev)
    sp = slr.compare(got, ref, name)
    print(f"\n[{name}] kernel vs float64: " + "  ".join(f"{k} {v:.1e}" for k, v in sp.items()))
    again = run_term(c["trans"], c["pairs"], dev)
    assert got["bits"] == again["bits"] and np.array_equal(got["grad"], again["grad"]) and np.array_equal(got["edge_cost"], again["edge_cost"])
    # no gradient asked for: the same value, no gradient buffer
    plain = run_term(c["trans"], c["pairs"], dev, grad=False)
    assert plain["bits"] == got["bits"] and plain["grad"] is None


@pytest.mark.parametrize("tag", GOLDEN_CASES)
def test_structure_term_against_the_reference(dev, tag):
    trans, pairs, _ = golden_case(tag)
    got = run_term(trans, pairs, dev)
    sp = slr.compare(dict(got, edge_cost=None), golden_ref(tag), tag)
    print(f"\n[{tag}] kernel vs the reference's float32: " + "  ".join(f"{k} {v:.1e}" for k, v in sp.items()))
    slr.compare(got, slr.structure_term(trans, pairs), tag + " / float64")


def test_weight_and_upstream_scale(dev):
    c = slr.case("T9_P10_E9_mixed")
    one = run_term(c["trans"], c["pairs"], dev)
    w = run_term(c["trans"], c["pairs"], dev, weight=0.37)
    slr.compare(w, slr.case_ref("T9_P10_E9_mixed", 0.37), "weight 0.37")
    assert np.array_equal(w["edge_cost"], one["edge_cost"])                      # the weight is on the sum
    up = run_term(c["trans"], c["pairs"], dev, upstream=-2.5)
    assert up["bits"] == one["bits"]
    np.testing.assert_array_equal(up["grad"], one["grad"] * np.float32(-2.5))


def test_empty_edge_list(dev):
    c = slr.case("T2_E2")
    got = run_term(c["trans"], np.zeros((0, 2), np.int32), dev)
    assert got["loss"] == 0.0 and not got["grad"].any() and got["grad"].shape == c["trans"].shape


def test_shapes_beyond_the_limits_name_the_limit(dev):
    from reart_amd.networks.loss import StructureTerm, structure_loss
    from reart_amd.utils.graph_utils import compute_relative_trans

    eye = lambda *s: torch.eye(4, device=dev).repeat(*s, 1, 1)
    with pytest.raises(NotImplementedError, match="1024"):
        StructureTerm([(0, 1)])(eye(1025, 2))
    with pytest.raises(NotImplementedError, match="64"):
        StructureTerm([(0, 64)])(eye(2, 65))
    with pytest.raises(NotImplementedError, match="4096"):
        StructureTerm([(0, 1)] * 4097)(eye(2, 2))
    with pytest.raises(NotImplementedError, match="4096"):
        structure_loss(eye(1, 2, 2), None, None, None, None, torch.zeros((4097, 2), dtype=torch.long))
    with pytest.raises(NotImplementedError, match="64"):
        compute_relative_trans(eye(1, 65).requires_grad_(True), return_trans=True)


def test_relative_motion_form_and_structure_loss(dev):
    """pairs == NULL on `rel` of screw_fit: the pairs form's value in every bit; structure_loss over compute_relative_trans, the
    arguments in the reference's order: StructureTerm's value and, within the bound, its gradient."""
    from reart_amd.networks.loss import _structure_term_call, structure_loss
    from reart_amd.utils.graph_utils import compute_relative_trans, screw_fit

    for name in ("T9_P10_E9_mixed", "E36_all_pairs_P6"):
        c = slr.case(name)
        direct = run_term(c["trans"], c["pairs"], dev)
        rel = screw_fit(t(c["trans"], dev), t(c["pairs"], dev), want=("rel",))["rel"]
        loss, cost, pris, grad = _structure_term_call(rel, None, 1.0, True)
        assert loss.cpu().numpy().tobytes() == direct["bits"]
        assert np.array_equal(cost.cpu().numpy(), direct["edge_cost"]) and np.array_equal(pris.bool().cpu().numpy(), direct["prismatic"])
        assert not grad[:, :, 3].any()
        ref_rel = slr.structure_term(rel.cpu().numpy(), None)
        slr.compare(dict(loss=float(loss), grad=grad.cpu().numpy()), ref_rel, name + " relative form")

        tl = t(c["trans"], dev).requires_grad_(True)
        axis, moment, theta, distance, rel5 = compute_relative_trans(tl, return_trans=True)
        assert rel5.grad_fn is not None and not any(v.requires_grad for v in (axis, moment, theta, distance))
        out = structure_loss(rel5, axis, moment, theta, distance, t(c["pairs"], dev).long())
        assert out.detach().cpu().numpy().tobytes() == direct["bits"]
        out.backward()
        slr.compare(dict(loss=float(out.detach()), grad=tl.grad.cpu().numpy()), slr.case_ref(name), name + " structure_loss")


def test_compute_relative_trans_without_grad_is_unchanged(dev):
    from reart_amd.utils.graph_utils import compute_relative_trans, screw_fit

    c = slr.case("E36_all_pairs_P6")
    tl = t(c["trans"], dev)
    T, P = tl.shape[:2]
    ar = torch.arange(P, device=dev)
    f = screw_fit(tl, torch.stack([ar.repeat_interleave(P), ar.repeat(P)], dim=1), want=("screw", "rel"))
    for x in (tl, tl.clone().requires_grad_(True)):
        axis, moment, theta, distance, rel = compute_relative_trans(x, return_trans=True)
        assert torch.equal(rel, f["rel"].reshape(T, P, P, 4, 4)) and (rel.grad_fn is not None) == x.requires_grad
        s = f["screw"].reshape(T, P, P, 8)
        assert torch.equal(axis, s[..., :3]) and torch.equal(moment, s[..., 3:6]) and torch.equal(theta, s[..., 6]) and torch.equal(distance, s[..., 7])
    assert len(compute_relative_trans(tl)) == 4


@pytest.mark.parametrize("name", ("T9_P10_E9_mixed", "E36_all_pairs_P6", "T257_E3", "P64_E5"))
def test_rel_trans_backward(dev, name):
    from reart_amd import _lib

    c = slr.case(name)
    T, P = c["trans"].shape[:2]
    E = len(c["pairs"])
    up = np.random.default_rng(17).normal(size=(T, E, 4, 4)).astype(np.float32)          # row 3 non-zero: ignored
    ref = slr.rel_trans_backward(c["trans"], c["pairs"], up)
    L = _lib.lib()
    tr, pp, g = t(c["trans"], dev), t(c["pairs"], dev), t(up, dev)
    outs = []
    for _ in range(2):
        out = torch.full_like(tr, float("nan"))
        ws = _lib.workspace(L.reart_rel_trans_backward_workspace_bytes(T, P, E), tr.device)
        _lib.check(L.reart_rel_trans_backward(_lib.ptr(tr), T, P, _lib.ptr(pp), E, _lib.ptr(g), _lib.ptr(out), _lib.ptr(ws),
                                              ws.numel(), _lib.stream()), "reart_rel_trans_backward")
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and not outs[0][:, :, 3].any()
    sp = float(np.abs(outs[0] - ref).max() / np.abs(ref).max())
    print(f"\n[{name}] rel backward vs float64: {sp:.1e}")
    assert sp <= slr.GRAD_TOL


def test_end_to_end_through_base_model(dev):
    """d StructureTerm(edges)(model(cano)[2]) / d proposal_6d, proposal_t of a small BaseModel against the float64 chain."""
    from reart_amd.networks.loss import StructureTerm
    from reart_amd.networks.model import BaseModel

    T, N, P = 5, 64, 4
    edges = np.array([(0, 1), (1, 2), (3, 2)], np.int32)
    c = slr.make_case(T, P, edges, "irrp", seed=1)
    rng = np.random.default_rng(3)
    p6d = np.ascontiguousarray(c["trans"][:, :, :2, :3].reshape(T, P, 6))
    pt = np.ascontiguousarray(c["trans"][:, :, :3, 3])
    model = BaseModel(num_parts=P, pose_len=T).to(dev)
    with torch.no_grad():
        model.proposal_6d.copy_(t(p6d, dev))
        model.proposal_t.copy_(t(pt, dev))
    cano = t(rng.uniform(-0.3, 0.3, (N, 3)).astype(np.float32), dev)
    trans = model(cano, tau=1.0)[2]
    assert trans.requires_grad
    loss = StructureTerm(edges, weight=0.5)(trans)
    loss.backward()
    trans_np = trans.detach().cpu().numpy()
    slr.assert_clear_of_thresholds(trans_np, edges)
    a, b = (torch.as_tensor(v, dtype=torch.float64).requires_grad_(True) for v in (p6d, pt))
    top = torch.cat([rg.rotation_6d_to_matrix(a), b[..., None]], -1)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64).expand(T, P, 1, 4)
    ref_loss, _, _ = slr.term_of(torch.cat([top, bottom], -2), edges, 0.5, slr.decisions(trans_np, edges))
    ref_loss.backward()
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= slr.VALUE_TOL * abs(float(ref_loss.detach()))
    for name, got, ref in (("proposal_6d", model.proposal_6d.grad, a.grad), ("proposal_t", model.proposal_t.grad, b.grad)):
        sp = float((got.cpu().double() - ref).abs().max() / ref.abs().max())
        print(f"\n[end to end] {name}: {sp:.1e}")
        assert sp <= slr.GRAD_TOL, name


def test_compute_connection_loss_against_the_reference(dev):
    import os

    from reart_amd.networks.loss import compute_connection_loss
    from reart_amd.utils.chamfer import ChamferDistance

    z, g = np.load(os.path.join(GOLD, "structure.npz")), np.load(os.path.join(GOLD, "loss_terms.npz"))
    cano, seg, conn = t(z["cano"], dev), t(z["new_seg"], dev), t(z["new_conn"], dev)
    pred = t(z["pred"], dev).requires_grad_(True)
    cd = ChamferDistance()
    loss = compute_connection_loss(cano, seg, conn, pred, cd, k=int(g["conn_k"]))
    loss.backward()
    assert abs(float(loss.detach()) - float(g["conn_loss"])) <= slr.VALUE_TOL * float(g["conn_loss"])
    grad = pred.grad.cpu().numpy()
    rows = g["conn_rows"]
    assert not np.delete(grad, rows, axis=1).any()                                # the selected pairs, and only they
    top = float(np.abs(g["conn_grad_rows"]).max())
    assert np.abs(grad[:, rows] - g["conn_grad_rows"]).max() <= slr.GRAD_TOL * top
    for e, edge in enumerate(conn):                                               # the selection itself, as sets per edge
        sm, tm = seg == edge[0], seg == edge[1]
        d, nn = cd(cano[sm][None], cano[tm][None], return_index=True)
        _, si = torch.topk(d[0], k=int(g["conn_k"]), largest=False)
        src = torch.where(sm)[0][si].cpu().numpy()
        tgt = torch.where(tm)[0][nn[0][si].long()].cpu().numpy()
        order = np.argsort(src)
        ref_order = np.argsort(g["conn_src"][e])
        assert np.array_equal(src[order], g["conn_src"][e][ref_order]) and np.array_equal(tgt[order], g["conn_tgt"][e][ref_order]), e
