"""The consumers of the searches -- the fused step's (step.hip), ChamferLoss / ChamferPoints (chamfer_loss.hip), FlowTerm
(flow_term.hip), the blend and the flow loss (flow.hip), the kinematic post (kinpost.hip) -- against what the library computed
BEFORE their shared device pieces moved into csrc/consumer_dev.h: every recorded array (losses, parameters after the last
step, gradients, fixed-point bits, .last) must be equal BIT FOR BIT (compared as unsigned integers, so -0 and NaN patterns
count).  tests/golden/consumers_parent.npz is written by tools/record_consumers_golden.py from that earlier library on an
MI355X; this module regenerates the same seeded inputs and reads nothing but that fixture.

The shapes are the smallest that reach every instantiation and edge of the shared code: N = 300 is no multiple of 64, 256 or
1024; the reference sets have 3, 50 and 257 points; P1 = 300 / P2 = 77 give two consumer ranges for x and one for y.  With
brute-force searches N = 300 leaves two partial lists per query (the SL = 4 forms of flow_blend_body / merge_slices) and
N = 1100 eight (the SL = 0 forms, and two target ranges of chamfer_grad_kernel); every pruned search leaves one (SL = 1)."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "consumers_parent.npz")
REF_LENS = (3, 50, 257)
KIN_KEYS = ("cano_pc", "seg_part", "parent", "edge_of_part", "order", "axis", "moment", "theta")   # of the kinematic model


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(x):
    return x.detach().cpu().numpy().copy()


# ---------------------------------------------------------------------------------------------------- the fused step
def _sequence(pts_per_part=75, lens=REF_LENS):
    from reart_amd.synthetic import make_sequence

    seq = make_sequence(T=4, n_parts=4, pts_per_part=pts_per_part, seed=5, n_ref=max(lens), with_flow=True)
    seq["ref_loc"] = [r[:n] for r, n in zip(seq["ref_loc"], lens)]
    seq["ref_flow"] = [f[:n] for f, n in zip(seq["ref_flow"], lens)]
    return seq


def _engine(dev, seq, k=1, flow=True, **kw):
    """B = 3 frame pairs, P = 4 parts, H = 32 hidden units; canonical frame k, the model's weights from seed 10 + k."""
    from reart_amd.networks.blocks import MLPConv1d
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine
    from reart_amd.synthetic import split_canonical

    cano, pcs = split_canonical(seq["complete"], k)
    torch.manual_seed(10 + k)
    model = BaseModel(num_parts=4, pose_len=3)
    model.seg_head = MLPConv1d(3, (32, 4), bn=False, gn=False, last_activation="none")
    model = model.to(dev)
    refs = [t(r, dev) for r in seq["ref_loc"]] if flow else None
    flows = [t(f, dev) for f in seq["ref_flow"]] if flow else None
    kw.setdefault("tuning", {})
    return RelaxEngine(t(cano, dev), t(pcs, dev), model, k, refs, flows, n_iter=200, seed=100 + k, **kw)


def _step_state(eng, tag=""):
    it, log = eng.loss_log()
    out = {tag + "loss_log": _np(log)}
    for name, p in zip(("W1", "b1", "W2", "p6d", "pt"), eng.params):
        out[tag + name] = _np(p)
    return out


def _assign(eng, N):
    rng = np.random.default_rng(7)
    src, tgt = rng.permutation(N)[:128], np.stack([rng.permutation(N)[:128] for _ in range(3)])
    eng.set_assignment(torch.from_numpy(src), torch.from_numpy(tgt), 0.3)


def _step(dev, steps=3, assign=False, pts_per_part=75, lens=REF_LENS, **kw):
    seq = _sequence(pts_per_part, lens)
    eng = _engine(dev, seq, **kw)
    if assign:
        _assign(eng, seq["complete"].shape[1])
    eng.step(steps)
    return _step_state(eng)


def _step_batch(dev):
    from reart_amd.relax import RelaxBatch

    seq = _sequence()
    engines = [_engine(dev, seq, k=k) for k in range(2)]
    RelaxBatch(engines).step(3)
    out = {}
    for k, e in enumerate(engines):
        out.update(_step_state(e, f"k{k}_"))
    return out


# ---------------------------------------------------------------------------------------- ChamferLoss, ChamferPoints
def _clouds(pile_up):
    """x [2,300,3], y [2,77,3]; pile_up: every x picks y[:, 0] (one target takes all 300 addends of the fixed-point sums)."""
    rng = np.random.default_rng(21)
    x = rng.uniform(-0.3, 0.3, (2, 300, 3)).astype(np.float32)
    y = rng.uniform(-0.3, 0.3, (2, 77, 3)).astype(np.float32)
    if pile_up:
        y[:, 1:] += 5.0
        y[:, 0] = 0.0
    return x, y


def _chamfer_loss(dev, pile_up, spatial_sort):
    from reart_amd.utils.chamfer import ChamferLoss

    x, y = _clouds(pile_up)
    x, y = t(x, dev).requires_grad_(), t(y, dev).requires_grad_()
    mod = ChamferLoss(spatial_sort=spatial_sort)
    loss = mod(x, y)
    loss.backward()
    d_xy, i_xy, d_yx, i_yx = mod.last
    return dict(loss=_np(loss), grad_x=_np(x.grad), grad_y=_np(y.grad), fx_bits=_np(mod.fx_bits), d_xy=_np(d_xy), i_xy=_np(i_xy),
                d_yx=_np(d_yx), i_yx=_np(i_yx))


def _chamfer_points(dev, pile_up, directions, use_yx=True):
    from reart_amd.utils.chamfer import ChamferPoints

    x, y = _clouds(pile_up)
    rng = np.random.default_rng(22)
    w = [rng.normal(0, 1, (2, P)).astype(np.float32) * (rng.uniform(0, 1, (2, P)) >= 0.1) for P in (300, 77)]   # a tenth exact zeros
    x, y = t(x, dev).requires_grad_(), t(y, dev).requires_grad_()
    mod = ChamferPoints()
    d_xy, d_yx = mod(x, y, directions=directions)
    total = 0.0
    if d_xy is not None:
        total = total + (d_xy * t(w[0].astype(np.float32), dev)).sum()
    if d_yx is not None and use_yx:            # not used: its upstream arrives as None
        total = total + (d_yx * t(w[1].astype(np.float32), dev)).sum()
    total.backward()
    return dict(grad_x=_np(x.grad), grad_y=_np(y.grad), fx_bits=_np(mod.fx_bits))


# --------------------------------------------------------------------------------------------- FlowTerm and flow.hip
def _flow_inputs(dev):
    from reart_amd.synthetic import split_canonical

    seq = _sequence()
    cano, pcs = split_canonical(seq["complete"], 1)
    return t(cano, dev), t(pcs, dev), [t(r, dev) for r in seq["ref_loc"]], [t(f, dev) for f in seq["ref_flow"]]


def _flow_term(dev, robust, knn_squared):
    from reart_amd.utils.flow_utils import FlowTerm

    cano, pcs, refs, flows = _flow_inputs(dev)
    pcs.requires_grad_()
    mod = FlowTerm(refs, flows, 1, weight=0.7, robust=robust, knn_squared=knn_squared)
    assert mod.serves(pcs, cano)
    loss = mod(pcs, cano)
    loss.backward()
    gt, mask, dists, idx = mod.last
    return dict(loss=_np(loss), grad=_np(pcs.grad), gt_flow=_np(gt), mask=_np(mask).astype(np.uint8), dists=_np(dists), idx=_np(idx))


def _flow_ops(dev, robust):
    from reart_amd.networks.loss import flow_loss
    from reart_amd.utils.flow_utils import _Knn3, blend_anchor_motion_batch, pad_reference_sets

    cano, pcs, refs, flows = _flow_inputs(dev)
    comp = torch.cat((pcs[:1], cano[None], pcs[1:]), dim=0)
    gt, mask = blend_anchor_motion_batch(comp[:-1], *pad_reference_sets(refs, flows), _Knn3(False), return_mask=True)
    pred = (comp[1:] - comp[:-1]).requires_grad_()
    loss = flow_loss(gt, pred, flow_mask_list=mask, robust=robust)
    loss.backward()
    return dict(gt_flow=_np(gt), mask=_np(mask).astype(np.uint8), loss=_np(loss), grad=_np(pred.grad))


# ------------------------------------------------------------------------------------------------------ kinpost.hip
def _kinematic(dev, kin):
    """One KinematicEngine iteration (assignment + flow loss through reart_kin_post) at pose_len 2 over the first 300 points of
    the kinematic model `kin` (the KIN_KEYS arrays; the fixture carries them)."""
    from reart_amd.kinematic_engine import KinematicEngine
    from reart_amd.knn_cuda import KNN
    from reart_amd.networks.model import KinematicModel

    B, N = 2, 300
    cano = t(kin["cano_pc"][:N], dev)
    parent, edge = kin["parent"], kin["edge_of_part"]
    edge_index = {f"{c}_{int(parent[c])}": int(edge[c]) for c in range(len(parent)) if parent[c] >= 0}

    def model():
        return KinematicModel(pose_len=B, seg_part=t(kin["seg_part"][:N], dev), cano_pc=cano, knn=KNN(k=1, transpose_mode=True),
                              edge_index=edge_index, paths_to_base=None, reverse_topo=[int(v) for v in kin["order"]],
                              axis_list=t(kin["axis"], dev), moment_list=t(kin["moment"], dev), theta_list=t(kin["theta"][:B], dev)).to(dev)

    rng = np.random.default_rng(5)
    with torch.no_grad():
        pcs = model()(cano)[0]
    pcs = (pcs + t(rng.normal(0, 0.004, (B, N, 3)).astype(np.float32), dev)).contiguous()
    comp = torch.cat((pcs[:1], cano[None], pcs[1:]), dim=0)
    sel = [torch.from_numpy(rng.permutation(N)[:100 + 7 * f]).to(dev) for f in range(B)]
    refs = [comp[f][s] for f, s in enumerate(sel)]
    flows = [(comp[f + 1][s] - comp[f][s]) * 0.5 for f, s in enumerate(sel)]
    eng = KinematicEngine(model(), cano, pcs, 1, refs, flows, assign_iter=0, assign_gap=1, downsample=2)
    eng.GRAPHS = False
    losses = eng.iteration(0)
    assert eng.lap_fallbacks == 0 and sorted(losses) == ["flow Loss", "opt assignment loss", "total Loss"]
    out = {"G": _np(eng.G)}
    for key, v in losses.items():
        out[key.replace(" ", "_")] = _np(v)
    return out


CASES = {
    # the merged iteration (post_kernel: flow_blend_body<1>, chamfer_grad_body<1>), plain and robust; K = 2 in shared launches
    "step_merged": lambda dev, kin: _step(dev),
    "step_merged_robust": lambda dev, kin: _step(dev, use_robust_loss=True),
    "step_batch": lambda dev, kin: _step_batch(dev),
    # the stand-alone consumers of the pruned searches: chamfer_grad_kernel<1>, flow_blend_kernel<1>, assign_grad_kernel
    "step_chamfer_only": lambda dev, kin: _step(dev, flow=False),
    "step_assign_flow": lambda dev, kin: _step(dev, steps=2, assign=True),
    "step_assign_only": lambda dev, kin: _step(dev, steps=2, assign=True, flow=False),
    # brute-force slices: two partial lists per query at N = 300 (the <4> forms), eight at N = 1100 (the <0> forms); the grids
    "step_brute": lambda dev, kin: _step(dev, tuning={"search_mode": 1}),
    "step_brute_robust": lambda dev, kin: _step(dev, tuning={"search_mode": 1}, use_robust_loss=True),
    "step_brute_1100": lambda dev, kin: _step(dev, pts_per_part=275, lens=(3, 1100, 1100), tuning={"search_mode": 1}),
    "step_grid": lambda dev, kin: _step(dev, use_grid=True),
    "chamfer_loss": lambda dev, kin: _chamfer_loss(dev, False, True),
    "chamfer_loss_unsorted": lambda dev, kin: _chamfer_loss(dev, False, False),
    "chamfer_loss_pile_up": lambda dev, kin: _chamfer_loss(dev, True, True),
    "chamfer_loss_pile_up_unsorted": lambda dev, kin: _chamfer_loss(dev, True, False),
    "chamfer_points": lambda dev, kin: _chamfer_points(dev, False, "both"),
    "chamfer_points_pile_up": lambda dev, kin: _chamfer_points(dev, True, "both"),
    "chamfer_points_xy": lambda dev, kin: _chamfer_points(dev, False, "xy"),
    "chamfer_points_yx_unused": lambda dev, kin: _chamfer_points(dev, False, "both", use_yx=False),
    "flow_term": lambda dev, kin: _flow_term(dev, False, False),
    "flow_term_robust": lambda dev, kin: _flow_term(dev, True, False),
    "flow_term_squared": lambda dev, kin: _flow_term(dev, False, True),
    "flow_term_robust_squared": lambda dev, kin: _flow_term(dev, True, True),
    "flow_ops": lambda dev, kin: _flow_ops(dev, False),
    "flow_ops_robust": lambda dev, kin: _flow_ops(dev, True),
    "kinematic": _kinematic,
}


def bits(a):
    """The array as unsigned integers of its element size (what is compared)."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def fixture():
    return np.load(GOLDEN)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_bits_of_the_parent(case, fixture):
    assert torch.cuda.is_available(), "needs an MI355X: there is no other path to compare"
    got = CASES[case](torch.device("cuda:0"), {k: fixture[f"kin_in__{k}"] for k in KIN_KEYS})
    want = {k[len(case) + 2:]: fixture[k] for k in fixture.files if k.startswith(case + "__")}
    assert sorted(got) == sorted(want) and want
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (case, k)
        same = bits(got[k]) == bits(want[k])
        assert np.array_equal(bits(got[k]), bits(want[k])), f"{case}: {k} differs from the parent in {int((~same).sum())} of {same.size} words"
