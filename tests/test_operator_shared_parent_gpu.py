"""The operators that were written after csrc/consumer_dev.h -- ConnectionTerm (connection_term.hip), the PointNet++ gradients
(pointnet_grad.hip), StructureTerm (structure_term.hip), DescriptorInfoNCE (infonce.hip) -- against what the library computed
BEFORE their inverse-list builder moved into csrc/invlist_dev.h and their block sums, wave fence and lane mask into
csrc/common.h: every recorded array must be equal BIT FOR BIT (compared as unsigned integers, so -0 and NaN patterns count).
tests/golden/operator_shared_parent.npz is written by tools/record_operator_shared_golden.py from that earlier library on an
MI355X; this module regenerates the same seeded inputs and reads nothing but that fixture.

The shapes are the smallest at which the shared code can go wrong.  Connection: N = 40 (one partial tile of 512 points) and
513 (a second tile of one point); R = 2 E k = 2 records (wave 0 alone) and 1152 (more than 1024: every wave takes two steps);
piles (64 lanes on one point in one turn, one point fed from all 16 runs); one invalid edge, an index of -1 and one of N;
T = 1 and 3; with the gradient (the tail of ct_grad_kernel adds the loss) and without (ct_loss_kernel).  Layer backward with
a gather: Npts = 100 and 257 (two tiles of 256), B = 2, Rb = 64 and 300 records per cloud (three of the four runs), all
records on one point, records -1 and Npts.  Interpolation backward: B = 2, N = 90 onto S2 = 5 coarse points (dozens of records
each) and one case of the range table.  Structure: E = 1 and 300 (more than 256: the strided loss sum), T = 1 and 5, with and
without the gradient, the relative-motion form, reart_rel_trans_backward.  InfoNCE: 40 and 257 rows (one and two blocks of
nce_rows_kernel), a column mask that leaves rows unused, every row unused, symmetric and not.

Equal bits pin the ORDER of a point's list only where the sum over the list depends on it: tests/test_operator_shared_cpu.py
(no GPU) adds every pile-up point's contributions in float32 in ascending and in descending record order and demands that the
two differ; the inputs are spread over decades so that they do.  (Where every source AND every target is one point, as in
`*_pile_both`, all contributions are equal and no order shows: those cases pin the counts and offsets, the `_pile_tgt` and
`_pile_src` cases the order.)"""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "operator_shared_parent.npz")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(x):
    return x.detach().cpu().numpy().copy()


def decades(rng, shape, lo=-2.0, hi=2.0):
    """float32 normal values times 10^uniform(lo, hi): sums of a few dozen of them depend on the order."""
    return (rng.normal(size=shape) * 10.0 ** rng.uniform(lo, hi, shape)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------- connection
CONN = {   # name -> (N, E, k, T, pile)
    "conn_n40_r2_t1": (40, 1, 1, 1, None),
    "conn_n40_r1152_t3": (40, 9, 64, 3, None),
    "conn_n513_r1152_t1": (513, 9, 64, 1, None),
    "conn_n513_r1152_t3_pile_both": (513, 9, 64, 3, "both"),
    "conn_n40_r1152_t1_pile_both": (40, 9, 64, 1, "both"),
    "conn_n513_r1152_t3_pile_tgt": (513, 9, 64, 3, "tgt"),
    "conn_n513_r1152_t1_pile_src": (513, 9, 64, 1, "src"),
    "conn_n40_r1152_t3_pile_tgt": (40, 9, 64, 3, "tgt"),
}
CONN_WEIGHT = 0.7


def conn_inputs(name):
    """pc [T,N,3], src / tgt [E,k] int32, valid [E] uint8.  pile: "tgt" every target is point 0, "src" every source is point
    N - 1, "both" both.  Without a pile: edge 1 invalid, one source -1 and one target N (E = 1: everything live)."""
    N, E, k, T, pile = CONN[name]
    rng = np.random.default_rng([31, N, E, k, T])
    pc = decades(rng, (T, N, 3))
    src = rng.integers(0, N, (E, k)).astype(np.int32)
    tgt = rng.integers(0, N, (E, k)).astype(np.int32)
    valid = np.ones(E, np.uint8)
    if pile in ("tgt", "both"):
        tgt[:] = 0
    if pile in ("src", "both"):
        src[:] = N - 1
    if pile is None and E > 1:
        valid[1] = 0
        src[2, 5] = -1
        tgt[3, 7] = N
    return pc, src, tgt, valid


def _connection(dev, name, grad):
    from reart_amd.networks.loss import _connection_term_call

    pc, src, tgt, valid = conn_inputs(name)
    loss, cost, g = _connection_term_call(t(pc, dev), t(src, dev), t(tgt, dev), t(valid, dev), CONN[name][2], CONN_WEIGHT, grad)
    out = dict(loss=_np(loss), edge_cost=_np(cost))
    if grad:
        out["grad"] = _np(g)
    return out


def conn_pile_contributions(name):
    """[(point label, contributions [records, 3 T] float32 in ascending record order)] of the pile-up points: record
    2 (e k + r) + role adds +scale (p[src] - p[tgt]) to its source (role 0) and the negative to its target (role 1)."""
    N, E, k, T, pile = CONN[name]
    pc, src, tgt, valid = conn_inputs(name)
    scale = np.float32(2.0) * np.float32(CONN_WEIGHT) / np.float32(k)
    d = scale * (pc[:, src.reshape(-1)] - pc[:, tgt.reshape(-1)])              # [T, E k, 3], the kernel's float32 expression
    d = np.ascontiguousarray(d.transpose(1, 0, 2)).reshape(E * k, 3 * T)
    out = []
    if pile in ("tgt", "both"):
        out.append(("point 0", -d))
    if pile in ("src", "both"):
        out.append((f"point {N - 1}", d))
    return out


# ------------------------------------------------------------------------------------------------- the layer backward
LAYER = {   # name -> (Npts, S, K, pile)      B = 2, D = 5 feature channels, Rb = S K records per cloud
    "layer_n100_rb64": (100, 8, 8, None),
    "layer_n257_rb300": (257, 20, 15, None),
    "layer_n257_rb300_pile": (257, 20, 15, 256),
    "layer_n100_rb300_pile": (100, 20, 15, 0),
}
LAYER_B, LAYER_D = 2, 5


def layer_inputs(name):
    """idx [B,S,K] int64 (without a pile one record -1 and one Npts per cloud; with one every record names point `pile`),
    F, Q, C, dY [rows, D], and the weight [D + 3, D]: the identity on the feature rows and zeros on the coordinates', so that
    dX's feature columns are dY exactly and a point's contributions are known without a device."""
    Npts, S, K, pile = LAYER[name]
    B, D = LAYER_B, LAYER_D
    rng = np.random.default_rng([32, Npts, S, K])
    idx = rng.integers(0, Npts, (B, S, K)).astype(np.int64)
    if pile is None:
        idx[:, 1, 2] = -1
        idx[:, 3, 1] = Npts
    else:
        idx[:] = pile
    F = rng.normal(size=(B, Npts, D)).astype(np.float32)
    Q = rng.normal(size=(B, Npts, 3)).astype(np.float32)
    C = rng.normal(size=(B, S, 3)).astype(np.float32)
    dY = decades(rng, (B * S * K, D))
    Wt = np.concatenate([np.eye(D), np.zeros((3, D))]).astype(np.float32)
    return idx, F, Q, C, dY, Wt


def _layer(dev, name):
    from reart_amd import _lib

    Npts, S, K, _ = LAYER[name]
    B, D = LAYER_B, LAYER_D
    idx, F, Q, C, dY, Wt = (t(a, dev) for a in layer_inputs(name))
    rows = B * S * K
    A = torch.zeros((rows, D), device=dev)                        # no ReLU, no pooling: dZ = dY, A is not read
    dF = torch.full((B * Npts, D), -7.0, device=dev)
    L = _lib.lib()
    ws = _lib.workspace(L.reart_mlp_layer_backward_scratch_bytes(rows, D + 3, D, B, Npts, D), dev)
    rc = L.reart_mlp_layer_backward(None, 0, _lib.ptr(idx), K, S, Npts, _lib.ptr(F), D, _lib.ptr(Q), _lib.ptr(C), 0, _lib.ptr(Wt), rows,
                                    D + 3, D, 0, 0, _lib.ptr(A), _lib.ptr(dY), D, 0, None, None, None, 0, _lib.ptr(dF), _lib.ptr(ws),
                                    ws.numel(), _lib.stream())
    _lib.check(rc, "reart_mlp_layer_backward")
    return dict(dF=_np(dF))


def layer_pile_contributions(name):
    Npts, S, K, pile = LAYER[name]
    dY = layer_inputs(name)[4]
    return [(f"cloud {b} point {pile}", dY[b * S * K:(b + 1) * S * K]) for b in range(LAYER_B)]


# ---------------------------------------------------------------------------------------------- interpolation backward
INTERP = {"interp_n90_s5": None, "interp_range_case": 3}     # None: B = 2, N = 90, S2 = 5, D = 4; else an index of G.TNN_CASES
INTERP_COL0 = 2


def interp_inputs(name):
    """fine [B,N,3], coarse [B,S2,3], dOut [B N, col0 + D + 1]"""
    i = INTERP[name]
    if i is not None:
        from tests import pointnet_grad_ref as G

        fine, coarse, dOut = G.interp_data(i)
        c = G.TNN_CASES[i]
        return fine.copy(), coarse.copy(), dOut[:, G.INTERP_COL0 - INTERP_COL0:].copy(), c.D     # the table's arrays are read-only
    rng = np.random.default_rng(33)
    fine = rng.uniform(-1, 1, (2, 90, 3)).astype(np.float32)
    coarse = rng.uniform(-0.3, 0.3, (2, 5, 3)).astype(np.float32)     # near the centre: each is among the three nearest of dozens
    return fine, coarse, decades(rng, (2 * 90, INTERP_COL0 + 4 + 1)), 4


def _interp(dev, name):
    from reart_amd import _lib

    fine, coarse, dOut, D = interp_inputs(name)
    (B, N, _), S2 = fine.shape, coarse.shape[1]
    x1, x2, dO = t(fine, dev), t(coarse, dev), t(dOut, dev)
    dP = torch.full((B, S2, D), -7.0, device=dev)
    W = torch.full((B, N, 3), -7.0, device=dev)
    L = _lib.lib()
    ws = _lib.workspace(L.reart_three_interpolate_backward_scratch_bytes(B, N, S2), dev)
    rc = L.reart_three_interpolate_backward(_lib.ptr(x1), _lib.ptr(x2), _lib.ptr(dO), dOut.shape[1], INTERP_COL0, B, N, S2, D, _lib.ptr(dP),
                                            _lib.ptr(W), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "reart_three_interpolate_backward")
    return dict(dpoints2=_np(dP), weights=_np(W))


def interp_pile_contributions(name):
    """Every coarse point of interp_n90_s5 is a pile: record (n, j) adds w[n, j] dOut[n] to coarse point idx[n, j].  The three
    nearest and their weights are restated in float32 numpy (the forward's expression, tests/pointnet_grad_ref.py)."""
    from tests import pointnet_grad_ref as G

    fine, coarse, dOut, D = interp_inputs(name)
    (B, N, _), S2 = fine.shape, coarse.shape[1]
    out = []
    for b in range(B):
        diff = fine[b][:, None, :] - coarse[b][None, :, :]
        d2 = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
        idx = np.argsort(d2, axis=1, kind="stable")[:, :3]
        w = G.interp_weights(np.take_along_axis(d2, idx, axis=1))
        g = dOut[b * N:(b + 1) * N, INTERP_COL0:INTERP_COL0 + D]
        contrib = (w[:, :, None] * g[:, None, :]).reshape(N * 3, D)            # ascending record number 3 n + j
        for s in range(S2):
            out.append((f"cloud {b} coarse point {s}", contrib[idx.reshape(-1) == s]))
    return out


# -------------------------------------------------------------------------------------------------------- structure
def struct_inputs(T, E):
    """trans [T,P,4,4], pairs [E,2] int32: E = 1 two parts; else 12 revolute parts and E random pairs of distinct parts."""
    from tests import structure_loss_ref as slr

    if E == 1:
        c = slr.make_case(T, 2, [(0, 1)], "ir", seed=34)
    else:
        rng = np.random.default_rng([34, T, E])
        a = rng.integers(0, 12, E)
        b = (a + rng.integers(1, 12, E)) % 12
        c = slr.make_case(T, 12, np.stack([a, b], axis=1), "i" + "r" * 11, seed=34)
    return c["trans"], c["pairs"]


def _structure(dev, T, E, grad):
    from reart_amd.networks.loss import _structure_term_call

    trans, pairs = struct_inputs(T, E)
    loss, cost, pris, g = _structure_term_call(t(trans, dev), t(pairs, dev), 0.37, grad)
    out = dict(loss=_np(loss), edge_cost=_np(cost), prismatic=_np(pris))
    if grad:
        out["grad"] = _np(g)
    return out


def _structure_rel(dev):
    """The relative-motion form: the parts' transforms of a case read as the motions of as many edges."""
    from reart_amd.networks.loss import _structure_term_call
    from tests import structure_loss_ref as slr

    rel = slr.make_case(5, 7, [(0, 1)], "rrrrrrr", seed=35)["trans"]
    loss, cost, pris, g = _structure_term_call(t(rel, dev), None, 1.0, True)
    return dict(loss=_np(loss), edge_cost=_np(cost), prismatic=_np(pris), grad=_np(g))


def _rel_trans_backward(dev):
    from reart_amd import _lib

    trans, pairs = struct_inputs(5, 300)
    (T, P), E = trans.shape[:2], len(pairs)
    up = np.random.default_rng(36).normal(size=(T, E, 4, 4)).astype(np.float32)
    tr, pp, g = t(trans, dev), t(pairs, dev), t(up, dev)
    out = torch.full_like(tr, -7.0)
    L = _lib.lib()
    ws = _lib.workspace(L.reart_rel_trans_backward_workspace_bytes(T, P, E), dev)
    _lib.check(L.reart_rel_trans_backward(_lib.ptr(tr), T, P, _lib.ptr(pp), E, _lib.ptr(g), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                          _lib.stream()), "reart_rel_trans_backward")
    return dict(grad_trans=_np(out))


# ---------------------------------------------------------------------------------------------------------- InfoNCE
NCE = {   # name -> (B, N1, N2, C, mask, symmetric)   mask: None, "some" (a third of the columns dead), "all" (every column dead)
    "nce_r40": (2, 20, 33, 12, None, False),
    "nce_r40_masked_sym": (2, 20, 33, 12, "some", True),
    "nce_r257": (1, 257, 70, 5, None, False),
    "nce_r257_masked": (1, 257, 70, 5, "some", False),
    "nce_r257_sym": (1, 257, 70, 5, None, True),
    "nce_r40_unused": (2, 20, 33, 12, "all", False),
    "nce_r257_unused_sym": (1, 257, 70, 5, "all", True),
}
NCE_TAU = 0.5


def nce_inputs(name):
    B, N1, N2, C, mask, _ = NCE[name]
    rng = np.random.default_rng([37, N1, N2, C])
    f1 = rng.normal(size=(B, N1, C)).astype(np.float32)
    f2 = rng.normal(size=(B, N2, C)).astype(np.float32)
    pos = rng.integers(-1, N2 + 1, (B, N1)).astype(np.int64)                   # -1 and N2: rows that are not used
    m = None
    if mask == "some":
        m = (rng.uniform(size=(B, N2)) >= 1.0 / 3.0).astype(np.uint8)
    if mask == "all":
        m = np.zeros((B, N2), np.uint8)
    return f1, f2, pos, m


def _infonce(dev, name):
    from reart_amd.networks.loss import DescriptorInfoNCE, _infonce_backward_call, _infonce_forward_call

    f1, f2, pos, m = (None if a is None else t(a, dev) for a in nce_inputs(name))
    loss, row_loss, lse, top, count = _infonce_forward_call(f1, f2, pos, m, NCE_TAU)
    d1, d2 = _infonce_backward_call(f1, f2, pos, m, lse, count, None, NCE_TAU, True, True)
    out = dict(loss=_np(loss), count=_np(count), row_loss=_np(row_loss), lse=_np(lse), top=_np(top), dF1=_np(d1), dF2=_np(d2))
    if NCE[name][5]:                   # the module's two calls, the second on the transposed problem (N2 rows)
        a, b = f1.clone().requires_grad_(), f2.clone().requires_grad_()
        mod = DescriptorInfoNCE(tau=NCE_TAU, symmetric=True)
        total = mod(a, b, pos, m)
        total.backward()
        out.update(sym_loss=_np(total), sym_dF1=_np(a.grad), sym_dF2=_np(b.grad))
    return out


CASES = {}
for _n in CONN:
    CASES[_n] = lambda dev, n=_n: _connection(dev, n, True)
    CASES[_n + "_nograd"] = lambda dev, n=_n: _connection(dev, n, False)
for _n in LAYER:
    CASES[_n] = lambda dev, n=_n: _layer(dev, n)
for _n in INTERP:
    CASES[_n] = lambda dev, n=_n: _interp(dev, n)
for _T in (1, 5):
    for _E in (1, 300):
        CASES[f"struct_t{_T}_e{_E}"] = lambda dev, T=_T, E=_E: _structure(dev, T, E, True)
        CASES[f"struct_t{_T}_e{_E}_nograd"] = lambda dev, T=_T, E=_E: _structure(dev, T, E, False)
CASES["struct_relative_form"] = _structure_rel
CASES["rel_trans_backward"] = _rel_trans_backward
for _n in NCE:
    CASES[_n] = lambda dev, n=_n: _infonce(dev, n)


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
    got = CASES[case](torch.device("cuda:0"))
    want = {k[len(case) + 2:]: fixture[k] for k in fixture.files if k.startswith(case + "__")}
    assert sorted(got) == sorted(want) and want
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (case, k)
        same = bits(got[k]) == bits(want[k])
        assert np.array_equal(bits(got[k]), bits(want[k])), f"{case}: {k} differs from the parent in {int((~same).sum())} of {same.size} words"
