"""The forward kernel's prologue -- the first batch of loads of every group (pose entries, W1|b1 words, a W2 column per
thread) and the guarded loops behind it -- at every block size the kernel is instantiated with: the C entry runs the
32-point workgroups, the fused engine's tune_fwd_pts both geometries.  Shapes (N, P, B, H): B P and 4 H below one block,
between one and two, and beyond two blocks of their instantiation (so the first batch alone, one further turn and several
turns of each loop run), a last workgroup of 1 point, an H without 16-byte rows.  Reference: oracle.base_forward at the
tolerances of tests/test_model_gpu.py::test_base_model_ragged_sizes_and_determinism (labels exact).  (Written with a
one-batch prologue that was measured and dropped; the shapes hold for any layout of these loads.)"""
import numpy as np
import pytest
import torch

# block sizes (32-point | 64-point workgroups): P = 20: 320 | 640, 10: 192 | 320, 8: 128 | 256, other: 512 | 1024
SHAPES = [(33, 8, 40, 30), (65, 20, 19, 128), (97, 32, 19, 48), (129, 10, 58, 128), (31, 7, 1, 30)]
TAU = 2.5


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _block(P, pts):
    pmax = P if P in (20, 10, 8) else 32
    return 64 * ((pmax + 3) // 4 if pts == 32 else (pmax + 1) // 2)


def _inputs(shape):
    rng = np.random.default_rng(17)
    N, P, B, H = shape
    d = dict(cano=rng.uniform(-0.3, 0.3, (N, 3)), W1=rng.normal(0, 0.5, (H, 3)), b1=rng.normal(0, 0.1, H),
             W2=rng.normal(0, 0.3, (P, H)), p6d=rng.normal(size=(B, P, 6)), pt=rng.normal(0, 0.1, (B, P, 3)),
             noise=-np.log(rng.exponential(size=(N, P))))
    return {k: v.astype(np.float32) for k, v in d.items()}


_REF = {}


def _reference(oracle, shape):
    if shape not in _REF:
        d = _inputs(shape)
        _REF[shape] = (d, oracle.base_forward(d["cano"], d["W1"], d["b1"], d["W2"], d["p6d"], d["pt"], d["noise"], TAU))
    return _REF[shape]


def test_listed_shapes_cover_the_cases_and_the_oracle_accepts_them(oracle):
    """CPU side of the collection: over the list and both geometries B P and 4 H each fall below one block, between one and
    two and beyond two; a last workgroup of one point and an H without 16-byte rows are there; the oracle takes every shape."""
    pose, words = set(), set()
    for N, P, B, H in SHAPES:
        for pts in (32, 64):
            bs = _block(P, pts)
            pose.add(min((B * P - 1) // bs, 2))
            words.add(min((4 * H - 1) // bs, 2))
    assert pose == {0, 1, 2} and words == {0, 1, 2}
    assert any(N % 32 == 1 for N, _, _, _ in SHAPES) and any(H % 4 for _, _, _, H in SHAPES)
    assert {P for _, P, _, _ in SHAPES} == {8, 20, 32, 10, 7}
    for shape in SHAPES:
        N, P, B, H = shape
        d, f = _reference(oracle, shape)
        assert f["out"].shape == (B, N, 3) and np.isfinite(f["out"]).all()
        assert f["y_soft"].shape == (N, P) and np.isfinite(f["y_soft"]).all()
        assert f["trans_list"].shape == (B, P, 4, 4) and np.isfinite(f["trans_list"]).all()
        assert f["hard_idx"].shape == (N,) and 0 <= f["hard_idx"].min() and f["hard_idx"].max() < P
        assert f["seg_part"].shape == (N,) and 0 <= f["seg_part"].min() and f["seg_part"].max() < P


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_entry_matches_oracle(oracle, dev, shape):
    from reart_amd import _lib

    N, P, B, H = shape
    d, f = _reference(oracle, shape)
    L = _lib.lib()
    g = {k: t(v, dev) for k, v in d.items()}
    out = torch.full((B, N, 3), float("nan"), device=dev); seg = torch.full((N,), -1, dtype=torch.int64, device=dev)
    trans = torch.full((B, P, 4, 4), float("nan"), device=dev); yT = torch.full((P, N), float("nan"), device=dev)
    hT = torch.full((H, N), float("nan"), device=dev); hard = torch.full((N,), -1, dtype=torch.int32, device=dev)
    _lib.check(L.reart_base_forward(_lib.ptr(g["cano"]), N, P, B, _lib.ptr(g["W1"]), _lib.ptr(g["b1"]), _lib.ptr(g["W2"]), H,
                                    _lib.ptr(g["p6d"]), _lib.ptr(g["pt"]), _lib.ptr(g["noise"]), TAU, _lib.ptr(out), _lib.ptr(seg),
                                    _lib.ptr(trans), _lib.ptr(yT), _lib.ptr(hT), _lib.ptr(hard), _lib.stream()), "fwd")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(hard.cpu().numpy(), f["hard_idx"])
    np.testing.assert_array_equal(seg.cpu().numpy(), f["seg_part"])
    for name, got, ref in (("y", yT.cpu().numpy().T, f["y_soft"]), ("out", out.cpu().numpy(), f["out"]),
                           ("trans", trans.cpu().numpy(), f["trans_list"])):
        print(f"{shape} {name}: max abs err {np.abs(got - ref).max():.3e}")
    np.testing.assert_allclose(yT.cpu().numpy().T, f["y_soft"], rtol=2e-6, atol=1e-9)
    np.testing.assert_allclose(out.cpu().numpy(), f["out"], rtol=0, atol=5e-7)
    np.testing.assert_allclose(trans.cpu().numpy(), f["trans_list"], rtol=0, atol=5e-7)
    # the hidden layer: relu(W1 x + b1), the kernel's own operation order in float64 is within a few ulp of it
    h = np.maximum(d["cano"].astype(np.float64) @ d["W1"].astype(np.float64).T + d["b1"], 0.0)
    np.testing.assert_allclose(hT.cpu().numpy().T, h, rtol=2e-6, atol=5e-7)


@pytest.mark.gpu
@pytest.mark.parametrize("pts", [32, 64])
@pytest.mark.parametrize("shape", SHAPES)
def test_engine_forward_matches_oracle(oracle, dev, shape, pts):
    """The same forward through the fused engine (in-situ arguments: temperature from device memory, the SoA copy and the
    boxes for the searches, block 0 publishing the pose table) with 32- and 64-point workgroups."""
    from reart_amd.networks.blocks import MLPConv1d
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine

    N, P, B, H = shape
    d, f = _reference(oracle, shape)
    model = BaseModel(num_parts=P, pose_len=B)
    model.seg_head = MLPConv1d(3, (H, P))            # the seg head at this shape's hidden width (BaseModel builds 128)
    model = model.to(dev)
    with torch.no_grad():
        model.seg_head.model[0].weight.copy_(t(d["W1"], dev)[:, :, None]); model.seg_head.model[0].bias.copy_(t(d["b1"], dev))
        model.seg_head.model[2].weight.copy_(t(d["W2"], dev)[:, :, None])
        model.proposal_6d.copy_(t(d["p6d"], dev)); model.proposal_t.copy_(t(d["pt"], dev))
    pcs = np.repeat(d["cano"][None], B, 0)
    eng = RelaxEngine(t(d["cano"], dev), t(pcs, dev), model, 0, n_iter=50, fixed_tau=TAU, tuning={"tune_fwd_pts": pts})
    eng.set_gumbel(t(d["noise"], dev))
    eng.peek_forward()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(eng.seg_part.cpu().numpy(), f["seg_part"])
    print(f"{shape} pts {pts}: out max abs err {np.abs(eng.pc_trans.cpu().numpy() - f['out']).max():.3e}")
    np.testing.assert_allclose(eng.pc_trans.cpu().numpy(), f["out"], rtol=0, atol=5e-7)     # a wrong hard index moves a point by far more
    np.testing.assert_allclose(eng.trans_list.cpu().numpy(), f["trans_list"], rtol=0, atol=5e-7)
