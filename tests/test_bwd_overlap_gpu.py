"""The backward block kernel's wave-specialised tail (matrix-core waves: gR|gt and gW2 tiles; VALU waves: hidden gradient, then
gW1 / gb1 of their own rows) and its LDS copy of the yT tile, on the shapes that stress them: every template instance of P
and the generic one, odd P, last chunks of 1 / 15 / 17 / 31 points, H without a whole 32-wide tile or 16-byte rows, B from 1
to 19; the 16- and 64-point workgroup geometries and the batched launch in situ.  Reference: the oracle's backward / step, at
the tolerance and scaling of tests/test_model_gpu.py::test_base_model_ragged_sizes_and_determinism and
tests/test_step_gpu.py::test_fused_step_with_flow_matches_oracle."""
import numpy as np
import pytest
import torch

# (N, P, B, H): N = 32 k + {1, 15, 17, 31} (the C entry runs 32-point workgroups)
SHAPES = [(129, 20, 19, 128), (175, 10, 2, 48), (113, 8, 1, 30), (223, 7, 2, 128), (81, 32, 1, 48), (255, 20, 2, 30),
          (33, 7, 19, 30), (303, 32, 19, 128), (97, 10, 19, 48), (143, 8, 19, 128)]
TAU = 2.5


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _inputs(shape):
    rng = np.random.default_rng(41)
    N, P, B, H = shape
    d = dict(cano=rng.uniform(-0.3, 0.3, (N, 3)), W1=rng.normal(0, 0.5, (H, 3)), b1=rng.normal(0, 0.1, H),
             W2=rng.normal(0, 0.3, (P, H)), p6d=rng.normal(size=(B, P, 6)), pt=rng.normal(0, 0.1, (B, P, 3)),
             noise=-np.log(rng.exponential(size=(N, P))), G=rng.normal(size=(B, N, 3)))
    return {k: v.astype(np.float32) for k, v in d.items()}


def _oracle_backward(oracle, d):
    f = oracle.base_forward(d["cano"], d["W1"], d["b1"], d["W2"], d["p6d"], d["pt"], d["noise"], TAU)
    return f, oracle.base_backward(d["cano"], d["W1"], d["b1"], d["W2"], d["p6d"], d["pt"], f["y_soft"], f["hard_idx"], TAU, d["G"])


def test_listed_shapes_cover_the_cases_and_the_oracle_accepts_them(oracle):
    """CPU side of the collection: the list holds every P / last-chunk / H / B case, and the oracle's backward takes
    each shape and returns finite gradients of the right shapes (so no GPU case compares against nothing)."""
    assert {s[1] for s in SHAPES} == {20, 10, 8, 7, 32}
    assert {s[0] % 32 for s in SHAPES} == {1, 15, 17, 31}
    assert {s[3] for s in SHAPES} == {128, 48, 30}
    assert {s[2] for s in SHAPES} == {1, 2, 19}
    for shape in SHAPES:
        N, P, B, H = shape
        d = _inputs(shape)
        f, ref = _oracle_backward(oracle, d)
        assert f["hard_idx"].shape == (N,) and 0 <= f["hard_idx"].min() and f["hard_idx"].max() < P <= 32
        for k, shp in (("gW1", (H, 3)), ("gb1", (H,)), ("gW2", (P, H)), ("g6d", (B, P, 6)), ("gt", (B, P, 3))):
            assert ref[k].shape == shp and np.isfinite(ref[k]).all() and np.abs(ref[k]).max() > 0, (shape, k)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_matches_oracle_and_is_deterministic(oracle, dev, shape):
    from reart_amd import _lib

    N, P, B, H = shape
    d = _inputs(shape)
    f, ref = _oracle_backward(oracle, d)
    L = _lib.lib()
    g = {k: t(v, dev) for k, v in d.items()}
    out = torch.empty((B, N, 3), device=dev); seg = torch.empty(N, dtype=torch.int64, device=dev)
    trans = torch.empty((B, P, 4, 4), device=dev); yT = torch.empty((P, N), device=dev)
    hT = torch.empty((H, N), device=dev); hard = torch.empty(N, dtype=torch.int32, device=dev)
    _lib.check(L.reart_base_forward(_lib.ptr(g["cano"]), N, P, B, _lib.ptr(g["W1"]), _lib.ptr(g["b1"]), _lib.ptr(g["W2"]), H,
                                    _lib.ptr(g["p6d"]), _lib.ptr(g["pt"]), _lib.ptr(g["noise"]), TAU, _lib.ptr(out), _lib.ptr(seg),
                                    _lib.ptr(trans), _lib.ptr(yT), _lib.ptr(hT), _lib.ptr(hard), _lib.stream()), "fwd")
    np.testing.assert_array_equal(hard.cpu().numpy(), f["hard_idx"])
    runs = []
    for _ in range(2):
        grads = [torch.full_like(g[k], float("nan")) for k in ("W1", "b1", "W2", "p6d", "pt")]
        ws = _lib.workspace(L.reart_base_backward_workspace_bytes(N, P, B, H), dev)
        _lib.check(L.reart_base_backward(_lib.ptr(g["cano"]), N, P, B, _lib.ptr(g["W1"]), _lib.ptr(g["b1"]), _lib.ptr(g["W2"]), H,
                                         _lib.ptr(g["p6d"]), _lib.ptr(g["pt"]), _lib.ptr(yT), _lib.ptr(hT), _lib.ptr(hard), TAU,
                                         _lib.ptr(g["G"]), *[_lib.ptr(x) for x in grads], _lib.ptr(ws), ws.numel(), _lib.stream()),
                   "bwd")
        torch.cuda.synchronize()
        runs.append(grads)
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    for x, k in zip(runs[0], ("gW1", "gb1", "gW2", "g6d", "gt")):
        err = np.abs(x.cpu().numpy() - ref[k]).max()
        print(f"{shape} {k}: max err {err:.3e} of scale {np.abs(ref[k]).max():.3e}")
        np.testing.assert_allclose(x.cpu().numpy(), ref[k], rtol=0, atol=3e-5 * np.abs(ref[k]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("bwd_pts", [16, 64])
def test_other_workgroup_geometries_and_batches_match_the_oracle_step(oracle, dev, bwd_pts, K):
    """tune_bwd_pts 16 / 64 (the C entry above always runs 32) and K instances in shared launches: three iterations of the
    fused step, every instance against its own oracle iteration."""
    from oracle.step import RelaxOracle
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxBatch, RelaxEngine

    N, P, B, H, cano_idx = 300, 20, 4, 128, 1
    lens = [211, 137, 300, 64]
    inst = []
    for k in range(K):
        rng = np.random.default_rng(80 + k)
        cano = rng.uniform(-0.3, 0.3, (N, 3)).astype(np.float32)
        pcs = (cano[None] + rng.normal(0, 0.02, (B, N, 3))).astype(np.float32)
        W1, b1 = rng.normal(0, 0.6, (H, 3)).astype(np.float32), rng.normal(0, 0.1, H).astype(np.float32)
        W2 = rng.normal(0, 0.2, (P, H)).astype(np.float32)
        p6d = (np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), (B, P, 1)) + rng.normal(0, 0.05, (B, P, 6))).astype(np.float32)
        pt = rng.normal(0, 0.01, (B, P, 3)).astype(np.float32)
        refs = [rng.uniform(-0.3, 0.3, (m, 3)).astype(np.float32) for m in lens]
        flows = [rng.normal(0, 0.02, (m, 3)).astype(np.float32) for m in lens]
        orc = RelaxOracle(cano, pcs, W1, b1, W2, p6d, pt, cano_idx, refs, flows, lambda_flow=0.7, robust=False, n_iter=50)
        model = BaseModel(num_parts=P, pose_len=B).to(dev)
        with torch.no_grad():
            model.seg_head.model[0].weight.copy_(t(W1, dev)[:, :, None]); model.seg_head.model[0].bias.copy_(t(b1, dev))
            model.seg_head.model[2].weight.copy_(t(W2, dev)[:, :, None])
            model.proposal_6d.copy_(t(p6d, dev)); model.proposal_t.copy_(t(pt, dev))
        eng = RelaxEngine(t(cano, dev), t(pcs, dev), model, cano_idx, [t(r, dev) for r in refs], [t(f, dev) for f in flows],
                          n_iter=50, lambda_flow=0.7, use_robust_loss=False, tuning={"tune_bwd_pts": bwd_pts})
        inst.append((rng, orc, model, eng))
    batch = RelaxBatch([e for _, _, _, e in inst])
    for i in range(3):
        expect = []
        for rng, orc, model, eng in inst:
            noise = -np.log(rng.exponential(size=(N, P))).astype(np.float32)
            expect.append(orc.step(noise))
            eng.set_gumbel(t(noise, dev))
        batch.step(1)
        torch.cuda.synchronize()
        for ref, (rng, orc, model, eng) in zip(expect, inst):
            row = eng.last_losses().cpu().numpy()
            assert abs(row[0] - ref["recon"]) <= 1e-5 * abs(ref["recon"]), (i, row, ref["recon"])
            assert abs(row[1] - ref["flow"]) <= 1e-5 * abs(ref["flow"]) + 1e-9, (i, row, ref["flow"])
            np.testing.assert_array_equal(eng.seg_part.cpu().numpy(), ref["seg_part"])
            for k, prm in (("p6d", model.proposal_6d), ("pt", model.proposal_t), ("W2", model.seg_head.model[2].weight),
                           ("W1", model.seg_head.model[0].weight), ("b1", model.seg_head.model[0].bias)):
                got = prm.detach().cpu().numpy().reshape(orc.params[k].shape)
                np.testing.assert_allclose(got, orc.params[k], rtol=0, atol=2e-5, err_msg=f"iter {i} param {k}")
