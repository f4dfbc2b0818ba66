"""The finalize kernel with everything it needs from memory requested in front of the partial rows (the bias corrections,
the parameter with its two moments, the 6-vector of the Gram-Schmidt backward).  Row counts nchunk = 1, 5, 33 and 129
(N = 32, 160, 1056, 4097 at the C entry's 32-point workgroups): a lane sums a quarter of the rows, so these cover empty
quarters (1: three of four; 5: one), the scalar tail alone (1, 5), the 8-wide batch with a tail (33: 9 + 9 + 9 + 6) and
the 32-wide batch with a tail (129: 33 + 33 + 33 + 30).  Gradients against oracle.base_backward at the tolerance of
tests/test_bwd_overlap_gpu.py, two runs with equal bits; the Adam half of the kernel in three fused steps against the
oracle's iteration at that file's tolerances."""
import numpy as np
import pytest
import torch

SIZES = [32, 160, 1056, 4097]       # N; nchunk = ceil(N / 32)
P, B, H, TAU = 20, 3, 128, 2.5


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _inputs(N):
    rng = np.random.default_rng(900 + N)
    d = dict(cano=rng.uniform(-0.3, 0.3, (N, 3)), W1=rng.normal(0, 0.5, (H, 3)), b1=rng.normal(0, 0.1, H),
             W2=rng.normal(0, 0.3, (P, H)), p6d=rng.normal(size=(B, P, 6)), pt=rng.normal(0, 0.1, (B, P, 3)),
             noise=-np.log(rng.exponential(size=(N, P))), G=rng.normal(size=(B, N, 3)))
    return {k: v.astype(np.float32) for k, v in d.items()}


_REF = {}


def _reference(oracle, N):
    if N not in _REF:
        d = _inputs(N)
        f = oracle.base_forward(d["cano"], d["W1"], d["b1"], d["W2"], d["p6d"], d["pt"], d["noise"], TAU)
        _REF[N] = (d, f, oracle.base_backward(d["cano"], d["W1"], d["b1"], d["W2"], d["p6d"], d["pt"], f["y_soft"], f["hard_idx"], TAU, d["G"]))
    return _REF[N]


def test_listed_sizes_cover_the_cases_and_the_oracle_accepts_them(oracle):
    quarters = {}
    for N in SIZES:
        n = -(-N // 32)
        rq = (n + 3) // 4
        quarters[n] = [max(0, min(rq, n - q * rq)) for q in range(4)]
    assert sorted(quarters) == [1, 5, 33, 129]
    assert quarters[1] == [1, 0, 0, 0] and quarters[5] == [2, 2, 1, 0]                # empty quarters, scalar tail
    assert quarters[33] == [9, 9, 9, 6]                                              # 8-wide batch + tail, tail alone
    assert quarters[129] == [33, 33, 33, 30]                                         # 32-wide batch + tail, 8-wide batches + tail
    for N in SIZES:
        d, f, ref = _reference(oracle, N)
        for k, shp in (("gW1", (H, 3)), ("gb1", (H,)), ("gW2", (P, H)), ("g6d", (B, P, 6)), ("gt", (B, P, 3))):
            assert ref[k].shape == shp and np.isfinite(ref[k]).all() and np.abs(ref[k]).max() > 0, (N, k)


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_gradients_match_oracle_and_are_deterministic(oracle, dev, N):
    from reart_amd import _lib

    d, f, ref = _reference(oracle, N)
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
        print(f"N {N} {k}: max err {err:.3e} of scale {np.abs(ref[k]).max():.3e}")
        np.testing.assert_allclose(x.cpu().numpy(), ref[k], rtol=0, atol=3e-5 * np.abs(ref[k]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES)
def test_fused_steps_match_the_oracle(oracle, dev, N):
    """The kernel's Adam half (parameter and moments loaded in front of the sums, bias corrections from device memory):
    three fused iterations, Chamfer + flow, against the oracle's iteration, at the same row counts."""
    from oracle.step import RelaxOracle
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine

    Bs, cano_idx = 4, 1
    rng = np.random.default_rng(60 + N)
    cano = rng.uniform(-0.3, 0.3, (N, 3)).astype(np.float32)
    pcs = (cano[None] + rng.normal(0, 0.02, (Bs, N, 3))).astype(np.float32)
    W1, b1 = rng.normal(0, 0.6, (H, 3)).astype(np.float32), rng.normal(0, 0.1, H).astype(np.float32)
    W2 = rng.normal(0, 0.2, (P, H)).astype(np.float32)
    p6d = (np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), (Bs, P, 1)) + rng.normal(0, 0.05, (Bs, P, 6))).astype(np.float32)
    pt = rng.normal(0, 0.01, (Bs, P, 3)).astype(np.float32)
    lens = [211, 137, 300, 64]
    refs = [rng.uniform(-0.3, 0.3, (m, 3)).astype(np.float32) for m in lens]
    flows = [rng.normal(0, 0.02, (m, 3)).astype(np.float32) for m in lens]
    orc = RelaxOracle(cano, pcs, W1, b1, W2, p6d, pt, cano_idx, refs, flows, lambda_flow=0.7, robust=False, n_iter=50)
    model = BaseModel(num_parts=P, pose_len=Bs).to(dev)
    with torch.no_grad():
        model.seg_head.model[0].weight.copy_(t(W1, dev)[:, :, None]); model.seg_head.model[0].bias.copy_(t(b1, dev))
        model.seg_head.model[2].weight.copy_(t(W2, dev)[:, :, None])
        model.proposal_6d.copy_(t(p6d, dev)); model.proposal_t.copy_(t(pt, dev))
    eng = RelaxEngine(t(cano, dev), t(pcs, dev), model, cano_idx, [t(r, dev) for r in refs], [t(f, dev) for f in flows],
                      n_iter=50, lambda_flow=0.7, use_robust_loss=False)
    for i in range(3):
        noise = -np.log(rng.exponential(size=(N, P))).astype(np.float32)
        ref = orc.step(noise)
        eng.set_gumbel(t(noise, dev))
        eng.step()
        row = eng.last_losses().cpu().numpy()
        assert abs(row[0] - ref["recon"]) <= 1e-5 * abs(ref["recon"]), (i, row, ref["recon"])
        assert abs(row[1] - ref["flow"]) <= 1e-5 * abs(ref["flow"]) + 1e-9, (i, row, ref["flow"])
        np.testing.assert_array_equal(eng.seg_part.cpu().numpy(), ref["seg_part"])
        for k, prm in (("p6d", model.proposal_6d), ("pt", model.proposal_t), ("W2", model.seg_head.model[2].weight),
                       ("W1", model.seg_head.model[0].weight), ("b1", model.seg_head.model[0].bias)):
            got = prm.detach().cpu().numpy().reshape(orc.params[k].shape)
            err = np.abs(got - orc.params[k]).max()
            print(f"N {N} iter {i} {k}: max err {err:.3e}")
            np.testing.assert_allclose(got, orc.params[k], rtol=0, atol=2e-5, err_msg=f"iter {i} param {k}")
