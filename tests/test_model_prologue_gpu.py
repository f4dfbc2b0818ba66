"""The backward block kernel's tile staging: tiles sized to the workgroup's points, 16-byte loads where the rows are 16-byte
aligned (N and H multiples of 4, aligned base pointers), the dword form otherwise, and a branch-free form for the full chunk
of the template's shape.  Four checks: against the oracle, the 16-byte path against the dword path (the same data at
pointers 4 mod 16), against a run recorded from the commit before (tests/golden/model_prologue_parent.npz, written by
tools/record_model_prologue_golden.py), and in situ in the fused step at the other workgroup geometries and batched."""
import os

import numpy as np
import pytest
import torch

# (N, P, B, H); the C entry runs 32-point workgroups
SHAPES = [(128, 20, 19, 128),   # everything aligned, all chunks full: the fast path
          (100, 20, 19, 128),   # aligned, last chunk of 4
          (44, 10, 2, 48),      # aligned, last chunk of 12
          (64, 32, 19, 128),    # P = 32
          (96, 8, 1, 32),       # a single gW2 tile
          (98, 20, 19, 128),    # N % 4 == 2: rows unaligned, dword form
          (132, 7, 3, 30)]      # H % 4 != 0: W2 rows unaligned, generic P
ALIGNED = [s for s in SHAPES if s[0] % 4 == 0 and s[3] % 4 == 0]
GOLDEN_SHAPES = [(128, 20, 19, 128), (100, 20, 19, 128), (98, 20, 19, 128)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_prologue_parent.npz")
FWD_KEYS = ("out", "yT", "hT", "hard_idx", "seg_part")
GRAD_KEYS = ("gW1", "gb1", "gW2", "g6d", "gt")
TAU = 2.5


def inputs(shape):
    rng = np.random.default_rng(41)
    N, P, B, H = shape
    d = dict(cano=rng.uniform(-0.3, 0.3, (N, 3)), W1=rng.normal(0, 0.5, (H, 3)), b1=rng.normal(0, 0.1, H),
             W2=rng.normal(0, 0.3, (P, H)), p6d=rng.normal(size=(B, P, 6)), pt=rng.normal(0, 0.1, (B, P, 3)),
             noise=-np.log(rng.exponential(size=(N, P))), G=rng.normal(size=(B, N, 3)))
    return {k: v.astype(np.float32) for k, v in d.items()}


def expected_shapes(shape):
    N, P, B, H = shape
    return {"out": (B, N, 3), "yT": (P, N), "hT": (H, N), "hard_idx": (N,), "seg_part": (N,), "gW1": (H, 3), "gb1": (H,),
            "gW2": (P, H), "g6d": (B, P, 6), "gt": (B, P, 3)}


def run_model(shape, d, dev, offset=0):
    """reart_base_forward + reart_base_backward on the device; every tensor (and the workspace) starts `offset` elements
    (4 bytes for the workspace) into its allocation.  Returns the forward outputs and the five gradients as numpy arrays."""
    from reart_amd import _lib

    def alloc(shp, dtype=torch.float32, fill=None):
        n = int(np.prod(shp))
        buf = torch.empty(n + offset, dtype=dtype, device=dev)
        v = buf[offset:].view(*shp)
        if fill is not None:
            v.fill_(fill)
        return v

    def put(a):
        v = alloc(a.shape)
        v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return v

    N, P, B, H = shape
    L = _lib.lib()
    g = {k: put(v) for k, v in d.items()}
    out, seg = alloc((B, N, 3)), alloc((N,), torch.int64)
    trans, yT, hT, hard = alloc((B, P, 4, 4)), alloc((P, N)), alloc((H, N)), alloc((N,), torch.int32)
    for x in list(g.values()) + [out, yT, hT]:
        assert x.data_ptr() % 16 == (4 * offset) % 16
    _lib.check(L.reart_base_forward(_lib.ptr(g["cano"]), N, P, B, _lib.ptr(g["W1"]), _lib.ptr(g["b1"]), _lib.ptr(g["W2"]), H,
                                    _lib.ptr(g["p6d"]), _lib.ptr(g["pt"]), _lib.ptr(g["noise"]), TAU, _lib.ptr(out), _lib.ptr(seg),
                                    _lib.ptr(trans), _lib.ptr(yT), _lib.ptr(hT), _lib.ptr(hard), _lib.stream()), "fwd")
    grads = [alloc(g[k].shape, fill=float("nan")) for k in ("W1", "b1", "W2", "p6d", "pt")]
    nws = L.reart_base_backward_workspace_bytes(N, P, B, H)
    ws = torch.empty(nws + 4 * offset, dtype=torch.uint8, device=dev)[4 * offset:]
    _lib.check(L.reart_base_backward(_lib.ptr(g["cano"]), N, P, B, _lib.ptr(g["W1"]), _lib.ptr(g["b1"]), _lib.ptr(g["W2"]), H,
                                     _lib.ptr(g["p6d"]), _lib.ptr(g["pt"]), _lib.ptr(yT), _lib.ptr(hT), _lib.ptr(hard), TAU,
                                     _lib.ptr(g["G"]), *[_lib.ptr(x) for x in grads], _lib.ptr(ws), ws.numel(), _lib.stream()),
               "bwd")
    torch.cuda.synchronize()
    r = {"out": out, "yT": yT, "hT": hT, "hard_idx": hard, "seg_part": seg}
    r.update(zip(GRAD_KEYS, grads))
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.fixture(scope="module")
def aligned_runs(dev):
    """One run per shape at the allocator's (at least 16-byte) alignment, shared by the checks below."""
    return {s: run_model(s, inputs(s), dev) for s in SHAPES}


def _oracle_backward(oracle, d):
    f = oracle.base_forward(d["cano"], d["W1"], d["b1"], d["W2"], d["p6d"], d["pt"], d["noise"], TAU)
    return f, oracle.base_backward(d["cano"], d["W1"], d["b1"], d["W2"], d["p6d"], d["pt"], f["y_soft"], f["hard_idx"], TAU, d["G"])


def test_listed_shapes_cover_the_cases_and_the_oracle_accepts_them(oracle):
    """CPU side: the list holds the full / short-chunk / unaligned / P / H cases, and the oracle's backward takes each shape
    and returns finite gradients of the right shapes."""
    assert (128, 20, 19, 128) in ALIGNED                                   # all chunks full, the template's shape
    assert {s[0] % 32 for s in ALIGNED} >= {0, 4, 12}                      # last chunks of 4 and 12 points on the 16-byte path
    assert any(s[0] % 4 == 2 for s in SHAPES) and any(s[3] % 4 != 0 and s[0] % 4 == 0 for s in SHAPES)
    assert {s[1] for s in SHAPES} >= {20, 10, 8, 32, 7} and any(s[3] <= 32 for s in SHAPES)
    assert set(GOLDEN_SHAPES) <= set(SHAPES)
    for shape in SHAPES:
        N, P, B, H = shape
        f, ref = _oracle_backward(oracle, inputs(shape))
        assert f["hard_idx"].shape == (N,) and 0 <= f["hard_idx"].min() and f["hard_idx"].max() < P <= 32
        for k in GRAD_KEYS:
            assert ref[k].shape == expected_shapes(shape)[k] and np.isfinite(ref[k]).all() and np.abs(ref[k]).max() > 0, (shape, k)


def test_the_recorded_parent_run_is_complete():
    """CPU side: the fixture holds every output of every recorded shape, finite and of the right shape and type."""
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    assert set(g) == {f"{s[0]}_{k}" for s in GOLDEN_SHAPES for k in FWD_KEYS + GRAD_KEYS}
    for s in GOLDEN_SHAPES:
        for k, shp in expected_shapes(s).items():
            v = g[f"{s[0]}_{k}"]
            assert v.shape == shp, (s, k, v.shape)
            assert v.dtype == {"hard_idx": np.int32, "seg_part": np.int64}.get(k, np.float32), (s, k, v.dtype)
            assert np.isfinite(v).all(), (s, k)
        assert np.abs(g[f"{s[0]}_gW2"]).max() > 0 and len(np.unique(g[f"{s[0]}_hard_idx"])) > 1
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_matches_oracle_and_is_deterministic(oracle, dev, aligned_runs, shape):
    d = inputs(shape)
    f, ref = _oracle_backward(oracle, d)
    a, b = aligned_runs[shape], run_model(shape, d, dev)
    np.testing.assert_array_equal(a["hard_idx"], f["hard_idx"])
    for k in GRAD_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
        err = np.abs(a[k] - ref[k]).max()
        print(f"{shape} {k}: max err {err:.3e} of scale {np.abs(ref[k]).max():.3e}")
        np.testing.assert_allclose(a[k], ref[k], rtol=0, atol=3e-5 * np.abs(ref[k]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ALIGNED)
def test_dword_path_at_offset_pointers_is_bit_equal_to_the_16_byte_path(dev, aligned_runs, shape):
    """The same data with every tensor one float into its allocation: base pointers 4 mod 16, so the kernel takes the
    dword form.  Loads move, arithmetic does not."""
    a, b = aligned_runs[shape], run_model(shape, inputs(shape), dev, offset=1)
    for k in FWD_KEYS + GRAD_KEYS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (shape, k)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", GOLDEN_SHAPES)
def test_reproduces_the_parent_commit_byte_for_byte(aligned_runs, shape):
    with np.load(GOLDEN) as z:
        for k in FWD_KEYS + GRAD_KEYS:
            ref, got = z[f"{shape[0]}_{k}"], aligned_runs[shape][k]
            assert got.dtype == ref.dtype and got.shape == ref.shape, (k, got.dtype, got.shape)
            assert got.tobytes() == ref.tobytes(), (shape, k, int((got.view(np.uint8) != ref.view(np.uint8)).sum()))


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("tuning", [{"tune_bwd_pts": 16}, {"tune_bwd_pts": 32}, {"tune_bwd_pts": 64}, {"tune_fwd_pts": 64}],
                         ids=["bwd16", "bwd32", "bwd64", "fwd64"])
def test_fused_step_geometries_and_batches_match_the_oracle_step(oracle, dev, tuning, K):
    """Three iterations of the fused step at an aligned N (the 16-byte path, with the flow terms added in the G tile), ragged
    flow lengths, every workgroup geometry, K instances in shared launches: every instance against its own oracle iteration."""
    from oracle.step import RelaxOracle
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxBatch, RelaxEngine

    N, P, B, H, cano_idx = 320, 20, 4, 128, 1
    lens = [211, 137, 320, 64]
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
                          n_iter=50, lambda_flow=0.7, use_robust_loss=False, tuning=dict(tuning))
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
