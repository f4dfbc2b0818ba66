"""GPU: the float32 D = 3 register-list K-nearest search of csrc/knn.hip (knn_slice_kernel<KK, FINAL>, knn_merge_kernel<KK>,
KK in {1, 2, 3, 4, 8, 16}) and its backward (knn_bwd_kernel<3>) at every K = 1 ... 16, every slice count S = 1 ... 16, ragged
lengths and exact workspaces, on the case table of tests/knn_ref.py (checked on the CPU by tests/test_knn_ref_cpu.py).
Every forward comparison is bit-exact against the C oracle; the zero fill for K > P2 and K > lengths2 is part of it."""
import functools

import numpy as np
import pytest
import torch

from tests import knn_ref as R

pytestmark = pytest.mark.gpu

CANARY, FILL = 64 << 10, 0xA5
INVALID_ARG = -1


def _t(a, dev):
    return None if a is None else torch.tensor(a, device=dev)       # a copy: the table's arrays are read-only


_truth, _gpu16 = {}, {}


def _oracle_knn(oracle, c, K):
    key = (c["name"], K)
    if key not in _truth:
        _truth[key] = oracle.knn_points(c["p1"], c["p2"], c["lengths1"], c["lengths2"], K=K)
    return _truth[key]


def _gpu_knn(c, K, dev):
    from reart_amd.utils.chamfer import knn_points

    out = knn_points(_t(c["p1"], dev), _t(c["p2"], dev), lengths1=_t(c["lengths1"], dev), lengths2=_t(c["lengths2"], dev), K=K)
    assert out.idx.dtype == torch.int64 and out.dists.dtype == torch.float32
    assert tuple(out.idx.shape) == tuple(out.dists.shape) == c["p1"].shape[:2] + (K,)
    return out.dists.cpu().numpy(), out.idx.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("K", R.ALL_K)
def test_register_search_matches_the_contract(oracle, dev, K):
    cases = R.cases_for(K)
    assert len(cases) >= len(R.SMALL)
    for c in cases:
        what = f"{c['name']} K={K}"
        d_ref, i_ref = _oracle_knn(oracle, c, K)
        d, i = _gpu_knn(c, K, dev)
        np.testing.assert_array_equal(i, i_ref, err_msg=what)
        np.testing.assert_array_equal(_bits(d), _bits(d_ref), err_msg=what)
        # the six instantiations agree: the first K columns of the 16-column result, wherever slot k < lengths2
        if c["name"] not in _gpu16:
            _gpu16[c["name"]] = _gpu_knn(c, 16, dev)
        d16, i16 = _gpu16[c["name"]]
        n2 = c["lengths2"] if c["lengths2"] is not None else np.full(len(c["p1"]), c["p2"].shape[1])
        live = np.arange(K)[None, None, :] < np.asarray(n2)[:, None, None]
        live = np.broadcast_to(live, d.shape)
        assert live.any()
        np.testing.assert_array_equal(i16[..., :K][live], i[live], err_msg=what)
        np.testing.assert_array_equal(_bits(d16[..., :K])[live], _bits(d)[live], err_msg=what)


# ---- exact workspaces -----------------------------------------------------------------------------------------------------
class _Guarded:
    """`nbytes` bytes in the middle of a larger 0xA5-filled uint8 tensor, 64 KiB of canary on each side."""

    def __init__(self, nbytes, dev):
        self.n = int(nbytes)
        self.buf = torch.full((2 * CANARY + self.n,), FILL, dtype=torch.uint8, device=dev)
        self.mid = self.buf[CANARY:CANARY + self.n]

    def view(self, dtype, shape):
        return self.mid.view(dtype).view(shape)

    def canaries_intact(self):
        return bool((self.buf[:CANARY] == FILL).all()) and bool((self.buf[CANARY + self.n:] == FILL).all())

    def untouched(self):
        return bool((self.buf == FILL).all())

    def refill(self):
        self.buf.fill_(FILL)


@pytest.mark.parametrize("K", [1, 2, 3, 5, 8, 9, 16])
def test_workspace_queries_are_sufficient(oracle, dev, K):
    from reart_amd import _lib

    L = _lib.lib()
    for name in ("s1_last", "s16_first", "empty_slice", "ragged"):
        c = R.make_case(name)
        N, P1, P2 = c["p1"].shape[0], c["p1"].shape[1], c["p2"].shape[1]
        p1, p2, l1, l2 = (_t(c[k], dev) for k in ("p1", "p2", "lengths1", "lengths2"))
        nbytes = L.reart_knn_points_workspace_bytes(N, P1, P2, K)
        assert nbytes == R.plan_workspace_bytes(N, P1, P2, K) > 0
        ws, gd, gi = _Guarded(nbytes, dev), _Guarded(4 * N * P1 * K, dev), _Guarded(8 * N * P1 * K, dev)
        dists, idx = gd.view(torch.float32, (N, P1, K)), gi.view(torch.int64, (N, P1, K))

        def forward(entry, size):
            if entry == "points":
                return L.reart_knn_points_idx(_lib.ptr(p1), _lib.ptr(p2), _lib.ptr(l1), _lib.ptr(l2), N, P1, P2, 3, K,
                                              _lib.ptr(dists), _lib.ptr(idx), _lib.ptr(ws.mid), size, _lib.stream())
            return L.reart_knn_cuda(_lib.ptr(p2), _lib.ptr(p1), N, P2, P1, 3, K, 1, _lib.ptr(dists), _lib.ptr(idx),
                                    _lib.ptr(ws.mid), size, _lib.stream())

        for entry in ("points", "cuda"):
            what = f"{name} K={K} {entry}"
            for g in (ws, gd, gi):
                g.refill()
            # one byte less: refused before anything is launched
            assert forward(entry, nbytes - 1) == INVALID_ARG, what
            torch.cuda.synchronize()
            assert ws.untouched() and gd.untouched() and gi.untouched(), what
            assert forward(entry, nbytes) == 0, what
            torch.cuda.synchronize()
            assert ws.canaries_intact() and gd.canaries_intact() and gi.canaries_intact(), what
            if entry == "points":
                d_ref, i_ref = _oracle_knn(oracle, c, K)
                np.testing.assert_array_equal(_bits(dists.cpu().numpy()), _bits(d_ref), err_msg=what)
            else:       # no lengths at this boundary; K <= P2 in all four cases
                d_ref, i_ref = oracle.knn_cuda(c["p2"], c["p1"], K, euclidean=True)
                np.testing.assert_allclose(dists.cpu().numpy(), d_ref, rtol=2e-7, atol=0, err_msg=what)
            np.testing.assert_array_equal(idx.cpu().numpy(), i_ref, err_msg=what)

        # backward, with the forward's own indices (the ragged ones)
        d_ref, i_ref = _oracle_knn(oracle, c, K)
        assert forward("points", nbytes) == 0
        grad = np.random.default_rng(K).normal(size=d_ref.shape).astype(np.float32)
        g1_ref, g2_ref = oracle.knn_points_backward(c["p1"], c["p2"], i_ref, grad, c["lengths1"], c["lengths2"])
        bbytes = L.reart_knn_points_backward_workspace_bytes(N, P1, P2, K)
        assert bbytes == 4 * N * (2 * P2 + 2 * P1 * K)
        bws, o1, o2 = _Guarded(bbytes, dev), _Guarded(12 * N * P1, dev), _Guarded(12 * N * P2, dev)
        g1, g2 = o1.view(torch.float32, (N, P1, 3)), o2.view(torch.float32, (N, P2, 3))
        gt = _t(grad, dev)
        idx_own = idx.clone()

        def backward(size):
            return L.reart_knn_points_backward(_lib.ptr(p1), _lib.ptr(p2), _lib.ptr(l1), _lib.ptr(l2), _lib.ptr(idx_own),
                                               _lib.ptr(gt), N, P1, P2, 3, K, _lib.ptr(g1), _lib.ptr(g2), _lib.ptr(bws.mid),
                                               size, _lib.stream())

        what = f"{name} K={K} backward"
        assert backward(bbytes - 1) == INVALID_ARG, what
        torch.cuda.synchronize()
        assert bws.untouched() and o1.untouched() and o2.untouched(), what
        assert backward(bbytes) == 0, what
        torch.cuda.synchronize()
        assert bws.canaries_intact() and o1.canaries_intact() and o2.canaries_intact(), what
        np.testing.assert_array_equal(_bits(g1.cpu().numpy()), _bits(g1_ref), err_msg=what)
        np.testing.assert_array_equal(_bits(g2.cpu().numpy()), _bits(g2_ref), err_msg=what)


# ---- the knn_cuda / pointnet2_cuda / flow boundaries ----------------------------------------------------------------------
@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("k", [2, 5, 8, 13, 16])
def test_knn_cuda_small_k(oracle, dev, k, squared):
    from reart_amd import _lib
    from reart_amd.knn_cuda import KNN

    def check(ref, qry, what):
        d_ref, i_ref = oracle.knn_cuda(ref, qry, k, euclidean=not squared)
        d, i = KNN(k, transpose_mode=True, squared=squared)(_t(ref, dev), _t(qry, dev))
        dt, it = KNN(k, transpose_mode=False, squared=squared)(_t(ref, dev).transpose(1, 2), _t(qry, dev).transpose(1, 2))
        assert i.dtype == torch.int64 and d.dtype == torch.float32
        assert tuple(it.shape) == (ref.shape[0], k, qry.shape[1])
        for dd, ii in ((d, i), (dt.transpose(1, 2), it.transpose(1, 2))):
            np.testing.assert_array_equal(ii.cpu().numpy(), i_ref, err_msg=what)
            if squared:
                np.testing.assert_array_equal(_bits(dd.cpu().numpy()), _bits(d_ref), err_msg=what)
            else:
                np.testing.assert_allclose(dd.cpu().numpy(), d_ref, rtol=2e-7, atol=0, err_msg=what)   # sqrtf 1 ulp

    for name in ("s2_first", "copies", "s16_first"):
        c = R.make_case(name)
        check(c["p2"], c["p1"], f"{name} k={k}")
    if k in (2, 16):        # k = nr is accepted, k = nr + 1 raises
        c = R.make_case("s2_first")
        check(c["p2"][:, :k], c["p1"], f"nr = k = {k}")
        with pytest.raises(_lib.ReartHipError, match="reart_knn_cuda"):
            KNN(k + 1, transpose_mode=True, squared=squared)(_t(c["p2"][:, :k], dev), _t(c["p1"], dev))


def test_pointnet_knn_wrapper_small_k(oracle, dev):
    from reart_amd import pointnet2_cuda as pc

    b, n = 2, 100
    rng = np.random.default_rng(21)
    unknown = rng.uniform(-0.35, 0.35, (b, n, 3)).astype(np.float32)
    known = rng.uniform(-0.35, 0.35, (b, 2049, 3)).astype(np.float32)
    m = 1017                                                             # S = 8: the result comes out of the merge kernel
    assert R.plan(b, n, m)[0] == 8 and R.plan(b, n, 2049)[0] == 16
    kn = np.ascontiguousarray(known[:, :m])
    for k in (2, 7, 16):
        d = torch.zeros((b, n, k), dtype=torch.float32, device=dev)
        i = torch.zeros((b, n, k), dtype=torch.int32, device=dev)
        pc.knn_wrapper(b, n, m, k, _t(unknown, dev), _t(kn, dev), d, i)
        d_ref, i_ref = oracle.knn_points(unknown, kn, K=k)
        assert i.dtype == torch.int32
        np.testing.assert_array_equal(i.cpu().numpy(), i_ref)
        np.testing.assert_array_equal(_bits(d.cpu().numpy()), _bits(d_ref))
    d3 = torch.zeros((b, n, 3), dtype=torch.float32, device=dev)
    i3 = torch.zeros((b, n, 3), dtype=torch.int32, device=dev)
    pc.three_nn_wrapper(b, n, 2049, _t(unknown, dev), _t(known, dev), d3, i3)
    d_ref, i_ref = oracle.knn_points(unknown, known, K=3)
    assert i3.dtype == torch.int32
    np.testing.assert_array_equal(i3.cpu().numpy(), i_ref)
    np.testing.assert_array_equal(_bits(d3.cpu().numpy()), _bits(d_ref))


def test_blend_anchor_motion_other_k(oracle, dev):
    from reart_amd.knn_cuda import KNN
    from reart_amd.utils.flow_utils import blend_anchor_motion, blend_anchor_motion_batch, pad_reference_sets

    rng = np.random.default_rng(22)
    ref = rng.uniform(-0.35, 0.35, (509, 3)).astype(np.float32)
    # queries inside and well outside the reference cloud, flows from tiny to large: both mask values occur
    qry = (rng.uniform(-0.35, 0.35, (700, 3)) * rng.choice([1.0, 4.0], (700, 1))).astype(np.float32)
    flo = (rng.normal(size=(509, 3)) * 10.0 ** rng.uniform(-3, 0, (509, 1))).astype(np.float32)
    assert R.plan(1, 700, 509)[0] == 4
    for k in (1, 2, 5, 16):
        flow, mask = blend_anchor_motion(_t(qry, dev), _t(ref, dev), _t(flo, dev), KNN(k, transpose_mode=True), return_mask=True)
        f_ref, m_ref = oracle.blend_anchor_motion(qry, ref, flo, k=k)
        assert mask.dtype == torch.bool and 0 < m_ref.sum() < m_ref.size
        np.testing.assert_array_equal(mask.cpu().numpy(), m_ref, err_msg=f"k={k}")
        np.testing.assert_allclose(flow.cpu().numpy(), f_ref, rtol=2e-6, atol=1e-9, err_msg=f"k={k}")
    # the batch at k = 5 with ragged reference sets: bit for bit the per-frame calls
    knn = KNN(5, transpose_mode=True)
    lens = (509, 5, 130, 300)
    refs = [_t(ref[:n], dev) for n in lens]
    flows = [_t(flo[:n], dev) for n in lens]
    qs = torch.stack([_t(np.roll(qry, 7 * f, axis=0), dev) for f in range(len(lens))])
    r, f, ref_len = pad_reference_sets(refs, flows)
    assert ref_len is not None
    bf, bm = blend_anchor_motion_batch(qs, r, f, ref_len, knn, return_mask=True)
    for b in range(len(lens)):
        of, om = blend_anchor_motion(qs[b], refs[b], flows[b], knn, return_mask=True)
        assert torch.equal(bf[b], of) and torch.equal(bm[b], om), b


# ---- backward -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bwd_problem(tag):
    if isinstance(tag, str):
        c = R.make_case(tag)
        return c["p1"], c["p2"], c["lengths1"], c["lengths2"]
    N, P1, P2 = tag
    rng = np.random.default_rng(N + P1 + P2)
    return (rng.uniform(-0.35, 0.35, (N, P1, 3)).astype(np.float32), rng.uniform(-0.35, 0.35, (N, P2, 3)).astype(np.float32),
            None, None)


# (2, 900, 8 | 9), (2, 300, 512 | 513), (1, 64, 4097): the index bits go 3 | 4, 9 | 10 and 13 -- one, two, three, four and
# five radix passes of RS_BITS = 3
BWD_PROBLEMS = ("ragged", "copies", (2, 900, 8), (2, 900, 9), (2, 300, 512), (2, 300, 513), (1, 64, 4097))


@pytest.mark.parametrize("K", [1, 3, 5, 8, 16])
def test_backward_small_k(oracle, dev, K):
    from reart_amd import _lib
    from reart_amd import chamferdist_C as C

    L = _lib.lib()
    for tag in BWD_PROBLEMS:
        a, b, l1, l2 = _bwd_problem(tag)
        what = f"{tag} K={K}"
        at, bt, l1t, l2t = _t(a, dev), _t(b, dev), _t(l1, dev), _t(l2, dev)
        idx, _ = C.knn_points_idx(at, bt, l1t, l2t, K)                  # the kernel's own forward
        g = np.random.default_rng(K).normal(size=tuple(idx.shape)).astype(np.float32)
        g1_ref, g2_ref = oracle.knn_points_backward(a, b, idx.cpu().numpy(), g, l1, l2)
        gt = _t(g, dev)
        # torch.empty_like inside the wrapper may hand out anything: run once into NaN-filled outputs through the C ABI
        N, P1, P2 = a.shape[0], a.shape[1], b.shape[1]
        o1 = torch.full((N, P1, 3), float("nan"), device=dev)
        o2 = torch.full((N, P2, 3), float("nan"), device=dev)
        ws = torch.empty(L.reart_knn_points_backward_workspace_bytes(N, P1, P2, K), dtype=torch.uint8, device=dev)
        rc = L.reart_knn_points_backward(_lib.ptr(at), _lib.ptr(bt), _lib.ptr(l1t), _lib.ptr(l2t), _lib.ptr(idx), _lib.ptr(gt),
                                         N, P1, P2, 3, K, _lib.ptr(o1), _lib.ptr(o2), _lib.ptr(ws), ws.numel(), _lib.stream())
        assert rc == 0, what
        assert not torch.isnan(o1).any() and not torch.isnan(o2).any(), what
        g1, g2 = C.knn_points_backward(at, bt, l1t, l2t, idx, gt)
        g1b, g2b = C.knn_points_backward(at, bt, l1t, l2t, idx, gt)
        np.testing.assert_array_equal(_bits(g1.cpu().numpy()), _bits(g1_ref), err_msg=what)
        np.testing.assert_array_equal(_bits(g2.cpu().numpy()), _bits(g2_ref), err_msg=what)
        assert torch.equal(g1, g1b) and torch.equal(g2, g2b) and torch.equal(g1, o1) and torch.equal(g2, o2), what
        if l1 is not None:      # zeros where nothing contributes: rows past lengths1, targets past lengths2
            for n in range(N):
                assert not g1[n, int(l1[n]):].any() and not g2[n, int(l2[n]):].any(), what


def test_autograd_small_k(dev):
    """knn_points(K = 5, return_nn = True) on `ragged`, loss = sum w_d * dists + sum w_n * knn: the gradients against the
    float64 form of knn_backward_ref plus the gather term, within the fp32 form's bound (the gather adds one addend per
    pair to grad_p2 and none to grad_p1)."""
    from reart_amd.utils.chamfer import knn_points

    c, K = R.make_case("ragged"), 5
    rng = np.random.default_rng(23)
    N, P1, P2 = c["p1"].shape[0], c["p1"].shape[1], c["p2"].shape[1]
    wd = rng.normal(size=(N, P1, K)).astype(np.float32)
    wn = rng.normal(size=(N, P1, K, 3)).astype(np.float32)
    p1 = _t(c["p1"], dev).requires_grad_(True)
    p2 = _t(c["p2"], dev).requires_grad_(True)
    out = knn_points(p1, p2, lengths1=_t(c["lengths1"], dev), lengths2=_t(c["lengths2"], dev), K=K, return_nn=True)
    assert tuple(out.knn.shape) == (N, P1, K, 3)
    ((out.dists * _t(wd, dev)).sum() + (out.knn * _t(wn, dev)).sum()).backward()
    idx = out.idx.cpu().numpy()
    ref = R.knn_backward_ref(c["p1"], c["p2"], idx, wd, c["lengths1"], c["lengths2"], dtype=np.float64)
    # gather term: d/dp2[n, j] of sum w_n * p2[n, idx] over the slots k < lengths2 (rows past lengths1 gather p2[n, 0] too)
    g2, a2, n2 = ref.grad_p2.copy(), ref.abs_p2.copy(), ref.n_p2.copy()
    for n in range(N):
        kk = min(K, int(c["lengths2"][n]))
        j = idx[n, :, :kk].reshape(-1)
        w = wn[n, :, :kk].reshape(-1, 3).astype(np.float64)
        np.add.at(g2[n], j, w)
        np.add.at(a2[n], j, np.abs(w))
        np.add.at(n2[n], j, 1)
    assert (np.abs(p1.grad.cpu().numpy() - ref.grad_p1) <= R.backward_bound(ref.n_p1, ref.abs_p1)).all()
    assert (np.abs(p2.grad.cpu().numpy() - g2) <= R.backward_bound(n2, a2)).all()
    assert np.abs(ref.grad_p1).max() > 0 and np.abs(g2).max() > 0
