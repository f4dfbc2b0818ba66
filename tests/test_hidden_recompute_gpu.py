"""reart_base_backward without saved hidden activations: hT == NULL makes the block kernel re-evaluate the hidden layer from
the points and W1 | b1 with the forward's own expression (hidden_unit, csrc/model_dev.h), so every gradient must carry the
bits of the run that reads the forward's hT.  One forward per case, then the backward twice on the same buffers."""
import numpy as np
import pytest
import torch

# (N, P, B, H, offset): offset = elements every tensor starts into its allocation (1: base pointers 4 mod 16, the dword form)
CASES = [(96, 20, 19, 128, 0),    # the template's shape, full 32-point chunks: the branch-free 16-byte form
         (100, 20, 19, 128, 0),   # 16-byte form, last chunk of 4 points
         (37, 20, 19, 128, 0),    # N % 4 != 0: dword form, last chunk of 5 points
         (96, 3, 1, 30, 0),       # H % 4 != 0: dword form; generic P, one frame
         (37, 3, 1, 128, 0),
         (96, 20, 1, 30, 0),
         (96, 20, 19, 128, 1)]    # aligned shape at pointers 4 mod 16: dword form
GRAD_KEYS = ("gW1", "gb1", "gW2", "g6d", "gt")
TAU = 2.5


def test_cases_cover_the_listed_shapes():
    """CPU side: both N, both kinds of H, both P and both B are present, each with the other values of the other axes, and
    one case sits at pointers 4 mod 16."""
    assert {c[0] for c in CASES} >= {37, 96} and 37 % 4 != 0 and 37 % 32 != 0
    assert 128 in {c[3] for c in CASES} and any(c[3] % 4 for c in CASES)
    assert {c[1] for c in CASES} >= {20, 3} and {c[2] for c in CASES} >= {1, 19}
    assert any(c[4] == 1 and c[0] % 4 == 0 and c[3] % 4 == 0 for c in CASES)
    assert len(set(CASES)) == len(CASES)


def _inputs(N, P, B, H):
    rng = np.random.default_rng(57)
    d = dict(cano=rng.uniform(-0.3, 0.3, (N, 3)), W1=rng.normal(0, 0.5, (H, 3)), b1=rng.normal(0, 0.1, H),
             W2=rng.normal(0, 0.3, (P, H)), p6d=rng.normal(size=(B, P, 6)), pt=rng.normal(0, 0.1, (B, P, 3)),
             noise=-np.log(rng.exponential(size=(N, P))), G=rng.normal(size=(B, N, 3)))
    return {k: v.astype(np.float32) for k, v in d.items()}


def _run(case, dev):
    """The forward once; the backward with the forward's hT and with hT = NULL.  Returns (hT, grads with hT, grads without)."""
    from reart_amd import _lib

    N, P, B, H, offset = case

    def alloc(shp, dtype=torch.float32, fill=None):
        buf = torch.empty(int(np.prod(shp)) + offset, dtype=dtype, device=dev)
        v = buf[offset:].view(*shp)
        if fill is not None:
            v.fill_(fill)
        return v

    def put(a):
        v = alloc(a.shape)
        v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return v

    L = _lib.lib()
    g = {k: put(v) for k, v in _inputs(N, P, B, H).items()}
    out, seg = alloc((B, N, 3)), alloc((N,), torch.int64)
    trans, yT, hT, hard = alloc((B, P, 4, 4)), alloc((P, N)), alloc((H, N)), alloc((N,), torch.int32)
    for x in list(g.values()) + [yT, hT]:
        assert x.data_ptr() % 16 == (4 * offset) % 16
    _lib.check(L.reart_base_forward(_lib.ptr(g["cano"]), N, P, B, _lib.ptr(g["W1"]), _lib.ptr(g["b1"]), _lib.ptr(g["W2"]), H,
                                    _lib.ptr(g["p6d"]), _lib.ptr(g["pt"]), _lib.ptr(g["noise"]), TAU, _lib.ptr(out), _lib.ptr(seg),
                                    _lib.ptr(trans), _lib.ptr(yT), _lib.ptr(hT), _lib.ptr(hard), _lib.stream()), "fwd")
    nws = L.reart_base_backward_workspace_bytes(N, P, B, H)
    res = []
    for saved in (hT, None):
        grads = [alloc(g[k].shape, fill=float("nan")) for k in ("W1", "b1", "W2", "p6d", "pt")]
        ws = torch.empty(nws + 4 * offset, dtype=torch.uint8, device=dev)[4 * offset:]
        _lib.check(L.reart_base_backward(_lib.ptr(g["cano"]), N, P, B, _lib.ptr(g["W1"]), _lib.ptr(g["b1"]), _lib.ptr(g["W2"]), H,
                                         _lib.ptr(g["p6d"]), _lib.ptr(g["pt"]), _lib.ptr(yT), _lib.ptr(saved), _lib.ptr(hard), TAU,
                                         _lib.ptr(g["G"]), *[_lib.ptr(x) for x in grads], _lib.ptr(ws), ws.numel(), _lib.stream()),
                   "bwd")
        torch.cuda.synchronize()
        res.append({k: v.cpu().numpy() for k, v in zip(GRAD_KEYS, grads)})
    return hT.cpu().numpy(), res[0], res[1]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d_P%d_B%d_H%d_off%d" % c)
def test_gradients_without_saved_hidden_layer_are_byte_identical(dev, case):
    hT, saved, recomputed = _run(case, dev)
    assert (hT > 0).any() and (hT == 0).any()            # the relu cuts on both sides: relu'(h) matters
    for k in GRAD_KEYS:
        a, b = saved[k], recomputed[k]
        assert np.isfinite(a).all() and np.abs(a).max() > 0, k
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (case, k, int((a.view(np.uint8) != b.view(np.uint8)).sum()))


@pytest.mark.gpu
def test_null_hidden_layer_needs_the_first_layer(dev):
    """hT == NULL and no W1 | b1 to re-evaluate it from: refused, nothing launched."""
    from reart_amd import _lib

    N, P, B, H = 32, 3, 1, 8
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    L = _lib.lib()
    ws = torch.empty(L.reart_base_backward_workspace_bytes(N, P, B, H), dtype=torch.uint8, device=dev)
    rc = L.reart_base_backward(_lib.ptr(z(N, 3)), N, P, B, None, None, _lib.ptr(z(P, H)), H, _lib.ptr(z(B, P, 6)), _lib.ptr(z(B, P, 3)),
                               _lib.ptr(z(P, N)), None, _lib.ptr(z(N, dt=torch.int32)), TAU, _lib.ptr(z(B, N, 3)), _lib.ptr(z(H, 3)),
                               _lib.ptr(z(H)), _lib.ptr(z(P, H)), _lib.ptr(z(B, P, 6)), _lib.ptr(z(B, P, 3)), _lib.ptr(ws), ws.numel(),
                               _lib.stream())
    assert rc < 0
