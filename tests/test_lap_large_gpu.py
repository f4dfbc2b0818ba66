"""The large assignment solve (reart_lap_auction_large, 1 <= n <= 8192; linear_sum_assignment_batch sends it
4096 < n <= 8192) against scipy.optimize.linear_sum_assignment, the solver the reference calls: the same optimum as the
solvers certify it (tests/test_lap_gpu.py `_within_certificate`) and, on continuous random costs, the same permutation."""
import math

import numpy as np
import pytest
import torch

from tests.test_lap_gpu import _within_certificate

pytestmark = pytest.mark.gpu


def _large(cost_np, dev, points=None):
    """The C entry on cost_np [B,n,n] -> (cols [B,n] int64, certified [B], prices [B,n] f64, stats [B,4])."""
    from reart_amd import _lib

    L = _lib.lib()
    cost = torch.from_numpy(cost_np).to(dev).contiguous()
    B, n, _ = cost.shape
    col = torch.full((B, n), -1, dtype=torch.int32, device=dev)
    cert = torch.zeros((B,), dtype=torch.int32, device=dev)
    prices = torch.zeros((B, n), dtype=torch.float64, device=dev)
    nbytes = L.reart_lap_large_workspace_bytes(B, n)
    assert nbytes > 0
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
    src, tgt = (None, None) if points is None else points
    rc = L.reart_lap_auction_large(_lib.ptr(cost), _lib.ptr(src), _lib.ptr(tgt), B, n, _lib.ptr(col), _lib.ptr(cert), _lib.ptr(prices),
                                   _lib.ptr(ws), ws.numel(), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    off = ((8 * B * n + 255) // 256) * 256
    stats = ws[off:off + 16 * B].view(torch.int32).reshape(B, 4).cpu().numpy()
    return col.cpu().numpy().astype(np.int64), cert.cpu().numpy(), prices.cpu().numpy(), stats


def _clouds(seed, B, n):
    """Clouds uniform in [-0.3, 0.3]^3; the target is the permuted source moved by N(0, 0.01)."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-0.3, 0.3, (B, n, 3)).astype(np.float32)
    tgt = np.stack([src[b][rng.permutation(n)] for b in range(B)]) + rng.normal(0.0, 0.01, (B, n, 3))
    return src, tgt.astype(np.float32)


def _small_cases():
    cases = []
    for n in (1, 2, 5, 64, 300, 1025):
        cases.append(pytest.param(n, id=f"uniform-{n}"))
    cases.append(pytest.param(2500, id="clouds-2500"))
    return cases


@pytest.mark.parametrize("n", _small_cases())
def test_large_instance_on_small_matrices(dev, n):
    """The whole logic of the large instance (bids through the workspace, eight columns per thread in a search, the 16-bit
    predecessor rows) at sizes that take milliseconds; 2500 crosses LAP_NLDS, where the 4096 instance changes its layout."""
    import oracle

    if n == 2500:     # the cloud costs of test_lap_above_the_lds_resident_size
        rng = np.random.default_rng(77)
        pts = rng.uniform(-0.3, 0.3, (2, 2500, 3)).astype(np.float32)
        cost = torch.cdist(torch.from_numpy(pts[:1]), torch.from_numpy(pts[1:] + 0.01)).numpy().astype(np.float32)
    else:
        cost = np.random.default_rng(n).uniform(0.0, 1.0, (3, n, n)).astype(np.float32)
    cols, cert, _, stats = _large(cost, dev)
    print("n", n, "stats (phases, rounds, bids, certificate rounds)", stats.tolist())
    ref = oracle.linear_sum_assignment(cost)
    rows = np.arange(n)
    assert cert.tolist() == [1] * cost.shape[0]
    for b in range(cost.shape[0]):
        assert sorted(cols[b].tolist()) == list(range(n))
        _within_certificate(cost[b], (rows, cols[b]), ref[b], what=(n, b))
        np.testing.assert_array_equal(cols[b], ref[b][1])


def test_large_instance_on_exact_ties(dev):
    """The two matrices of test_lap_ties: many optima; a permutation with the optimal cost.  A matrix the kernel reports
    uncertified is solved the way the Python path solves it (scipy), and that result is what is checked."""
    import oracle
    from scipy.optimize import linear_sum_assignment

    rng = np.random.default_rng(3)
    base = rng.uniform(0, 1, (1, 40, 40)).astype(np.float32)
    dup = np.concatenate([base, base], axis=1)
    dup = np.concatenate([dup, dup], axis=2)
    for cost in (dup, np.zeros((2, 17, 17), np.float32)):
        n = cost.shape[1]
        cols, cert, _, stats = _large(cost, dev)
        print("n", n, "certified", cert.tolist(), "stats", stats.tolist())
        ref = oracle.linear_sum_assignment(cost)
        for b in range(cost.shape[0]):
            c = cols[b] if cert[b] else linear_sum_assignment(cost[b])[1]
            assert sorted(c.tolist()) == list(range(n))
            _within_certificate(cost[b], (np.arange(n), c), ref[b], what=(n, b))


@pytest.fixture(scope="module")
def clouds4097(dev):
    """B = 2 problems of 4097 points: rows of 16 388 B (every second one misses 16-byte alignment) and one column in the
    last per-thread slot.  The scipy reference is computed once for the tests that share the clouds."""
    import oracle

    from reart_amd.utils.lap import cdist

    src, tgt = _clouds(4097, 2, 4097)
    s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    cost = cdist(s, t)
    cost_np = cost.cpu().numpy()
    return {"src": s, "tgt": t, "cost": cost, "cost_np": cost_np, "ref": oracle.linear_sum_assignment(cost_np)}


def _check_batch(out, cost_np, ref):
    n = cost_np.shape[1]
    for b, (r, c) in enumerate(out):
        assert sorted(c.tolist()) == list(range(n))
        _within_certificate(cost_np[b], (r, c), ref[b], what=b)
        np.testing.assert_array_equal(c, ref[b][1])


def test_first_size_above_the_limit(dev, clouds4097):
    """n = 4097 through linear_sum_assignment_batch: solved on the GPU (no fallback), with and without the points."""
    from reart_amd.utils.lap import linear_sum_assignment_batch

    k = clouds4097
    out, fallbacks, st = linear_sum_assignment_batch(k["cost"], return_stats="full")
    print("4097 stats (phases, rounds, bids, certificate rounds)", st.tolist())
    assert fallbacks == 0
    _check_batch(out, k["cost_np"], k["ref"])
    out_p, fallbacks_p = linear_sum_assignment_batch(k["cost"], return_stats=True, points=(k["src"], k["tgt"]))
    assert fallbacks_p == 0
    _check_batch(out_p, k["cost_np"], k["ref"])
    for (_, c), (_, cp) in zip(out, out_p):
        np.testing.assert_array_equal(c, cp)


def test_uniform_costs_above_the_limit(dev):
    """Uniform random costs (a price war, unlike the clouds) at n = 4100."""
    import oracle

    from reart_amd.utils.lap import linear_sum_assignment_batch

    cost = np.random.default_rng(4100).uniform(0.0, 1.0, (1, 4100, 4100)).astype(np.float32)
    out, fallbacks, st = linear_sum_assignment_batch(torch.from_numpy(cost).to(dev), return_stats="full")
    print("4100 stats (phases, rounds, bids, certificate rounds)", st.tolist())
    assert fallbacks == 0
    _check_batch(out, cost, oracle.linear_sum_assignment(cost))


def test_capacity_edge_by_weak_duality(dev):
    """n = 8192.  No scipy (15 s): for ANY potentials p,  sum_i min_j (c_ij + p_j) - sum_j p_j  is a lower bound of every
    assignment's cost, so an assignment within n x 1e-13 x max(c) of that bound under the returned potentials is optimal to
    the certificate's margin, whatever produced the potentials.  n x 1e-15 x max(c) is slack for the float64 rounding of
    the host's own sums of c + p."""
    from reart_amd.utils.lap import cdist, linear_sum_assignment_batch

    n = 8192
    src, tgt = _clouds(8192, 1, n)
    cost = cdist(torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev))
    state = {}
    out, fallbacks, st = linear_sum_assignment_batch(cost, return_stats="full", state=state)
    print("8192 stats (phases, rounds, bids, certificate rounds)", st.tolist())
    assert fallbacks == 0
    (r, c), = out
    assert sorted(c.tolist()) == list(range(n))
    assert tuple(state["prices"].shape) == (1, n) and state["prices"].dtype == torch.float64
    c_np = cost[0].cpu().numpy()
    p = state["prices"][0].cpu().numpy().astype(np.float64)
    mins = []
    for i0 in range(0, n, 512):
        mins.extend((c_np[i0:i0 + 512].astype(np.float64) + p[None, :]).min(axis=1).tolist())
    primal = math.fsum(c_np[r, c].astype(np.float64).tolist())
    dual = math.fsum(mins + (-p).tolist())
    mx = float(c_np.max())
    print("8192 primal", primal, "dual", dual, "gap", primal - dual, "bound", n * 1e-13 * mx + n * 1e-15 * mx)
    assert primal - dual <= n * 1e-13 * mx + n * 1e-15 * mx


def test_compute_ass_err_above_the_limit(dev, clouds4097):
    """The user-facing value: compute_ass_err at 4097 points is the expression under scipy's assignment, with no host solve."""
    from reart_amd.utils.model_utils import compute_ass_err

    k = clouds4097
    got = float(compute_ass_err(k["src"], k["tgt"]))
    assert compute_ass_err.last_fallbacks == 0
    cols = torch.from_numpy(np.stack([c for _, c in k["ref"]])).to(dev)
    matched = torch.gather(k["tgt"], 1, cols[..., None].expand(-1, -1, 3))
    want = float(((k["src"] - matched) ** 2).sum(dim=-1).mean())
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)
