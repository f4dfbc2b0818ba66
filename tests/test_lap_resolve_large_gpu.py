"""The large warm re-solve (reart_lap_resolve_large, 1 <= n <= 8192; linear_sum_assignment_batch sends it 4096 < n <= 8192
when a state carries the previous potentials and assignment) against scipy.optimize.linear_sum_assignment, the solver the
reference calls: the same optimum as the solvers certify it (tests/test_lap_gpu.py `_within_certificate`) and, on continuous
random costs, the same permutation.  Where scipy would take too long: the weak-duality bound of
tests/test_lap_large_gpu.py::test_capacity_edge_by_weak_duality, same expression, same margins."""
import math

import numpy as np
import pytest
import torch

from tests.test_lap_gpu import _within_certificate
from tests.test_lap_large_gpu import _clouds, _large

pytestmark = pytest.mark.gpu

GAVE_UP = 1 << 30         # bit 30 of stats[b][0]: the step limit was reached


def _resolve(cost_np, cols, prices, dev, max_steps=0):
    """The C entry on cost_np [B,n,n] from the state (cols [B,n], prices [B,n]) -> (cols int64, certified, prices, stats)."""
    from reart_amd import _lib

    L = _lib.lib()
    cost = torch.from_numpy(cost_np).to(dev).contiguous()
    B, n, _ = cost.shape
    col = torch.from_numpy(np.ascontiguousarray(cols)).to(device=dev, dtype=torch.int32)
    p_in = torch.from_numpy(np.ascontiguousarray(prices)).to(device=dev, dtype=torch.float64)
    p_out = torch.zeros((B, n), dtype=torch.float64, device=dev)
    cert = torch.zeros((B,), dtype=torch.int32, device=dev)
    nbytes = L.reart_lap_resolve_large_workspace_bytes(B, n)
    assert nbytes > 0
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
    rc = L.reart_lap_resolve_large(_lib.ptr(cost), B, n, max_steps, _lib.ptr(col), _lib.ptr(cert), _lib.ptr(p_in), _lib.ptr(p_out),
                                   _lib.ptr(ws), ws.numel(), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    off = ((8 * B * n + 255) // 256) * 256
    stats = ws[off:off + 16 * B].view(torch.int32).reshape(B, 4).cpu().numpy()
    return col.cpu().numpy().astype(np.int64), cert.cpu().numpy(), p_out.cpu().numpy(), stats


def _within_weak_duality(c_np, cols, p, what=None):
    """test_capacity_edge_by_weak_duality's bound: for ANY potentials p, sum_i min_j (c_ij + p_j) - sum_j p_j is a lower bound
    of every assignment's cost."""
    n = c_np.shape[0]
    p = np.asarray(p, dtype=np.float64)
    mins = []
    for i0 in range(0, n, 512):
        mins.extend((c_np[i0:i0 + 512].astype(np.float64) + p[None, :]).min(axis=1).tolist())
    primal = math.fsum(c_np[np.arange(n), cols].astype(np.float64).tolist())
    dual = math.fsum(mins + (-p).tolist())
    mx = float(c_np.max())
    print(what, "primal", primal, "dual", dual, "gap", primal - dual, "bound", n * 1e-13 * mx + n * 1e-15 * mx)
    assert primal - dual <= n * 1e-13 * mx + n * 1e-15 * mx, what


def _moved(cost0, seed):
    """C1 = C0 + a seeded perturbation of 1e-3 x max(C0) (non-negative, like the costs)."""
    rng = np.random.default_rng(seed)
    return (cost0 + np.float32(1e-3 * float(cost0.max())) * rng.uniform(0.0, 1.0, cost0.shape).astype(np.float32)).astype(np.float32)


def _small_costs(n):
    if n == 2500:     # the cloud costs of test_large_instance_on_small_matrices
        rng = np.random.default_rng(77)
        pts = rng.uniform(-0.3, 0.3, (2, 2500, 3)).astype(np.float32)
        return torch.cdist(torch.from_numpy(pts[:1]), torch.from_numpy(pts[1:] + 0.01)).numpy().astype(np.float32)
    return np.random.default_rng(n).uniform(0.0, 1.0, (3, n, n)).astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 5, 64, 300, 1025, 2500])
def test_large_instance_on_small_matrices(dev, n):
    """The whole logic of the large instance (index arrays in LDS, row potentials in the workspace, sixteen columns per
    thread) at sizes that take milliseconds: a cold solve of C0, then C1 = C0 + 1e-3 x max(C0) x noise from that state."""
    import oracle

    cost0 = _small_costs(n)
    B = cost0.shape[0]
    cols0, cert0, prices0, _ = _large(cost0, dev)
    assert cert0.tolist() == [1] * B
    cost1 = _moved(cost0, 1000 + n)
    cols, cert, prices, stats = _resolve(cost1, cols0, prices0, dev)
    print("n", n, "stats (released, left for the searches, search steps, rounds + reduction steps << 8)", stats.tolist())
    ref = oracle.linear_sum_assignment(cost1)
    rows = np.arange(n)
    assert cert.tolist() == [1] * B
    assert not (stats[:, 0] & GAVE_UP).any()
    for b in range(B):
        assert sorted(cols[b].tolist()) == list(range(n))
        _within_certificate(cost1[b], (rows, cols[b]), ref[b], what=(n, b))
        np.testing.assert_array_equal(cols[b], ref[b][1])
    if n != 300:
        return
    # the same matrix again from its own result: nothing is released
    cols2, cert2, _, stats2 = _resolve(cost1, cols, prices, dev)
    assert cert2.tolist() == [1] * B
    assert (stats2[:, 0] & ~GAVE_UP).tolist() == [0] * B and not (stats2[:, 0] & GAVE_UP).any(), stats2.tolist()
    np.testing.assert_array_equal(cols2, cols)
    # the same call twice from the same state: the same bits
    cols3, cert3, prices3, _ = _resolve(cost1, cols0, prices0, dev)
    assert cert3.tolist() == [1] * B
    np.testing.assert_array_equal(cols3, cols)
    assert prices3.tobytes() == prices.tobytes()


@pytest.mark.parametrize("start", ["all_free", "all_zero", "out_of_range"])
def test_useless_state_is_legal_input(dev, start):
    import oracle

    n, B = 300, 3
    cost = np.random.default_rng(300).uniform(0.0, 1.0, (B, n, n)).astype(np.float32)
    cols_in = {"all_free": np.full((B, n), -1), "all_zero": np.zeros((B, n)),
               "out_of_range": n + np.arange(B * n).reshape(B, n)}[start].astype(np.int32)
    cols, cert, _, stats = _resolve(cost, cols_in, np.zeros((B, n)), dev)
    print(start, "stats", stats.tolist())
    ref = oracle.linear_sum_assignment(cost)
    assert cert.tolist() == [1] * B
    for b in range(B):
        assert sorted(cols[b].tolist()) == list(range(n))
        _within_certificate(cost[b], (np.arange(n), cols[b]), ref[b], what=(start, b))
        np.testing.assert_array_equal(cols[b], ref[b][1])


def test_exact_ties(dev):
    """The two matrices of test_large_instance_on_exact_ties, re-solved from a cold solve of themselves: a permutation with
    the optimal cost, or an honest certified = 0 that the Python path then solves (scipy here, as there)."""
    import oracle
    from scipy.optimize import linear_sum_assignment

    rng = np.random.default_rng(3)
    base = rng.uniform(0, 1, (1, 40, 40)).astype(np.float32)
    dup = np.concatenate([base, base], axis=1)
    dup = np.concatenate([dup, dup], axis=2)
    for cost in (dup, np.zeros((2, 17, 17), np.float32)):
        n = cost.shape[1]
        cols0, cert0, prices0, _ = _large(cost, dev)
        cols, cert, _, stats = _resolve(cost, cols0, prices0, dev)
        print("n", n, "cold certified", cert0.tolist(), "warm certified", cert.tolist(), "stats", stats.tolist())
        ref = oracle.linear_sum_assignment(cost)
        for b in range(cost.shape[0]):
            c = cols[b] if cert[b] else linear_sum_assignment(cost[b])[1]
            assert sorted(c.tolist()) == list(range(n))
            _within_certificate(cost[b], (np.arange(n), c), ref[b], what=(n, b))


def test_step_limit_through_the_entry(dev):
    """max_steps = 1 from the all-free state: every matrix is given up, honestly, and the call itself succeeds."""
    n, B = 300, 3
    cost = np.random.default_rng(300).uniform(0.0, 1.0, (B, n, n)).astype(np.float32)
    _, cert, _, stats = _resolve(cost, np.full((B, n), -1, np.int32), np.zeros((B, n)), dev, max_steps=1)
    print("stats", stats.tolist())
    assert cert.tolist() == [0] * B
    assert ((stats[:, 0] & GAVE_UP) != 0).all()


def test_step_limit_through_the_wrapper(dev, monkeypatch):
    """n = 4097, B = 1, the module's limit at one step: the warm attempt is given up and the matrix is solved cold on the GPU
    in the same call."""
    from reart_amd.utils import lap

    n = 4097
    src, tgt = _clouds(4097 + 1, 1, n)
    s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    state = {}
    _, fb0 = lap.linear_sum_assignment_batch(lap.cdist(s, t), return_stats=True, state=state, warm_assignment=True)
    assert fb0 == 0 and state["resolve_form"] == "cold" and state["resolve_cold"] == 0
    moved = s + torch.from_numpy(np.random.default_rng(5).normal(0.0, 1e-2, src.shape).astype(np.float32)).to(dev)
    cost = lap.cdist(moved, t)
    monkeypatch.setattr(lap, "RESOLVE_LARGE_MAX_STEPS", 1)
    out, fallbacks, st = lap.linear_sum_assignment_batch(cost, return_stats="full", state=state, warm_assignment=True)
    print("4097 stats of the warm attempt", st.tolist())
    assert fallbacks == 0
    assert state["resolve_cold"] == 1
    assert state["resolve_form"] == "jv"
    assert st[0, 0] & GAVE_UP
    (r, c), = out
    assert sorted(c.tolist()) == list(range(n))
    np.testing.assert_array_equal(state["cols"][0].cpu().numpy(), c)
    _within_weak_duality(cost[0].cpu().numpy(), c, state["prices"][0].cpu().numpy(), what="4097 after the cold second attempt")


def test_first_size_above_the_limit_moving(dev):
    """n = 4097, B = 2 (rows of 16 388 B: every second one misses 16-byte alignment; one column in the last per-thread slot):
    four calls of linear_sum_assignment_points with the source moving by N(0, 1e-3) per call -- cold, then warm."""
    import oracle

    from reart_amd.utils.lap import cdist, linear_sum_assignment_points

    n, B = 4097, 2
    src, tgt = _clouds(4097, B, n)
    rng = np.random.default_rng(11)
    t = torch.from_numpy(tgt).to(dev)
    state = {}
    forms = []
    for call in range(4):
        src = (src + rng.normal(0.0, 1e-3, src.shape)).astype(np.float32)
        s = torch.from_numpy(src).to(dev)
        out, fallbacks, st = linear_sum_assignment_points(s, t, state, return_stats="full")
        print("call", call, "form", state.get("resolve_form"), "stats", st.tolist())
        forms.append(state.get("resolve_form"))
        assert fallbacks == 0
        assert state["resolve_cold"] == 0
        cost_np = cdist(s, t).cpu().numpy()
        prices = state["prices"].cpu().numpy()
        for b, (r, c) in enumerate(out):
            assert sorted(c.tolist()) == list(range(n))
            _within_weak_duality(cost_np[b], c, prices[b], what=(call, b))
    assert forms == ["cold", "jv", "jv", "jv"]
    ref = oracle.linear_sum_assignment(cost_np)
    for b, (r, c) in enumerate(out):
        _within_certificate(cost_np[b], (r, c), ref[b], what=b)
        np.testing.assert_array_equal(c, ref[b][1])


def test_uniform_costs_above_the_limit(dev):
    """Uniform random costs (a price war, unlike the clouds) at n = 4100: cold, then warm on costs moved by 1e-4 x noise."""
    import oracle

    from reart_amd.utils.lap import linear_sum_assignment_batch

    rng = np.random.default_rng(4100)
    cost0 = rng.uniform(0.0, 1.0, (1, 4100, 4100)).astype(np.float32)
    state = {}
    _, fb0 = linear_sum_assignment_batch(torch.from_numpy(cost0).to(dev), return_stats=True, state=state, warm_assignment=True)
    assert fb0 == 0
    cost1 = (cost0 + np.float32(1e-4) * rng.uniform(0.0, 1.0, cost0.shape).astype(np.float32)).astype(np.float32)
    out, fallbacks, st = linear_sum_assignment_batch(torch.from_numpy(cost1).to(dev), return_stats="full", state=state, warm_assignment=True)
    print("4100 form", state["resolve_form"], "cold after warm", state["resolve_cold"], "stats", st.tolist())
    assert fallbacks == 0
    assert state["resolve_form"] == "jv"
    ref = oracle.linear_sum_assignment(cost1)
    (r, c), = out
    assert sorted(c.tolist()) == list(range(4100))
    _within_certificate(cost1[0], (r, c), ref[0], what=4100)
    np.testing.assert_array_equal(c, ref[0][1])


def test_capacity_edge_warm(dev):
    """n = 8192, B = 1: a cold solve into a state, the source moved by N(0, 1e-3), the warm re-solve.  No scipy at this size."""
    from reart_amd.utils.lap import cdist, linear_sum_assignment_batch

    n = 8192
    src, tgt = _clouds(8192, 1, n)
    t = torch.from_numpy(tgt).to(dev)
    state = {}
    _, fb0 = linear_sum_assignment_batch(cdist(torch.from_numpy(src).to(dev), t), return_stats=True, state=state, warm_assignment=True)
    assert fb0 == 0 and state["resolve_form"] == "cold"
    moved = (src + np.random.default_rng(8).normal(0.0, 1e-3, src.shape)).astype(np.float32)
    cost = cdist(torch.from_numpy(moved).to(dev), t)
    out, fallbacks, st = linear_sum_assignment_batch(cost, return_stats="full", state=state, warm_assignment=True)
    print("8192 form", state["resolve_form"], "cold after warm", state["resolve_cold"], "stats", st.tolist())
    assert fallbacks == 0
    assert state["resolve_form"] == "jv" and state["resolve_cold"] == 0       # certified by the warm re-solve itself
    (r, c), = out
    assert sorted(c.tolist()) == list(range(n))
    _within_weak_duality(cost[0].cpu().numpy(), c, state["prices"][0].cpu().numpy(), what=8192)


def test_through_the_engine(dev):
    """A KinematicEngine whose sparse point count is 4097 (two problems): after three iterations the refresh has been the warm
    large re-solve, without a host solve, and its assignment is the cold solve's of the same points."""
    from reart_amd.utils.lap import cdist, linear_sum_assignment_batch
    from tests.test_kinematic_long_gpu import _engine, _sequence

    s = _sequence(dev, 2, 8194, 0, False, seed=8194)
    _, eng = _engine(dev, s, 0)
    assert eng.src_idx.numel() == 4097
    for i in range(3):
        eng.iteration(i)
    assert eng.lap_solves == 3
    assert eng.lap_fallbacks == 0
    assert eng.lap_state["resolve_form"] == "jv"
    cold = linear_sum_assignment_batch(cdist(eng._pc_src, eng.tgt_pts))
    got = eng.lap_state["cols"].cpu().numpy()
    for b, (_, c) in enumerate(cold):
        np.testing.assert_array_equal(got[b], c)
