"""GPU: the exact box-pruned searches (csrc/prune.hip), their operators and the brute-force yardstick beyond 4112 points, on
the large cases of tests/search_cases.py (``LARGE``): a third and later coarse round, box numbers above 4096, target
indices above 65 535, more than 2^20 distance evaluations by one cold wave, the last size the cloud-resident form takes and
the first it hands on, a launch order left alone (more than 4096 (frame, group) pairs), 70 000 addends in one fixed-point
sum.  Neighbours and distances are compared bit for bit with oracle.knn_points, computed once per (case, K, direction);
the helpers are those of tests/test_search_hostile_gpu.py, tests/test_chamfer_ragged_gpu.py and tests/test_flow_term_gpu.py.
No matrix above 64 M entries is built (search_cases.MAX_ENTRIES): the tie rules are evaluated in blocks of 256 queries, the
farthest-target seeds in blocks of at most 64 M / P2 queries."""
import functools
import time

import numpy as np
import pytest
import torch

from tests import search_cases as sc
from tests.test_chamfer_ragged_gpu import _cls, _exact as _exact_ragged, _trimmed_equal, _upstream
from tests.test_chamfer_ragged_gpu import _grad_ok, _loss_ok, _run, _same
from tests.test_flow_term_gpu import _loss_ok as _flow_loss_ok, _run as _flow_run, _same as _flow_same, _yardstick
from tests.test_search_hostile_gpu import _garbage2, _state, _trajectory, _up, _warm_all_regimes

pytestmark = pytest.mark.gpu

GRAD_CASES = ("scan70k", "lattice27k", "fanin70k")      # the cases whose gradients are held to the derived bound


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    print(f"\ntests/test_search_large_gpu.py: {time.time() - t0:.1f} s")


def _clouds(name, swapped=False, seed=0):
    """(queries, targets) of a large case; `three` is `round3` against its first three stored targets."""
    q, t = sc.large_case("round3" if name == "three" else name, seed)
    t = t[:3] if name == "three" else t
    return (t, q) if swapped else (q, t)


@functools.lru_cache(maxsize=None)
def _ref(name, K, swapped=False, seed=0):
    """oracle.knn_points of one case, one way round: (dists [P1,K], idx [P1,K]), computed once.  K = 16 is read off the
    K = 17 result (the contract is the head of ONE sorted row, tests/test_search_cases_cpu.py)."""
    import oracle

    if K == 16:
        return tuple(a[:, :16] for a in _ref(name, 17, swapped, seed))
    q, t = _clouds(name, swapped, seed)
    d, i = oracle.knn_points(q[None], t[None], K=K)
    d, i = d[0], i[0]
    d.setflags(write=False)
    i.setflags(write=False)
    return d, i


@functools.lru_cache(maxsize=None)
def _must_equal(name, K, swapped=False):
    """[P1,K] bool, as in tests/test_search_hostile_gpu.py but in blocks of 256 queries: slots where any exact search must
    name the oracle's target -- the only target at that distance, or every target at that distance coincides with it.
    `scan70k` is free of ties (asserted on the CPU): every slot."""
    q, t = _clouds(name, swapped)
    d_ref, i_ref = _ref(name, K, swapped)
    if name == "scan70k":
        return np.ones(i_ref.shape, bool)
    out = np.zeros(i_ref.shape, bool)
    for r, D in sc.blocks(q, t):
        rows = slice(r, r + D.shape[0])
        for k in range(min(K, t.shape[0])):
            tr, tc = np.nonzero(D == d_ref[rows, k, None])                      # the tied (query, target) entries
            other = (t[tc] != t[i_ref[rows, k]][tr]).any(-1)                    # ... at another place than the oracle's target
            out[rows, k] = np.bincount(tr[other], minlength=D.shape[0]) == 0
    return out


def _check(name, K, swapped, d, i, exact_idx, what, rows=None):
    """d [P1,K], i [P1,K] of one direction against the oracle (``rows``: the case's query rows they belong to).  With
    ``exact_idx`` False (a storage order of the operator's own) the tie rule between DISTINCT equidistant targets differs:
    the index must still attain the distance exactly, coincident targets resolve to the lowest index, no target twice.
    No slot of `scan70k` is excused: it has no ties."""
    q, t = _clouds(name, swapped)
    d_ref, i_ref = _ref(name, K, swapped)
    must = None if exact_idx or name == "scan70k" else _must_equal(name, K, swapped)
    if rows is not None:
        q, d_ref, i_ref, must = q[rows], d_ref[rows], i_ref[rows], None if must is None else must[rows]
    np.testing.assert_array_equal(d, d_ref, err_msg=what)
    if must is None:
        np.testing.assert_array_equal(i, i_ref, err_msg=what)
        return
    assert i.min() >= 0 and i.max() < t.shape[0], what
    n = min(K, t.shape[0])
    dx, dy, dz = (q[:, None, a] - t[i[:, :n], a] for a in range(3))
    np.testing.assert_array_equal((dx * dx + dy * dy) + dz * dz, d_ref[:, :n], err_msg=what + " (distance of the named target)")
    np.testing.assert_array_equal(i[must], i_ref[must], err_msg=what + " (unique or coincident targets)")
    if n > 1:
        s = np.sort(i[:, :n], 1)
        assert (s[:, 1:] != s[:, :-1]).all(), what + " (a target named twice)"


def _far(dev, q, t):
    """[P1] the farthest target of every query: a chunked arg-max on the device, in blocks of as many queries as keep the
    distance matrix of a block within search_cases.MAX_ENTRIES (958 queries at 70 000 targets).  A hostile seed: which of
    several far targets it names does not matter."""
    tq, tt = _up(q, dev), _up(t, dev)
    rows = max(1, min(4096, sc.MAX_ENTRIES // t.shape[0]))
    assert rows * t.shape[0] <= sc.MAX_ENTRIES
    return torch.cat([torch.cdist(tq[r:r + rows], tt).argmax(1) for r in range(0, q.shape[0], rows)]).cpu().numpy()


# ---- a. knn_points_idx_warm -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.LARGE_NAMES)
def test_warm_search_every_seed_regime(dev, name):
    """Cold, stale, all zero, farthest target, garbage, row-mixed and the call's own seeds: indices, distances and returned
    seeds equal the oracle's, K = 1 and 3."""
    q, t = sc.large_case(name)
    refs = {K: tuple(a[None] for a in _ref(name, K)) for K in (1, 3)}
    if name == "coincident8k":
        assert not refs[1][1].any() and (refs[3][1] == np.arange(3)).all()
    _warm_all_regimes(dev, q[None], t[None], refs, name, far=_far(dev, q, t)[None])


def test_warm_search_batch_of_two(dev):
    """`scan70k` next to another generator seed of it, both cut to 69 950 queries: 1093 + 1093 query groups, no multiple of
    8 (the XCD dealing), the last group of each 2 queries short of full."""
    P1 = 69950
    q = np.stack([sc.large_case("scan70k", s)[0][:P1] for s in (0, 1)])
    t = np.stack([sc.large_case("scan70k", s)[1] for s in (0, 1)])
    assert (P1 + 63) // 64 == 1093 and (2 * 1093) % 8 == 2 and P1 % 64 == 62
    refs = {K: tuple(np.stack([_ref("scan70k", K, seed=s)[j][:P1] for s in (0, 1)]) for j in range(2)) for K in (1, 3)}
    far = np.stack([_far(dev, q[n], t[n]) for n in range(2)])
    _warm_all_regimes(dev, q, t, refs, "scan70k x 2, P1 = 69950", far=far)


# ---- b. the yardstick -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["round3", "lattice27k", "scan70k"])
def test_brute_force_yardstick(dev, name):
    """knn_points (csrc/knn.hip) at K = 1, 3, 16 and KNN(k=17) (csrc/knn_list.hip) against the oracle, bit for bit."""
    from reart_amd.knn_cuda import KNN
    from reart_amd.utils.chamfer import knn_points

    q, t = sc.large_case(name)
    tq, tt = _up(q[None], dev), _up(t[None], dev)
    for K in (1, 3, 16):
        d_ref, i_ref = _ref(name, K)
        out = knn_points(tq, tt, K=K)
        np.testing.assert_array_equal(out.idx[0].cpu().numpy(), i_ref, err_msg=f"{name} K={K}")
        np.testing.assert_array_equal(out.dists[0].cpu().numpy(), d_ref, err_msg=f"{name} K={K}")
    d_ref, i_ref = _ref(name, 17)
    d, i = KNN(k=17, transpose_mode=True, squared=True)(tt, tq)
    np.testing.assert_array_equal(i[0].cpu().numpy(), i_ref, err_msg=f"{name} KNN(k=17)")
    np.testing.assert_array_equal(d[0].cpu().numpy(), d_ref, err_msg=f"{name} KNN(k=17)")


# ---- c. ChamferLoss and ChamferPoints ---------------------------------------------------------------------------------
RATIOS = {}


def _note(key, ratio):
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"worst gradient error / bound, {key}: {RATIOS[key]:.3f}")


@pytest.mark.parametrize("kind", ["loss", "points"])
@pytest.mark.parametrize("name", sc.LARGE_NAMES)
def test_chamfer_operators(dev, name, kind):
    """ChamferLoss, and ChamferPoints in every choice of directions, with the case's clouds as x and y and the other way
    round, stored as given and in the operator's own order; cold, then the module's own seeds, then garbage seeds: the
    oracle's distances and indices (tie rules: _check), the same bits all three times, the loss within one ulp, gradients
    inside the derived bound on GRAD_CASES (ChamferPoints: upstreams in (-2, 2))."""
    rng = np.random.default_rng(3)
    for swapped in (False, True):
        x, y = _clouds(name, swapped)
        P1, P2 = x.shape[0], y.shape[0]
        g = _upstream(name, x[None], y[None])
        tx, ty = _up(x[None], dev).requires_grad_(True), _up(y[None], dev).requires_grad_(True)
        for spatial_sort in (False, True):
            for directions in (("both",) if kind == "loss" else ("both", "xy", "yx")):
                what = f"{name} {kind} swapped={swapped} spatial_sort={spatial_sort} directions={directions}"
                g_xy, g_yx = (None, None) if kind == "loss" else (g[0] if directions != "yx" else None, g[1] if directions != "xy" else None)
                mod = _cls(kind)(spatial_sort=spatial_sort)
                first = None
                for call in ("cold", "own seeds", "garbage seeds"):
                    if call == "garbage seeds":
                        mod.seed(tx, ty, *_garbage2(rng, P1, P2))
                    out = _run(kind, mod, tx, ty, None, None, dev, g_xy, g_yx, directions)
                    for dname, sw, want in (("xy", swapped, directions != "yx"), ("yx", not swapped, directions != "xy")):
                        if not want:
                            assert out["d_" + dname] is None and out["i_" + dname] is None and out["o_" + dname] is None, what
                            continue
                        _check(name, 1, sw, out["d_" + dname][0][:, None], out["i_" + dname][0][:, None], not spatial_sort, f"{what} {call} {dname}")
                        if kind == "points":
                            np.testing.assert_array_equal(out["o_" + dname], out["d_" + dname], err_msg=f"{what} {call} {dname}")
                    if first is not None:
                        _same(out, first)
                        continue
                    first = out
                    if kind == "loss":
                        _loss_ok(out, [P1], [P2])
                    if name in GRAD_CASES:      # with the oracle's indices wherever the checks above demand them
                        _note(f"{name} {kind}", _grad_ok(kind, out, x[None], y[None], [P1], [P2], g_xy, g_yx, label=what + " "))


def _points_bits(g, d, P=70000):
    """consumer_dev.h, reart_fx_bits, as chamfer_points_bwd_kernel calls it: m = max |g| sqrt(d) in float32, times 1.000002f;
    m < 2^e from its exponent field; clamp(61 - ceil(log2 P) - e, 0, 39)."""
    m = np.float32((np.abs(g).astype(np.float32) * np.sqrt(d.astype(np.float32))).max()) * np.float32(1.000002)
    e = int((np.float32(m).view(np.uint32) >> 23) & 0xff) - 126
    return int(np.clip(61 - int(np.ceil(np.log2(P))) - e, 0, 39))


@pytest.mark.parametrize("kind", ["loss", "points"])
def test_fan_in_of_70000_at_coordinates_near_600(dev, kind):
    """`fanin70k` scaled by 64 (exactly: distances x 4096): 70 000 addends of magnitude up to 2^11 leave fewer than 39
    fractional bits, clamp(61 - ceil(log2 P) - e, 0, 39) with m < 2^e the largest |coordinate| (ChamferLoss) or the largest
    |upstream| x distance (ChamferPoints, per cloud); both are asserted."""
    y, x = (np.ascontiguousarray(c * np.float32(64)) for c in sc.large_case("fanin70k"))
    m = max(np.abs(x).max(), np.abs(y).max())
    e = int(np.floor(np.log2(m))) + 1
    want_bits = int(np.clip(61 - int(np.ceil(np.log2(70000))) - e, 0, 39))
    assert want_bits < 39 and e == 10
    g = _upstream("fanin70k", x[None], y[None]) if kind == "points" else (None, None)
    for spatial_sort in (False, True):
        out = _run(kind, _cls(kind)(spatial_sort=spatial_sort), x[None], y[None], None, None, dev, *g)
        for dname, sw in (("xy", True), ("yx", False)):
            d_ref, i_ref = _ref("fanin70k", 1, sw)
            np.testing.assert_array_equal(out["d_" + dname][0], d_ref[:, 0] * np.float32(4096))
            np.testing.assert_array_equal(out["i_" + dname][0], i_ref[:, 0])
        assert np.bincount(out["i_yx"][0]).max() == 70000
        if kind == "loss":
            assert out["bits"].tolist() == [want_bits]
            _loss_ok(out, [8], [70000])
        else:
            # ChamferPoints scales a cloud's sums by m = the largest |upstream| x distance among the OTHER cloud's points,
            # times 1.000002: column 0 (sums into x, fed by the 70 000 y points at distances below 4) keeps 39 bits,
            # column 1 (sums into y, fed by the far x points) falls below
            want = [_points_bits(g[1], out["d_yx"]), _points_bits(g[0], out["d_xy"])]
            assert out["bits"].tolist() == [want] and want[0] == 39 and want[1] < 39, (out["bits"], want)
        _note(f"fanin70k x 64 {kind}", _grad_ok(kind, out, x[None], y[None], [8], [70000], *g, label=f"x 64 {kind} sort={spatial_sort} "))


@pytest.mark.parametrize("spatial_sort", [False, True])
@pytest.mark.parametrize("kind", ["loss", "points"])
def test_chamfer_ragged_batch_of_two(oracle, dev, kind, spatial_sort):
    """N = 2 padded to 70 000 with NaN: lengths (70 000, 8209) and (17, 70 000) of `scan70k`.  Live rows equal the oracle
    with lengths, element n a dense call on its trimmed clouds in every bit."""
    q, t = sc.large_case("scan70k")
    lx, ly = [70000, 17], [8209, 70000]
    x, y = np.stack([q, q]), np.stack([t, t])
    for n in range(2):
        x[n, lx[n]:] = np.nan
        y[n, ly[n]:] = np.nan
    g_xy, g_yx = _upstream("ragged", x, y) if kind == "points" else (None, None)
    out = _run(kind, _cls(kind)(spatial_sort=spatial_sort), x, y, lx, ly, dev, g_xy, g_yx)
    _exact_ragged(oracle, out, x, y, lx, ly)
    if kind == "loss":
        _loss_ok(out, lx, ly)
    _note(f"ragged {kind}", _grad_ok(kind, out, x, y, lx, ly, g_xy, g_yx, label=f"ragged {kind} sort={spatial_sort} "))
    _trimmed_equal(kind, spatial_sort, out, x, y, lx, ly, dev, g_xy, g_yx)


# ---- d. FlowTerm ------------------------------------------------------------------------------------------------------
N_FLOW = 4000


@pytest.mark.parametrize("names", [("three", "round3", "lattice27k"), ("scan70k",)], ids=["3-8208-27000", "70000"])
def test_flow_term(dev, names):
    """K = 3 over ragged reference sets: pair f searches case f's queries (cut or tiled to 4000) in case f's targets.
    cano_idx 0 and B, stored as given and in the operator's own order, cold, own and garbage seeds: distances and indices
    against the oracle (tie rules: _check); value (one ulp of the float64 sum), blended flow, mask and gradient are the
    composition's (blend_anchor_motion_batch + flow_loss + autograd) in every bit -- in both storage orders wherever no query
    has a tie between distinct targets (`scan70k`; and the triple stored as given).  The triple in the operator's own order:
    a `lattice27k` query with such a tie may blend another, equally near target's flow, so blend, mask and gradient are
    compared at every point whose pairs have no such tie (all of frames 0 and 1, a quarter of frame 2 and of the frame after
    it), and the value -- one sum over all points, tied ones included -- is not compared there."""
    from reart_amd.utils.flow_utils import FlowTerm

    B, N = len(names), N_FLOW
    lens = [_clouds(n)[1].shape[0] for n in names]
    rows = [np.arange(N) % _clouds(n)[0].shape[0] for n in names]
    queries = [_clouds(n)[0][r] for n, r in zip(names, rows)]
    rng = np.random.default_rng(6)
    complete = np.stack(queries + [(queries[-1] + rng.normal(0, 0.01, (N, 3))).astype(np.float32)])
    refs = [_up(_clouds(n)[1], dev) for n in names]
    flows = [_up(rng.normal(0, 0.02, (m, 3)).astype(np.float32), dev) for m in lens]
    untied = np.stack([_must_equal(n, 3)[r].all(1) for n, r in zip(names, rows)])        # [B,N]
    print("share of the queries without a tie among distinct targets:", dict(zip(names, untied.mean(1).round(3).tolist())))
    for c in (0, B):
        pc, cano = _up(np.concatenate((complete[:c], complete[c + 1:])), dev), _up(complete[c], dev)
        want, total = _yardstick(pc, cano, refs, flows, c, True, False)
        for spatial_sort in (False, True):
            mod = FlowTerm(refs, flows, c, knn_squared=True, spatial_sort=spatial_sort)
            for call in ("cold", "own seeds", "garbage seeds"):
                if call == "garbage seeds":          # written where the native call reads them
                    g = np.stack([rng.integers(-5, m + 6, (N, 3)) for m in lens])
                    g[:, ::3, 1] = g[:, ::3, 0]
                    mod._get_state(N, cano)["seed"].copy_(torch.from_numpy(g.astype(np.int32)))
                got = _flow_run(mod, pc, cano)
                assert got["idx"].dtype == torch.int64 and got["dists"].dtype == torch.float32
                dists, idx = got["dists"].cpu().numpy(), got["idx"].cpu().numpy()
                what = f"cano_idx={c} spatial_sort={spatial_sort} {call}"
                for f, (n, r) in enumerate(zip(names, rows)):
                    _check(n, 3, False, dists[f], idx[f], not spatial_sort, f"{n} (pair {f}) {what}", rows=r)
                if not spatial_sort or untied.all():
                    _flow_same(got, want, what=what)
                    _flow_loss_ok(got, total, what=what)
                    continue
                # the operator's own order, and a pair with ties between distinct targets: the blend, the mask and the
                # gradient are per-point quantities -- point i of frame j reads pairs j - 1 and j at point i only
                for f in range(B):
                    ok = torch.from_numpy(untied[f]).to(dev)
                    assert torch.equal(got["gt"][f][ok], want["gt"][f][ok]) and torch.equal(got["mask"][f][ok], want["mask"][f][ok]), (f, what)
                for j in range(B + 1):
                    if j == c:
                        continue
                    ok = (untied[j] if j < B else True) & (untied[j - 1] if j >= 1 else True)
                    ok = torch.from_numpy(np.broadcast_to(ok, (N,)).copy()).to(dev)
                    xi = j if j < c else j - 1
                    assert ok.any() and torch.equal(got["G"][xi][ok], want["G"][xi][ok]), (j, what)


# ---- e. the fused step ------------------------------------------------------------------------------------------------
P_ENG = 20
EDGE_N = (6704, 6720, 6992, 7008)       # 6992: the last size the cloud-resident form takes; 7008: the first it hands to the group form
EDGE_VARIANTS = (("cloud4", {"tune_cloud": 4}), ("cloud1", {"tune_cloud": 1}), ("default", {}))
WIDE_N, WIDE_B = 12304, 22
WIDE_VARIANTS = (("default", {}), ("split1", {"tune_slices": 1, "tune_cloud": 0}), ("dense", {"tune_sparse": -1}),
                 ("queue64", {"tune_sparse": 64}), ("profiled", {"profile": 1}))


@functools.lru_cache(maxsize=None)
def _instance(N, B, shift=0):
    """B = 2: the canonical cloud is N `scan70k` targets from stored row ``shift``, the frames `round3` and `scan70k` targets
    cut to N, reference sets of N and 3 points.  B = 22: every frame is the canonical region from another stored row, with
    its own drift, re-stored in k-d leaf order; reference sets of 9000 points."""
    scan, r3 = sc.large_case("scan70k")[1], sc.large_case("round3")[1]
    rng = np.random.default_rng(12)
    cano = sc.stored(scan[shift:shift + N].copy())
    if B == 2:
        pcs = np.stack([sc.stored(r3[:N].copy()), sc.stored(scan[20000:20000 + N].copy())])
        refs = [scan[:N].copy(), r3[:3].copy()]
    else:
        pcs = np.stack([sc.stored(scan[500 * b:500 * b + N] + rng.normal(0, 5e-3, 3).astype(np.float32)) for b in range(B)])
        refs = [scan[2000 * b:2000 * b + 9000].copy() for b in range(B)]
    flows = [rng.normal(0, 0.02, r.shape).astype(np.float32) for r in refs]
    return cano, pcs, refs, flows


def _engine(dev, N, B, tuning, shift=0):
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine

    cano, pcs, refs, flows = _instance(N, B, shift)
    torch.manual_seed(0)
    model = BaseModel(num_parts=P_ENG, pose_len=B).to(dev)
    with torch.no_grad():       # R = I, t = 0: the first search sees the canonical cloud itself, bit for bit
        model.proposal_6d.copy_(torch.tensor([1.0, 0, 0, 0, 1, 0], device=dev).expand_as(model.proposal_6d))
        model.proposal_t.zero_()
    return RelaxEngine(_up(cano, dev), _up(pcs, dev), model, B // 2, [_up(r, dev) for r in refs], [_up(f, dev) for f in flows],
                       n_iter=200, tuning=dict(tuning))


_BRUTE = {}


def _brute_run(dev, N, B, shift=0):
    """Iterations 1 and 3 of the cold brute-force engine (search_mode 1), once per instance."""
    if (N, B, shift) not in _BRUTE:
        run = _trajectory(_engine(dev, N, B, {"search_mode": 1}, shift))
        cano = _instance(N, B, shift)[0]
        for st in run:
            assert all(np.isfinite(v).all() for v in st.values())
        # iteration 1 moved nothing: every frame of the forward is the canonical cloud, exactly
        np.testing.assert_array_equal(run[0]["pc_trans"], np.broadcast_to(cano, run[0]["pc_trans"].shape))
        assert run[0]["adam_m"].any() and not np.array_equal(run[1]["pc_trans"], run[0]["pc_trans"])
        _BRUTE[(N, B, shift)] = run
    return _BRUTE[(N, B, shift)]


def _equal_runs(run, want, what):
    for it, (got, ref) in zip((1, 3), zip(run, want)):
        for k in ref:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{what} iteration {it}: {k}")


@pytest.mark.parametrize("N", [6720, 7008])
def test_brute_force_engine_against_the_oracle(oracle, dev, N):
    """Iteration 1 of the brute-force run: with identity poses every forward frame is the canonical cloud, so the Chamfer
    loss is the float64 sum of oracle.knn_points distances both ways over the frames, within 1e-5 relative (the bound
    tests/test_step_grad_gpu.py has for its loss row)."""
    cano, pcs, _, _ = _instance(N, 2)
    want = sum(float(oracle.knn_points(a[None], b[None], K=1)[0].astype(np.float64).sum()) for f in pcs for a, b in ((cano, f), (f, cano)))
    got = float(_brute_run(dev, N, 2)[0]["losses"][0])
    print(f"N = {N}: Chamfer loss {got!r}, oracle {want!r}, relative difference {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-5 * want


@pytest.mark.parametrize("variant,tuning", EDGE_VARIANTS, ids=[v[0] for v in EDGE_VARIANTS])
@pytest.mark.parametrize("N", EDGE_N)
def test_engine_at_the_edge_of_the_resident_form(dev, N, variant, tuning):
    """Three iterations of B = 2 frames, Chamfer + flow, P = 20: losses, first moments, forward output and labels after
    iterations 1 and 3 equal the cold brute-force run's in every bit."""
    _equal_runs(_trajectory(_engine(dev, N, 2, tuning)), _brute_run(dev, N, 2), f"N = {N} {variant}")


@pytest.mark.parametrize("variant,tuning", WIDE_VARIANTS, ids=[v[0] for v in WIDE_VARIANTS])
def test_engine_with_the_launch_order_left_alone(dev, variant, tuning):
    """N = 12 304, B = 22: 22 x 193 = 4246 (frame, group) pairs, above the 4096 up to which the launch is re-ordered; 769
    boxes are 5 coarse rounds at the default three slices and 13 at one.  The profiled run shows that the statistics counter
    (which passes 2^20 evaluations here) changes no result; the pair count it reports is not asserted."""
    assert WIDE_B * ((WIDE_N + 63) // 64) == 4246 > 4096
    _equal_runs(_trajectory(_engine(dev, WIDE_N, WIDE_B, tuning)), _brute_run(dev, WIDE_N, WIDE_B), variant)


def test_batched_engines_of_6720_points(dev):
    """Two 6720-point instances with different canonical clouds in one RelaxBatch: each leaves what its own run leaves."""
    from reart_amd.relax import RelaxBatch

    shifts = (0, 16)
    solo = [_trajectory(_engine(dev, 6720, 2, {}, s)) for s in shifts]
    engines = [_engine(dev, 6720, 2, {}, s) for s in shifts]
    batch = RelaxBatch(engines)
    batch.step(1)
    first = [_state(e) for e in engines]
    batch.step(2)
    last = [_state(e) for e in engines]
    for k in range(2):
        assert np.isfinite(solo[k][1]["losses"]).all()
        _equal_runs((first[k], last[k]), solo[k], f"copy {k}")
    assert not np.array_equal(solo[0][1]["adam_m"], solo[1][1]["adam_m"])
