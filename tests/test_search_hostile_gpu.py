"""GPU: the exact box-pruned searches (csrc/prune.hip) on the hostile geometry of tests/search_cases.py, through every
caller -- knn_points_idx_warm, ChamferLoss, ChamferPoints, FlowTerm, the fused step (RelaxEngine, RelaxBatch) -- and every
form the engine can select, under every seed regime.  Everything is compared bit for bit with the brute-force contract
(oracle.knn_points); there is no tolerance in this file except the one the two ``bwd*`` engine variants already have.
That holds for `tiny70` (squares are denormal numbers) too: the build keeps float32 denormal numbers in every kernel."""
import functools

import numpy as np
import pytest
import torch

from tests import search_cases as sc

pytestmark = pytest.mark.gpu


def _up(a, dev):
    return torch.tensor(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _ref(name, K, swapped=False, seed=0):
    """oracle.knn_points of one case (queries -> targets, or the other way round): (dists [P1,K], idx [P1,K]), computed once."""
    import oracle

    q, t = sc.case(name, seed)[::-1] if swapped else sc.case(name, seed)
    d, i = oracle.knn_points(q[None], t[None], K=K)
    d, i = d[0], i[0]
    d.setflags(write=False)
    i.setflags(write=False)
    return d, i


# ---- a. knn_points_idx_warm -------------------------------------------------------------------------------------------
def _regimes(q, t, i_ref, rng, far=None):
    """Seed arrays [N,P1,K] (None: cold) by name, for batched clouds q [N,P1,3], t [N,P2,3] with exact neighbours i_ref.
    ``far`` [N,P1]: the farthest target of every query where the caller has it already (large clouds: a chunked arg-max)."""
    N, P1, K = i_ref.shape
    P2 = t.shape[1]
    if far is None:
        far = np.stack([sc.sqdist(q[n], t[n]).argmax(1) for n in range(N)])        # [N,P1]
    garbage = rng.integers(-5, P2 + 5, (N, P1, K))
    garbage[:, ::3, :] = 0                                                         # repeats inside a query
    mixed = rng.integers(-5, P2 + 5, (N, P1, K))
    mixed[:, 1::2, :] = mixed[:, 1::2, :1]
    lanes = np.arange(P1)
    exact = (lanes % 16) == ((lanes // 16) * 7 + 3) % 16                           # one lane of every row of 16
    mixed[:, exact] = i_ref[:, exact]
    return {"cold": None, "stale": np.roll(i_ref, 37, axis=1), "zero": np.zeros((N, P1, K), np.int64),
            "farthest": np.repeat(far[..., None], K, -1), "garbage": garbage, "row-mixed": mixed}


def _warm(dev, tq, tt, K, seed, d_ref, i_ref, what):
    from reart_amd.chamferdist_C import knn_points_idx_warm

    ts = None if seed is None else torch.from_numpy(np.ascontiguousarray(seed, dtype=np.int32)).to(dev)
    idx, dists, ts = knn_points_idx_warm(tq, tt, K, ts)
    np.testing.assert_array_equal(idx.cpu().numpy(), i_ref, err_msg=what)
    np.testing.assert_array_equal(dists.cpu().numpy(), d_ref, err_msg=what)
    want = i_ref.astype(np.int32)
    want[..., min(K, tt.shape[1]):] = -1             # a slot without a target: the oracle leaves 0, the seed says "none"
    np.testing.assert_array_equal(ts.cpu().numpy(), want, err_msg=what + " (returned seeds)")
    return ts


def _warm_all_regimes(dev, q, t, refs, label, far=None):
    """q [N,P1,3], t [N,P2,3]; refs {K: (d [N,P1,K], i [N,P1,K])}; far: see _regimes."""
    tq, tt = _up(q, dev), _up(t, dev)
    for K in (1, 3):
        d_ref, i_ref = refs[K]
        rng = np.random.default_rng(K)
        own = None
        for regime, seed in _regimes(q, t, i_ref, rng, far).items():
            ts = _warm(dev, tq, tt, K, seed, d_ref, i_ref, f"{label} K={K} seeds: {regime}")
            own = ts if own is None else own
        _warm(dev, tq, tt, K, own.cpu().numpy(), d_ref, i_ref, f"{label} K={K} seeds: the call's own")


@pytest.mark.parametrize("name", sc.NAMES)
def test_warm_search_every_seed_regime(dev, name):
    """Cold, the call's own result, stale (the neighbours of the query 37 rows away), all zero, all at the farthest target,
    garbage (-5 .. P2 + 5 with repeats) and row-mixed seeds (one lane of every 16 exact, fifteen garbage): indices,
    distances and returned seeds equal the oracle's, K = 1 and 3."""
    q, t = sc.case(name)
    refs = {K: tuple(a[None] for a in _ref(name, K)) for K in (1, 3)}
    _warm_all_regimes(dev, q[None], t[None], refs, name)


@pytest.mark.parametrize("P1", [1000, 900])
def test_warm_search_batch_of_three(dev, P1):
    """`jump` as a batch of three, element 1 from another generator seed.  1000 queries are 16 groups per element, 48 in
    all; cut to 900 they are 15 and 45, which is no multiple of 8 (the XCD dealing)."""
    seeds = (0, 1, 0)
    q = np.stack([sc.case("jump", s)[0][:P1] for s in seeds])
    t = np.stack([sc.case("jump", s)[1] for s in seeds])
    assert (3 * ((P1 + 63) // 64)) % 8 == (0 if P1 == 1000 else 5)
    refs = {K: tuple(np.stack([_ref("jump", K, seed=s)[j][:P1] for s in seeds]) for j in range(2)) for K in (1, 3)}
    _warm_all_regimes(dev, q, t, refs, f"jump x 3, P1 = {P1}")


# ---- b. ChamferLoss and ChamferPoints ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _must_equal(name, K, swapped=False):
    """[P1,K] bool: slots where any exact search must name the oracle's target -- it is the only target at that distance, or
    every target at that distance coincides with it (copies of a point keep the caller's order in every storage order)."""
    q, t = sc.case(name)[::-1] if swapped else sc.case(name)
    d_ref, i_ref = _ref(name, K, swapped)
    D = sc.sqdist(q, t)
    out = np.zeros(i_ref.shape, bool)
    for k in range(min(K, t.shape[0])):
        tied = D == d_ref[:, k, None]
        same = (t[None] == t[i_ref[:, k]][:, None]).all(-1)
        out[:, k] = (~tied | same).all(1)
    return out


def _check_search(name, K, swapped, d, i, exact_idx, what):
    """d [P1,K], i [P1,K] of one direction against the oracle; with ``exact_idx`` False (a storage order of the operator's
    own) the tie rule between DISTINCT equidistant targets differs: the index must still attain the distance exactly."""
    q, t = sc.case(name)[::-1] if swapped else sc.case(name)
    d_ref, i_ref = _ref(name, K, swapped)
    np.testing.assert_array_equal(d, d_ref, err_msg=what)
    if exact_idx:
        np.testing.assert_array_equal(i, i_ref, err_msg=what)
        return
    assert i.min() >= 0 and i.max() < t.shape[0], what
    n = min(K, t.shape[0])
    dx, dy, dz = (q[:, None, a] - t[i[:, :n], a] for a in range(3))
    np.testing.assert_array_equal((dx * dx + dy * dy) + dz * dz, d_ref[:, :n], err_msg=what + " (distance of the named target)")
    must = _must_equal(name, K, swapped)
    np.testing.assert_array_equal(i[must], i_ref[must], err_msg=what + " (unique or coincident targets)")
    if n > 1:
        s = np.sort(i[:, :n], 1)
        assert (s[:, 1:] != s[:, :-1]).all(), what + " (a target named twice)"


def _garbage2(rng, P1, P2):
    g_xy, g_yx = rng.integers(-5, P2 + 5, (1, P1)), rng.integers(-5, P1 + 5, (1, P2))
    g_xy[:, ::3], g_yx[:, ::3] = 0, 0
    return torch.from_numpy(g_xy), torch.from_numpy(g_yx)


def _orders(name):
    q, t = sc.case(name)
    return (False, True) if q.shape[0] != t.shape[0] else (False,)


def _same(a, b, what):
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _np(v):
    return None if v is None else v.detach().cpu().numpy()


@pytest.mark.parametrize("name", sc.NAMES)
def test_chamfer_loss(dev, name):
    """Both directions of ChamferLoss with the case's clouds as x and y and the other way round, stored as given and in the
    operator's own order; cold, then the module's own seeds, then garbage seeds: the same bits all three times."""
    from reart_amd.utils.chamfer import ChamferLoss

    rng = np.random.default_rng(3)
    for swapped in _orders(name):
        x, y = sc.case(name)[::-1] if swapped else sc.case(name)
        for spatial_sort in (False, True):
            what = f"{name} swapped={swapped} spatial_sort={spatial_sort}"
            mod = ChamferLoss(spatial_sort=spatial_sort)
            tx, ty = _up(x[None], dev).requires_grad_(True), _up(y[None], dev).requires_grad_(True)
            first = None
            for call in ("cold", "own seeds", "garbage seeds"):
                if call == "garbage seeds":
                    mod.seed(tx, ty, *_garbage2(rng, x.shape[0], y.shape[0]))
                tx.grad = ty.grad = None
                loss = mod(tx, ty)
                loss.backward()
                out = dict(zip(("d_xy", "i_xy", "d_yx", "i_yx"), map(_np, mod.last)), loss=_np(loss), gx=_np(tx.grad), gy=_np(ty.grad))
                _check_search(name, 1, swapped, out["d_xy"][0][:, None], out["i_xy"][0][:, None], not spatial_sort, f"{what} {call} xy")
                _check_search(name, 1, not swapped, out["d_yx"][0][:, None], out["i_yx"][0][:, None], not spatial_sort, f"{what} {call} yx")
                if first is None:
                    first = out
                else:
                    _same(out, first, f"{what} {call}")


@pytest.mark.parametrize("name", sc.NAMES)
def test_chamfer_points(dev, name):
    """ChamferPoints, directions both / xy / yx, as test_chamfer_loss; the returned distances are the oracle's too."""
    from reart_amd.utils.chamfer import ChamferPoints

    rng = np.random.default_rng(4)
    for swapped in _orders(name):
        x, y = sc.case(name)[::-1] if swapped else sc.case(name)
        tx, ty = _up(x[None], dev).requires_grad_(True), _up(y[None], dev).requires_grad_(True)
        for spatial_sort in (False, True):
            for directions in ("both", "xy", "yx"):
                what = f"{name} swapped={swapped} spatial_sort={spatial_sort} directions={directions}"
                mod = ChamferPoints(spatial_sort=spatial_sort)
                first = None
                for call in ("cold", "own seeds", "garbage seeds"):
                    if call == "garbage seeds":
                        mod.seed(tx, ty, *_garbage2(rng, x.shape[0], y.shape[0]))
                    tx.grad = ty.grad = None
                    o_xy, o_yx = mod(tx, ty, directions)
                    sum(o.sum() for o in (o_xy, o_yx) if o is not None).backward()
                    out = dict(zip(("d_xy", "i_xy", "d_yx", "i_yx"), map(_np, mod.last)), o_xy=_np(o_xy), o_yx=_np(o_yx),
                               gx=_np(tx.grad), gy=_np(ty.grad))
                    for dname, sw, want in (("xy", swapped, directions != "yx"), ("yx", not swapped, directions != "xy")):
                        if not want:
                            assert out["d_" + dname] is None and out["i_" + dname] is None and out["o_" + dname] is None, what
                            continue
                        _check_search(name, 1, sw, out["d_" + dname][0][:, None], out["i_" + dname][0][:, None], not spatial_sort,
                                      f"{what} {call} {dname}")
                        np.testing.assert_array_equal(out["o_" + dname], out["d_" + dname], err_msg=f"{what} {call} {dname}")
                    if first is None:
                        first = out
                    else:
                        _same(out, first, f"{what} {call}")


# ---- c. FlowTerm ------------------------------------------------------------------------------------------------------
#          three cases whose targets are the reference sets (one below 64, one above 1024 points), the common N
TRIPLES = [(("small_65x63", "lattice", "coincident"), 700), (("jump", "small_64x17", "line"), 513),
           (("sheet", "offset", "small_64x3"), 330), (("small_65x8", "sphere", "tiny70"), 650), (("cluster", "small_3x16", "big"), 800)]


@pytest.mark.parametrize("names,N", TRIPLES, ids=["-".join(n) for n, _ in TRIPLES])
def test_flow_term(dev, names, N):
    """K = 3 over ragged reference sets: pair f searches case f's queries (cut or tiled to N) in case f's targets.  Cold,
    random valid and garbage seeds, cano_idx 0 and B, stored as given and in the operator's own order."""
    from reart_amd.utils.flow_utils import FlowTerm

    B = len(names)
    lens = [sc.case(n)[1].shape[0] for n in names]
    assert len(set(lens)) == B and min(lens) < 64 and max(lens) > 1024
    rows = [np.arange(N) % sc.case(n)[0].shape[0] for n in names]
    queries = [sc.case(n)[0][r] for n, r in zip(names, rows)]
    rng = np.random.default_rng(6)
    complete = np.stack(queries + [(queries[-1] + rng.normal(0, 0.01, (N, 3))).astype(np.float32)])
    refs = [_up(sc.case(n)[1], dev) for n in names]
    flows = [_up(rng.normal(0, 0.02, (m, 3)).astype(np.float32), dev) for m in lens]
    for c in (0, B):
        pc, cano = _up(np.concatenate((complete[:c], complete[c + 1:])), dev), _up(complete[c], dev)
        for spatial_sort in (False, True):
            mod = FlowTerm(refs, flows, c, knn_squared=True, spatial_sort=spatial_sort)
            for call in ("cold", "random seeds", "garbage seeds"):
                if call == "random seeds":
                    mod.seed(cano, torch.from_numpy(np.stack([rng.integers(0, m, (N, 3)) for m in lens])).to(dev))
                elif call == "garbage seeds":        # written where the native call reads them
                    g = np.stack([rng.integers(-5, m + 6, (N, 3)) for m in lens])
                    g[:, ::3, 1] = g[:, ::3, 0]
                    mod._get_state(N, cano)["seed"].copy_(torch.from_numpy(g.astype(np.int32)))
                with torch.no_grad():
                    mod(pc, cano)
                gt, mask, dists, idx = mod.last
                assert idx.dtype == torch.int64 and dists.dtype == torch.float32
                dists, idx = dists.cpu().numpy(), idx.cpu().numpy()
                for f, (n, r) in enumerate(zip(names, rows)):
                    # every query row r of the case: tiling and cutting repeat / drop rows of the cached reference
                    d_ref, i_ref = (a[r] for a in _ref(n, 3))
                    what = f"{n} (pair {f}) cano_idx={c} spatial_sort={spatial_sort} {call}"
                    np.testing.assert_array_equal(dists[f], d_ref, err_msg=what)
                    if not spatial_sort:
                        np.testing.assert_array_equal(idx[f], i_ref, err_msg=what)
                        continue
                    q, t = sc.case(n)[0][r], sc.case(n)[1]
                    dx, dy, dz = (q[:, None, a] - t[idx[f], a] for a in range(3))
                    np.testing.assert_array_equal((dx * dx + dy * dy) + dz * dz, d_ref, err_msg=what + " (distance of the named target)")
                    must = _must_equal(n, 3)[r]
                    np.testing.assert_array_equal(idx[f][must], i_ref[must], err_msg=what + " (unique or coincident targets)")
                    s = np.sort(idx[f], 1)
                    assert (s[:, 1:] != s[:, :-1]).all(), what + " (a target named twice)"


# ---- d. the engine's forms, in situ -----------------------------------------------------------------------------------
N_ENG, P_ENG, B_ENG, CANO_IDX = 1100, 12, 4, 2
VARIANTS = (("pruned", {}), ("cloud1", {"tune_cloud": 1}), ("cloud2_dense", {"tune_cloud": 2, "tune_sparse": -1}), ("cloud8", {"tune_cloud": 8}),
            ("global_targets", {"tune_cloud": 0}), ("global_dense", {"tune_cloud": 0, "tune_sparse": -1}), ("dense", {"tune_sparse": -1}),
            ("sparse8", {"tune_sparse": 8}), ("sparse3", {"tune_sparse": 3}), ("queue64", {"tune_sparse": 64}),
            ("split1", {"tune_slices": 1, "tune_cloud": 0}), ("split2_flow4", {"tune_slices": 2, "tune_slices_flow": 4, "tune_cloud": 0}),
            ("split4_dense", {"tune_slices": 4, "tune_sparse": -1, "tune_cloud": 0}), ("static_order", {"tune_reorder": -1, "tune_cloud": 0}),
            ("xcd_chunks", {"tune_xcd": 1, "tune_cloud": 0}), ("profiled", {"profile": 1}), ("fwd64", {"tune_fwd_pts": 64}),
            ("bwd64", {"tune_bwd_pts": 64}), ("bwd16", {"tune_bwd_pts": 16}), ("share_off", {"tune_share": -1}), ("share_on", {"tune_share": 1}))


@functools.lru_cache(maxsize=None)
def _instance(shift=0):
    """Hostile frames for the fused step: the canonical cloud is N lattice points (from stored row ``shift``), the four frames
    are lattice, sheet, cluster + outliers and jump targets cut to N; reference sets of 40, 700, 1100 and 3 points.
    The lattice frame sits half a step off the canonical one, as the `lattice` case's queries do: a canonical point then has
    up to eight nearest frame points and the other way round (the very same lattice would give unique exact hits only;
    those are left to the first reference set, which is 40 canonical points)."""
    cut = lambda n, o=0: sc.case(n)[1][o:o + N_ENG]
    cano = cut("lattice", shift)
    pcs = np.stack([cut("lattice") + np.float32(0.025), cut("sheet"), cut("cluster"), cut("jump")])
    rng = np.random.default_rng(12)
    refs = [sc.case(n)[1][:m].copy() for n, m in (("lattice", 40), ("sheet", 700), ("cluster", 1100), ("jump", 3))]
    flows = [rng.normal(0, 0.02, r.shape).astype(np.float32) for r in refs]
    return cano, pcs, refs, flows


def _engine(dev, tuning, shift=0):
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine

    cano, pcs, refs, flows = _instance(shift)
    torch.manual_seed(0)
    model = BaseModel(num_parts=P_ENG, pose_len=B_ENG).to(dev)
    with torch.no_grad():       # R = I, t = 0: the first search sees the canonical lattice itself, bit for bit
        model.proposal_6d.copy_(torch.tensor([1.0, 0, 0, 0, 1, 0], device=dev).expand_as(model.proposal_6d))
        model.proposal_t.zero_()
    return RelaxEngine(_up(cano, dev), _up(pcs, dev), model, CANO_IDX, [_up(r, dev) for r in refs], [_up(f, dev) for f in flows],
                       n_iter=200, tuning=dict(tuning))


def _state(eng):
    return {"losses": eng.last_losses().cpu().numpy(), "adam_m": eng.adam_m.cpu().numpy().copy(),
            "pc_trans": eng.pc_trans.cpu().numpy().copy(), "seg_part": eng.seg_part.cpu().numpy().copy()}


def _trajectory(eng):
    """States after iteration 1 and after iteration 3."""
    eng.step(1)
    first = _state(eng)
    eng.step(2)
    return first, _state(eng)


@pytest.fixture(scope="module")
def brute_run(dev):
    run = _trajectory(_engine(dev, {"search_mode": 1}))
    cano = _instance()[0]
    for st in run:
        assert all(np.isfinite(v).all() for v in st.values())
    # iteration 1 moved nothing: every frame of the forward is the canonical lattice, exactly
    np.testing.assert_array_equal(run[0]["pc_trans"], np.broadcast_to(cano, run[0]["pc_trans"].shape))
    assert run[0]["adam_m"].any() and not np.array_equal(run[1]["pc_trans"], run[0]["pc_trans"])
    return run


@pytest.mark.parametrize("name,tuning", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_engine_forms_on_hostile_frames(dev, brute_run, name, tuning):
    """Three iterations of one instance per search form; losses, first moments, forward output and labels after iterations
    1 and 3 equal the cold brute-force run's in every bit (the bwd* variants add the same sums in another order)."""
    run = _trajectory(_engine(dev, tuning))
    for it, (got, want) in zip((1, 3), zip(run, brute_run)):
        for k in want:
            if name.startswith("bwd"):
                np.testing.assert_allclose(got[k], want[k], rtol=2e-5, atol=2e-6, err_msg=f"{name} iteration {it}: {k}")
            else:
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name} iteration {it}: {k}")


def test_batched_engines_on_hostile_frames(dev):
    """Three copies of the instance with different canonical clouds in one RelaxBatch (the batched group kernel): each
    leaves what its own single-engine run leaves."""
    from reart_amd.relax import RelaxBatch

    shifts = (0, 16, 23)
    solo = [_trajectory(_engine(dev, {}, s)) for s in shifts]
    engines = [_engine(dev, {}, s) for s in shifts]
    batch = RelaxBatch(engines)
    batch.step(1)
    first = [_state(e) for e in engines]
    batch.step(2)
    last = [_state(e) for e in engines]
    for k, s in enumerate(shifts):
        for it, got, want in ((1, first[k], solo[k][0]), (3, last[k], solo[k][1])):
            assert np.isfinite(want["losses"]).all()
            for key in want:
                np.testing.assert_array_equal(got[key], want[key], err_msg=f"copy {k} iteration {it}: {key}")
    assert not np.array_equal(solo[0][1]["adam_m"], solo[1][1]["adam_m"])
