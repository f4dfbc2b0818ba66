"""The fixed part of a search wave (prune.hip): the (batch, query group) pair split by a reciprocal, frame bases as 32-bit
products, the neighbour-seed bounds of the workgroup's waves exchanged by fixed-offset reads, the row summaries in one DPP
block, the seed count taken in the loop.  None of it may change a decision, so every case compares the fused pruned step with
the brute-force step (`search_mode` 1) of the same engine bit for bit after 6 iterations -- loss log, forward output, part
labels, the five parameter tensors -- and the flow neighbour indices with those of the other pruned runs of its shape.

Shape: N = 330 -- six query groups (not a power of two: a wrong reciprocal shows), the last with 10 live lanes (the clamped lanes
of a partial row box).  T = 4 and T = 6: G = 18 and 30 pairs, no multiples of 8, so padding positions exist.  Reference sets of
3 / 17 / 40 (/ 5 / 33) points: exactly K, one box + 1, more than two boxes, fewer than a box, two boxes + 1.  The flow job's seeds
are garbage before the first step (-1, an index >= the frame's count, two equal indices), as in test_search_head_gpu.py.

Two forms of the kernel are taken by very large shapes only -- frame offsets as 64-bit products (an array of 2^31 bytes or more:
no test shape comes near) and launch positions read through the order array and the query map instead of item words (more than
2^21 - 1 pairs or 2 047 frames: beyond what an engine accepts).  `search_mode` 2 / 3 / 4 select them at any shape (the first, the
second, both): those cases run the `OFF32 = false` instantiations and the scalar loads of `border[pos]` and `qmap[b]`.  The
stand-alone warm operators pass neither item words nor the two arrays: their pair is the launch position and their query frame
the batch.

Four engines (GOLDEN_CASES) also demand the executed pairs of each of their first three search launches as the library of the
commit BEFORE this part of the kernel changed reported them (tests/golden/search_fixed_parent.npz, written by
tools/record_search_fixed_golden.py from that library on an MI355X): executed pairs are a checksum of every filter decision and
of the statistics counter's seed term."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_fixed_parent.npz")
N, P, ITERS = 330, 8, 6
LENS = {4: (3, 17, 40), 6: (3, 17, 40, 5, 33)}
BRUTE = {"search_mode": 1}
GROUP = {"tune_cloud": 0}
SLICES = (1, 2, 3, 4)
GOLDEN_CASES = {
    "t4_waves3_flow3": (4, dict(GROUP, tune_slices=3, tune_slices_flow=3)),
    "t4_waves2_flow4": (4, dict(GROUP, tune_slices=2, tune_slices_flow=4)),
    "t6_waves4_flow1": (6, dict(GROUP, tune_slices=4, tune_slices_flow=1)),
    "t6_cloud": (6, {"tune_cloud": 1}),
}
_cache = {}


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _data(T, seed=5):
    B, lens = T - 1, LENS[T]
    rng = np.random.default_rng(seed)
    cano = rng.uniform(-0.3, 0.3, (N, 3)).astype(np.float32)
    pcs = (cano[None] + rng.normal(0, 0.02, (B, N, 3))).astype(np.float32)
    refs = [rng.uniform(-0.3, 0.3, (m, 3)).astype(np.float32) for m in lens]
    flows = [rng.normal(0, 0.02, (m, 3)).astype(np.float32) for m in lens]
    return cano, pcs, refs, flows


def _seed3(eng, B):
    """The flow job's warm-start seeds [B, N, 3] inside the workspace: the only run of B*N*3 int32 that `prepare` has just
    filled with 0, 1, 2, 0, 1, 2, ... (blocks of the workspace start at multiples of 256 bytes)."""
    ws = eng.workspace.view(torch.int32)
    n = B * N * 3
    want = (torch.arange(n, device=ws.device) % 3).to(torch.int32)
    starts = torch.arange(0, ws.numel() - n + 1, 64, device=ws.device)
    head = ws[starts[:, None] + torch.arange(6, device=ws.device)[None]]
    hits = [int(s) for s in starts[(head == want[:6]).all(1)].tolist() if torch.equal(ws[s:s + n], want)]
    assert len(hits) == 1, hits
    return ws[hits[0]:hits[0] + n].view(B, N, 3)


def _garbage(seeds, lens):
    """Unusable seeds, three kinds in turn, and one lane in four left usable (rows of 16 lanes then mix both)."""
    g = seeds.clone()
    ln = torch.tensor(lens, device=g.device, dtype=torch.int32)
    g[:, 0::4, 0] = -1
    g[:, 1::4, 2] = ln[:, None] + torch.arange(g[:, 1::4].shape[1], device=g.device, dtype=torch.int32)[None] % 3
    g[:, 2::4, 1] = g[:, 2::4, 0]
    seeds.copy_(g)


def _engine(dev, T, tuning, cano_idx=1, model_seed=0, data_seed=5, profile=False):
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine

    cano, pcs, refs, flows = _data(T, data_seed)
    torch.manual_seed(model_seed)
    model = BaseModel(num_parts=P, pose_len=T - 1).to(dev)
    eng = RelaxEngine(t(cano, dev), t(pcs, dev), model, cano_idx, [t(r, dev) for r in refs], [t(f, dev) for f in flows],
                      n_iter=100, seed=7, tuning=dict(tuning), profile=profile)
    seeds = None
    if tuning != BRUTE:
        seeds = _seed3(eng, T - 1)
        _garbage(seeds, LENS[T])
    return eng, model, seeds


def _state(eng, seeds=None):
    it, log = eng.loss_log()
    assert it == ITERS
    out = [log.cpu().numpy(), eng.pc_trans.cpu().numpy().copy(), eng.seg_part.cpu().numpy().copy()]
    out += [p.detach().cpu().numpy().copy() for p in eng.params]
    assert len(out) == 8
    return out, None if seeds is None else seeds.cpu().numpy().copy()


def _brute(dev, T, cano_idx=1, model_seed=0, data_seed=5):
    key = ("brute", T, cano_idx, model_seed, data_seed)
    if key not in _cache:
        eng, model, _ = _engine(dev, T, BRUTE, cano_idx, model_seed, data_seed)
        eng.step(ITERS)
        out, _ = _state(eng)
        assert np.isfinite(out[0]).all()
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _check(dev, T, out, nbr, what, **kw):
    want = _brute(dev, T, **kw)
    for k, (a, b) in enumerate(zip(out, want)):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: output {k} against brute force")
    # what the consumer left for the next search: three distinct valid indices per query, nothing of the garbage
    ln = np.array(LENS[T])[:, None, None]
    assert (nbr >= 0).all() and (nbr < ln).all()
    assert (nbr[..., 0] != nbr[..., 1]).all() and (nbr[..., 1] != nbr[..., 2]).all() and (nbr[..., 0] != nbr[..., 2]).all()
    # ... and the same ones whatever form the search took (the first pruned run of the shape is kept)
    key = ("nbr", T) + tuple(sorted(kw.items()))
    first = _cache.setdefault(key, (what, nbr))
    np.testing.assert_array_equal(nbr, first[1], err_msg=f"{what}: flow neighbour indices against {first[0]}")


def run_golden_case(dev, case, **more):
    """(outputs, flow neighbours, executed pairs of launches 1, 2, 3) -- tools/record_search_fixed_golden.py calls this too."""
    T, tuning = GOLDEN_CASES[case]
    eng, model, seeds = _engine(dev, T, dict(tuning, **more), profile=True)
    pairs, done = [], 0
    for k in range(3):
        eng.step(1)
        prof = eng.search_profile()
        assert prof["launches"] == k + 1
        pairs.append(prof["pairs"] - done)
        done = prof["pairs"]
    eng.step(ITERS - 3)
    out, nbr = _state(eng, seeds)
    return out, nbr, np.array(pairs, dtype=np.int64)


@pytest.mark.parametrize("flow", SLICES)
@pytest.mark.parametrize("waves", SLICES)
def test_every_pair_of_wave_counts_equals_brute_force(dev, waves, flow):
    """The exchange and the merge for every S; S1 != S3: the waves >= S of the narrower kind leave before the exchange's barrier."""
    eng, model, seeds = _engine(dev, 4, dict(GROUP, tune_slices=waves, tune_slices_flow=flow))
    eng.step(ITERS)
    out, nbr = _state(eng, seeds)
    _check(dev, 4, out, nbr, f"waves {waves} flow {flow}")


@pytest.mark.parametrize("name,T,tuning", [
    ("six_frames", 6, dict(GROUP)),
    ("own_seeds_only", 6, dict(GROUP, tune_share=-1)),
    ("row_seeds_no_exchange", 6, dict(GROUP, tune_share=1)),
    ("own_seeds_only_four_waves", 4, dict(GROUP, tune_share=-1, tune_slices=4, tune_slices_flow=2)),
    ("row_seeds_no_exchange_two_waves", 4, dict(GROUP, tune_share=1, tune_slices=2, tune_slices_flow=3)),
    ("xcd_chunks", 6, dict(GROUP, tune_xcd=1)),
    ("xcd_chunks_t4", 4, dict(GROUP, tune_xcd=1, tune_slices=4)),
    ("cloud_form", 4, {"tune_cloud": 1}),
    ("cloud_form_t6", 6, {"tune_cloud": 1}),
    ("cloud_form_four_slices", 6, {"tune_cloud": 4}),
    # the forms of very large shapes, forced (module docstring): 64-bit frame offsets | order array + query map | both
    ("wide_offsets", 6, dict(GROUP, search_mode=2)),
    ("wide_offsets_four_waves", 4, dict(GROUP, search_mode=2, tune_slices=4, tune_slices_flow=2)),
    ("wide_offsets_own_seeds_only", 4, dict(GROUP, search_mode=2, tune_share=-1, tune_slices=1)),
    ("order_array_and_query_map", 6, dict(GROUP, search_mode=3)),
    ("order_array_and_query_map_xcd_chunks", 4, dict(GROUP, search_mode=3, tune_xcd=1, tune_slices=2)),
    ("order_array_static_order", 6, dict(GROUP, search_mode=3, tune_reorder=-1)),
    ("order_array_cloud_form", 4, {"tune_cloud": 1, "search_mode": 3}),
    ("wide_offsets_and_order_array", 6, dict(GROUP, search_mode=4)),
])
def test_seed_sharing_layouts_and_forms_equal_brute_force(dev, name, T, tuning):
    eng, model, seeds = _engine(dev, T, tuning)
    eng.step(ITERS)
    out, nbr = _state(eng, seeds)
    _check(dev, T, out, nbr, name)


@pytest.mark.parametrize("mode", [0, 4])
def test_two_instances_in_one_launch_equal_brute_force(dev, mode):
    """RelaxBatch: the BATCH = true instantiations of the kernel, with 32-bit frame offsets and item words (0) and with 64-bit
    offsets, the order array and the query map (`search_mode` 4)."""
    from reart_amd.relax import RelaxBatch

    specs = [dict(cano_idx=0, model_seed=0, data_seed=5), dict(cano_idx=3, model_seed=1, data_seed=6)]
    made = [_engine(dev, 6, dict(GROUP, search_mode=mode), **s) for s in specs]
    RelaxBatch([e for e, _, _ in made]).step(ITERS)
    for s, (eng, model, seeds) in zip(specs, made):
        out, nbr = _state(eng, seeds)
        _check(dev, 6, out, nbr, f"batched {s}", **s)


@pytest.mark.parametrize("case", sorted(GOLDEN_CASES))
def test_first_three_launches_execute_the_parents_pairs(dev, case):
    T, _ = GOLDEN_CASES[case]
    out, nbr, pairs = run_golden_case(dev, case)
    _check(dev, T, out, nbr, case)
    gold = np.load(GOLDEN)
    print(f"{case}: pairs {pairs.tolist()} (parent {gold[f'{case}__pairs'].tolist()})")
    np.testing.assert_array_equal(nbr, gold[f"{case}__flow_neighbours"], err_msg=f"{case}: flow neighbour indices")
    assert (gold[f"{case}__pairs"] > 0).all()
    np.testing.assert_array_equal(pairs, gold[f"{case}__pairs"])


@pytest.mark.parametrize("case,mode", [("t4_waves3_flow3", 4), ("t4_waves2_flow4", 2), ("t6_waves4_flow1", 3)])
def test_forced_forms_execute_the_parents_pairs(dev, case, mode):
    """64-bit offsets and the order array change where a wave reads, not what it decides: the same pairs per launch."""
    T, _ = GOLDEN_CASES[case]
    out, nbr, pairs = run_golden_case(dev, case, search_mode=mode)
    _check(dev, T, out, nbr, f"{case} search_mode {mode}")
    gold = np.load(GOLDEN)
    print(f"{case} search_mode {mode}: pairs {pairs.tolist()} (parent {gold[f'{case}__pairs'].tolist()})")
    np.testing.assert_array_equal(nbr, gold[f"{case}__flow_neighbours"], err_msg=f"{case}: flow neighbour indices")
    np.testing.assert_array_equal(pairs, gold[f"{case}__pairs"])


def test_warm_chamfer_operator_equals_the_brute_force_operator(dev):
    """The stand-alone warm operator passes no item words, no order array and no query map: the pair is the launch position,
    the query frame the batch (the third way through the head of a workgroup).  Three calls on a moving x (cold, warm, warm) against knn_points in both directions, bit for bit."""
    from reart_amd.utils.chamfer import ChamferLoss, knn_points

    rng = np.random.default_rng(9)
    base = rng.uniform(-0.3, 0.3, (3, N, 3)).astype(np.float32)
    y = t(base + rng.normal(0, 0.02, base.shape).astype(np.float32), dev)
    mod = ChamferLoss(spatial_sort=False)
    for k in range(3):
        x = t(base + rng.normal(0, 0.01 * (k + 1), base.shape).astype(np.float32), dev)
        loss = mod(x, y)
        d_xy, i_xy, d_yx, i_yx = mod.last
        fwd, bwd = knn_points(x, y, K=1), knn_points(y, x, K=1)
        assert torch.isfinite(loss)
        assert torch.equal(d_xy, fwd.dists[..., 0]) and torch.equal(i_xy, fwd.idx[..., 0]), f"call {k}: x -> y"
        assert torch.equal(d_yx, bwd.dists[..., 0]) and torch.equal(i_yx, bwd.idx[..., 0]), f"call {k}: y -> x"
