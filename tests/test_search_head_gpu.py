"""The head of a search workgroup (prune.hip): item word, the job's arguments by value, query and seeds in one batch, every
seed target in flight before the first LDS store.  Nothing it computes may change, so every case compares the fused pruned
step with the brute-force step of the same engine, bit for bit: loss log, forward output, part labels and all five parameter
tensors (what the searches found decides every one of them), and between pruned runs also the flow neighbour indices.

Shape: T = 4 (B = 3), N = 200 -- four query groups, the last with 8 live lanes; G = 12 pairs is no multiple of 8, so four launch
positions are padding and must leave without reading an item word out of range.  Reference sets of 3, 17 and 40 points: exactly
K, one box + 1, more than two boxes (the target count per frame).  The flow job's seeds are garbage before the first step:
-1, an index >= the frame's count, two equal indices -- the lanes whose unconditional gather reads index 0 and parks +inf."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, P, B, LENS, ITERS = 200, 8, 3, (3, 17, 40), 6
BRUTE = {"search_mode": 1}
_cache = {}


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _data(seed=5):
    rng = np.random.default_rng(seed)
    cano = rng.uniform(-0.3, 0.3, (N, 3)).astype(np.float32)
    pcs = (cano[None] + rng.normal(0, 0.02, (B, N, 3))).astype(np.float32)
    refs = [rng.uniform(-0.3, 0.3, (m, 3)).astype(np.float32) for m in LENS]
    flows = [rng.normal(0, 0.02, (m, 3)).astype(np.float32) for m in LENS]
    return cano, pcs, refs, flows


def _seed3(eng):
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


def _garbage(seeds):
    """Unusable seeds, three kinds in turn, and one lane in four left usable (rows of 16 lanes then mix both)."""
    g = seeds.clone()
    lens = torch.tensor(LENS, device=g.device, dtype=torch.int32)
    g[:, 0::4, 0] = -1
    g[:, 1::4, 2] = lens[:, None] + torch.arange(g[:, 1::4].shape[1], device=g.device, dtype=torch.int32)[None] % 3   # n2, n2 + 1, n2 + 2
    g[:, 2::4, 1] = g[:, 2::4, 0]
    seeds.copy_(g)


def _engine(dev, cano_idx, tuning, model_seed=0, data_seed=5, garbage=True, **kw):
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine

    cano, pcs, refs, flows = _data(data_seed)
    torch.manual_seed(model_seed)
    model = BaseModel(num_parts=P, pose_len=B).to(dev)
    eng = RelaxEngine(t(cano, dev), t(pcs, dev), model, cano_idx, [t(r, dev) for r in refs], [t(f, dev) for f in flows],
                      n_iter=100, seed=7, tuning=dict(tuning), **kw)
    seeds = None
    if tuning != BRUTE:
        seeds = _seed3(eng)
        if garbage:
            _garbage(seeds)
    return eng, model, seeds


def _state(eng, model, seeds=None):
    it, log = eng.loss_log()
    out = [log.cpu().numpy(), eng.pc_trans.cpu().numpy().copy(), eng.seg_part.cpu().numpy().copy()]
    out += [p.detach().cpu().numpy().copy() for p in eng.params]
    return it, out, None if seeds is None else seeds.cpu().numpy().copy()


def _brute(dev, cano_idx, iters=ITERS, model_seed=0, data_seed=5):
    key = (cano_idx, iters, model_seed, data_seed)
    if key not in _cache:
        eng, model, _ = _engine(dev, cano_idx, BRUTE, model_seed, data_seed)
        eng.step(iters)
        it, out, _ = _state(eng, model)
        assert it == iters and np.isfinite(out[0]).all()
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _same(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: output {k}")


@pytest.mark.parametrize("cano_idx", [0, 1, 2, 3])
def test_pruned_step_with_garbage_flow_seeds_equals_brute_force(dev, cano_idx):
    """The canonical frame (query cloud q_alt, frame index -1 in the item word) first, in the middle, last, and -- cano_idx 3 --
    behind every flow pair, so that no word holds it."""
    eng, model, seeds = _engine(dev, cano_idx, {})
    bad = seeds.cpu().numpy().copy()
    lens = np.array(LENS)[:, None]
    assert (bad[:, 0::4, 0] == -1).all() and (bad[:, 1::4, 2] >= lens).all() and (bad[:, 2::4, 0] == bad[:, 2::4, 1]).all()
    eng.step(ITERS)
    it, out, after = _state(eng, model, seeds)
    assert it == ITERS
    _same(out, _brute(dev, cano_idx), f"cano_idx {cano_idx}")
    # what the consumer left for the next search: three distinct valid indices per query, nothing of the garbage
    assert (after >= 0).all() and (after < lens[:, :, None]).all()
    assert (after[..., 0] != after[..., 1]).all() and (after[..., 1] != after[..., 2]).all() and (after[..., 0] != after[..., 2]).all()


def test_graph_of_three_iterations_replayed_twice_equals_eager(dev):
    """The words of iteration k are written by iteration k - 1's consumers, inside the graph as outside.  `capture` runs one
    eager iteration first, so both runs make 1 + 2 x 3 = 7."""
    runs = []
    for graph in (False, True):
        eng, model, seeds = _engine(dev, 1, {})
        done = eng.capture(steps_per_graph=3) if graph else 0
        eng.step(7 - done)
        assert eng.graph_replays == (2 if graph else 0)
        it, out, after = _state(eng, model, seeds)
        assert it == 7
        runs.append((out, after))
    _same(runs[1][0], runs[0][0], "graph against eager")
    np.testing.assert_array_equal(runs[1][1], runs[0][1])
    _same(runs[0][0], _brute(dev, 1, iters=7), "eager against brute force")


def test_second_prepare_in_mid_run_equals_a_fresh_engine(dev):
    """`prepare` lays the item words (and the seeds) down again: three iterations, prepare, three more must be what a fresh
    engine does that starts from the same parameters, moments and iteration count -- and what brute force does in six."""
    from reart_amd import _lib
    from reart_amd.relax import _lib_fns

    eng, model, seeds = _engine(dev, 2, {})
    eng.step(3)
    torch.cuda.synchronize()
    params3 = [p.detach().clone() for p in eng.params]
    m3, v3, log3 = eng.adam_m.clone(), eng.adam_v.clone(), eng.losses.clone()
    rc = _lib_fns().reart_relax_prepare(ctypes.byref(eng.cfg), ctypes.byref(eng._bufs), _lib.ptr(eng.workspace),
                                        eng.workspace.numel(), _lib.stream())
    assert rc == 0
    assert torch.equal(seeds.reshape(-1), (torch.arange(B * N * 3, device=dev) % 3).to(torch.int32))
    _garbage(seeds)
    eng.step(3)
    it, out, after = _state(eng, model, seeds)
    assert it == 6

    fresh, fmodel, fseeds = _engine(dev, 2, {}, garbage=False, start_iter=3)
    with torch.no_grad():
        for p, q in zip(fresh.params, params3):
            p.copy_(q)
        fresh.adam_m.copy_(m3); fresh.adam_v.copy_(v3); fresh.losses.copy_(log3)
    # the temperature of iteration 4 is what prepare computed from start_iter; the parameters were copied behind it
    fresh.step(3)
    fit, fout, fafter = _state(fresh, fmodel, fseeds)
    assert fit == 6
    _same(out, fout, "re-prepared against fresh")
    np.testing.assert_array_equal(after, fafter)
    _same(out, _brute(dev, 2), "re-prepared against brute force")


@pytest.mark.parametrize("name,tuning", [("reorder_off", {"tune_reorder": -1}),
                                         ("reorder_off_group_form", {"tune_reorder": -1, "tune_cloud": 0}),
                                         ("static_order_cloud_form", {"tune_cloud": 1}),
                                         ("xcd_chunks", {"tune_xcd": 1, "tune_cloud": 0}),
                                         ("one_wave", {"tune_slices": 1, "tune_cloud": 0}),
                                         ("own_seeds_only", {"tune_share": -1, "tune_cloud": 0})])
def test_launch_orders_and_forms_equal_brute_force(dev, name, tuning):
    """Words that are never re-sorted, the cloud-resident form (which reads no word at all), positions in XCD chunks, one
    wave per workgroup, and the prologue without neighbour seeds (its gathers have the same form)."""
    eng, model, seeds = _engine(dev, 1, tuning)
    eng.step(ITERS)
    it, out, _ = _state(eng, model, seeds)
    assert it == ITERS
    _same(out, _brute(dev, 1), name)


def test_two_instances_in_one_launch_equal_two_solo_engines(dev):
    """RelaxBatch: the BATCH = true instantiation picks its argument block, and with it its item words, by blockIdx.y."""
    from reart_amd.relax import RelaxBatch

    specs = [(0, 0, 5), (2, 1, 6)]          # (cano_idx, model seed, data seed)
    made = [_engine(dev, c, {}, ms, ds) for c, ms, ds in specs]
    RelaxBatch([e for e, _, _ in made]).step(ITERS)
    for (c, ms, ds), (eng, model, seeds) in zip(specs, made):
        it, out, after = _state(eng, model, seeds)
        assert it == ITERS
        solo, smodel, sseeds = _engine(dev, c, {}, ms, ds)
        solo.step(ITERS)
        _, sout, safter = _state(solo, smodel, sseeds)
        _same(out, sout, f"batched against solo, cano_idx {c}")
        np.testing.assert_array_equal(after, safter)
        _same(out, _brute(dev, c, model_seed=ms, data_seed=ds), f"batched against brute force, cano_idx {c}")
