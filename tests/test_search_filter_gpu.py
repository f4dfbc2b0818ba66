"""The filter loop of a search wave (prune.hip, knn_pruned_wave): the coarse round, the precise test of two boxes per step,
the queue appends and the statistics counter.  Its form may change (operands paired by axis, box addresses and the counter in
scalar registers, candidates updated in place); nothing it decides may.  Every case therefore compares the fused pruned step
with the brute-force step (`search_mode` 1) of the same engine bit for bit after 6 iterations -- loss log, forward output,
part labels, the five parameter tensors -- takes the flow neighbour indices from the pruned run, and demands the executed
pairs and the launch count that the library of the commit BEFORE the filter loop changed reported for the same case
(tests/golden/search_filter_parent.npz, written by tools/record_search_filter_golden.py from that library on an MI355X):
executed pairs are a checksum of every filter decision, and the work counts that order the next launch follow from the
same decisions.

Shapes, the smallest at which the loop takes each of its paths:
  * small: T = 4 (B = 3), N = 200, reference sets of 3 / 17 / 40 points -- 1, 2 and 3 target boxes per frame for the flow job:
    a round with ONE survivor (a step without a second box), rounds with odd and with even survivor counts; the Chamfer
    jobs see 13 boxes.
  * two_rounds: N = 1 056 = 66 boxes.  With one wave per item a second coarse round holds 2 boxes; with the default three
    waves every wave has one round of 22.  Reference sets of 40 / 1 030 / 1 056 points give the K = 3 instantiation 3, 65 (the
    last one partly filled) and 66 boxes.
Tunings: 1, 2, 3 and 4 waves per item (every value of the wave index); every needed box densely scanned (`tune_sparse` -1),
queued only when one query needs it (1), the default (40); the cloud-resident form with 1 and 4 slices.
No wave comes near 2^20 executed pairs (the counter's documented wrap): 1 056 targets x 64 lanes = 67 584 at the most."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_filter_parent.npz")
P, B, ITERS = 8, 3, 6
BRUTE = {"search_mode": 1}
SHAPES = {"small": (200, (3, 17, 40)), "two_rounds": (1056, (40, 1030, 1056))}
GROUP = {"tune_cloud": 0}
CASES = {
    "small_default": ("small", {}),
    "small_waves1": ("small", dict(GROUP, tune_slices=1)),
    "small_waves2": ("small", dict(GROUP, tune_slices=2)),
    "small_waves3": ("small", dict(GROUP, tune_slices=3)),
    "small_waves4": ("small", dict(GROUP, tune_slices=4)),
    "small_waves1_flow4": ("small", dict(GROUP, tune_slices=1, tune_slices_flow=4)),
    "small_dense": ("small", dict(GROUP, tune_sparse=-1)),
    "small_queue1": ("small", dict(GROUP, tune_sparse=1)),
    "small_cloud1": ("small", {"tune_cloud": 1}),
    "small_cloud4": ("small", {"tune_cloud": 4}),
    "two_rounds_waves1": ("two_rounds", dict(GROUP, tune_slices=1)),
    "two_rounds_default": ("two_rounds", {}),
    "two_rounds_waves1_dense": ("two_rounds", dict(GROUP, tune_slices=1, tune_sparse=-1)),
    "two_rounds_waves1_queue1": ("two_rounds", dict(GROUP, tune_slices=1, tune_sparse=1)),
}
_cache = {}


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _data(shape, seed=11):
    n, lens = SHAPES[shape]
    rng = np.random.default_rng(seed)
    cano = rng.uniform(-0.3, 0.3, (n, 3)).astype(np.float32)
    pcs = (cano[None] + rng.normal(0, 0.02, (B, n, 3))).astype(np.float32)
    refs = [rng.uniform(-0.3, 0.3, (m, 3)).astype(np.float32) for m in lens]
    flows = [rng.normal(0, 0.02, (m, 3)).astype(np.float32) for m in lens]
    return cano, pcs, refs, flows


def _seed3(eng, n):
    """The flow job's warm-start seeds [B, N, 3] inside the workspace: the only run of B*N*3 int32 that `prepare` has just
    filled with 0, 1, 2, 0, 1, 2, ... (blocks of the workspace start at multiples of 256 bytes)."""
    ws = eng.workspace.view(torch.int32)
    m = B * n * 3
    want = (torch.arange(m, device=ws.device) % 3).to(torch.int32)
    starts = torch.arange(0, ws.numel() - m + 1, 64, device=ws.device)
    head = ws[starts[:, None] + torch.arange(6, device=ws.device)[None]]
    hits = [int(s) for s in starts[(head == want[:6]).all(1)].tolist() if torch.equal(ws[s:s + m], want)]
    assert len(hits) == 1, hits
    return ws[hits[0]:hits[0] + m].view(B, n, 3)


def _run(dev, shape, tuning):
    """Six iterations of a fresh engine -> (arrays compared with brute force, flow neighbour indices or None, profile or None)."""
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine

    n, lens = SHAPES[shape]
    cano, pcs, refs, flows = _data(shape)
    torch.manual_seed(0)
    model = BaseModel(num_parts=P, pose_len=B).to(dev)
    pruned = tuning != BRUTE
    eng = RelaxEngine(t(cano, dev), t(pcs, dev), model, 1, [t(r, dev) for r in refs], [t(f, dev) for f in flows],
                      n_iter=100, seed=7, tuning=dict(tuning), profile=pruned)
    seeds = _seed3(eng, n) if pruned else None
    eng.step(ITERS)
    it, log = eng.loss_log()
    assert it == ITERS
    out = [log.cpu().numpy(), eng.pc_trans.cpu().numpy().copy(), eng.seg_part.cpu().numpy().copy()]
    out += [p.detach().cpu().numpy().copy() for p in eng.params]
    assert len(out) == 8
    prof = eng.search_profile() if pruned else None
    return out, None if seeds is None else seeds.cpu().numpy().copy(), prof


def _brute(dev, shape):
    if shape not in _cache:
        out, _, _ = _run(dev, shape, BRUTE)
        assert np.isfinite(out[0]).all()
        for a in out:
            a.setflags(write=False)
        _cache[shape] = out
    return _cache[shape]


def run_case(dev, case):
    """What the golden file records of a case (tools/record_search_filter_golden.py calls this too)."""
    shape, tuning = CASES[case]
    out, nbr, prof = _run(dev, shape, tuning)
    return out, nbr, np.array([prof["pairs"], prof["launches"]], dtype=np.int64)


@pytest.mark.parametrize("case", sorted(CASES))
def test_pruned_step_equals_brute_force_and_executes_the_parents_pairs(dev, case):
    shape, _ = CASES[case]
    n, lens = SHAPES[shape]
    out, nbr, counts = run_case(dev, case)
    want = _brute(dev, shape)
    for k, (a, b) in enumerate(zip(out, want)):
        np.testing.assert_array_equal(a, b, err_msg=f"{case}: output {k} against brute force")
    # the flow neighbours the consumer left for the next search: three distinct valid indices per query
    ln = np.array(lens)[:, None, None]
    assert (nbr >= 0).all() and (nbr < ln).all()
    assert (nbr[..., 0] != nbr[..., 1]).all() and (nbr[..., 1] != nbr[..., 2]).all() and (nbr[..., 0] != nbr[..., 2]).all()
    gold = np.load(GOLDEN)
    np.testing.assert_array_equal(nbr, gold[f"{case}__flow_neighbours"], err_msg=f"{case}: flow neighbour indices")
    pairs, launches = (int(v) for v in gold[f"{case}__pairs_launches"])
    print(f"{case}: pairs {int(counts[0])} (parent {pairs}), launches {int(counts[1])} (parent {launches})")
    assert launches == ITERS and pairs > 0
    assert int(counts[1]) == launches
    assert int(counts[0]) == pairs
