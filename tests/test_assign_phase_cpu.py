"""The host side of the assignment phase without a GPU: the schedule of ``AssignmentPhase.run`` -- which refreshes, captures,
steps and snapshots it issues, in which order -- against the sequences recorded from the two ``run`` loops it replaced
(tests/golden/assign_schedule.json, written by tests/golden/make_golden_assign_schedule.py on the commit that still had
both), and the sampled assignment problem (``lap.AssignmentSample``) on injected samples."""
import json
import os

import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")


class Stepper:
    """What ``run`` advances the engines through: logs the calls."""

    def __init__(self, log):
        self.log = log

    def capture(self, steps_per_graph=1):
        self.log.append(f"c{steps_per_graph}")
        return 1

    def step(self, n=1):
        self.log.append(f"s{n}")


def _phase(cls, gap, first, log):
    """A phase of class ``cls`` with what ``run`` reads, and a stubbed ``refresh`` (the first one returns ``first``)."""
    ph = cls.__new__(cls)
    ph.gap, ph._have, ph.capture_guard, ph.work_guard, ph.stepper = gap, False, None, None, Stepper(log)
    state = {"first": first}

    def refresh():
        log.append("r")
        ph._have = True
        return state.pop("first", False)

    ph.refresh = refresh
    return ph


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(G, "assign_schedule.json")) as f:
        return json.load(f)


def test_the_grid_of_the_recorded_schedules(recorded):
    """assign_gap 1, 2, 5 x first iteration 0..6 x 0..12 iterations x first refresh True / False; the solo form with
    snapshot_gap 0 and 3, the batch form without snapshots."""
    grid = {(gap, start, iters, first) for gap in (1, 2, 5) for start in range(7) for iters in range(13) for first in (True, False)}
    assert {tuple(c) for c, _ in recorded["solo"]} == {(g, s, n, sg, f) for g, s, n, f in grid for sg in (0, 3)}
    assert {tuple(c) for c, _ in recorded["batch"]} == {(g, s, n, 0, f) for g, s, n, f in grid}
    assert len(recorded["solo"]) == 2 * len(recorded["batch"]) == 2 * len(grid) == 1092


def test_run_issues_the_recorded_sequence_for_one_engine(recorded):
    from reart_amd.run_robot import AssignmentPhase

    for (gap, start, iters, snapshot_gap, first), want in recorded["solo"]:
        log = []
        ph = _phase(AssignmentPhase, gap, first, log)
        end = ph.run(start, start + iters, snapshot_gap, lambda i: log.append(f"n{i}"))
        assert end == start + iters and " ".join(log) == want, (gap, start, iters, snapshot_gap, first)


def test_run_issues_the_recorded_sequence_for_a_batch(recorded):
    """The batch form's own recorded sequences, which are the solo ones without their snapshots."""
    from reart_amd.run_robot import AssignmentPhaseBatch

    solo = {tuple(c): seq for c, seq in recorded["solo"]}
    for case, want in recorded["batch"]:
        gap, start, iters, _, first = case
        assert want == " ".join(w for w in solo[tuple(case)].split() if not w.startswith("n"))
        log = []
        ph = _phase(AssignmentPhaseBatch, gap, first, log)
        assert ph.run(start, start + iters) == start + iters and " ".join(log) == want, case


def test_assignment_sample_on_injected_samples():
    """N = 64, B = 2, n = 16, CPU tensors, no FPS: the columns are the injected sample renumbered by ``tgt_order`` (or the
    injected sample itself with the Z-order off), ``tgt_pts`` are their points, ``slot`` inverts ``src_idx``."""
    from reart_amd.networks.pointnet2_utils import index_points
    from reart_amd.utils.lap import AssignmentSample, spatial_order

    g = torch.Generator().manual_seed(11)
    N, B, n = 64, 2, 16
    cano, pcs = torch.randn((N, 3), generator=g), torch.randn((B, N, 3), generator=g)
    src = torch.randperm(N, generator=g)[:n]
    tgt_fps = torch.stack([torch.randperm(N, generator=g)[:n] for _ in range(B)])
    s = AssignmentSample(cano, pcs, 4, src_idx=src, tgt_idx=tgt_fps)
    assert s.n == n and torch.equal(s.src_idx, src)
    assert torch.equal(s.tgt_order.sort(dim=1).values, torch.arange(n).expand(B, n))          # a permutation per frame
    assert torch.equal(s.tgt_order, spatial_order(index_points(pcs, tgt_fps)))
    assert torch.equal(s.tgt_idx, tgt_fps.gather(1, s.tgt_order))
    assert tuple(s.tgt_pts.shape) == (B, n, 3) and torch.equal(s.tgt_pts, index_points(pcs, s.tgt_idx))
    assert s.slot.dtype == torch.int32 and tuple(s.slot.shape) == (N,)
    assert torch.equal(s.slot[src], torch.arange(n, dtype=torch.int32))
    rest = torch.ones(N, dtype=torch.bool)
    rest[src] = False
    assert bool((s.slot[rest] == -1).all()) and int(rest.sum()) == N - n
    flat = AssignmentSample(cano, pcs, 4, src_idx=src, tgt_idx=tgt_fps, z_order=False)
    assert flat.tgt_order is None and torch.equal(flat.tgt_idx, tgt_fps)
    assert torch.equal(flat.tgt_pts, index_points(pcs, tgt_fps)) and torch.equal(flat.slot, s.slot)
