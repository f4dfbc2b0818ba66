#!/usr/bin/env python3
"""The fused step's three loss modes side by side on the headline workload (synthetic T = 20 frames x N = 4096 points, P = 20
parts, flow loss on, 3000 reference points per frame pair): iterations per second of ONE engine with

  chamfer   Chamfer + flow (the default; what bench.py measures),
  assign    assignment loss + flow (``set_assignment``: the pairs replace the Chamfer term, no K = 1 search),
  both      Chamfer + assignment loss + flow (``RelaxEngine(recon_with_assign=True)`` after ``set_assignment``:
            the objective of the reference's run_real.py:175-203).

The pairs are fixed: the N / 4 farthest-point samples of the canonical cloud matched to the N / 4 samples of every frame by
ONE linear-assignment solve on the initial state (``AssignmentPhase.refresh`` with --downsample 4: what a run holds between
two refreshes), the same pairs in both modes that use them.  Every mode is its own engine on the same clouds with its
iteration captured in a graph; after --warmup replayed iterations, --reps windows of --iters replays each between two device
events, the modes alternating in one process; median (min - max) it/s.  Afterwards --phase-steps eager iterations of every
engine with device events between the launches (``step_timed``: event pairs over-read short kernels, the modes compare like
with like) give the milliseconds of the consumer launch the modes differ in.  Writes --out (default
profiles/relax_both_bench.json) and prints it as one JSON line.
Without a GPU it fails."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v, nd=1):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], nd), min=round(v[0], nd), max=round(v[-1], nd))


def main():
    import numpy as np
    import torch

    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine
    from reart_amd.run_robot import AssignmentPhase
    from reart_amd.synthetic import make_sequence, split_canonical

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--cano_idx", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lambda_assign", type=float, default=0.3)
    ap.add_argument("--phase-steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relax_both_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    T, N = a.frames, a.points
    seq = make_sequence(T=T, n_parts=8, pts_per_part=N // 8, seed=2, n_ref=3000, with_flow=True)
    cano, pcs = split_canonical(seq["complete"], a.cano_idx)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    refs, flows = [t(r) for r in seq["ref_loc"]], [t(f) for f in seq["ref_flow"]]
    n = N // 4
    engines, pairs, fallbacks = {}, None, 0
    for mode in ("chamfer", "assign", "both"):
        torch.manual_seed(2)
        model = BaseModel(num_parts=20, pose_len=T - 1).to(dev)
        eng = RelaxEngine(t(cano), t(pcs), model, a.cano_idx, refs, flows, n_iter=15000, seed=2, recon_with_assign=mode == "both")
        if mode != "chamfer":
            if pairs is None:      # the engines start from one state: solved once
                phase = AssignmentPhase(eng, t(cano), t(pcs), 4, 5, a.lambda_assign)
                phase.refresh()
                pairs, fallbacks = (phase.src_idx[0].clone(), phase.tgt_idx.gather(1, phase.lap_state["cols"].long()).clone()), phase.fallbacks
                assert pairs[0].numel() == n
            eng.set_assignment(pairs[0], pairs[1], a.lambda_assign)
        eng.capture()
        eng.step(a.warmup)
        engines[mode] = eng
    torch.cuda.synchronize()
    rates = {m: [] for m in engines}
    for _ in range(a.reps):
        for mode, eng in engines.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.step(a.iters)
            e1.record()
            torch.cuda.synchronize()
            rates[mode].append(a.iters / (e0.elapsed_time(e1) * 1e-3))
    phases = {m: {k: round(v, 5) for k, v in e.step_timed(a.phase_steps).items() if v > 0} for m, e in engines.items()}
    out = {"workload": dict(frames=T, points=N, parts=20, flow=True, pairs_per_frame=n, lambda_assign=a.lambda_assign,
                            cano_idx=a.cano_idx, pairs="FPS samples matched by one assignment solve on the initial state",
                            lap_fallbacks=int(fallbacks)),
           "method": dict(iters=a.iters, warmup=a.warmup, reps=a.reps, timing="device events around graph replays, modes alternating"),
           "device": torch.cuda.get_device_name(0),
           "it_per_s": {m: stats(v) for m, v in rates.items()},
           "eager_phase_ms": phases,
           "it_per_s_runs": {m: [round(x, 1) for x in v] for m, v in rates.items()},
           "last_losses": {m: [float(x) for x in e.last_losses().cpu()] for m, e in engines.items()},
           "last_assign_loss": {m: float(e.last_assign_loss().cpu()) for m, e in engines.items()}}
    for m, e in engines.items():
        assert e.cfg.use_assign == int(m != "chamfer") and e.cfg.recon_with_assign == int(m == "both")
        assert e.graph_replays >= a.warmup + a.reps * a.iters and all(np.isfinite(out["last_losses"][m])), m
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
