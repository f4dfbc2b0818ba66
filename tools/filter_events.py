#!/usr/bin/env python3
"""Events of the search kernel's filter loop per launch at the headline shape (T = 20, N = 4096), from the diagnostic build:

    make -C reart_amd/csrc stats
    REART_LIB=reart_amd/csrc/libreart_hip_stats.so python tools/filter_events.py [--iters 300] [--probe 50]

Runs `--iters` iterations of the bench's instance, then counts over `--probe` more and prints, per kind of item (K = 1: the two
Chamfer directions, K = 3: the flow search) and per launch: waves, coarse rounds, boxes passing the coarse filter, precise
steps (two boxes each), boxes some lane needs, enqueued, densely scanned, drain steps.  The events are the filter's decisions,
so they do not depend on the form of the loop that takes them: multiply by the static instruction counts of
profiles/filter_stream_isa_counts.txt for the instructions a launch issues on each path."""
import argparse, ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from reart_amd import _lib

NAMES = ("coarse_rounds", "coarse_survivors", "precise_steps", "needed_boxes", "enqueued", "dense_scans", "drain_steps", "waves")
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=300)
ap.add_argument("--probe", type=int, default=50)
args = ap.parse_args()
lib = ctypes.CDLL(_lib.LIB_PATH)
if not hasattr(lib, "reart_debug_prune_events"):
    sys.exit("filter_events: the loaded library has no counters (make -C reart_amd/csrc stats; REART_LIB=...libreart_hip_stats.so)")
dev = torch.device("cuda:0")
eng, seq, model = bench.build_instance(dev, 20, 4096, 0, 2, n_iter=15000)
eng.capture()
eng.step(args.iters)
torch.cuda.synchronize()
buf = (ctypes.c_ulonglong * 16)()
lib.reart_debug_prune_events(buf, 1)
eng.step(args.probe)
torch.cuda.synchronize()
lib.reart_debug_prune_events(buf, 1)
out = {"after_iterations": args.iters, "launches": args.probe}
for row, kind in enumerate(("K1", "K3")):
    out[kind] = {n: buf[8 * row + k] / args.probe for k, n in enumerate(NAMES)}
print(json.dumps(out))
