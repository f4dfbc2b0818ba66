#!/usr/bin/env python3
"""Where a search wave's lifetime goes (stats build: make -C reart_amd/csrc phase):
    REART_LIB=reart_amd/csrc/libreart_hip_phase.so python tools/phase_prof.py"""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from reart_amd import _lib

dev = torch.device("cuda:0")
eng, seq, model = bench.build_instance(dev, 20, 4096, 10, 2)
lib = ctypes.CDLL(_lib.LIB_PATH)
buf = (ctypes.c_ulonglong * 8)()
head = (ctypes.c_ulonglong * 16)()
has_head = hasattr(lib, "reart_debug_prune_head")     # the head of a workgroup: entry -> search, and stamps inside the prologue
head_names = ["head (entry -> search)", "  -> query loaded", "  -> seeds loaded", "  -> seed targets parked", "prologue (whole)"]
names = ["prologue", "coarse", "precise", "dense scan", "enqueue", "drain", "barrier wait", "waves"]
done = 0
for target in (300, 1500, 6000):
    eng.step(target - done - 50); done = target
    torch.cuda.synchronize()
    lib.reart_debug_prune_phase(buf, 1)
    if has_head: lib.reart_debug_prune_head(head, 1)
    eng.step(50)
    torch.cuda.synchronize()
    lib.reart_debug_prune_phase(buf, 1)
    if has_head: lib.reart_debug_prune_head(head, 1)
    v = list(buf)
    tot = sum(v[:7])
    print(f"iteration {target}: waves/launch {v[7] / 50:.0f}, ticks per wave {tot / max(v[7], 1):.0f}")
    for n, x in zip(names[:7], v[:7]):
        print(f"   {n:14s} {100 * x / tot:5.1f} %   {x / max(v[7], 1):8.0f} ticks/wave")
    if has_head:
        for row, kind in ((0, "K = 1"), (1, "K = 3")):
            h = list(head)[8 * row: 8 * row + 8]
            w, life = max(h[6], 1), max(h[5], 1)
            print(f"   {kind} items: waves/launch {h[6] / 50:.0f}, ticks per wave from kernel entry to the end of its search {life / w:.0f}")
            for n, x in zip(head_names, h[:5]):
                print(f"      {n:26s} {100 * x / life:5.1f} %   {x / w:8.0f} ticks/wave")
