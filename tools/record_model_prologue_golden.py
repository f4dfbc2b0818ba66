#!/usr/bin/env python3
"""Records tests/golden/model_prologue_parent.npz: the forward outputs and the five gradients of reart_base_forward +
reart_base_backward for the seeded inputs and shapes of tests/test_model_prologue_gpu.py (GOLDEN_SHAPES), from whatever
library is loaded.  Run it on an MI355X with the library of the commit BEFORE the block kernel's tile staging changed:
    REART_LIB=reart_amd/csrc/libreart_hip_parent.so python tools/record_model_prologue_golden.py [out.npz]
The test then demands byte equality from the tree's library."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tests import test_model_prologue_gpu as tm

out = sys.argv[1] if len(sys.argv) > 1 else tm.GOLDEN
dev = torch.device("cuda:0")
rec = {}
for shape in tm.GOLDEN_SHAPES:
    a, b = tm.run_model(shape, tm.inputs(shape), dev), tm.run_model(shape, tm.inputs(shape), dev)
    for k in tm.FWD_KEYS + tm.GRAD_KEYS:
        assert a[k].tobytes() == b[k].tobytes() and np.isfinite(a[k]).all(), (shape, k)   # deterministic before it is a reference
        rec[f"{shape[0]}_{k}"] = a[k]
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
np.savez_compressed(out, **rec)
print(f"{out}: {len(rec)} arrays, {os.path.getsize(out)} bytes")
