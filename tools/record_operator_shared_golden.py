#!/usr/bin/env python3
"""Records tests/golden/operator_shared_parent.npz: every array of every case of tests/test_operator_shared_parent_gpu.py
(CASES), from whatever library is loaded.  Run it on an MI355X with the library of the commit BEFORE the operators' inverse-list
builder moved into csrc/invlist_dev.h and their block sums into csrc/common.h:
    REART_LIB=<checkout of that commit>/reart_amd/csrc/libreart_hip.so python tools/record_operator_shared_golden.py [out.npz]
The test then demands equal bits from the tree's library.  There is no path without a GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tests import test_operator_shared_parent_gpu as tc


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else tc.GOLDEN
    if not torch.cuda.is_available():
        sys.exit("record_operator_shared_golden: needs an MI355X (nothing is recorded from any other path)")
    dev = torch.device("cuda:0")
    rec = {}
    for case in sorted(tc.CASES):
        a, b = tc.CASES[case](dev), tc.CASES[case](dev)
        assert sorted(a) == sorted(b)
        for key in sorted(a):
            # deterministic, and finite where it is a number, before it is a reference
            assert np.array_equal(tc.bits(a[key]), tc.bits(b[key])), (case, key)
            assert a[key].dtype.kind != "f" or np.isfinite(a[key]).all(), (case, key)
            rec[f"{case}__{key}"] = a[key]
        print(f"{case}: {len(a)} arrays", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **rec)
    print(f"{out}: {len(rec)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
