#!/usr/bin/env python3
"""Records tests/golden/search_fixed_parent.npz: for the four engines of tests/test_search_fixed_gpu.py (GOLDEN_CASES) the
executed pairs of each of the first three search launches and the flow neighbour indices after the case's six iterations, from
whatever library is loaded.  Run it on an MI355X with the library of the commit BEFORE the fixed part of a search wave changed:
    REART_LIB=<checkout of that commit>/reart_amd/csrc/libreart_hip.so python tools/record_search_fixed_golden.py [out.npz]
The test then demands the same numbers from the tree's library.  There is no path without a GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tests import test_search_fixed_gpu as tc


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else tc.GOLDEN
    if not torch.cuda.is_available():
        sys.exit("record_search_fixed_golden: needs an MI355X (nothing is recorded from any other path)")
    dev = torch.device("cuda:0")
    rec = {}
    for case in sorted(tc.GOLDEN_CASES):
        T, _ = tc.GOLDEN_CASES[case]
        a, b = tc.run_golden_case(dev, case), tc.run_golden_case(dev, case)
        # deterministic, and what brute force computes, before it is a reference
        for x, y in zip(a[0], b[0]):
            assert np.array_equal(x, y), case
        for x, y in zip(a[0], tc._brute(dev, T)):
            assert np.array_equal(x, y), case
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (case, a[2], b[2])
        assert (a[2] > 0).all(), (case, a[2])
        rec[f"{case}__flow_neighbours"] = a[1].astype(np.int32)
        rec[f"{case}__pairs"] = a[2]
        print(f"{case}: pairs {a[2].tolist()}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **rec)
    print(f"{out}: {len(rec)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
