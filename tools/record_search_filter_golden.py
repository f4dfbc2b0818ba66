#!/usr/bin/env python3
"""Records tests/golden/search_filter_parent.npz: for every case of tests/test_search_filter_gpu.py (CASES) the executed pairs
and the launch count of `search_profile()` after the case's six iterations, and the flow neighbour indices the run left, from
whatever library is loaded.  Run it on an MI355X with the library of the commit BEFORE the filter loop of prune.hip changed:
    REART_LIB=<checkout of that commit>/reart_amd/csrc/libreart_hip.so python tools/record_search_filter_golden.py [out.npz]
The test then demands the same numbers from the tree's library.  There is no path without a GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tests import test_search_filter_gpu as tc


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else tc.GOLDEN
    if not torch.cuda.is_available():
        sys.exit("record_search_filter_golden: needs an MI355X (nothing is recorded from any other path)")
    dev = torch.device("cuda:0")
    rec = {}
    for case in sorted(tc.CASES):
        shape, _ = tc.CASES[case]
        a, b = tc.run_case(dev, case), tc.run_case(dev, case)
        # deterministic, and what brute force computes, before it is a reference
        for x, y in zip(a[0], b[0]):
            assert np.array_equal(x, y), case
        for x, y in zip(a[0], tc._brute(dev, shape)):
            assert np.array_equal(x, y), case
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (case, a[2], b[2])
        assert a[2][1] == tc.ITERS and 0 < a[2][0], (case, a[2])
        rec[f"{case}__flow_neighbours"] = a[1].astype(np.int32)
        rec[f"{case}__pairs_launches"] = a[2]
        print(f"{case}: pairs {int(a[2][0])} launches {int(a[2][1])}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **rec)
    print(f"{out}: {len(rec)} arrays, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
