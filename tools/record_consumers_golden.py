#!/usr/bin/env python3
"""Records tests/golden/consumers_parent.npz: every array of every case of tests/test_consumers_parent_gpu.py (CASES), from
whatever library is loaded, and the slices of tests/golden/kinematic.npz that the kinematic case builds its model from (so
that the test reads one file).  Run it on an MI355X with the library of the commit BEFORE the consumers' shared device
pieces moved into csrc/consumer_dev.h:
    REART_LIB=<checkout of that commit>/reart_amd/csrc/libreart_hip.so python tools/record_consumers_golden.py [out.npz]
The test then demands equal bits from the tree's library.  There is no path without a GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tests import test_consumers_parent_gpu as tc


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else tc.GOLDEN
    if not torch.cuda.is_available():
        sys.exit("record_consumers_golden: needs an MI355X (nothing is recorded from any other path)")
    dev = torch.device("cuda:0")
    k = np.load(os.path.join(ROOT, "tests", "golden", "kinematic.npz"))
    cut = {"cano_pc": 300, "seg_part": 300, "theta": 2}        # what the case uses of them
    kin = {key: np.ascontiguousarray(k[key][:cut[key]] if key in cut else k[key]) for key in tc.KIN_KEYS}
    rec = {f"kin_in__{key}": v for key, v in kin.items()}
    for case in sorted(tc.CASES):
        a, b = tc.CASES[case](dev, kin), tc.CASES[case](dev, kin)
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
