"""The headline path as `bench.py` runs it -- in-kernel Philox noise drawn from the iteration counter, the temperature read
from the device, block 0 publishing the pose tables, the captured graph -- against a recorded run.  tests/golden/
bench_dump_small.npz holds every file that `bench.py --gpus 1 --frames 6 --points 512 --steps 20 --warmup 5 --dump-outputs DIR`
wrote on an MI355X from the commit BEFORE the small kernels' loads were batched (the forward's, the search consumers' and the
finalize kernel's).  Those changes move loads and touch no arithmetic, so the same command must reproduce every array byte
for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bench_dump_small.npz")
ARGS = ["--gpus", "1", "--frames", "6", "--points", "512", "--steps", "20", "--warmup", "5"]
T, N, P, H = 6, 512, 20, 128
SHAPES = {"losses": (4,), "loss_log": (20, 4), "pc_trans": (T - 1, N, 3), "seg_part": (N,), "trans_list": (T - 1, P, 4, 4),
          "iterations": (1,), "seg_w1": (H, 3, 1), "seg_b1": (H,), "seg_w2": (P, H, 1), "proposal_6d": (T - 1, P, 6),
          "proposal_t": (T - 1, P, 3)}


def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_recorded_run_is_complete():
    """CPU side: the fixture holds every file of a dump, finite, of the run's shapes, and the run did optimise something."""
    g = _golden()
    assert set(g) == set(SHAPES)
    for k, v in g.items():
        assert v.shape == SHAPES[k], (k, v.shape)
        assert v.dtype == (np.float64 if k in ("seg_part", "iterations") else np.float32), (k, v.dtype)
        assert np.isfinite(v).all(), k
    assert g["iterations"].tolist() == [25.0]
    np.testing.assert_array_equal(g["loss_log"][-1], g["losses"])
    assert len({r.tobytes() for r in g["loss_log"]}) == 20          # twenty different iterations
    assert len(np.unique(g["seg_part"])) > 1 and g["losses"][0] > 0 and g["losses"][1] > 0


@pytest.mark.gpu
def test_bench_dump_reproduces_the_recorded_run_byte_for_byte(dev, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, "--dump-outputs", str(tmp_path)],
                       capture_output=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    g = _golden()
    assert {f[:-4] for f in os.listdir(tmp_path)} == set(g)
    bad = []
    for k, ref in g.items():
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == ref.dtype and got.shape == ref.shape, (k, got.dtype, got.shape, ref.dtype, ref.shape)
        if got.tobytes() != ref.tobytes():
            bad.append((k, int((got.view(np.uint8) != ref.view(np.uint8)).sum())))
    assert not bad, bad
