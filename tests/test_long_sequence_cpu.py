"""CPU side of the long-sequence path of the relaxation model (csrc/model_long.hip): the C oracle against the reference's
own BaseModel at pose_len 150 and 60 (tests/golden/base_model_long_{a,b}.npz), which pins the yardstick the GPU tests use;
the size limit's mirror; and the switch points of reart_base_path, which are the parent's behaviour written as literals:
no shape the in-LDS kernels of csrc/model.hip took before has moved to the new ones."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = ("g6d", "gt", "gW1", "gb1", "gW2")


def load(tag):
    return np.load(os.path.join(ROOT, "tests", "golden", f"base_model_long_{tag}.npz"))


@pytest.mark.parametrize("tag,B,P", [("a", 150, 20), ("b", 60, 32)])
def test_oracle_matches_the_reference_on_long_sequences(oracle, tag, B, P):
    g = load(tag)
    assert g[f"p6d_{tag}"].shape == (B, P, 6) and g[f"cano_{tag}"].shape == (192, 3)
    tau = float(g[f"tau_{tag}"])
    a = [g[f"{k}_{tag}"] for k in ("cano", "W1", "b1", "W2", "p6d", "pt")]
    f = oracle.base_forward(*a, g[f"noise_{tag}"], tau)
    np.testing.assert_array_equal(f["seg_part"], g[f"seg_{tag}"])
    np.testing.assert_allclose(f["out"], g[f"out_{tag}"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(f["trans_list"], g[f"trans_{tag}"], rtol=0, atol=1e-6)
    ref = oracle.base_backward(*a, f["y_soft"], f["hard_idx"], tau, g[f"G_{tag}"])
    for k in PARAMS:
        want = g[f"{k}_{tag}"]
        np.testing.assert_allclose(ref[k], want, rtol=0, atol=2e-4 * np.abs(want).max(), err_msg=k)


def test_pose_len_limit_mirrors_the_header():
    from reart_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "reart_hip.h")).read()
    m = re.search(r"#define\s+REART_MAX_POSE_LEN\s+(\d+)", hdr)
    assert m, "include/reart_hip.h does not define REART_MAX_POSE_LEN"
    assert _lib.MAX_POSE_LEN == int(m.group(1)) == 1024


# P -> (largest B the in-LDS forward takes, largest B the in-LDS backward takes) at H = 128: the two launcher
# expressions of csrc/model.hip as they stood before the long path existed
SWITCH = {20: (90, 58), 32: (56, 38), 10: (181, 88), 8: (226, 97), 5: (362, 87), 2: (906, 101)}


@pytest.mark.parametrize("P", sorted(SWITCH))
def test_base_path_switches_exactly_where_lds_ends(P):
    from reart_amd import _lib

    L = _lib.lib()
    fwd, bwd = SWITCH[P]
    for backward, last in ((0, fwd), (1, bwd)):
        assert L.reart_base_path(P, 1, 128, backward) == 0
        assert L.reart_base_path(P, last, 128, backward) == 0, (P, last, backward)
        assert L.reart_base_path(P, last + 1, 128, backward) == 1, (P, last + 1, backward)
        assert all(L.reart_base_path(P, B, 128, backward) == (0 if B <= last else 1) for B in range(1, 1025))
        assert L.reart_base_path(P, 1024, 128, backward) == 1
        assert L.reart_base_path(P, 1025, 128, backward) < 0


def test_base_path_refuses_what_neither_path_takes():
    from reart_amd import _lib

    L = _lib.lib()
    for backward in (0, 1):
        assert L.reart_base_path(33, 4, 128, backward) < 0
        assert L.reart_base_path(20, 1025, 128, backward) < 0
        assert L.reart_base_path(20, 0, 128, backward) < 0
        assert L.reart_base_path(0, 4, 128, backward) < 0


def test_tune_long_reaches_the_config_from_the_environment():
    from reart_amd import relax

    assert relax.tuning_from_env({"REART_LONG": "1"}) == {"tune_long": 1}
    assert relax.tuning_from_env({}) == {}
    assert relax.RelaxConfig._fields_[-1][0] == "tune_long" and "tune_long" in relax.RelaxBatch.SAME
