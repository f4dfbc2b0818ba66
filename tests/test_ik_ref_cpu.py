"""The yardstick of tests/test_ik_fused_gpu.py, checked without a GPU: every case that test holds to the float64 loop
(tests/ik_ref.py) is well enough conditioned for its bound to mean something, every planted error lands outside that bound,
and ik_fit / ik(fused=True) refuse what they do not take before they ask for a device.

The conditions (not measurements): spread(theta) <= 1e-3 rad and spread(loss) <= 1e-5 for every case, where spread is the
deviation of the float32 loop from the float64 loop; the GPU bound is 8 x spread.  Measured (torch CPU, one thread):
  P2_root_owns_nothing  theta 2.3e-08  loss 7.9e-08      chain_P64 (seed 1)  theta 3.8e-05  loss 1.6e-07
  star_P64              theta 1.4e-07  loss 6.3e-08      random_P33_empty5   theta 2.2e-07  loss 9.8e-08
  n1024_ragged_P7       theta 7.6e-08  loss 5.0e-08
"""
import numpy as np
import pytest
import torch

from tests import ik_ref


@pytest.mark.parametrize("name", ik_ref.REF_CASES)
def test_case_is_well_conditioned(name):
    sp = ik_ref.spread(name)
    print(f"{name}: spread(theta) {sp[0]:.3e} rad, spread(loss) {sp[1]:.3e}")
    assert sp[0] <= ik_ref.SPREAD_THETA_MAX and sp[1] <= ik_ref.SPREAD_LOSS_MAX, sp
    assert sp[0] > 0 and sp[1] > 0, "a bound of zero holds nothing"


def test_warm_start_is_well_conditioned():
    """The warm start restarts Adam at zero, so its first step moves every angle by lr = 0.1 rad whatever the gradient: the loss
    leaves loss[0] by a large factor at once and its float32 / float64 gap, measured in units of loss[0], cannot meet 1e-5 -- on
    a settled case loss[0] is ~1e-8 (the gap is then 1e4 of it), on the chain, which 200 steps do not settle, 1.1e-4 at this seed
    and 1.5e-5 .. 4.5e-3 over the seeds 0..11.  The angles meet their condition (4.6e-6 rad); the loss condition is recorded
    here as not met and is not asserted, and the GPU bound of the warm start stays 8 x this spread."""
    sp = ik_ref.warm_spread()
    print(f"warm start: spread(theta) {sp[0]:.3e} rad, spread(loss) {sp[1]:.3e}")
    assert 0 < sp[0] <= ik_ref.SPREAD_THETA_MAX and 0 < sp[1], sp


def test_cases_are_what_they_are_named_for():
    c = ik_ref.make_ik_case("random_P33_empty5")
    assert (c["counts"] == 0).sum() == 5 and len(ik_ref.pointless_edges(c)) >= 1
    th = ik_ref.case_ref("random_P33_empty5")[0]
    assert (th[:, ik_ref.pointless_edges(c)].astype(np.float32) == np.float32(1e-6)).all()
    c = ik_ref.make_ik_case("P2_root_owns_nothing")
    assert c["counts"][c["tree"][2][0]] == 0 and c["n"] == 3
    c = ik_ref.make_ik_case("n1024_ragged_P7")
    assert c["n"] == 1024 and sorted(c["counts"])[0] == 1 and sorted(c["counts"])[-1] == 600
    depth = lambda c, p: 0 if c["tree"][0][p] < 0 else 1 + depth(c, int(c["tree"][0][p]))
    assert max(depth(ik_ref.make_ik_case("chain_P64"), p) for p in range(64)) == 63
    assert max(depth(ik_ref.make_ik_case("star_P64"), p) for p in range(64)) == 1
    c = ik_ref.make_ik_case("P1_no_joint")
    assert c["E"] == 0 and (ik_ref.case_ref("P1_no_joint")[1] > 0).all()


@pytest.mark.parametrize("mutate", ik_ref.MUTATIONS)
def test_the_comparison_rejects_a_planted_error(mutate):
    """On the case with the most joints that settles (random_P33_empty5) every mutation is farther from the float64 loop than
    the GPU bound, in the angles or in the loss history: check_fit raises."""
    name = "random_P33_empty5"
    sp, ref = ik_ref.spread(name), ik_ref.case_ref(name)
    th, ls = ik_ref.case_ref(name, "float64", mutate)
    d = ik_ref.deviation(th, ls, ref)
    print(f"{mutate}: theta {d[0]:.3e} rad (bound {8 * sp[0]:.3e}), loss {d[1]:.3e} (bound {8 * sp[1]:.3e})")
    with pytest.raises(AssertionError):
        ik_ref.check_fit(th, ls, ref, sp, mutate)
    ik_ref.check_fit(*ik_ref.case_ref(name, "float32"), ref, sp, "the float32 loop")


def _cpu_model(**extra):
    from reart_amd.networks.model import KinematicModel

    seg = torch.arange(3).repeat_interleave(4)
    return KinematicModel(pose_len=2, seg_part=seg, cano_pc=torch.rand(12, 3), knn=None, edge_index={"1_0": 0, "2_1": 1},
                          paths_to_base=None, reverse_topo=[0, 1, 2], axis_list=torch.eye(3)[:2], moment_list=torch.zeros(2, 3),
                          theta_list=torch.zeros(2, 2), **extra)


def test_ik_fit_refuses_before_it_asks_for_a_device():
    from reart_amd import _lib
    from reart_amd.utils.kinematic_utils import ik_fit

    x = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="ik_single"):
        ik_fit(_cpu_model(distance_list=torch.zeros(2, 2)), x, x[None])
    with pytest.raises(NotImplementedError, match="ik_single"):
        ik_fit(_cpu_model(joint_type_list=["revolute", "revolute"]), x, x[None])
    with pytest.raises(NotImplementedError, match="ik_single"):
        ik_fit(_cpu_model(load_root_trans=True), x, x[None])
    big = torch.zeros(_lib.IK_MAX_POINTS + 1, 3)
    assert _lib.IK_MAX_POINTS == 1024
    with pytest.raises(NotImplementedError, match="REART_IK_MAX_POINTS"):
        ik_fit(_cpu_model(), big, big[None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ik_fit(_cpu_model(), x, x)


def test_fused_ik_refuses_a_base_model():
    from reart_amd.networks.model import BaseModel
    from reart_amd.utils.kinematic_utils import ik, ik_batch  # noqa: F401

    with pytest.raises(NotImplementedError, match="ik_single"):
        ik(None, BaseModel(num_parts=3, pose_len=2), torch.device("cpu"), fused=True)


def test_c_abi_refuses_without_a_launch():
    from reart_amd import _lib

    L = _lib.lib()
    d = 4096          # a non-null dummy address: the calls are refused before anything is launched
    call = lambda P, E, n, M, n_iter, src=d: L.reart_ik_fit(d, d, d, P, d, d, E, src, d, n, d, M, None, n_iter, 0.1, 0.9, 0.999, 1e-8, d, None, None)
    assert call(0, -1, 4, 1, 10) == -1 and call(65, 64, 4, 1, 10) == -1 and call(5, 5, 4, 1, 10) == -1
    assert call(5, 4, 0, 1, 10) == -1 and call(5, 4, 4, -1, 10) == -1 and call(5, 4, 4, 1, -1) == -1
    assert call(5, 4, 4, 1, 10, src=None) == -1
    assert call(5, 4, 1025, 1, 10) == -2
    assert call(5, 4, 1024, 0, 10) == 0
