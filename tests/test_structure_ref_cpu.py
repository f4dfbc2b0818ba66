"""tests/structure_ref.py (the float64 restatement of csrc/structure.hip's four kernels, its case generator and the
acceptance rule of tests/test_structure_range_gpu.py) on the CPU:

* every case of the GPU test builds, i.e. passes the generator's clearance and coverage assertions;
* the float32 oracle (oracle/structure.py) stays near the restatement on every case -- its deviation is printed per quantity,
  since the GPU tolerances are formed from it;
* the restatement agrees with the reference's own results (tests/golden/structure.npz and structure_long.npz) at the tolerances
  of tests/test_structure_oracle_cpu.py, and so does the oracle on the long fixture;
* the acceptance rule is not vacuous: it rejects six deliberately wrong float32 variants of the oracle at T = 130 and T = 1024.
"""
import os

import numpy as np
import pytest

from oracle import structure as S
from tests import structure_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "structure.npz"))
TOL = 2e-6                # tests/test_structure_oracle_cpu.py


def close(a, b, tol=TOL):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=0, atol=tol)


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_builds_and_the_oracle_stays_near_the_restatement(name):
    """Bounds of the oracle's float32 error, relative to the largest entry of each array: 1e-4 (the project's float32 parity)
    times the longest lever arm max(1, max|mean moment|), by which an error of the fitted axis moves the reconstruction; the
    moment itself is, in a no-rotation frame, 0.5 (t x l + l x (t x l) / tan(5e-7)) with l = t / |t|: the rounding of t x l,
    |t| 2^-23, amplified 2e6 times -- up to a quarter of |t| <= 1, and as much per unit of |f64| elsewhere."""
    c = R.case(name)
    f, o = R.case_refs(name)
    fr = c["dec"]["frames"]
    print(f"{name}: seed {c['seed']}, T = {c['T']}, E = {c['E']}, candidates {np.bincount(fr['best'].reshape(-1).numpy(), minlength=4).tolist()}, "
          f"flipped {int(fr['flip'].sum())}, unit frames {int(fr['unit'].sum())}, no_rot {int(fr['no_rot'].sum())}, "
          f"prismatic edges {int(c['dec']['pris'].sum())}")
    lever = max(1.0, float(np.abs(f["mean_moment"]).max()))
    for key in f:
        if key not in o:
            continue
        top = float(np.abs(f[key]).max())
        dev = float(np.abs(o[key] - f[key]).max())
        print(f"   {key:15s} max|o32-f64| = {dev:.3e}   max|f64| = {top:.3e}")
        bound = 0.25 * max(1.0, top) if key in ("screw_moment", "mean_moment") else 1e-4 * lever * top
        assert dev <= bound, (name, key, dev, bound)
    if c["T"] == 1024:
        assert sorted(np.unique(fr["best"].numpy()).tolist()) == [0, 1, 2, 3]
        assert bool(fr["flip"].any()) and not bool(fr["flip"].all())
        nk = c["dec"]["raw"]["nkeep"].numpy()
        assert ((nk >= 1) & (nk <= c["T"] - 1)).any()
    if name.endswith("exact"):      # a pure screw against the root: its fit cost is rounding noise
        e = R.all_pairs(c["P"]).tolist().index([0, 1])
        assert f["cost_r"][e] < 1e-9 * c["T"]


def test_restatement_matches_the_reference_fixture():
    P = 20
    f = R.screw_fit_ref(G["trans0"], R.all_pairs(P))
    off = ~np.eye(P, dtype=bool)
    for k, gk in (("screw_axis", "rel_axis"), ("screw_moment", "rel_moment"), ("screw_theta", "rel_theta"),
                  ("screw_distance", "rel_distance")):
        a = f[k].reshape((9, P, P) + f[k].shape[2:])
        close(a[:, off], G[gk][:, off])
    uni = G["uni_merged"]
    pairs = np.stack([np.repeat(uni, len(uni)), np.tile(uni, len(uni))], 1)
    close(R.screw_fit_ref(G["trans0"], pairs)["cost_min"].reshape(len(uni), len(uni)), G["geo_cost"])
    close(R.screw_fit_ref(G["new_trans"], G["new_conn"])["mean_cost"][0], G["screw_err"], 1e-8)
    comp = np.concatenate([G["pred"][:2], G["cano"][None], G["pred"][2:]])
    close(R.group_err_ref(comp, G["new_seg"], np.unique(G["new_seg"])).max(), G["group_err"], 1e-8)
    idx = G["fps_idx0"]
    cd, pair, joint = R.part_pair_ref(G["cano"][idx], G["pred0"][:, idx])
    np.testing.assert_array_equal(pair, G["pair_idx0"])
    close(cd, G["cano_dist0"])
    close(joint, G["joint0"])


def _pair_oracle(pc, frames=None):
    pred = pc["pred"] if frames is None else pc["pred"][:frames]
    return S.part_pair_cost(pc["cano"], pred, pc["fps_idx"])


@pytest.mark.parametrize("name", ["T130_P6", "T1024_P6"])
def test_the_acceptance_rule_rejects_wrong_variants(name):
    c = R.case(name)
    f, o = R.case_refs(name)
    R.accept_fit(name, c["T"], o, f, o, quiet=True)                       # the oracle itself passes its own rule
    assert int(((c["dec"]["raw"]["nkeep"] >= 1) & (c["dec"]["raw"]["nkeep"] < c["T"])).sum()) >= 1
    for variant in R.VARIANTS:
        wrong = R.oracle_screw_fit(c["trans"], c["pairs"], c["plain_mean"], variant=variant)
        with pytest.raises(AssertionError, match="outside the rule"):
            R.accept_fit(f"{name} [{variant}]", c["T"], wrong, f, o, quiet=True)
    pc = R.pair_case(17, 20, c["T"], 0)
    _, pair, joint = R.part_pair_ref(pc["cano_fps"], pc["frame_fps"])
    cd_o, pair_o, joint_o = _pair_oracle(pc)
    np.testing.assert_array_equal(pair_o, pair)
    R.accept(f"{name} joint", joint_o, joint, joint_o, c["T"], quiet=True)
    with pytest.raises(AssertionError, match="outside the rule"):
        R.accept(f"{name} joint [frame 0 only]", _pair_oracle(pc, 1)[2], joint, joint_o, c["T"], quiet=True)


@pytest.mark.parametrize("Ps,F,T", [(1, 20, 21), (17, 20, 1), (17, 1, 21), (17, 33, 21), (64, 20, 21)])
def test_pair_cases_build_and_match_the_oracle(Ps, F, T):
    pc = R.pair_case(Ps, F, T, 0)
    cd, pair, joint = R.part_pair_ref(pc["cano_fps"], pc["frame_fps"])
    cd_o, pair_o, joint_o = _pair_oracle(pc)
    np.testing.assert_array_equal(pair_o, pair)
    np.testing.assert_allclose(cd_o, cd, rtol=1e-6, atol=0)
    np.testing.assert_allclose(joint_o, joint, rtol=1e-5, atol=0)


def test_group_error_restatement_matches_the_oracle():
    pcs, seg = R.group_case(21, 257)
    lab = np.unique(seg)
    per = R.group_err_ref(pcs, seg, np.array([2, 5, 7, 11]))
    assert per[1] == 0 and per[2] == 0 and (per[[0, 3]] > 0).all()
    np.testing.assert_allclose(S.group_temporal_err(pcs, seg), R.group_err_ref(pcs, seg, lab).max(), rtol=1e-6)
    np.testing.assert_allclose(R.oracle_group_err(pcs, seg, np.array([2, 5, 7, 11])), per, rtol=1e-6)


# ------------------------------------------------------------------------------------------------ the long fixture
LONG = os.path.join(GOLD, "structure_long.npz")


def test_restatement_and_oracle_match_the_long_reference_fixture():
    """tests/golden/structure_long.npz: the reference's own functions on the T = 130, P = 6 case and on the end-to-end scene
    (make_golden_structure_long.py).  rel / recon are stored for every tenth frame."""
    L = np.load(LONG)
    c = R.case("T130_P6")
    np.testing.assert_array_equal(L["trans"], c["trans"])
    f, o = R.case_refs("T130_P6")
    P, T = c["P"], c["T"]
    off = ~np.eye(P, dtype=bool)
    sq = lambda a: np.asarray(a).reshape((T, P, P) + np.asarray(a).shape[2:])
    rot = np.abs(L["rel_theta"]) > 1e-5       # a no-rotation frame's moment is amplified rounding noise (test_screw_edge_cases)
    for side in (f, o):
        close(sq(side["rel"])[::10][:, off], L["rel_trans_10"][:, off])
        for k, gk in (("screw_axis", "rel_axis"), ("screw_theta", "rel_theta"), ("screw_distance", "rel_distance")):
            close(sq(side[k])[:, off], L[gk][:, off])
        close(sq(side["screw_moment"])[rot & off[None]], L["rel_moment"][rot & off[None]], 5e-6)
        np.testing.assert_allclose(side["cost_min"].reshape(P, P), L["geo_cost"], rtol=1e-4, atol=TOL)
    sc = R.tail_scene()
    np.testing.assert_array_equal(L["scene_trans"], sc["trans"])
    ot = R.oracle_tail(sc)
    np.testing.assert_array_equal(ot["merged"], L["seg_merged"])
    np.testing.assert_array_equal(ot["conn"], L["new_conn"])
    np.testing.assert_array_equal(ot["seg"], L["new_seg"])
    fe = R.screw_fit_ref(ot["trans"], ot["conn"])
    close(fe["mean_cost"][0], L["screw_err"], 1e-8)
    close(fe["recon"][::10], L["screw_recon_10"], 5e-6)
    close(S.screw_cost(ot["trans"], ot["conn"])[0], L["screw_err"], 1e-8)
    close(S.root_cost(ot["trans"]), L["root_cost"])
    import oracle

    pred = oracle.compute_pc_transform(sc["cano"], ot["trans"], ot["seg"])
    comp = np.concatenate([pred[:sc["cano_idx"]], sc["cano"][None], pred[sc["cano_idx"]:]])
    close(R.group_err_ref(comp, ot["seg"], np.unique(ot["seg"])).max(), L["group_err"], 1e-8)
    close(S.group_temporal_err(comp, ot["seg"]), L["group_err"], 1e-8)
