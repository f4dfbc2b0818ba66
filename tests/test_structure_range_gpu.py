"""The four kernels of csrc/structure.hip (reart_screw_fit, reart_part_fps, reart_part_pair_cost, reart_group_temporal_err)
and the tail built on them (reart_amd/tail.py, utils/graph_utils.py, kinematic_utils.build_graph, compute_group_temporal_err)
over their documented range: up to 1024 frames (1025 for the group error), 4096 edges, 64 parts, clouds of up to 19200 points.

Floating-point results are held by the rule of tests/structure_ref.py (`accept`): per case and per array
    |kernel - f64| <= 4 max|oracle32 - f64| + c 2^-24 |f64|,   c = T for sums over the frames, 8 for per-frame values,
with f64 the float64 restatement and oracle32 oracle/structure.py on the same input; every test prints both maxima.  Integer
results (FPS indices, closest pairs, labels, trees) are exact.  No frame, edge or part is left out of a comparison."""
import os

import numpy as np
import pytest
import torch

from tests import structure_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("cpu_rules")]

ALL = ("screw", "rel", "recon", "mean_cost")


def T_(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def same(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    np.testing.assert_array_equal(a, b)


def arranged(out):
    """gu.screw_fit's dict under the names of structure_ref."""
    o = {k: v.cpu().numpy() for k, v in out.items()}
    res = dict(cost_r=o["cost"][:, 0], cost_p=o["cost"][:, 1], cost_min=o["cost"][:, 2], cost_id=o["cost"][:, 3],
               mean_axis=o["mean"][:, :3], mean_moment=o["mean"][:, 3:])
    if "screw" in o:
        s = o["screw"]
        res.update(screw_axis=s[..., 0:3], screw_moment=s[..., 3:6], screw_theta=s[..., 6], screw_distance=s[..., 7])
    for k in ("rel", "recon", "mean_cost"):
        if k in o:
            res[k] = o[k]
    return res


def run_fit(dev, c, want=ALL):
    from reart_amd.utils import graph_utils as gu

    return gu.screw_fit(T_(c["trans"], dev), T_(c["pairs"], dev), plain_mean=c["plain_mean"], want=want)


# ------------------------------------------------------------------------------------------------ reart_screw_fit
@pytest.mark.parametrize("name", [n for n in R.CASES if n != "T3_P64_E4096"])
def test_screw_fit_over_the_range(dev, oracle, name):
    """T in {1, 2, 21, 130, 1024} with all 36 ordered pairs of 6 parts; E = 400 and E = 257 at T = 64 (a thread owns two
    edges); pure screws; plain_mean: every output against the rule, bottom rows exact, two runs the same bits."""
    c = R.case(name)
    f, o = R.case_refs(name)
    out = run_fit(dev, c)
    R.accept_fit(name, c["T"], arranged(out), f, o)
    for k in ("rel", "recon"):
        same(out[k][..., 3, :], np.broadcast_to(np.array([0, 0, 0, 1], np.float32), (c["T"], c["E"], 4)))
    again = run_fit(dev, c)
    for k in out:
        same(again[k], out[k])


def test_screw_fit_4096_edges_through_compute_relative_trans(dev, oracle):
    from reart_amd.utils import graph_utils as gu

    name = "T3_P64_E4096"
    c = R.case(name)
    f, o = R.case_refs(name)
    T, P = c["T"], c["P"]
    axis, moment, theta, dist, rel = gu.compute_relative_trans(T_(c["trans"], dev), return_trans=True)
    assert rel.shape == (T, P, P, 4, 4)
    k = dict(screw_axis=axis.reshape(T, P * P, 3), screw_moment=moment.reshape(T, P * P, 3), screw_theta=theta.reshape(T, P * P),
             screw_distance=dist.reshape(T, P * P), rel=rel.reshape(T, P * P, 4, 4))
    R.accept_fit(name, T, {a: b.cpu().numpy() for a, b in k.items()}, f, o)
    R.accept_fit(name, T, arranged(run_fit(dev, c)), f, o, keys=("cost_r", "cost_p", "cost_min", "cost_id", "mean_cost", "mean_axis",
                                                                  "mean_moment", "recon"))


def test_relative_motion_form_and_every_wrapper_give_the_bits_of_the_pairs_form(dev, oracle):
    """At T = 130: the pairs=None form on the `rel` the pairs form returned, and each `want` combination the wrappers use."""
    from reart_amd.utils import graph_utils as gu

    c = R.case("T130_P6")
    T, P = c["T"], c["P"]
    trans, pairs = T_(c["trans"], dev), T_(c["pairs"], dev)
    full = run_fit(dev, c)
    direct = gu.screw_fit(full["rel"], None, want=ALL)
    for k in ("cost", "mean", "recon", "mean_cost", "screw", "rel"):
        same(direct[k], full[k])
    same(gu.compute_geo_cost(full["rel"].reshape(T, P, P, 4, 4)), full["cost"][:, 2].reshape(P, P))
    recon, mc = gu.compute_screw_trans(full["rel"], return_cost=True)
    same(recon, full["recon"])
    same(mc, full["mean_cost"][0])
    same(gu.compute_screw_trans(full["rel"]), full["recon"])
    same(gu.compute_screw_cost(trans, pairs), full["mean_cost"][0])
    same(gu.screw_fit(trans, pairs)["cost"], full["cost"])                                  # merge_graph's identity column
    same(gu.screw_fit(trans, pairs, want=("screw",))["screw"], full["screw"])


def test_build_graph_with_joint_types_at_130_frames(dev, oracle):
    """build_graph(revolute_only=False): every edge fitted on its own with the plain mean (E = 1) -> mean axis / moment, the
    joint type by the edge's own costs, theta or distance per frame."""
    from reart_amd.utils import kinematic_utils as ku

    c = R.case("T130_P6")
    T = c["T"]
    edges = np.array([[1, 0], [0, 2], [3, 0], [0, 4], [5, 0]])
    out = ku.build_graph(T_(edges, dev), T_(c["trans"], dev), revolute_only=False, return_joint_type=True)
    tree, root, axis, moment, theta, dist, edge_index, types = out
    assert root == 0 and sorted(tree.edges) == [(1, 0), (2, 0), (3, 0), (4, 0), (5, 0)]
    axis, moment, theta, dist = (a.cpu().numpy() for a in (axis, moment, theta, dist))
    seen = set()
    for k, (ch, pa) in enumerate(tree.edges):
        pair = np.array([[pa, ch]], np.int32)
        assert R.clearance(c["trans"], pair, True) is None
        f, o = R.screw_fit_ref(c["trans"], pair, True), R.oracle_screw_fit(c["trans"], pair, True)
        pris = bool(f["dec"]["pris"][0])
        assert types[k] == ("prismatic" if pris else "revolute")
        seen.add(types[k])
        tag = f"build_graph edge {ch}_{pa}"
        R.accept(f"{tag} mean_axis", axis[k], f["mean_axis"][0], o["mean_axis"][0], T)
        R.accept(f"{tag} mean_moment", moment[k], f["mean_moment"][0], o["mean_moment"][0], T)
        key, got = ("screw_distance", dist) if pris else ("screw_theta", theta)
        R.accept(f"{tag} {key}", got[:, k], f[key][:, 0], o[key][:, 0], 8)
        same((theta if pris else dist)[:, k], np.full(T, 1e-6, np.float32))
    assert seen == {"prismatic", "revolute"}


def test_screw_fit_c_abi_without_mean_buffer(dev):
    """mean == NULL: the means live in the caller's workspace of reart_screw_fit_workspace_bytes; the costs are the bits of the
    call with `mean`; a workspace one byte short is refused."""
    from reart_amd import _lib

    c = R.case("T21_P6")
    T, P, E = c["T"], c["P"], c["E"]
    with_mean = run_fit(dev, c, want=())["cost"]
    L = _lib.lib()
    trans, pairs = T_(c["trans"], dev), T_(c["pairs"], dev)
    need = L.reart_screw_fit_workspace_bytes(T, E)
    assert need == E * 6 * 4
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    cost = torch.empty((E, 4), dtype=torch.float32, device=dev)
    rc = L.reart_screw_fit(_lib.ptr(trans), T, P, _lib.ptr(pairs), E, 0, None, None, None, None, _lib.ptr(cost), None,
                           _lib.ptr(ws), need, _lib.stream())
    assert rc == 0
    same(cost, with_mean)
    same(ws.view(torch.float32).reshape(E, 6), run_fit(dev, c, want=())["mean"])
    untouched = torch.full((E, 4), -1.0, dtype=torch.float32, device=dev)
    rc = L.reart_screw_fit(_lib.ptr(trans), T, P, _lib.ptr(pairs), E, 0, None, None, None, None, _lib.ptr(untouched), None,
                           _lib.ptr(ws), need - 1, _lib.stream())
    assert rc == -1                                                        # REART_ERR_INVALID_ARG
    assert bool((untouched == -1).all())


# ------------------------------------------------------------------------------------------------ reart_part_fps
@pytest.mark.parametrize("N", R.FPS_SIZES)
def test_part_fps_large_clouds(dev, oracle, N):
    """N = 6144 is the last cloud of the default LDS window, 6145 .. 19200 need the opt-in; indices exact, both tie rules."""
    from reart_amd.utils import graph_utils as gu

    c = R.fps_case(N)
    cano, seg, lab = T_(c["cano"], dev), T_(c["seg"], dev), T_(c["labels"], dev)
    for cuda_mode in (False, True):
        pts, idx = gu.fps_sample_cano(cano, seg, lab, num_fps=20, cuda_mode=cuda_mode)
        same(idx, R.oracle_part_fps(c["cano"], c["seg"], c["labels"], 20, cuda_mode))
        same(pts, c["cano"][idx.cpu().numpy()])


def test_part_fps_errors(dev):
    from reart_amd import _lib
    from reart_amd.utils import graph_utils as gu

    c = R.fps_case(6145)
    seg = c["seg"].copy()
    seg[np.nonzero(seg == 23)[0][0]] = R.FPS_REST                     # part 23: num_fps - 1 members
    cano = T_(c["cano"], dev)
    with pytest.raises(ValueError, match="part id 23 too small, only 19 points"):
        gu.fps_sample_cano(cano, T_(seg, dev), T_(c["labels"], dev), num_fps=20)
    with pytest.raises(ValueError, match="part id 99 too small, only 0 points"):
        gu.fps_sample_cano(cano, T_(c["seg"], dev), T_(np.array([3, 99]), dev), num_fps=20)
    assert _lib.PART_FPS_MAX_N == 19200
    n = _lib.PART_FPS_MAX_N + 1
    with pytest.raises(NotImplementedError, match="19200"):
        gu.fps_sample_cano(torch.zeros((n, 3), device=dev), torch.zeros(n, dtype=torch.long, device=dev),
                           torch.zeros(1, dtype=torch.long, device=dev), num_fps=20)
    idx = torch.full((1, 20), 7, dtype=torch.int64, device=dev)        # the C entry point keeps its status
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _lib.lib().reart_part_fps(_lib.ptr(torch.zeros((n, 3), device=dev)), _lib.ptr(torch.zeros(n, dtype=torch.long, device=dev)), n,
                                   _lib.ptr(torch.zeros(1, dtype=torch.long, device=dev)), 1, 20, 0, _lib.ptr(idx), _lib.ptr(cnt),
                                   _lib.stream())
    assert rc == -2 and bool((idx == 7).all())                          # REART_ERR_UNSUPPORTED, nothing launched


# ------------------------------------------------------------------------------------------------ reart_part_pair_cost
@pytest.mark.parametrize("Ps,F,T", [(1, 20, 21), (16, 20, 21), (17, 20, 1), (17, 20, 1024), (32, 20, 21), (64, 20, 21),
                                    (17, 1, 21), (17, 33, 21)])
def test_part_pair_cost_over_the_range(dev, oracle, Ps, F, T):
    """Ps^2 <= 256 is one block, 17 .. 64 parts two to sixteen; F = 1, 20, 33 points per part; joint over 1 .. 1024 frames."""
    from oracle import structure as S
    from reart_amd.utils import graph_utils as gu

    pc = R.pair_case(Ps, F, T, 0)
    cd64, pair64, joint64 = R.part_pair_ref(pc["cano_fps"], pc["frame_fps"])
    cd_o, pair_o, joint_o = S.part_pair_cost(pc["cano"], pc["pred"], pc["fps_idx"])
    same(pair_o, pair64)
    dist, pair, joint = gu._pair_cost(T_(pc["cano_fps"], dev), T_(pc["frame_fps"], dev))
    same(dist, cd_o)
    same(pair, pair_o)
    R.accept(f"pair cost Ps={Ps} F={F} T={T} joint", joint.cpu().numpy(), joint64, joint_o, T)
    dist2, pair2, none = gu._pair_cost(T_(pc["cano_fps"], dev))
    assert none is None
    same(dist2, dist)
    same(pair2, pair)
    d3, p3 = gu.compute_spatial_cost(T_(pc["cano_fps"], dev), None, return_index=True)
    same(d3, dist)
    same(p3, pair)


def test_part_pair_cost_without_frames_leaves_joint_alone(dev):
    """The C ABI with frame_fps == NULL and T = 0 beside a `joint` buffer: cano_dist and pair as always, joint untouched."""
    from reart_amd import _lib
    from reart_amd.utils import graph_utils as gu

    pc = R.pair_case(17, 20, 1, 0)
    cf = T_(pc["cano_fps"], dev)
    dist0, pair0, _ = gu._pair_cost(cf)
    dist = torch.empty((17, 17), dtype=torch.float32, device=dev)
    pair = torch.empty((17, 17, 2), dtype=torch.int64, device=dev)
    joint = torch.full((17, 17), -3.0, dtype=torch.float32, device=dev)
    rc = _lib.lib().reart_part_pair_cost(_lib.ptr(cf), None, 0, 17, 20, _lib.ptr(dist), _lib.ptr(pair), _lib.ptr(joint), _lib.stream())
    assert rc == 0
    same(dist, dist0)
    same(pair, pair0)
    assert bool((joint == -3.0).all())


# ------------------------------------------------------------------------------------------------ reart_group_temporal_err
@pytest.mark.parametrize("T,N", [(1, 1), (1, 4097), (21, 255), (21, 257), (1025, 1), (1025, 4097)])
def test_group_temporal_err_over_the_range(dev, oracle, T, N):
    """Labels 2, 5 (one point, where N allows), 7 (nobody: 0, and no NaN reaches the maximum) and 11."""
    from reart_amd import _lib
    from reart_amd.utils.model_utils import compute_group_temporal_err

    pcs, seg = R.group_case(T, N)
    labels = np.array([2, 5, 7, 11], np.int64)
    f64, o32 = R.group_err_ref(pcs, seg, labels), R.oracle_group_err(pcs, seg, labels)
    d_pcs, d_seg, d_lab = T_(pcs, dev), T_(seg, dev), T_(labels, dev)
    per = torch.full((4,), float("nan"), dtype=torch.float32, device=dev)
    worst = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    rc = _lib.lib().reart_group_temporal_err(_lib.ptr(d_pcs), T, N, _lib.ptr(d_seg), _lib.ptr(d_lab), 4, _lib.ptr(per), _lib.ptr(worst),
                                             _lib.stream())
    assert rc == 0
    per, worst = per.cpu().numpy(), worst.cpu().numpy()
    R.accept(f"group err T={T} N={N}", per, f64, o32, 8)
    for k, lab in enumerate(labels):
        if (seg == lab).sum() <= 1:
            assert per[k] == 0
    assert worst[0].tobytes() == per.max().tobytes()
    through = compute_group_temporal_err(d_pcs, d_seg)
    assert np.float32(through).tobytes() == worst[0].tobytes()


# ------------------------------------------------------------------------------------------------ the tail end to end
def test_tail_end_to_end_at_pose_len_130(dev, oracle):
    """T = 131 frames of N = 512 points, 4 true parts as 12 model parts: tail.extract_structure, energy_terms and kinematic_init
    against the oracle's denoise -> merging -> spanning tree -> relabelling and its energies."""
    from oracle import structure as S
    from reart_amd import tail
    from reart_amd.utils.kinematic_utils import fk

    sc = R.tail_scene()
    ot = R.oracle_tail(sc)
    assert np.unique(ot["merged"]).tolist() == [0, 3, 6, 9]            # the splits that carry the parts' own motions survive
    cano, pcs = T_(sc["cano"], dev), T_(sc["pc_list"], dev)
    seg, trans, conn = tail.extract_structure(T_(sc["seg"], dev), T_(sc["trans"], dev), cano)
    same(seg, ot["seg"])
    same(seg, sc["true_part"])
    same(trans, ot["trans"])
    und = lambda e: sorted(tuple(sorted(x)) for x in np.asarray(e).tolist())
    assert und(conn.cpu().numpy()) == und(ot["conn"]) == [(0, 1), (1, 2), (2, 3)]
    e = tail.energy_terms(cano, pcs, seg, trans, conn, sc["cano_idx"])
    assert e["lap_fallbacks"] == 0
    conn_np = conn.cpu().numpy()
    T = ot["trans"].shape[0]
    f64 = R.screw_fit_ref(ot["trans"], conn_np)["mean_cost"]
    R.accept("tail screw_err", [e["screw_err"]], f64, [S.screw_cost(ot["trans"], conn_np)[0]], T)
    pred = oracle.compute_pc_transform(sc["cano"], ot["trans"], ot["seg"])
    comp = np.concatenate([pred[:sc["cano_idx"]], sc["cano"][None], pred[sc["cano_idx"]:]])
    R.accept("tail group_err", [e["group_err"]], [R.group_err_ref(comp, ot["seg"], np.unique(ot["seg"])).max()],
             [S.group_temporal_err(comp, ot["seg"])], 8)
    ass = 100 * float(S.ass_err(pred, sc["pc_list"]))
    print(f"tail ass_err {e['ass_err']!r} against {ass!r}")
    np.testing.assert_allclose(e["ass_err"], ass, rtol=2e-5, atol=1e-7)
    new_seg, kw = tail.kinematic_init(seg, trans, conn)
    same(new_seg, ot["seg"])
    rec = fk(kw["paths_to_base"], kw["reverse_topo"], kw["edge_index"], kw["axis_list"], kw["moment_list"], kw["theta_list"])
    err = float((rec - trans).abs().max())
    print(f"tail fk of kinematic_init against the transforms: max abs {err:.3e}")
    np.testing.assert_allclose(rec.cpu().numpy(), ot["trans"], rtol=1e-4, atol=2e-4)


# ------------------------------------------------------------------------------------------------ the long fixture
def test_kernels_match_the_long_reference_fixture(dev):
    """tests/golden/structure_long.npz (the reference's own functions on the T = 130 case and the end-to-end scene) at the
    tolerances tests/test_structure_gpu.py uses for the same quantities."""
    from reart_amd import tail
    from reart_amd.utils import graph_utils as gu
    from reart_amd.utils import model_utils as mu

    def close(a, b, atol=2e-6, rtol=1e-4):
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)

    L = np.load(os.path.join(os.path.dirname(__file__), "golden", "structure_long.npz"))
    c = R.case("T130_P6")
    P = c["P"]
    axis, moment, theta, dist, rel = gu.compute_relative_trans(T_(L["trans"], dev), return_trans=True)
    off = ~np.eye(P, dtype=bool)
    for ours, key in ((axis, "rel_axis"), (theta, "rel_theta"), (dist, "rel_distance")):
        close(ours.cpu().numpy()[:, off], L[key][:, off], atol=5e-6)
    rot = (np.abs(L["rel_theta"]) > 1e-5) & off[None]     # a no-rotation frame's moment is amplified rounding noise
    close(moment.cpu().numpy()[rot], L["rel_moment"][rot], atol=5e-6)
    close(rel.cpu().numpy()[::10], L["rel_trans_10"], atol=1e-6)
    close(gu.compute_geo_cost(rel), L["geo_cost"], atol=2e-6)
    sc = R.tail_scene()
    cano = T_(sc["cano"], dev)
    seg = gu.merging_wrapper(T_(L["seg_denoised"], dev), T_(L["scene_trans"], dev), cano, None, 3e-2, n_it=2)
    same(seg, L["seg_merged"])
    seg2, trans2, conn2 = tail.extract_structure(T_(sc["seg"], dev), T_(L["scene_trans"], dev), cano)
    same(seg2, L["new_seg"])
    same(conn2, L["new_conn"])
    close(gu.compute_root_cost(trans2), L["root_cost"])
    close(gu.compute_screw_cost(trans2, conn2), L["screw_err"], atol=1e-8)
    from reart_amd.screw_se3 import inverse_transformation

    rel_e = torch.matmul(inverse_transformation(trans2[:, conn2[:, 0]]), trans2[:, conn2[:, 1]])
    recon, cost = gu.compute_screw_trans(rel_e, return_cost=True)
    close(recon[::10], L["screw_recon_10"], atol=5e-6)
    close(cost, L["screw_cost_direct"], atol=1e-8)
    pred = mu.compute_pc_transform(cano, trans2, seg2)
    comp = torch.cat((pred[:sc["cano_idx"]], cano[None], pred[sc["cano_idx"]:]), dim=0)
    close(mu.compute_group_temporal_err(comp, seg2), L["group_err"], atol=1e-9, rtol=1e-5)
