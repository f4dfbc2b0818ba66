"""Stage two of the sweep on the GPU (python -m reart_amd.sweep --project): the winner of every sequence is projected onto a
kinematic model by the function run_robot's own command line uses (run_robot.project_from_base) -- the same files, bit for
bit --, and two ranks that share one GPU (--backend gloo --devices 0,0) go through launcher -> shard -> gather -> relay with
the real engines and end where one rank ends."""
import json
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_one_rank_projects_the_winner_as_run_robot_does(dev, tmp_path):
    """tests/golden/seq_tiny, the arguments of test_sweep_command_line_one_rank + --project --project_iter 60 --use_assign_loss:
    result.pkl / model.pth.tar / result.txt under seq_tiny/kinematic/ with the reference's keys (run_robot.py:333-356), no
    assignment problem sent to the host solver, and the same poses, labels, tree and parameters -- bit for bit -- as
    `run_robot --model kinematic --base_result_path <the winner's result.pkl>` (README.md:125) with the same flags."""
    from reart_amd import run_robot as rr
    from reart_amd import sweep

    out = tmp_path / "sweep"
    rc = sweep.main(["--seq_root", GOLDEN, "--seqs", "seq_tiny", "--cano", "all", "--n_iter", "300", "--energy", "--num_points", "80",
                     "--num_parts", "6", "--per_gpu", "2", "--save_root", str(out), "--project", "--project_iter", "60",
                     "--use_assign_loss"])
    assert rc == 0
    sw = json.load(open(out / "sweep.json"))
    seq = sw["sequences"]["seq_tiny"]
    w = seq["winner_cano_idx"]
    proj = seq["projection"]
    print("projection:", proj)
    assert w is not None and proj["failed"] == 0 and proj["cano_idx"] == w and proj["iterations"] == 60
    assert (proj["rank"], proj["device"]) == (0, "cuda:0")
    assert proj["assign_refreshes"] == 60 and proj["lap_fallbacks"] == 0          # --assign_iter 0 --assign_gap 1: one solve per iteration
    assert abs(proj["total_err"] - (proj["ass_err"] + proj["screw_err"] + proj["group_err"])) <= 1e-5 * abs(proj["total_err"])
    kin = out / "seq_tiny" / "kinematic"
    res = pickle.load(open(kin / "result.pkl", "rb"))
    assert set(res) >= {"pred_cano_part", "pred_pose_list", "cano_idx", "joint_connection", "cano_pc", "pc_list"}
    assert res["cano_idx"] == w and res["pred_cano_part"].shape == (80,) and res["pred_pose_list"].shape[0] == 3
    assert res["pred_pose_list"].shape[1] == proj["parts"] and res["joint_connection"] == proj["joint_connection"]
    ck = torch.load(kin / "model.pth.tar", weights_only=False)
    assert set(ck) >= {"state_dict", "tau", "cano_idx", "seg_part", "cano_pc", "edge_index", "paths_to_base", "reverse_topo"}
    assert ck["cano_idx"] == w
    txt = dict(line.split(": ") for line in open(kin / "result.txt").read().splitlines())
    assert set(txt) >= {"retarget_err", "cd_err", "ass_err", "screw_err", "group_err", "total_err", "assign_refreshes", "lap_fallbacks"}
    assert txt["lap_fallbacks"] == "0" and float(txt["total_err"]) == pytest.approx(proj["total_err"], abs=6e-4)
    # the base result of the sequence is still the winner's (the projection has a directory of its own)
    base_path = out / "seq_tiny" / f"cano_{w}" / "result.pkl"
    assert open(out / "seq_tiny" / "result.pkl", "rb").read() == open(base_path, "rb").read()
    assert pickle.load(open(base_path, "rb"))["cano_idx"] == w

    # the same projection from run_robot's command line, in another save root
    rr.main(rr.build_parser().parse_args(["--seq_path", os.path.join(GOLDEN, "seq_tiny"), "--num_points", "80", "--cano_idx", str(w),
                                          "--model", "kinematic", "--base_result_path", str(base_path), "--use_assign_loss",
                                          "--assign_iter", "0", "--assign_gap", "1", "--downsample", "2", "--n_iter", "60",
                                          "--save_root", str(tmp_path / "solo")]))
    solo = tmp_path / "solo" / "seq_tiny"
    ref = pickle.load(open(solo / "result.pkl", "rb"))
    np.testing.assert_array_equal(res["pred_pose_list"], ref["pred_pose_list"])
    np.testing.assert_array_equal(res["pred_cano_part"], ref["pred_cano_part"])
    assert res["joint_connection"] == ref["joint_connection"]
    ck_ref = torch.load(solo / "model.pth.tar", weights_only=False)
    assert list(ck["state_dict"]) == list(ck_ref["state_dict"]) and len(ck["state_dict"]) > 0
    for k, v in ck["state_dict"].items():
        assert torch.equal(v, ck_ref["state_dict"][k]), k
    assert open(kin / "result.txt").read() == open(solo / "result.txt").read()


# The two-rank child's time limit: five times the wall time of its first pass on an MI355X machine.
TWO_RANK_WALL_S = 8.1           # measured: the child's first pass, launcher start to exit (stage one 0.76 s, stage two 0.16 s inside it)
CHILD_TIMEOUT_S = 5 * TWO_RANK_WALL_S        # = 40.5 s
LAUNCH_TIMEOUT_S = CHILD_TIMEOUT_S - 10.5    # = 30 s: the launcher takes its ranks down before the test gives up on the child


def _close(a, b, rtol=1e-6):
    if a is None or b is None:
        return a is None and b is None
    return abs(a - b) <= rtol * abs(b)


def test_two_ranks_on_one_gpu_end_where_one_rank_ends(dev, tmp_path):
    """--gpus 2 --backend gloo --devices 0,0: the launcher starts two ranks of the real engine on GPU 0, each relaxes the
    instances the deal gives it and projects one of the two winners; records and reports travel through gloo (host memory).
    One rank with the same arguments picks the same winners and ends every instance and both projections with the same
    figures (rtol 1e-6: the bound between a sweep and a solo engine in test_sweep_command_line_readme_recipe)."""
    from reart_amd import sweep

    common = ["--synthetic", "2", "--synthetic_frames", "5", "--num_points", "512", "--n_iter", "150", "--use_flow_loss", "--energy",
              "--project", "--project_iter", "40"]
    two = tmp_path / "two"
    t0 = time.perf_counter()
    child = subprocess.run([sys.executable, "-m", "reart_amd.sweep", "--gpus", "2", "--backend", "gloo", "--devices", "0,0", *common,
                            "--save_root", str(two), "--launch_timeout", str(LAUNCH_TIMEOUT_S)],
                           cwd=ROOT, stdout=subprocess.PIPE, timeout=CHILD_TIMEOUT_S)
    print(f"two-rank child: exit {child.returncode}, wall {time.perf_counter() - t0:.1f} s")
    assert child.returncode == 0
    line = json.loads(child.stdout.decode().strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["backend"] == "gloo" and len(line["ranks"]) == 2
    inst = [{"cano_idx": c} for _ in range(2) for c in range(5)]
    plan = sweep.deal(inst, 2, "round_robin")
    for r, info in enumerate(line["ranks"]):
        assert info["rank"] == r and info["device"] == "cuda:0" and info["instances"] == plan[r]
    assert line["projected"] == {"synthetic_0": 0, "synthetic_1": 1}              # the two projections ran on different ranks
    sw2 = json.load(open(two / "sweep.json"))
    print("two ranks: stage one", sw2["wall_s"], "s, stage two", sw2["project_wall_s"], "s, total", sw2["total_wall_s"], "s;",
          {k: v["projection"]["wall_s"] for k, v in sw2["sequences"].items()})
    assert sw2["world_size"] == 2 and sw2["backend"] == "gloo"

    one = tmp_path / "one"
    assert sweep.main([*common, "--save_root", str(one)]) == 0
    sw1 = json.load(open(one / "sweep.json"))
    print("one rank: stage one", sw1["wall_s"], "s, stage two", sw1["project_wall_s"], "s")
    for name in ("synthetic_0", "synthetic_1"):
        a, b = sw2["sequences"][name], sw1["sequences"][name]
        assert a["winner_cano_idx"] == b["winner_cano_idx"] is not None, name
        assert [r["rank"] for r in a["instances"]] == [(5 * int(name[-1]) + c) % 2 for c in range(5)]
        for ra, rb in zip(a["instances"], b["instances"]):
            assert ra["failed"] == rb["failed"] == 0 and ra["iterations"] == rb["iterations"] == 150
            for k in ("recon_loss", "flow_loss", "total_loss", "total_err"):
                print(name, ra["cano_idx"], k, ra[k], rb[k])
                assert _close(ra[k], rb[k]), (name, ra["cano_idx"], k, ra[k], rb[k])
        pa, pb = a["projection"], b["projection"]
        print(name, "projection total_err", pa["total_err"], pb["total_err"])
        assert pa["failed"] == pb["failed"] == 0 and pa["iterations"] == pb["iterations"] == 40
        assert pa["device"] == pb["device"] == "cuda:0" and pa["cano_idx"] == pb["cano_idx"] == a["winner_cano_idx"]
        assert _close(pa["total_err"], pb["total_err"]), (name, pa["total_err"], pb["total_err"])
        for d in (two, one):
            assert all((d / name / "kinematic" / f).exists() for f in ("result.pkl", "model.pth.tar", "result.txt"))
