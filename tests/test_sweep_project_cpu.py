"""CPU: the device map of the ranks (launch.parse_devices / local_device, --devices) and stage two of the sweep (--project: the
winners dealt to the ranks and projected) with two gloo ranks.  The per-instance runner and the projector are stand-ins that
record who was called with what: the dealing, the reporting and the failure handling are what is tested here; the GPU
projection itself is tests/test_sweep_project_gpu.py."""
import json
import os
import shutil

import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ_TINY = os.path.join(ROOT, "tests", "golden", "seq_tiny")
POINTS = 64


def test_parse_devices():
    from reart_amd import launch

    assert launch.parse_devices("0,0", 2) == [0, 0]
    assert launch.parse_devices(" 3, 1 ,2", 3) == [3, 1, 2]
    assert launch.parse_devices("5", 1) == [5]
    for text, nproc, word in (("0", 2, "one entry per rank"), ("0,1,2", 2, "one entry per rank"), ("0,-1", 2, "negative"),
                              ("0,x", 2, "not a GPU ordinal"), ("0,,1", 3, "not a GPU ordinal"), ("0,1.5", 2, "not a GPU ordinal"),
                              ("", 1, "not a GPU ordinal")):
        with pytest.raises(SystemExit) as e:
            launch.parse_devices(text, nproc)
        assert word in str(e.value), (text, str(e.value))


def test_local_device():
    from reart_amd import launch

    assert [launch.local_device(r, env={}) for r in range(4)] == [0, 1, 2, 3]          # the default: rank r on GPU r
    assert [launch.local_device(r, [0, 0, 2], env={}) for r in range(3)] == [0, 0, 2]  # an explicit map
    assert launch.local_device(1, "4,6", env={}) == 6                                   # ... as the flag's text
    env = {"REART_LOCAL_DEVICES": "1,1"}
    assert [launch.local_device(r, env=env) for r in range(2)] == [1, 1]               # the environment variable
    assert [launch.local_device(r, [0, 3], env=env) for r in range(2)] == [0, 3]       # the flag wins over it
    assert launch.local_device(2, env={"REART_LOCAL_DEVICES": ""}) == 2                # empty = unset
    for kw in (dict(devices=[0, 0], env={}), dict(env=env)):
        with pytest.raises(SystemExit):
            launch.local_device(2, **kw)                                                # a rank the map does not name
    with pytest.raises(SystemExit):
        launch.local_device(0, env={"REART_LOCAL_DEVICES": "0,a"})


def test_launch_imports_nothing_from_torch():
    import subprocess
    import sys

    # the file on its own (the package's __init__ is not the launcher's business), in a fresh interpreter
    code = ("import importlib.util, sys\n"
            f"spec = importlib.util.spec_from_file_location('launch_alone', {os.path.join(ROOT, 'reart_amd', 'launch.py')!r})\n"
            "l = importlib.util.module_from_spec(spec); spec.loader.exec_module(l)\n"
            "assert l.local_device(1) == 1 and l.parse_devices('0,0', 2) == [0, 0]\n"
            "assert not [m for m in sys.modules if m == 'torch' or m.startswith('torch.')]\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr.decode()


def test_parent_checks_the_device_map_before_it_spawns(monkeypatch):
    from reart_amd import launch, sweep

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "REART_LOCAL_DEVICES"):
        monkeypatch.delenv(k, raising=False)
    reached = []

    def no_launch(*a, **kw):
        reached.append((a, kw))
        return 77

    monkeypatch.setattr(launch, "self_launch", no_launch)
    base = ["--gpus", "2", "--synthetic", "1", "--save_root", "unused"]
    for extra in ([], ["--backend", "nccl"]):                       # the default backend counts as "not gloo"
        with pytest.raises(SystemExit) as e:
            sweep.main(base + ["--devices", "0,0"] + extra)
        assert "--backend gloo" in str(e.value)
    for bad in ("0", "0,1,2", "0,-1", "0,x"):
        with pytest.raises(SystemExit):
            sweep.main(base + ["--devices", bad, "--backend", "gloo"])
    monkeypatch.setenv("REART_LOCAL_DEVICES", "1,1")                 # the environment variable is checked like the flag
    with pytest.raises(SystemExit) as e:
        sweep.main(base)
    assert "--backend gloo" in str(e.value)
    assert not reached, "a refused device map must not start ranks"
    # what is allowed reaches the launcher, with the time limit of --launch_timeout (default: none)
    assert sweep.main(base + ["--devices", "0,0", "--backend", "gloo", "--launch_timeout", "12.5"]) == 77
    assert sweep.main(base + ["--devices", "0,1"]) == 77
    monkeypatch.delenv("REART_LOCAL_DEVICES")
    assert sweep.main(base) == 77
    assert [kw.get("timeout") for _, kw in reached] == [12.5, None, None]
    assert reached[0][0][1][-2:] == ["--launch_timeout", "12.5"] and reached[0][0][2] == 2


def test_project_with_a_runner_needs_a_projector(tmp_path):
    from reart_amd import sweep

    with pytest.raises(SystemExit) as e:
        sweep.main(["--synthetic", "1", "--project", "--save_root", str(tmp_path)], runner=lambda spec: {})
    assert "projector" in str(e.value) and not os.listdir(tmp_path)


# ---------------------------------------------------------------------------------------------------------------------------
# two gloo ranks, a runner and a projector

def _runner(spec):
    """Made-up results that depend on the instance alone; every instance of seq_c fails (a sequence without a winner).  The
    labels carry the instance id: a projector can tell whose result.pkl it was handed."""
    import numpy as np

    if spec["seq"] == "seq_c":
        raise RuntimeError("injected failure")
    c, B, P = spec["cano_idx"], spec["frames"] - 1, 3
    ass = 1.0 + abs(c - 1) + 0.125 * len(spec["seq"])
    return dict(recon=0.5 + c, flow=0.0, total=0.5 + c, iterations=2, parts=P, ass_err=ass, screw_err=0.25, group_err=0.5,
                total_err=ass + 0.75, cd_err=0.1, seg_part=np.full(POINTS, spec["id"], np.int64),
                trans_list=np.tile(np.eye(4, dtype=np.float32), (B, P, 1, 1)), joint_connection=np.array([[0, 1], [1, 2]]))


def _projector(spec, base):
    """Records the call (one line per call in a file of this rank), fails for seq_d, and reports what it saw in the base result."""
    with open(os.path.join(os.environ["PROJECT_LOG_DIR"], f"calls_{os.environ['RANK']}.txt"), "a") as f:
        f.write(f"{spec['seq']} {spec['cano_idx']} {int(base['pred_cano_part'][0])} {base['cano_idx']}\n")
    if spec["seq"] == "seq_d":
        raise RuntimeError("injected projection failure")
    return dict(iterations=7, parts=int(base["pred_cano_part"][0]), joint_connection=base["joint_connection"], total_err=1.5,
                ass_err=1.0, screw_err=0.25, group_err=0.25, cd_err=0.5, assign_refreshes=7, lap_fallbacks=0, model=object())


def _rank(rank, world, port, seq_root, save_root, project):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      PROJECT_LOG_DIR=save_root)
    os.environ.pop("REART_LOCAL_DEVICES", None)
    from reart_amd import sweep

    argv = ["--seq_root", seq_root, "--cano", "all", "--n_iter", "2", "--energy", "--gpus", str(world), "--shard", "lpt",
            "--num_points", str(POINTS), "--save_root", save_root]
    rc = sweep.main(argv + (["--project"] if project else []), runner=_runner, projector=_projector if project else None)
    assert rc == 0


@pytest.fixture(scope="module")
def two_jobs(tmp_path_factory):
    """The same two-rank sweep with and without --project, side by side (four processes) -> (sequence root, the two save roots)."""
    from reart_amd.launch import free_port

    tmp = tmp_path_factory.mktemp("sweep_project")
    root = tmp / "seqs"
    for name in ("seq_a", "seq_c", "seq_d"):                            # 4 frames each
        shutil.copytree(SEQ_TINY, root / name)
    (root / "seq_b").mkdir()
    for f in ("state_0.pkl", "state_1.pkl", "pose_1.pkl"):            # a 2-frame sequence in the reference's layout
        shutil.copy(os.path.join(SEQ_TINY, f), root / "seq_b" / f)
    ctx = mp.get_context("spawn")
    procs = []
    for out, project in ((tmp / "with", True), (tmp / "without", False)):
        out.mkdir()
        port = free_port()
        procs += [ctx.Process(target=_rank, args=(r, 2, port, str(root), str(out), project)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    return root, tmp / "with", tmp / "without"


def test_winners_are_projected_once_by_the_rank_the_deal_names(two_jobs):
    from reart_amd import sweep

    root, out, _ = two_jobs
    sw = json.load(open(out / "sweep.json"))
    seqs = sw["sequences"]
    assert {k: v["winner_cano_idx"] for k, v in seqs.items()} == {"seq_a": 1, "seq_b": 1, "seq_c": None, "seq_d": 1}
    # the deal of stage two, from the winners' specs as every rank knows them: longest first, seq_b (2 frames) fills up rank 0
    inst = sweep.enumerate_instances(sweep.list_sequences(str(root)), "all")
    for s in inst:
        s["points"] = POINTS
    won = [inst[seqs[n]["winner_instance"]] for n in seqs if seqs[n]["winner_instance"] is not None]
    assert [s["seq"] for s in won] == ["seq_a", "seq_b", "seq_d"]
    plan = sweep.deal(won, 2, "lpt")
    assert plan == [[0, 1], [2]] and plan != sweep.deal(won, 2, "round_robin")
    want_rank = {won[k]["seq"]: r for r, ids in enumerate(plan) for k in ids}
    calls = {r: [line.split() for line in open(out / f"calls_{r}.txt")] for r in range(2)}
    seen = [(c[0], r) for r in calls for c in calls[r]]
    assert sorted(seen) == sorted(want_rank.items())                   # each exactly once, on the rank the deal names; seq_c never
    for r in calls:
        for name, cano, marker, base_cano in calls[r]:
            w = seqs[name]
            # the base result is the WINNER's own file (its labels carry its instance id), not another instance's
            assert int(cano) == int(base_cano) == w["winner_cano_idx"] and int(marker) == w["winner_instance"]
    assert [c[0] for c in calls[0]] == ["seq_a", "seq_b"]              # one after another, in the deal's order


def test_projection_reports(two_jobs):
    _, out, _ = two_jobs
    sw = json.load(open(out / "sweep.json"))
    seqs = sw["sequences"]
    fields = {"rank", "device", "cano_idx", "iterations", "failed", "parts", "joint_connection", "total_err", "ass_err", "screw_err",
              "group_err", "cd_err", "assign_refreshes", "lap_fallbacks", "wall_s"}
    assert "projection" not in seqs["seq_c"]                           # no winner: skipped
    for name in ("seq_a", "seq_b", "seq_d"):
        assert set(seqs[name]["projection"]) == fields, name
    a, b, d = (seqs[n]["projection"] for n in ("seq_a", "seq_b", "seq_d"))
    assert (a["rank"], b["rank"], d["rank"]) == (0, 0, 1) and a["device"] == "cpu"
    for p, name in ((a, "seq_a"), (b, "seq_b")):
        assert p["failed"] == 0 and p["iterations"] == 7 and p["parts"] == seqs[name]["winner_instance"] and p["cano_idx"] == 1
        assert p["joint_connection"] == [[0, 1], [1, 2]] and p["total_err"] == 1.5 and p["cd_err"] == 0.5
        assert p["assign_refreshes"] == 7 and p["lap_fallbacks"] == 0 and p["wall_s"] >= 0
    # a projection that raises is reported and the others finish
    assert d["failed"] == 1 and d["cano_idx"] == 1 and d["total_err"] is None and d["iterations"] is None
    assert sw["project_wall_s"] >= 0 and sw["total_wall_s"] >= sw["wall_s"]


def test_existing_fields_keep_their_values(two_jobs):
    _, out, plain = two_jobs
    sw, ref = json.load(open(out / "sweep.json")), json.load(open(plain / "sweep.json"))
    timing = {"wall_s", "iterations_per_s"}
    assert list(ref) == [k for k in sw if k in ref]                    # keys only added, the old ones in their places
    assert set(sw) - set(ref) == {"project_wall_s", "total_wall_s"}
    for k in ref:
        if k in timing or k == "sequences":
            continue
        assert sw[k] == ref[k], k
    for name, seq in ref["sequences"].items():
        got = dict(sw["sequences"][name])
        got.pop("projection", None)
        assert got == seq, name
    # the winners' base results stay where they were, next to the (stand-in: empty) kinematic stage
    for name in ("seq_a", "seq_b", "seq_d"):
        assert open(out / name / "result.pkl", "rb").read() == open(plain / name / "result.pkl", "rb").read()
