"""The bench command lines themselves (short runs): the JSON contract of every configuration -- one line on stdout, the
metric / config / roofline / cpu_baseline keys the driver and the judge read."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*argv, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines                     # exactly ONE line on stdout
    return json.loads(lines[0])


def test_headline_line_contract(dev):
    d = _run("--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--no-cpu-baseline", "--no-secondary", "--no-tail",
             "--sweep-instances", "0")
    assert d["metric"] == "relaxation-loop iterations/sec" and d["unit"] == "iterations/s" and d["n_gpus"] == 1
    assert d["steps"] == 20 and d["warmup"] == 5 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert abs(d["ms_per_step"] * d["value"] - 1e3) < 1.0 and d["value"] > 1000
    c = d["config"]
    assert c["frames"] == 20 and c["points"] == 4096 and c["flow"] is True and c["eager_steps"] == 0 and c["graph_replays"] >= 1
    r = d["roofline"]
    assert r["bound"] == "valu" and 0 < r["frac"] < 1 and r["kernel_ms"] < d["ms_per_step"]
    assert r["algorithmic_frac"] > r["frac"] and r["hbm_gbs"] < 0.2 * 8000 and r["executed_pairs_per_launch"] < r["algorithmic_pairs_per_launch"]
    assert r["traffic"] is None or isinstance(r["traffic"], (int, float))        # a number of bytes (or null), as the contract says
    # the launch chain with its arithmetic removed, measured in the run: below the step, the small kernels' share below the whole
    assert 0 < r["step_floor_small_kernels_us"] < r["step_floor_us"] < 1e3 * d["ms_per_step"] and 0 < r["step_floor_frac"] < 1


def test_plain_run_is_the_headline_alone(dev):
    """Without --full the line carries the headline and what the timed steps measured themselves (the search launch's device
    stamps), and nothing that takes runs of its own: no sweep, phases, launch-chain floor, CPU baselines, end-of-run or secondary."""
    d = _run("--gpus", "1", "--steps", "20", "--warmup", "5")
    assert d["metric"] == "relaxation-loop iterations/sec" and d["unit"] == "iterations/s" and d["n_gpus"] == 1
    assert d["steps"] == 20 and d["warmup"] == 5 and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["ms_per_step"] * d["value"] - 1e3) < 1.0 and d["value"] > 1000
    assert d["config"]["graph_replays"] >= 1 and d["config"]["eager_steps"] == 0
    r = d["roofline"]
    assert r["bound"] == "valu" and 0 < r["frac"] < 1 and r["kernel_ms"] < d["ms_per_step"] and r["launches_measured"] == 20
    assert not any(k.startswith("step_floor") for k in r), r
    assert d["sweep"] is None and d["phases_ms"] == {} and d["end_of_run"] is None
    assert d["cpu_baseline"] is None and d["cpu_baseline_torch"] is None and "secondary" not in d


def test_dump_outputs(dev, tmp_path):
    """--dump-outputs DIR: what the last timed iteration computed, as float32 / float64 .npy files under 64 MB, consistent with the
    line; --steps sets the timed iterations (one loss row each) and the warm-up comes on top."""
    d = _run("--gpus", "1", "--steps", "7", "--warmup", "3", "--no-cpu-baseline", "--no-secondary", "--no-tail", "--sweep-instances", "0",
             "--profile-steps", "0", "--dump-outputs", str(tmp_path))
    a = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(a) == {"losses", "loss_log", "pc_trans", "seg_part", "trans_list", "iterations",
                      "seg_w1", "seg_b1", "seg_w2", "proposal_6d", "proposal_t"}
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert d["steps"] == 7 and a["loss_log"].shape == (7, 4) and a["iterations"].tolist() == [10.0]
    np.testing.assert_array_equal(a["loss_log"][-1], a["losses"])
    np.testing.assert_allclose(a["losses"][:2], [d["final_losses"]["recon"], d["final_losses"]["flow"]], rtol=1e-4)
    assert a["pc_trans"].shape == (19, 4096, 3) and a["trans_list"].shape == (19, 20, 4, 4)
    seg = a["seg_part"]
    assert seg.shape == (4096,) and (seg == np.round(seg)).all() and 0 <= seg.min() and seg.max() < 20


def _strings(x, path=""):
    if isinstance(x, dict):
        for k, v in x.items():
            yield from _strings(v, f"{path}.{k}")
    elif isinstance(x, list):
        for i, v in enumerate(x):
            yield from _strings(v, f"{path}[{i}]")
    elif isinstance(x, str):
        yield path, x


def test_default_line_fits_the_drivers_record(dev):
    """`python bench.py --full` with every leg (short windows): ONE line of at most 5 KB -- numbers and labels of at most 80
    characters, no prose -- so that the tail the driver stores holds secondary.*.value, sweep.per_gpu, end_of_run, rccl_world
    and ranks; per-solve percentiles and the bounded sample of the README.md:125 projection are in it."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "100", "--warmup", "150"], capture_output=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1
    assert len(lines[0]) <= 5 * 1024, len(lines[0])
    d = json.loads(lines[0])
    long_ = [(p_, len(s_)) for p_, s_ in _strings(d) if len(s_) > 80]
    assert not long_, long_
    assert d["rccl_world"] == 1 and d["ranks"][0]["rank"] == 0 and d["sweep"]["per_gpu"] > 0 and "energy_ms" in d["end_of_run"]
    sec = d["secondary"]
    for name in ("kinematic", "extractor", "nao", "nao_recipe", "nao_projection"):
        assert "error" not in sec[name], sec[name]
        assert sec[name]["value"] > 0
    for name in ("kinematic", "nao_recipe", "nao_projection"):
        rf = sec[name]["roofline"]
        assert rf["solve_ms_p50"] <= rf["solve_ms_p95"] <= rf["solve_ms_max"] and sec[name]["lap_fallbacks"] == 0
    assert 0 < sec["nao_recipe"]["roofline"]["frac_search_only"] <= sec["nao_recipe"]["roofline"]["frac"] < 1
    assert sec["nao_recipe"]["snapshots"] == 150 and sec["nao_projection"]["snapshots"] == 151
    assert len(sec["nao_projection"]["iterations_per_s_by_window"]) == 3
    # BASELINE configs[4] on its own data (VERDICT r05 missing #2): CPU baseline, latency fraction, and both modes of the loop
    pr = sec["nao_projection"]
    assert pr["cpu_baseline"]["value"] > 0 and pr["cpu_baseline"]["cores"] >= 1
    assert 0 < pr["roofline"]["frac_search_only"] <= pr["roofline"]["frac"] < 1
    assert pr["deterministic"] is True and pr["other_mode"]["deterministic"] is False and pr["other_mode"]["value"] > 0
    assert len(pr["ties"]) == 2 and pr["ties"][0] >= pr["ties"][1] >= 0
    # 1 500 iterations x 9 problems meet one to three tied problems.  A dozen means the certificate is REPAIRING potentials (such a
    # problem comes back flagged 2, its pairs stale, and the host lists them): a form of the row reduction that rounded the incoming
    # prices by 1e-14 of the cost scale did that -- every solver test green, this leg 11 % slower (profiles/r06_lap_arr_packed_variant.hip.txt)
    assert pr["ties"][0] <= 5, pr["ties"]
    assert sec["nao"]["cpu_baseline_torch"]["value"] > 0
    assert d["ranks"][0]["it_per_s"] > 1000 and d["ranks"][0]["elapsed_s"] > 0


def test_nao_config_line(dev):
    """BASELINE configs[2] on the reference's demo sequence (data inside tests/golden/structure.npz), shortened."""
    d = _run("--config", "nao", "--steps", "400", "--no-cpu-baseline")
    assert d["metric"] == "relaxation-loop iterations/sec" and d["config"]["frames"] == 10 and d["config"]["points"] == 4096
    assert d["steps"] + d["warmup"] == 400 and d["value"] > 1000 and d["config"]["eager_steps"] < 50
    assert len(d["config"]["matches_per_pair"]) == 9 and all(v == v for v in d["final_losses"])
    assert d["roofline"]["launches_measured"] == d["steps"]


def test_extractor_config_line(dev):
    d = _run("--config", "extractor", "--steps", "3", "--warmup", "1", "--no-cpu-baseline")
    assert d["unit"] == "clouds/s" and d["config"]["clouds"] == 38 and d["roofline"]["bound"] == "mfma" and d["finite"] is True
    assert 0.1 < d["roofline"]["frac"] < 1
