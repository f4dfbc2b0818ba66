"""The consumers of the searches with their loads batched: the single-record forms of the Chamfer merge and of the flow
blend's partial merge (taken when a query has ONE partial list: the box-pruned default) against the four-slice / looped
forms (search_mode 1: brute-force slices), alone and as K = 3 instances in shared launches.  Ragged reference sets, one of
3 points: fewer than three finite 8-target blocks, so the blend's rescan runs with absent blocks.  The trajectories must be
bit-identical across the forms and match the oracle's iteration at the tolerances of
tests/test_bwd_overlap_gpu.py::test_other_workgroup_geometries_and_batches_match_the_oracle_step."""
import numpy as np
import pytest
import torch

N, P, B, H, CANO_IDX = 300, 20, 4, 128, 1
LENS = [211, 137, 300, 3]
ITERS = 5
# (name, tuning, engines, stepped through a RelaxBatch).  The brute-force slices run as a single engine only: a RelaxBatch
# steps through reart_relax_step_batch, which takes the box-pruned geometry alone and answers REART_ERR_UNSUPPORTED for
# search_mode 1 at every K, 1 included.  At N = 300 the slices split every query's search in two (S = 2): the four-slice form.
FORMS = [("pruned", {}, 1, False), ("slices", {"search_mode": 1}, 1, False), ("pruned_batch1", {}, 1, True), ("pruned_batch3", {}, 3, True)]


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _instance(k):
    rng = np.random.default_rng(300 + k)
    cano = rng.uniform(-0.3, 0.3, (N, 3)).astype(np.float32)
    d = dict(cano=cano, pcs=(cano[None] + rng.normal(0, 0.02, (B, N, 3))).astype(np.float32),
             W1=rng.normal(0, 0.6, (H, 3)).astype(np.float32), b1=rng.normal(0, 0.1, H).astype(np.float32),
             W2=rng.normal(0, 0.2, (P, H)).astype(np.float32),
             p6d=(np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), (B, P, 1)) + rng.normal(0, 0.05, (B, P, 6))).astype(np.float32),
             pt=rng.normal(0, 0.01, (B, P, 3)).astype(np.float32),
             refs=[rng.uniform(-0.3, 0.3, (m, 3)).astype(np.float32) for m in LENS],
             flows=[rng.normal(0, 0.02, (m, 3)).astype(np.float32) for m in LENS],
             noise=[-np.log(rng.exponential(size=(N, P))).astype(np.float32) for _ in range(ITERS)])
    return d


_ORACLE = {}


def _oracle_trajectory(k):
    """ITERS oracle iterations of instance k, computed once: per iteration the losses, labels, clouds and parameters."""
    if k not in _ORACLE:
        from oracle.step import RelaxOracle

        d = _instance(k)
        orc = RelaxOracle(d["cano"], d["pcs"], d["W1"], d["b1"], d["W2"], d["p6d"], d["pt"], CANO_IDX, d["refs"], d["flows"],
                          lambda_flow=0.7, robust=False, n_iter=50)
        rows = []
        for i in range(ITERS):
            ref = orc.step(d["noise"][i])
            rows.append(dict(recon=ref["recon"], flow=ref["flow"], seg_part=np.array(ref["seg_part"]),
                             pc_trans=np.array(ref["pc_trans"]), params={k_: np.array(v) for k_, v in orc.params.items()}))
        _ORACLE[k] = rows
    return _ORACLE[k]


def test_the_oracle_accepts_every_instance(oracle):
    """CPU side: the oracle iterates all three instances (the 3-point reference set included) to finite losses."""
    assert min(LENS) == 3 and N % 64 and len(set(LENS)) == len(LENS)
    for k in range(3):
        rows = _oracle_trajectory(k)
        assert len(rows) == ITERS
        for r in rows:
            assert np.isfinite(r["recon"]) and np.isfinite(r["flow"]) and r["recon"] > 0 and r["flow"] > 0
            assert r["pc_trans"].shape == (B, N, 3) and np.isfinite(r["pc_trans"]).all()


def _run(dev, tuning, K, batched):
    """ITERS iterations of K engines, on their own or in one RelaxBatch; per engine and iteration every output."""
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxBatch, RelaxEngine

    inst = []
    for k in range(K):
        d = _instance(k)
        model = BaseModel(num_parts=P, pose_len=B).to(dev)
        with torch.no_grad():
            model.seg_head.model[0].weight.copy_(t(d["W1"], dev)[:, :, None]); model.seg_head.model[0].bias.copy_(t(d["b1"], dev))
            model.seg_head.model[2].weight.copy_(t(d["W2"], dev)[:, :, None])
            model.proposal_6d.copy_(t(d["p6d"], dev)); model.proposal_t.copy_(t(d["pt"], dev))
        eng = RelaxEngine(t(d["cano"], dev), t(d["pcs"], dev), model, CANO_IDX, [t(r, dev) for r in d["refs"]],
                          [t(f, dev) for f in d["flows"]], n_iter=50, lambda_flow=0.7, use_robust_loss=False, tuning=tuning)
        inst.append((d, model, eng))
    batch = RelaxBatch([e for _, _, e in inst]) if batched else None
    traj = [[] for _ in range(K)]
    for i in range(ITERS):
        for d, model, eng in inst:
            eng.set_gumbel(t(d["noise"][i], dev))
        if batch is not None:
            batch.step(1)
        else:
            inst[0][2].step()
        torch.cuda.synchronize()
        for k, (d, model, eng) in enumerate(inst):
            traj[k].append(dict(losses=eng.last_losses().cpu().numpy(), seg_part=eng.seg_part.cpu().numpy(),
                                pc_trans=eng.pc_trans.cpu().numpy(),
                                params={"p6d": model.proposal_6d.detach().cpu().numpy().copy(),
                                        "pt": model.proposal_t.detach().cpu().numpy().copy(),
                                        "W2": model.seg_head.model[2].weight.detach().cpu().numpy().copy(),
                                        "W1": model.seg_head.model[0].weight.detach().cpu().numpy().copy(),
                                        "b1": model.seg_head.model[0].bias.detach().cpu().numpy().copy()}))
    return traj


_GPU = {}


def _trajectory(dev, name):
    if name not in _GPU:
        _, tuning, K, batched = next(f for f in FORMS if f[0] == name)
        _GPU[name] = _run(dev, tuning, K, batched)
    return _GPU[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [f[0] for f in FORMS])
def test_trajectory_matches_the_oracle(oracle, dev, name):
    for k, traj in enumerate(_trajectory(dev, name)):
        for i, (got, ref) in enumerate(zip(traj, _oracle_trajectory(k))):
            row = got["losses"]
            print(f"{name} instance {k} iter {i}: recon {row[0]:.8e} (oracle {ref['recon']:.8e}), flow {row[1]:.8e} (oracle {ref['flow']:.8e})")
            assert abs(row[0] - ref["recon"]) <= 1e-5 * abs(ref["recon"]), (name, k, i, row, ref["recon"])
            assert abs(row[1] - ref["flow"]) <= 1e-5 * abs(ref["flow"]) + 1e-9, (name, k, i, row, ref["flow"])
            np.testing.assert_array_equal(got["seg_part"], ref["seg_part"])
            for key, v in got["params"].items():
                np.testing.assert_allclose(v.reshape(ref["params"][key].shape), ref["params"][key], rtol=0, atol=2e-5,
                                           err_msg=f"{name} instance {k} iter {i} param {key}")


@pytest.mark.gpu
def test_single_record_and_sliced_forms_agree_bit_for_bit(dev):
    """Instance 0 alone on the pruned path, alone on the brute-force slices, alone in a RelaxBatch and as the first of three
    in shared launches: the same bits in every output of every iteration."""
    base = _trajectory(dev, "pruned")[0]
    for name in ("slices", "pruned_batch1", "pruned_batch3"):
        other = _trajectory(dev, name)[0]
        for i, (x, y) in enumerate(zip(base, other)):
            for key in ("losses", "seg_part", "pc_trans"):
                assert x[key].tobytes() == y[key].tobytes(), (name, i, key)
            for key in x["params"]:
                assert x["params"][key].tobytes() == y["params"][key].tobytes(), (name, i, key)
