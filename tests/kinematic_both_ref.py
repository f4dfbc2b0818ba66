"""Helpers of tests/test_kinematic_both_gpu.py (KinematicEngine's recon_with_assign mode): the inputs of one
``reart_kin_post_recon`` call, the same part as tensor expressions that round as the kernel does, and the golden kinematic
problem of tests/test_kinematic_engine_gpu.py at a chosen size.  Not a test module."""
import os

import numpy as np
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAM_A, LAM_F, SMOOTH = 0.3, 0.7, 1e-2


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def kernel_case(dev, B, N, n, c, flow, perm, seed=0):
    """Random inputs of one call: clouds in (-0.3, 0.3), g_recon in (-2, 2), a sample of n points (the slot array is -1
    elsewhere), a permutation per frame as the optimum, ragged reference sets of 3 ... 40 points, inv_x None or a permutation."""
    rng = np.random.default_rng(1000 * B + N + 7 * c + seed)
    f32 = lambda lo, hi, *s: rng.uniform(lo, hi, s).astype(np.float32)
    case = {"B": B, "N": N, "n": n, "c": c, "flow": flow}
    case["pc_trans"], case["cano"] = t(f32(-0.3, 0.3, B, N, 3), dev), t(f32(-0.3, 0.3, N, 3), dev)
    src = np.sort(rng.permutation(N)[:n])
    slot = np.full((N,), -1, np.int32)
    slot[src] = np.arange(n, dtype=np.int32)
    case["src"], case["slot"] = t(src.astype(np.int64), dev), t(slot, dev)
    case["pc_src"] = case["pc_trans"][:, case["src"]].contiguous() if n else None
    case["tgt"] = t(f32(-0.3, 0.3, B, n, 3), dev) if n else None
    case["cols"] = t(np.stack([rng.permutation(n) for _ in range(B)]).astype(np.int32), dev) if n else None
    case["g_recon"] = t(f32(-2.0, 2.0, B, N, 3), dev)
    case["inv_x"] = t(rng.permutation(N).astype(np.int32), dev) if perm else None
    case["loss_recon"] = t(np.float32(rng.uniform(1.0, 5.0)).reshape(()), dev)
    case["refs"] = case["flows"] = None
    if flow:
        lens = rng.integers(3, 41, B)
        lens[0], lens[-1] = 3, 40
        case["refs"] = [t(f32(-0.3, 0.3, int(m), 3), dev) for m in lens]
        case["flows"] = [t(rng.normal(0, 0.02, (int(m), 3)).astype(np.float32), dev) for m in lens]
    return case


def padded_refs(case, dev):
    """(ref, ref_flow, ref_len or None, nr_max) as KinematicEngine passes the reference sets."""
    if not case["flow"]:
        return None, None, None, 0
    lens = [int(r.shape[0]) for r in case["refs"]]
    nr = max(lens)
    rp = torch.zeros((case["B"], nr, 3), dtype=torch.float32, device=dev)
    fp = torch.zeros((case["B"], nr, 3), dtype=torch.float32, device=dev)
    for f, (r, fl) in enumerate(zip(case["refs"], case["flows"])):
        rp[f, :lens[f]], fp[f, :lens[f]] = r, fl
    ln = torch.tensor(lens, dtype=torch.int64, device=dev) if min(lens) != nr else None
    return rp, fp, ln, nr


def expressions(case, inv_x="case"):
    """(G, matched, [assignment, flow, Chamfer, total]) as tensor expressions, each sum rounded once in the kernel's order:
    the Chamfer gradient through inv_x (0 where the entry is outside [0, N)), + two_lambda x (pc_src - matched) at the sampled
    points, + the flow term's gradient (autograd of run_robot.py:194-209 over the per-frame blend and flow_loss); the total as
    OperatorLoop adds it: (assignment + Chamfer) + flow."""
    from reart_amd.knn_cuda import KNN
    from reart_amd.networks.loss import flow_loss
    from reart_amd.utils.flow_utils import blend_anchor_motion

    B, N, n, c = case["B"], case["N"], case["n"], case["c"]
    dev = case["pc_trans"].device
    inv = case["inv_x"] if isinstance(inv_x, str) else inv_x
    inv = torch.arange(N, device=dev) if inv is None else inv.long()
    ok = (inv >= 0) & (inv < N)
    sel = case["g_recon"].index_select(1, inv.clamp(0, N - 1))
    Gx = torch.where(ok[None, :, None], sel, torch.zeros_like(sel))
    ass = torch.zeros((), dtype=torch.float32, device=dev)
    matched = None
    if n:
        matched = case["tgt"].gather(1, case["cols"].long()[..., None].expand(-1, -1, 3))
        diff = case["pc_src"] - matched
        ass = LAM_A * (diff * diff).sum()
        Gx[:, case["src"]] = Gx[:, case["src"]] + (2.0 * LAM_A) * diff
    fl = torch.zeros((), dtype=torch.float32, device=dev)
    if case["flow"]:
        x = case["pc_trans"].clone().requires_grad_(True)
        comp = torch.cat((x[:c], case["cano"][None], x[c:]), dim=0)
        knn = KNN(k=3, transpose_mode=True)
        with torch.no_grad():
            blended = [blend_anchor_motion(q, r, f, knn, return_mask=True) for q, r, f in zip(comp[:-1], case["refs"], case["flows"])]
            gt, mask = torch.stack([b[0] for b in blended]), torch.stack([b[1] for b in blended])
        fl = LAM_F * flow_loss(gt, comp[1:] - comp[:-1], flow_mask_list=mask, robust=False, smooth_weight=SMOOTH)
        fl.backward()
        Gx = Gx + x.grad
        fl = fl.detach()
    total = (ass + case["loss_recon"]) + fl
    return Gx, matched, [float(ass), float(fl), float(case["loss_recon"]), float(total)]


def golden_model(dev, k, cano, seg, B=9):
    from reart_amd.knn_cuda import KNN
    from reart_amd.networks.model import KinematicModel

    edge_index = {f"{c}_{int(k['parent'][c])}": int(k["edge_of_part"][c]) for c in range(len(k["parent"])) if k["parent"][c] >= 0}
    return KinematicModel(pose_len=B, seg_part=seg, cano_pc=cano, knn=KNN(k=1, transpose_mode=True), edge_index=edge_index,
                          paths_to_base=None, reverse_topo=[int(v) for v in k["order"]], axis_list=t(k["axis"], dev),
                          moment_list=t(k["moment"], dev), theta_list=t(k["theta"][:B], dev)).to(dev)


def golden_problem(dev, seed, with_flow, N=1024, B=9):
    """The set-up of test_engine_equals_the_autograd_loop on the golden kinematic-2 checkpoint, its cloud subsampled to N points
    (labels included): frames of the model's own forward + continuous noise, every frame in its own point order, ragged
    reference sets.  -> (k, cano, seg, pcs, refs, flows, make_model)."""
    k = np.load(os.path.join(G, "kinematic.npz"))
    rng = np.random.default_rng(seed)
    keep = np.sort(rng.permutation(k["cano_pc"].shape[0])[:N])
    cano, seg = t(k["cano_pc"][keep], dev), t(k["seg_part"][keep], dev)
    make = lambda: golden_model(dev, k, cano, seg, B)
    with torch.no_grad():
        pcs = make()(cano)[0]
    pcs = (pcs + t(rng.normal(0, 0.004, (B, N, 3)).astype(np.float32), dev)).contiguous()
    pcs = torch.stack([p[torch.from_numpy(rng.permutation(N)).to(dev)] for p in pcs])
    refs = flows = None
    if with_flow:
        comp = torch.cat((pcs[:2], cano[None], pcs[2:]), dim=0)
        sel = [torch.from_numpy(rng.permutation(N)[:100 + 7 * f]).to(dev) for f in range(B)]
        refs = [comp[f][s] for f, s in enumerate(sel)]
        flows = [(comp[f + 1][s] - comp[f][s]) * 0.5 for f, s in enumerate(sel)]
    return k, cano, seg, pcs, refs, flows, make
