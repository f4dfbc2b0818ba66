"""Yardstick of the fused step's combined loss mode (reart_relax_config.recon_with_assign): one relaxation iteration with
the Chamfer loss AND the assignment loss, as the reference's run_real.py:175-203 / run_sapien.py:174-203 add them.

``step_both`` restates ``oracle.step.RelaxOracle.step`` from the same oracle functions and works on a ``RelaxOracle``'s
state (parameters, Adam moments, iteration counter), so that the two can be compared bit for bit where they overlap
(tests/test_relax_both_ref_cpu.py): with ``assign=None`` it is that method, with ``chamfer=False`` it is that method with
``assign=``.  With both terms the gradient w.r.t. pc_trans is summed in float32 in the order

    G = (gx1 + gx2) + G_assign (+ G_flow)

which is the order the HIP consumer uses: the complete Chamfer gradient, then the assignment term, then the flow term (added
by the model's backward)."""
import numpy as np

from oracle import (adam, base_backward, base_forward, blend_anchor_motion, flow_loss, knn_points, knn_points_backward)
from oracle.step import tau_cosine


def step_both(orc, gumbel, tau=None, assign=None, chamfer=True):
    """One iteration on the state of ``orc`` (a RelaxOracle).  assign = (src_idx [n], tgt_idx [B,n], lambda_assign) or None.
    -> dict with recon (Chamfer sum, 0.0 without it), ass (lambda * sum of squared pair distances, 0.0 without pairs), flow,
    total, tau, pc_trans, G, grads, seg_part, hard_idx."""
    assert chamfer or assign is not None
    p = orc.params
    if tau is None:
        tau = tau_cosine(orc.it + 1, orc.n_iter, orc.end_tau, orc.start_tau)
    tau = float(np.float32(tau))
    fw = base_forward(orc.cano, p["W1"], p["b1"], p["W2"], p["p6d"], p["pt"], gumbel, tau)
    X, Y = fw["out"], orc.pc_list
    B, N = X.shape[:2]
    recon, ass, G = 0.0, 0.0, None
    if chamfer:
        d1, i1 = knn_points(X, Y)
        d2, i2 = knn_points(Y, X)
        recon = float((d1[..., 0] + d2[..., 0]).astype(np.float64).sum())
        ones = np.ones((B, N, 1), np.float32)
        gx1, _ = knn_points_backward(X, Y, i1, ones)
        _, gx2 = knn_points_backward(Y, X, i2, ones)
        G = gx1 + gx2
    if assign is not None:
        src, tgt, lam = assign
        lam = np.float32(lam)
        Ga = np.zeros_like(X)
        for b_ in range(B):
            d = X[b_, src] - Y[b_, tgt[b_]]
            ass += float(((d * d)[:, 0] + (d * d)[:, 1] + (d * d)[:, 2]).astype(np.float64).sum())
            Ga[b_, src] = lam * (np.float32(2.0) * d)
        ass *= float(lam)
        G = Ga if G is None else G + Ga
    flow = 0.0
    if orc.refs is not None:
        comp = np.concatenate([X[: orc.cano_idx], orc.cano[None], X[orc.cano_idx:]], axis=0)
        gtf = np.empty((B, N, 3), np.float32)
        msk = np.empty((B, N), bool)
        for f_ in range(B):
            gtf[f_], msk[f_] = blend_anchor_motion(comp[f_], orc.refs[f_], orc.ref_flows[f_], 3, orc.euclidean)
        pred = comp[1:] - comp[:-1]
        fl, gpf = flow_loss(gtf, pred, msk, orc.robust, orc.smooth)
        flow = orc.lambda_flow * fl
        gpf = gpf * np.float32(orc.lambda_flow)
        gcomp = np.zeros_like(comp)
        gcomp[1:] += gpf
        gcomp[:-1] -= gpf
        G = G + np.concatenate([gcomp[: orc.cano_idx], gcomp[orc.cano_idx + 1:]], axis=0)
    assert G.dtype == np.float32
    g = base_backward(orc.cano, p["W1"], p["b1"], p["W2"], p["p6d"], p["pt"], fw["y_soft"], fw["hard_idx"], tau, G)
    orc.it += 1
    for k, gk in (("W1", "gW1"), ("b1", "gb1"), ("W2", "gW2"), ("p6d", "g6d"), ("pt", "gt")):
        gr = g[gk].reshape(-1)
        if orc.weight_decay != 0:
            gr = (gr + orc.weight_decay * p[k].reshape(-1)).astype(np.float32)
        adam(p[k].reshape(-1), gr, orc.m[k].reshape(-1), orc.v[k].reshape(-1), orc.it, orc.lr[k])
    return dict(recon=recon, ass=ass, flow=flow, total=recon + ass + flow, tau=tau, pc_trans=X, G=G, grads=g,
                seg_part=fw["seg_part"], hard_idx=fw["hard_idx"])


def problem(seed=21, N=260, P=12, B=3, H=128, ref_lens=(150, 90, 200)):
    """The instance of tests/test_step_gpu.py::test_assignment_loss_step_matches_oracle (same draws in the same order for the
    defaults): clouds, initial parameters, ragged flow references; the generator is returned for the noise and the pairs."""
    rng = np.random.default_rng(seed)
    cano = rng.uniform(-0.3, 0.3, (N, 3)).astype(np.float32)
    pcs = (cano[None] + rng.normal(0, 0.02, (B, N, 3))).astype(np.float32)
    W1, b1 = rng.normal(0, 0.6, (H, 3)).astype(np.float32), rng.normal(0, 0.1, H).astype(np.float32)
    W2 = rng.normal(0, 0.2, (P, H)).astype(np.float32)
    p6d = (np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), (B, P, 1)) + rng.normal(0, 0.05, (B, P, 6))).astype(np.float32)
    pt = rng.normal(0, 0.01, (B, P, 3)).astype(np.float32)
    refs = [rng.uniform(-0.3, 0.3, (m, 3)).astype(np.float32) for m in ref_lens]
    flows = [rng.normal(0, 0.02, r.shape).astype(np.float32) for r in refs]
    return dict(cano=cano, pcs=pcs, W1=W1, b1=b1, W2=W2, p6d=p6d, pt=pt, refs=refs, flows=flows, rng=rng, N=N, P=P, B=B, H=H)


def gumbel(rng, N, P):
    return -np.log(rng.exponential(size=(N, P))).astype(np.float32)
