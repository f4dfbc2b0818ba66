"""numpy float64 restatement of one iteration's flow term (reference run_robot.py:194-209): brute-force K = 3 neighbours with
the lowest-index tie rule, blend_anchor_motion (utils/flow_utils.py:147-170), flow_loss (networks/loss.py:10-21) and the gradient
that autograd carries through ``cat`` and the subtraction.  Test infrastructure: held to tests/golden/flow_term.npz by
test_flow_term_cpu.py, used by the GPU tests for the double sum of the per-point terms."""
import numpy as np


def complete(pc_trans, cano, c):
    return np.concatenate((pc_trans[:c], cano[None], pc_trans[c:]), axis=0)


def knn3(query, ref, squared=False):
    """(dists [m,3], idx [m,3]) ascending by (distance, index)."""
    d = ((query[:, None, :] - ref[None, :, :]) ** 2).sum(-1)
    idx = np.argsort(d, axis=1, kind="stable")[:, :3]
    dd = np.take_along_axis(d, idx, axis=1)
    return (dd if squared else np.sqrt(dd)), idx


def blend(dists, idx, ref_flow):
    d = np.maximum(dists, 1e-10)
    w = 1.0 / d
    w = w / w.sum(-1, keepdims=True)
    f = ref_flow[idx]                                        # [m,3,3]
    flow = (f * w[..., None]).sum(1)
    mask = (d.min(-1) <= (f ** 2).sum(-1).max(-1)) | (d.min(-1) <= 0.05)
    return flow, mask


def point_terms(gt, pred, mask, robust=False, smooth_weight=1e-2):
    """Per-point loss terms [B,N] and d (sum of them) / d pred [B,N,3]."""
    d = pred - gt
    if robust:
        a = np.abs(d)
        f = np.where(a <= 1.0, 0.5 * d * d, a - 0.5).sum(-1)
        gf = np.where(a <= 1.0, d, np.sign(d))
    else:
        f = (d * d).sum(-1)
        gf = 2.0 * d
    terms = np.where(mask, f, smooth_weight * (pred ** 2).sum(-1))
    grad = np.where(mask[..., None], gf, smooth_weight * 2.0 * pred)
    return terms, grad


def flow_term(pc_trans, cano, refs, flows, c, weight=1.0, robust=False, smooth_weight=1e-2, squared=False):
    """-> dict(gt [B,N,3], mask [B,N], dists, idx [B,N,3], terms [B,N], loss, grad [B,N,3] = d loss / d pc_trans), float64."""
    pc_trans, cano = np.asarray(pc_trans, np.float64), np.asarray(cano, np.float64)
    comp = complete(pc_trans, cano, c)
    B = pc_trans.shape[0]
    out = [[], [], [], []]
    for f in range(B):
        d, i = knn3(comp[f], np.asarray(refs[f], np.float64), squared)
        fl, m = blend(d, i, np.asarray(flows[f], np.float64))
        for o, v in zip(out, (fl, m, d, i)):
            o.append(v)
    gt, mask, dists, idx = (np.stack(o) for o in out)
    terms, gp = point_terms(gt, comp[1:] - comp[:-1], mask, robust, smooth_weight)
    gp = gp * weight
    gcomp = np.zeros_like(comp)
    gcomp[1:] += gp
    gcomp[:-1] -= gp
    grad = np.concatenate((gcomp[:c], gcomp[c + 1:]), axis=0)
    return dict(gt=gt, mask=mask, dists=dists, idx=idx, terms=terms, loss=weight * terms.sum(), grad=grad)
