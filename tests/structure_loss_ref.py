"""Torch-autograd restatement of reart_structure_term (csrc/structure_term.hip; networks/loss.py structure_loss :32-57 of the
reference with compute_relative_trans, transform_to_dq, dq_to_screw, compute_mean_screw_param and the screw -> SE(3) map) and
of the reverse mode of the relative transform.  A restatement takes the dtype it computes in: float64 is the reference of
tests/test_structure_term_gpu.py, float32 is what rounding alone costs a correct implementation.  It builds on tests/kin_ref.py
(screw_ref, F32_1EM6), imports nothing of reart_amd and reads nothing outside the repository.

DECISIONS -- the quaternion branch of matrix_to_quaternion, no_rot, the sign alignment l . (1,1,1) >= 0, the |d| <= 1e-8 rule,
`unit`, `prismatic` and the no-rotation test and clamp of the screw map -- are taken on a float32 evaluation (against the
float32 constants the kernel holds) and handed to the evaluation in the requested dtype.  `assert_clear_of_thresholds` refuses a
case whose float32 and float64 decisions differ or whose decision inputs lie within a margin of a threshold.  The relative
transform is written entry by entry in the kernel's order of operations: a self pair (a, a) is then exactly the identity in
every dtype (the products of R^T R commute, the translation cancels term by term).

`mutate` plants one known error, so that a test can show that the comparison rejects it:
  "target_not_detached"   the fitted target takes part in the graph
  "cost_rule"             prismatic(e) decided like compute_screw_trans (prismatic cost <= revolute cost)
  "drop_src"              the gradient of the src part dropped
  "ignore_e1"             the plain mean of E <= 1 ignored (masked mean instead)
  ("scale", 1.001)        value and gradient times 1.001
"""
import functools
import math
import os

import numpy as np
import torch

from tests import kin_ref as kr

F32 = lambda v: float(np.float32(v))
EPS6, EPS5, EPS4, EPS8, PI_F = kr.F32_1EM6, F32(1e-5), kr.F32_1EM4, F32(1e-8), F32(math.pi)
VALUE_TOL = 1e-4            # README: fp32 parity of a loss value, relative
GRAD_TOL = kr.FK_GRAD_TOL   # per tensor: max |g - g_ref| <= GRAD_TOL * max |g_ref|  (transform_grad_ref.TOL)
MARGIN = 1e-3               # angles, axis sums; see assert_clear_of_thresholds


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a, np.float32), dtype=dtype)


def rel_from_trans(tl, pairs, drop_src=False):
    """[T,P,4,4], pairs [E,2] -> rel rows 0..2 [T,E,3,4] = inv(T_src) T_tgt with the rigid inverse, in rel_transform's order."""
    pairs = torch.as_tensor(np.asarray(pairs)).long().reshape(-1, 2)
    A, B = tl[:, pairs[:, 0]], tl[:, pairs[:, 1]]
    if drop_src:
        A = A.detach()
    rows = []
    for i in range(3):
        tinv = (-A[..., 0, i] * A[..., 0, 3] + -A[..., 1, i] * A[..., 1, 3]) + -A[..., 2, i] * A[..., 2, 3]
        r = [(A[..., 0, i] * B[..., 0, j] + A[..., 1, i] * B[..., 1, j]) + A[..., 2, i] * B[..., 2, j] for j in range(3)]
        r.append(((A[..., 0, i] * B[..., 0, 3] + A[..., 1, i] * B[..., 1, 3]) + A[..., 2, i] * B[..., 2, 3]) + tinv)
        rows.append(torch.stack(r, -1))
    return torch.stack(rows, -2)


def _qmul(q1, q2):
    w = ((q2[..., 0] * q1[..., 0] - q2[..., 1] * q1[..., 1]) - q2[..., 2] * q1[..., 2]) - q2[..., 3] * q1[..., 3]
    x = ((q2[..., 0] * q1[..., 1] + q2[..., 1] * q1[..., 0]) - q2[..., 2] * q1[..., 3]) + q2[..., 3] * q1[..., 2]
    y = ((q2[..., 0] * q1[..., 2] + q2[..., 1] * q1[..., 3]) + q2[..., 2] * q1[..., 0]) - q2[..., 3] * q1[..., 1]
    z = ((q2[..., 0] * q1[..., 3] - q2[..., 1] * q1[..., 2]) + q2[..., 2] * q1[..., 1]) + q2[..., 3] * q1[..., 0]
    return torch.stack([w, x, y, z], -1)


def _safe_sqrt(x):
    pos = x > 0
    return torch.where(pos, torch.where(pos, x, torch.ones_like(x)).sqrt(), torch.zeros_like(x))


def decompose(M, dec=None):
    """M [...,3,4] -> (l, m [...,3], theta, d [...]) and the decisions taken (or, with `dec`, followed); raw inputs of the
    decisions come back under "raw"."""
    R, t = M[..., :3, :3], M[..., :3, 3]
    m = lambda i, j: R[..., i, j]
    a = torch.stack([((1.0 + m(0, 0)) + m(1, 1)) + m(2, 2), ((1.0 + m(0, 0)) - m(1, 1)) - m(2, 2),
                     ((1.0 - m(0, 0)) + m(1, 1)) - m(2, 2), ((1.0 - m(0, 0)) - m(1, 1)) + m(2, 2)], -1)
    qa = _safe_sqrt(a)
    best = dec["best"] if dec else qa.argmax(-1)
    q2 = qa * qa
    cand = torch.stack([
        torch.stack([q2[..., 0], m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1)], -1),
        torch.stack([m(2, 1) - m(1, 2), q2[..., 1], m(1, 0) + m(0, 1), m(0, 2) + m(2, 0)], -1),
        torch.stack([m(0, 2) - m(2, 0), m(1, 0) + m(0, 1), q2[..., 2], m(1, 2) + m(2, 1)], -1),
        torch.stack([m(1, 0) - m(0, 1), m(2, 0) + m(0, 2), m(2, 1) + m(1, 2), q2[..., 3]], -1)], -2)
    c = torch.gather(cand, -2, best[..., None, None].expand(best.shape + (1, 4)))[..., 0, :]
    qb = torch.gather(qa, -1, best[..., None])[..., 0]
    qr = c / (2.0 * torch.clamp(qb, min=0.1))[..., None]
    tq = torch.cat([torch.zeros_like(t[..., :1]), t], -1)
    qd = 0.5 * _qmul(tq, qr)
    nq = (((qr[..., 0] * qr[..., 0] + qr[..., 1] * qr[..., 1]) + qr[..., 2] * qr[..., 2]) + qr[..., 3] * qr[..., 3]).sqrt()
    qn = qr / nq[..., None]
    nim = _safe_sqrt((qn[..., 1] * qn[..., 1] + qn[..., 2] * qn[..., 2]) + qn[..., 3] * qn[..., 3])
    th_raw = 2.0 * torch.atan2(nim, qn[..., 0])
    no_rot = dec["no_rot"] if dec else ((th_raw.abs() < EPS6) | ((th_raw - PI_F).abs() < EPS6))
    conj = qr * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=M.dtype)
    tt = _qmul(2.0 * qd, conj)[..., 1:]
    s = torch.sin(th_raw / 2.0)
    l_rot = qr[..., 1:] / torch.where(no_rot, torch.ones_like(s), s)[..., None]
    d0 = _safe_sqrt((tt[..., 0] * tt[..., 0] + tt[..., 1] * tt[..., 1]) + tt[..., 2] * tt[..., 2])
    l = torch.where(no_rot[..., None], tt / (d0 + 1e-10)[..., None], l_rot)
    cs = (l[..., 0] + l[..., 1]) + l[..., 2]
    flip = dec["flip"] if dec else ~(cs >= 0)
    th = torch.where(flip, -th_raw, th_raw)
    l = torch.where(flip[..., None], -l, l)
    d = torch.where(no_rot, torch.where(flip, -d0, d0), (tt * l).sum(-1))
    axis_one = dec["axis_one"] if dec else (no_rot & (d.abs() <= EPS8))
    l = torch.where(axis_one[..., None] & torch.tensor([True, False, False]), torch.ones_like(l), l)
    th = torch.where(no_rot, torch.full_like(th, EPS6), th)
    tl = torch.cross(tt, l, dim=-1)
    mom = 0.5 * (tl + torch.cross(l, tl / torch.tan(th / 2.0)[..., None], dim=-1))
    unit = dec["unit"] if dec else (((th.abs() <= EPS5) | ((th - PI_F).abs() <= EPS5)) & (d <= EPS5))
    srt = torch.sort(qa.detach(), -1).values
    out = dict(best=best, no_rot=no_rot, flip=flip, axis_one=axis_one, unit=unit,
               raw=dict(q_gap=srt[..., 3] - srt[..., 2], th_raw=th_raw.detach(), cs=cs.detach(), d=d.detach(), tt=tt.detach()))
    return l, mom, th, d, out


def _frob(M, G):
    """|M inv(G) - I|^2 over rows 0..2 (frobenius_cost(predict = M, gt = G)); G [...,4,4] or [...,3,4]."""
    GR, gt = G[..., :3, :3], G[..., :3, 3]
    MR = M[..., :3, :3] @ GR.transpose(-1, -2)
    eR = MR - torch.eye(3, dtype=M.dtype)
    et = M[..., :3, 3] - (MR @ gt[..., None])[..., 0]
    return (eR * eR).sum((-1, -2)) + (et * et).sum(-1)


def _fit(M, E_total, dec, mutate):
    """The fitted target G [T,E,4,4] of relative motions M [T,E,3,4] and the decisions (all of them, nested)."""
    T = M.shape[0]
    l, mom, th, d, dd = decompose(M, dec["frames"] if dec else None)
    keep = (~dd["unit"]).to(M.dtype)
    nkeep = keep.sum(0)
    plain = (nkeep == 0) if mutate == "ignore_e1" else ((nkeep == 0) | (E_total <= 1))
    w = torch.where(plain[None], torch.ones_like(keep), keep)
    n = w.sum(0)
    ml, mm = (l * w[..., None]).sum(0) / n[:, None], (mom * w[..., None]).sum(0) / n[:, None]
    mean_th, mean_d = th.abs().mean(0), d.abs().mean(0)
    pris = dec["pris"] if dec else (mean_d > mean_th)
    mle, mme = ml[None].expand(T, -1, 3), mm[None].expand(T, -1, 3)

    def target(p, follow=True):
        tht = torch.where(p[None], torch.full_like(th, EPS6), th)
        dt = torch.where(p[None], d, torch.full_like(d, EPS6))
        if dec and follow:
            nr, cl = dec["t_no_rot"], dec["t_clamped"]
        else:
            nr = (tht.abs() < EPS6) | ((tht - PI_F).abs() < EPS6)
            om = torch.where(nr[..., None], torch.zeros_like(mle), mle * tht[..., None])
            cl = ((om[..., 0] * om[..., 0] + om[..., 1] * om[..., 1]) + om[..., 2] * om[..., 2]) < EPS4
        return kr.screw_ref(mle, mme, tht, dt, nr, cl), nr, cl, tht

    if mutate == "cost_rule":     # compute_screw_trans: revolute against prismatic reconstruction cost
        Gr, Gp = target(torch.zeros_like(pris), False)[0], target(torch.ones_like(pris), False)[0]
        cr = _frob(Gr, M).sum(0)
        Mp = torch.cat([torch.eye(3, dtype=M.dtype).expand(M.shape[:-2] + (3, 3)), M[..., :3, 3:]], -1)
        cp = _frob(Gp, Mp).sum(0) + ((Gp[..., :3, :3] - M[..., :3, :3]) ** 2).mean()
        pris = cp <= cr
        G, nr, cl, tht = target(pris, False)
    else:
        G, nr, cl, tht = target(pris)
    out = dict(frames={k: v for k, v in dd.items() if k != "raw"}, pris=pris, t_no_rot=nr, t_clamped=cl,
               raw=dict(dd["raw"], mean_gap=(mean_d - mean_th).detach(), mean_d=mean_d.detach(), t_theta=tht.detach(), ml=ml.detach(), nkeep=nkeep))
    return G, out


def decisions(trans, pairs):
    """The decisions of a float32 evaluation (pairs None: `trans` holds the relative motions [T,E,4,4])."""
    with torch.no_grad():
        x = _t(trans, torch.float32)
        M = x[..., :3, :] if pairs is None else rel_from_trans(x, pairs)
        return _fit(M, M.shape[1], None, None)[1]


def term_of(x, pairs, weight=1.0, dec=None, mutate=None):
    """The term on a tensor of the caller's graph (transforms [T,P,4,4], or relative motions with pairs None) ->
    (loss, edge costs, the decisions used)."""
    M = x[..., :3, :] if pairs is None else rel_from_trans(x, pairs, drop_src=mutate == "drop_src")
    E = M.shape[1]
    if mutate == "target_not_detached":
        G, used = _fit(M, E, dec, mutate)
    else:
        with torch.no_grad():
            G, used = _fit(M.detach(), E, dec, mutate)
    cost = _frob(M, G).sum(0)
    return weight * cost.sum(), cost, used


def structure_term(trans, pairs, weight=1.0, dtype=torch.float64, mutate=None, dec="f32"):
    """-> dict(loss, edge_cost [E], prismatic [E] bool, grad (shape of trans, float64 numpy), dec).  dec: "f32" (the decisions of
    a float32 evaluation), "own" (of this one) or a decisions dict."""
    if dec == "f32":
        dec = decisions(trans, pairs)
    elif dec == "own":
        dec = None
    x = _t(trans, dtype).requires_grad_(True)
    loss, cost, used = term_of(x, pairs, weight, dec, mutate)
    if cost.numel():
        loss.backward()
    g = np.zeros(tuple(x.shape), np.float64) if x.grad is None else x.grad.detach().to(torch.float64).numpy()
    k = mutate[1] if isinstance(mutate, tuple) and mutate[0] == "scale" else 1.0
    return dict(loss=float(loss.detach()) * k, edge_cost=cost.detach().to(torch.float64).numpy() * k,
                prismatic=used["pris"].numpy().astype(bool), grad=g * k, dec=used)


def rel_trans_backward(trans, pairs, upstream, dtype=torch.float64):
    """Autograd of rel = inv(T_src) T_tgt with upstream [T,E,4,4] (row 3 ignored) -> gradient [T,P,4,4] float64 numpy."""
    x = _t(trans, dtype).requires_grad_(True)
    (rel_from_trans(x, pairs) * _t(upstream, dtype)[..., :3, :]).sum().backward()
    return x.grad.detach().to(torch.float64).numpy()


def _same(a, b):
    return all(bool((a[k] == b[k]).all()) for k in ("pris", "t_no_rot", "t_clamped")) and \
        all(bool((a["frames"][k] == b["frames"][k]).all()) for k in a["frames"])


def assert_clear_of_thresholds(trans, pairs):
    """The float32 and the float64 evaluation decide alike, and in float64 every decision input keeps its distance:
    the two largest quaternion candidates differ by MARGIN; theta is exactly 0 or MARGIN away from 0 and pi; the axis sum
    l . (1,1,1) is exactly 0 (an identity frame) or MARGIN away from 0; a no-rotation frame's d is exactly 0 or 1e-4 away
    from 0 and from 1e-5; mean|d| is exactly 0 (never above mean|theta|) or differs from mean|theta| by 1e-4; the target's |theta| |l| stays outside [0.008, 0.012]."""
    d32 = decisions(trans, pairs)
    with torch.no_grad():
        x = _t(trans, torch.float64)
        M = x[..., :3, :] if pairs is None else rel_from_trans(x, pairs)
        d64 = _fit(M, M.shape[1], None, None)[1]
    assert _same(d32, d64), "float32 and float64 decide differently"
    r, nr = d64["raw"], d64["frames"]["no_rot"]
    assert bool((r["q_gap"] > MARGIN).all()), "quaternion branch within the margin"
    th = r["th_raw"]
    assert bool(((th == 0) | ((th.abs() > MARGIN) & ((th - math.pi).abs() > MARGIN))).all()), "theta next to 0 or pi"
    zero_t = (r["tt"] == 0).all(-1)
    assert bool(((nr & zero_t & (r["cs"] == 0)) | (r["cs"].abs() > MARGIN)).all()), "axis sum next to 0"
    dn = r["d"][nr]
    assert bool(((dn == 0) | ((dn.abs() > 1e-4) & ((dn - 1e-5).abs() > 1e-4))).all()), "no-rotation distance next to a threshold"
    assert bool(((r["mean_d"] == 0) | (r["mean_gap"].abs() > 1e-4)).all()), "mean|d| next to mean|theta|"
    live = r["t_theta"].to(torch.float32) != torch.tensor(EPS6, dtype=torch.float32)
    rot = r["t_theta"].abs() * r["ml"].norm(dim=-1)[None]
    assert not bool((live & (((rot >= 0.008) & (rot <= 0.012)) | (r["t_theta"].abs() <= 1e-4)
                             | ((r["t_theta"] - math.pi).abs() <= MARGIN))).any()), "target next to a threshold of the screw map"
    return d64


# ------------------------------------------------------------------------------------------------------------ cases
def _rot(axis, ang):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)


QUARTER = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])     # entries in {0, +-1}


def make_case(T, P, edges, kinds, seed=0, big=()):
    """Part motions as one screw per part plus small noise -> dict(trans [T,P,4,4] float32, pairs [E,2] int32).
    kinds[p]: "r" a revolute part (angle sweeping 80 % .. 100 % of +-[0.4, 1.2] rad about a random axis through a random
    point; parts named in `big` sweep 90 % .. 100 % of +-[2.3, 2.9] about the x, y, z axis in turn: the other quaternion
    branches), "p" a prismatic part: the identity as rotation and a translation along a random direction, "q" the same with
    the rotation QUARTER (entries in {0, +-1}: two "q" parts have exactly the identity as relative rotation in float32 as in
    float64; next to an "i" or "p" part a quarter turn would tie two quaternion branches).  "i" the identity in every frame.
    "x" a prismatic part that slides through the origin: seen from an "i" part its signed distance is negative in the first
    frames, which `unit` then counts as unit transforms, and positive in the others (the masked mean differs from the plain).
    "h" a helical part: a quarter radian about an axis two units away with a slide of 0.4 along it -- mean|d| > mean|theta|
    calls it prismatic, the reconstruction costs of compute_screw_trans call it revolute."""
    rng = np.random.default_rng([seed, T, P])
    tr = np.tile(np.eye(4), (T, P, 1, 1))
    s = np.linspace(0.8, 1.0, T) if T > 1 else np.ones(1)
    for p, kind in enumerate(kinds):
        if kind == "i":
            continue
        if kind == "x":
            sweep = 0.3 * np.linspace(-1.0, 1.3, T)          # no frame at 0
            tr[:, p, :3, 3] = sweep[:, None] * np.array([0.8, 0.5, -0.33]) + rng.normal(0, 3e-3, (T, 3))
            continue
        if kind in "pq":
            base, direc = rng.uniform(-0.3, 0.3, 3), rng.normal(size=3)
            amp = rng.uniform(0.2, 0.5) * rng.choice([-1.0, 1.0])
            tr[:, p, :3, :3] = QUARTER if kind == "q" else np.eye(3)
            tr[:, p, :3, 3] = base + (amp * s)[:, None] * direc / np.linalg.norm(direc) + rng.normal(0, 1e-3, (T, 3))
            continue
        if p in big:
            axis = np.eye(3)[list(big).index(p) % 3] + rng.normal(0, 0.05, 3)
            ang = rng.uniform(2.3, 2.9) * rng.choice([-1.0, 1.0])
        else:
            axis, ang = rng.normal(size=3), rng.uniform(0.4, 1.2) * rng.choice([-1.0, 1.0])
        point, slide = rng.uniform(-0.3, 0.3, 3), 0.0
        if kind == "h":
            across = np.cross(axis, point)
            ang, point, slide = 0.25 * np.sign(ang), 2.0 * across / np.linalg.norm(across), 0.4
        for t in range(T):
            R = _rot(axis, ang * (0.5 + 0.5 * s[t] if p in big else s[t]))
            tr[t, p, :3, :3] = R + rng.normal(0, 1e-3, (3, 3))
            tr[t, p, :3, 3] = point - R @ point + slide * s[t] * axis / np.linalg.norm(axis) + rng.normal(0, 1e-3, 3)
    return dict(trans=tr.astype(np.float32), pairs=np.asarray(edges, np.int32).reshape(-1, 2))


def _all_pairs(P):
    return [(a, b) for a in range(P) for b in range(P)]


# name -> (T, P, edges, kinds, seed, big)
CASES = {
    "T1_E3": (1, 4, [(0, 1), (1, 2), (2, 3)], "irrr", 0, ()),
    "T2_E2": (2, 3, [(0, 1), (2, 1)], "rrr", 0, ()),
    "T9_P10_E9_mixed": (9, 10, [(0, 1), (0, 2), (2, 3), (3, 4), (5, 4), (5, 6), (6, 7), (7, 8), (8, 9)], "irrqqqrrii", 0, (2, 7)),
    "T65_E2": (65, 3, [(0, 1), (1, 2)], "irr", 0, (1,)),
    "T257_E3": (257, 4, [(0, 1), (1, 2), (3, 2)], "irqq", 0, ()),
    "T1024_P3_E3": (1024, 3, [(0, 1), (1, 2), (0, 2)], "irr", 0, ()),
    "E1_plain_mean": (9, 2, [(0, 1)], "ix", 0, ()),
    "E2_masked_mean_helical": (9, 3, [(0, 1), (0, 2)], "ixh", 0, ()),
    "E36_all_pairs_P6": (5, 6, _all_pairs(6), "irrrpp", 0, (1, 2, 3)),
    "P64_E5": (3, 64, [(0, 63), (63, 31), (31, 32), (7, 32), (7, 0)], "r" * 64, 0, ()),
}


@functools.lru_cache(maxsize=None)
def case(name):
    T, P, edges, kinds, seed, big = CASES[name]
    return make_case(T, P, edges, kinds, seed, big)


@functools.lru_cache(maxsize=None)
def case_ref(name, weight=1.0):
    c = case(name)
    return structure_term(c["trans"], c["pairs"], weight)


def compare(got, ref, what=""):
    """The comparison of both tests: value and edge costs within VALUE_TOL relative (edge costs: of the largest), flags equal,
    gradient within GRAD_TOL of its largest reference entry, row 3 exactly zero -> the measured ratios."""
    lv = abs(got["loss"] - ref["loss"]) / abs(ref["loss"]) if ref["loss"] else abs(got["loss"])
    assert lv <= VALUE_TOL, f"{what}: value {got['loss']!r} against {ref['loss']!r}: {lv:.2e}"
    out = {"loss": lv}
    if got.get("edge_cost") is not None and len(ref["edge_cost"]):
        top = float(np.abs(ref["edge_cost"]).max())
        out["edge_cost"] = float(np.abs(np.asarray(got["edge_cost"], np.float64) - ref["edge_cost"]).max()) / (top if top else 1.0)
        assert out["edge_cost"] <= VALUE_TOL, f"{what}: edge costs off by {out['edge_cost']:.2e}"
    if got.get("prismatic") is not None:
        assert np.array_equal(np.asarray(got["prismatic"], bool), ref["prismatic"]), f"{what}: prismatic flags"
    if got.get("grad") is not None:
        g, r = np.asarray(got["grad"], np.float64), ref["grad"]
        assert g.shape == r.shape and np.isfinite(g).all(), what
        assert not g[..., 3, :].any(), f"{what}: row 3 of the gradient"
        top = float(np.abs(r).max())
        out["grad"] = float(np.abs(g - r).max()) / top if top else float(np.abs(g).max())
        assert out["grad"] <= GRAD_TOL, f"{what}: gradient off by {out['grad']:.2e} of max|g| = {top:.3g}"
    return out


# ---------------------------------------------------------------------------------------------------------- goldens
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_CASES = ("raw", "new", "synA", "synB")      # of tests/golden/loss_terms.npz: the reference's own float32 results


def golden_case(tag):
    """(trans, pairs, golden entries) of a case of loss_terms.npz; the large inputs live in structure.npz."""
    g = np.load(os.path.join(GOLD, "loss_terms.npz"))
    if tag in ("raw", "new"):
        z = np.load(os.path.join(GOLD, "structure.npz"))
        trans, pairs = {"raw": (z["trans0"], z["joint_connection_raw"]), "new": (z["new_trans"], z["new_conn"])}[tag]
    else:
        trans, pairs = g[tag + "_trans"], g[tag + "_pairs"]
    return trans, np.asarray(pairs, np.int32), {k: g[f"{tag}_{k}"] for k in ("loss", "grad", "pris")}


def golden_ref(tag):
    """The golden as a reference of structure_loss_ref.compare: rows 0..2 of the gradient are the reference's, row 3 the
    project's zero."""
    trans, pairs, g = golden_case(tag)
    grad = np.zeros(trans.shape, np.float64)
    grad[:, :, :3] = g["grad"]
    return dict(loss=float(g["loss"]), edge_cost=np.zeros(0), prismatic=g["pris"].astype(bool), grad=grad)
