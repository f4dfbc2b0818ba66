"""float64 restatement of the kinematic projection's pieces (csrc/kinematic.hip, csrc/kinpost.hip) with torch autograd on the
CPU, and the inputs and comparisons of tests/test_kin_ref_cpu.py and tests/test_kinematic_long_gpu.py.  Nothing of reart_amd
is imported here.

  fk_ref / apply_parts   screw joints -> SE(3) -> the tree (utils/kinematic_utils.py:151-198, screw_se3/screw_utils.py:6-30,
                         screw_se3/geo_utils.py:90-222).  The DECISIONS -- the strict no-rotation test |theta| < 1e-6 and the
                         clamp of the squared rotation norm at 1e-4 -- are taken on float32 copies of the inputs, as
                         the kernel and the reference take them; the arithmetic is float64.  A prismatic joint runs as
                         theta = float32(1e-6): in float32 |theta| < 1e-6 is false (the literal rounds to the same float) and the
                         joint goes through the rotation branch with h = d / theta, a translation of d l; as doubles
                         9.99999997e-7 < 1e-6 is true, and a restatement that decides in float64 returns 1e-6 l instead.
                         A float32 and a float64 evaluation may land on different sides of a threshold, and the derivative
                         jumps there: `assert_clear_of_thresholds` refuses inputs near one.
  kin_post_ref           run_robot.py:177-209 between the assignment re-solve and the FK backward: matched targets, the
                         assignment loss, the flow loss of networks/loss.py:10-21 on pred = comp[1:] - comp[:-1] with the
                         canonical frame spliced in at c, and G = dL / d pc_trans.  The blended flow target and its mask are
                         inputs (the reference computes them under no_grad).
  kin_post_f32           the same in numpy float32, closed form: what rounding alone costs (the bound of G, see post_g_tol).
  random_tree            chain / star / random joint trees with permuted part labels and edge numbers.

`mutate` plants one known error in a restatement, so that a test can show that the comparison rejects it:
  kin_post_ref  "drop_last_frame"   the flow-gradient term of the last articulated frame dropped
                "flip_prev_sign"    the sign of the comp[:-1] term of the flow gradient flipped
                "cano_shift"        the canonical frame spliced in at c + 1 (c - 1 at c = B)
                "single_lambda"     2 lambda_assign replaced by lambda_assign in the gradient
  fk_ref        ("skip_axis_frame", t)   frame t's term left out of the sums over frames (axis and moment gradients)
"""
import functools
import math

import numpy as np
import torch

F32_1EM6 = float(np.float32(1e-6))         # the placeholder theta of a prismatic joint / distance of a revolute one, as the kernel holds it
F32_1EM4 = float(np.float32(1e-4))
FK_FWD_TOL = 5e-6                          # forward: FK_FWD_TOL * max(1, max|out|)
FK_GRAD_TOL = 2e-4                         # gradients: per tensor FK_GRAD_TOL * max|g|
LOSS_TOL = 1e-6                            # the three losses of reart_kin_post, relative


def _t64(a):
    return torch.as_tensor(np.asarray(a, np.float32), dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------------------- FK
def fk_decisions(axis, theta):
    """(no_rot [B,E], clamped [B,E]) as float32 arithmetic decides them: csrc/screw_dev.h, geo_utils.py:90-144."""
    th = torch.as_tensor(np.asarray(theta.detach() if torch.is_tensor(theta) else theta), dtype=torch.float64).to(torch.float32)
    l = torch.as_tensor(np.asarray(axis.detach() if torch.is_tensor(axis) else axis), dtype=torch.float64).to(torch.float32)
    eps, pi = torch.tensor(1e-6, dtype=torch.float32), torch.tensor(math.pi, dtype=torch.float32)
    no_rot = (th.abs() < eps) | ((th - pi).abs() < eps)
    om = torch.where(no_rot[..., None], torch.zeros((), dtype=torch.float32), l[None] * th[..., None])
    n2 = (om[..., 0] * om[..., 0] + om[..., 1] * om[..., 1]) + om[..., 2] * om[..., 2]
    return no_rot, n2 < torch.tensor(1e-4, dtype=torch.float32)


def assert_clear_of_thresholds(axis, theta):
    """Every joint value that is not the prismatic placeholder float32(1e-6) stays away from the places where the function
    is not smooth: the clamp of the rotation norm (|theta| |l| outside [0.008, 0.012]), theta = 0 (|theta| > 1e-4: h = d /
    theta) and theta = pi (|theta - pi| > 1e-3)."""
    th = np.asarray(theta.detach() if torch.is_tensor(theta) else theta, np.float64)
    l = np.asarray(axis.detach() if torch.is_tensor(axis) else axis, np.float64)
    live = th.astype(np.float32) != np.float32(1e-6)
    rot = np.abs(th) * np.linalg.norm(l, axis=-1)[None]
    bad = live & (((rot >= 0.008) & (rot <= 0.012)) | (np.abs(th) <= 1e-4) | (np.abs(th - math.pi) <= 1e-3))
    assert not bad.any(), f"joint values next to a threshold of the screw map at {np.argwhere(bad)[:5].tolist()}: {th[bad][:5]}"


def _hat(w):
    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], z, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def screw_ref(l, m, theta, d, no_rot, clamped):
    """(l, m [B,E,3], theta, d [B,E]) float64, the decisions given -> [B,E,4,4]."""
    q = torch.cross(l, m, dim=-1)
    safe = torch.where(no_rot, torch.ones_like(theta), theta)
    v_rot = torch.cross(q, l, dim=-1) + (d / safe)[..., None] * l
    w = torch.where(no_rot[..., None], torch.zeros_like(l), l)
    v = torch.where(no_rot[..., None], l, v_rot)
    om, u = w * theta[..., None], v * theta[..., None]
    n2 = torch.where(clamped, torch.full_like(theta, F32_1EM4), (om * om).sum(-1))        # the clamp of the SQUARED norm
    ph = n2.sqrt()
    s, c = torch.sin(ph), torch.cos(ph)
    K = _hat(om)
    K2 = K @ K
    eye = torch.eye(3, dtype=l.dtype).expand(K.shape)
    f = lambda x: x[..., None, None]
    R = eye + f(s / ph) * K + f((1.0 - c) / n2) * K2
    V = eye + f((1.0 - c) / n2) * K + f((ph - s) / (ph * n2)) * K2
    t = (V @ u[..., None])[..., 0]
    top = torch.cat([R, t[..., None]], -1)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=l.dtype).expand(top.shape[:-2] + (1, 4))
    return torch.cat([top, bottom], -2)


def fk_ref(parent, edge_of_part, order, axis, moment, theta, distance=None, check=True, mutate=None):
    """FK[c] = FK[parent(c)] T_rel(edge of c), parts visited in `order` (root first) -> [B,P,4,4] float64.  axis, moment [E,3],
    theta [B,E], distance [B,E] or None (= float32(1e-6), utils/kinematic_utils.py:176): float64 tensors holding float32
    values, leaves of the caller's graph."""
    assert theta.dtype == torch.float64 and axis.dtype == torch.float64 and moment.dtype == torch.float64
    if check:
        assert_clear_of_thresholds(axis, theta)
    B, E = theta.shape
    no_rot, clamped = fk_decisions(axis, theta)
    d = torch.full_like(theta, F32_1EM6) if distance is None else distance
    l, m = axis[None].expand(B, E, 3), moment[None].expand(B, E, 3)
    if mutate is not None:
        kind, frame = mutate
        assert kind == "skip_axis_frame" and 0 <= frame < B
        keep = torch.ones((B, 1, 1), dtype=torch.bool)
        keep[frame] = False
        l, m = torch.where(keep, l, l.detach()), torch.where(keep, m, m.detach())
    T = screw_ref(l, m, theta, d, no_rot, clamped)
    out = [None] * len(parent)
    eye = torch.eye(4, dtype=theta.dtype).expand(B, 4, 4)
    for c in order:
        c = int(c)
        out[c] = eye if parent[c] < 0 else out[int(parent[c])] @ T[:, int(edge_of_part[c])]
    return torch.stack(out, 1)


def apply_parts(x, trans, part):
    """networks/model.py:160-165: point n moved by the transform of its part -> [B,N,3]."""
    Tn = trans[:, torch.as_tensor(np.asarray(part)).long()]
    return (Tn[..., :3, :3] @ x[None, :, :, None])[..., 0] + Tn[..., :3, 3]


def effective_joint_values(theta, distance, prismatic):
    """utils/kinematic_utils.py:174-186: prismatic joints run with theta = float32(1e-6) and their distance, revolute joints
    with their theta and distance = float32(1e-6); torch.where hands the masked entries no gradient."""
    pris = torch.as_tensor(np.asarray(prismatic, bool))[None, :]
    return (torch.where(pris, torch.full_like(theta, F32_1EM6), theta), torch.where(pris, distance, torch.full_like(distance, F32_1EM6)))


def random_tree(rng, P, kind="random", empty=0):
    """A joint tree of P parts as (parent, edge_of_part, order) int32 [P] and the parts that may own points.  kind: "chain"
    (depth P - 1), "star" (every part hangs off the root) or "random" (the parent of a part is any earlier one).  The parts
    are relabelled by a random permutation, so `order` (root first) is not the identity and a parent's label may exceed its
    child's; `edge_of_part` numbers the edges by another one.  `empty` of the parts are named as owning no point."""
    assert kind in ("chain", "star", "random") and P >= 1
    par = {"chain": lambda c: c - 1, "star": lambda c: 0, "random": lambda c: int(rng.integers(0, c))}[kind]
    label = rng.permutation(P)
    parent = np.full(P, -1, np.int32)
    for c in range(1, P):
        parent[label[c]] = label[par(c)]
    edge_of = np.full(P, -1, np.int32)
    edge_of[label[1:]] = rng.permutation(P - 1)
    order = label.astype(np.int32)
    owners = np.sort(rng.permutation(P)[:P - empty]) if empty else np.arange(P)
    return parent, edge_of, order, owners


def make_fk_case(name):
    """The inputs of one row of FK_CASES, float32 numpy: tree, axis, moment, theta, distance (or None), x, part, Gw, and for
    the case with joint types `prismatic` [E] (theta / distance are then the model's lists, before effective_joint_values)."""
    kind, P, B, N, dist, extra = FK_CASES[name]
    rng = np.random.default_rng(FK_SEEDS[name])
    E = P - 1
    parent, edge_of, order, owners = random_tree(rng, P, kind, empty=P // 3 if extra == "empty" else 0)
    axis = rng.normal(size=(E, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    moment = rng.normal(0, 0.3, (E, 3))
    lim = 0.3 if kind == "chain" else 2.5                        # 63 joints deep: small angles keep the cloud where it is
    theta = rng.uniform(0.02, lim, (B, E)) * rng.choice([-1.0, 1.0], (B, E))
    theta[0, :min(3, E)] = 3e-3                                  # |theta l| under the clamp of the rotation norm (1e-2)
    c = dict(parent=parent, edge_of=edge_of, order=order, axis=axis, moment=moment, theta=theta,
             distance=rng.normal(0, 0.05, (B, E)) if dist else None, x=rng.uniform(-0.3, 0.3, (N, 3)),
             part=owners[rng.integers(0, len(owners), N)].astype(np.int64), Gw=rng.normal(size=(B, N, 3)), prismatic=None)
    if extra == "prismatic":
        c["prismatic"] = np.arange(E) % 3 == 1
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    return {k: (f32(v) if k in ("axis", "moment", "theta", "distance", "x", "Gw") else v) for k, v in c.items()}


# name -> (tree, P, B, N, with distance, extra)
FK_CASES = {
    "one_full_workgroup": ("random", 12, 64, 300, True, None),
    "second_workgroup_one_lane": ("random", 12, 65, 300, True, None),
    "star_P64_three_workgroups": ("star", 64, 130, 257, True, None),
    "chain_P64_no_distance": ("chain", 64, 65, 257, False, None),
    "B1024_empty_parts": ("random", 33, 1024, 100, True, "empty"),
    "N5_B1": ("random", 2, 1, 5, True, None),
    "N40000_dynamic_lds": ("random", 5, 2, 40000, True, None),
    "prismatic_joints": ("random", 8, 70, 200, True, "prismatic"),
}
FK_SEEDS = {k: 100 + i for i, k in enumerate(FK_CASES)}


def fk_case_ref(c, mutate=None):
    """float64 forward and autograd gradients of sum(out * Gw) for a case of make_fk_case -> dict(out, trans, grads)."""
    A, M, TH = (_t64(c[k]).requires_grad_(True) for k in ("axis", "moment", "theta"))
    D = None if c["distance"] is None else _t64(c["distance"]).requires_grad_(True)
    th, d = (TH, D) if c["prismatic"] is None else effective_joint_values(TH, D, c["prismatic"])
    trans = fk_ref(c["parent"], c["edge_of"], c["order"], A, M, th, d, mutate=mutate)
    out = apply_parts(_t64(c["x"]), trans, c["part"])
    (out * _t64(c["Gw"])).sum().backward()
    grads = dict(axis=A.grad.numpy(), moment=M.grad.numpy(), theta=TH.grad.numpy())
    if D is not None:
        grads["distance"] = D.grad.numpy()
    return dict(out=out.detach().numpy(), trans=trans.detach().numpy(), grads=grads)


def fk_case_f32(c):
    """The same evaluation in float32 on the CPU (torch autograd): a correct float32 implementation's distance from fk_case_ref."""
    t32 = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    A, M, TH = (t32(c[k]).requires_grad_(True) for k in ("axis", "moment", "theta"))
    D = None if c["distance"] is None else t32(c["distance"]).requires_grad_(True)
    th, d = (TH, D) if c["prismatic"] is None else effective_joint_values(TH, D, c["prismatic"])
    B, E = th.shape
    no_rot, clamped = fk_decisions(A, th)
    dd = torch.full_like(th, 1e-6) if d is None else d
    T = screw_ref(A[None].expand(B, E, 3), M[None].expand(B, E, 3), th, dd, no_rot, clamped)
    F = [None] * len(c["parent"])
    for p in c["order"]:
        p = int(p)
        F[p] = torch.eye(4).expand(B, 4, 4) if c["parent"][p] < 0 else F[int(c["parent"][p])] @ T[:, int(c["edge_of"][p])]
    out = apply_parts(t32(c["x"]), torch.stack(F, 1), c["part"])
    (out * t32(c["Gw"])).sum().backward()
    grads = dict(axis=A.grad.numpy(), moment=M.grad.numpy(), theta=TH.grad.numpy())
    if D is not None:
        grads["distance"] = D.grad.numpy()
    return out.detach().numpy(), grads


def check_fk(out, grads, ref, what=""):
    """The comparison of the FK tests: forward within FK_FWD_TOL * max(1, max|out|), every gradient within FK_GRAD_TOL of its
    largest entry -> {name: measured ratio}."""
    scale = max(1.0, float(np.abs(ref["out"]).max()))
    sp = {"out": float(np.abs(np.asarray(out, np.float64) - ref["out"]).max()) / scale}
    assert sp["out"] <= FK_FWD_TOL, f"{what}: forward off by {sp['out']:.2e} of max(1, max|out|) = {scale:.3g}"
    assert set(grads) == set(ref["grads"]), (what, sorted(grads), sorted(ref["grads"]))
    for k, r in ref["grads"].items():
        g = np.asarray(grads[k], np.float64)
        assert g.shape == r.shape and np.isfinite(g).all(), (what, k)
        sp[k] = float(np.abs(g - r).max()) / float(np.abs(r).max())
    bad = {k: v for k, v in sp.items() if k != "out" and not v <= FK_GRAD_TOL}
    assert not bad, f"{what}: gradient spread above {FK_GRAD_TOL:g} of max|g| in {bad} (all: {sp})"
    return sp


# ------------------------------------------------------------------------------------------------------- kin_post
def _splice(X, cano, c):
    return torch.cat((X[:c], cano[None], X[c:]), dim=0)


def kin_post_ref(pc_trans, cano, c, pc_src, tgt, cols, src_idx, lam_a, gt=None, mask=None, lam_f=1.0, robust=False, smooth=1e-2,
                 mutate=None):
    """run_robot.py:177-209 in float64.  pc_trans [B,N,3], cano [N,3], pc_src = pc_trans[:, src_idx] [B,n,3], tgt [B,n,3],
    cols [B,n] (the optimum), gt [B,N,3] / mask [B,N] (the blended flow targets of the B frame pairs; None: no flow branch) ->
    dict(G [B,N,3] float64, matched [B,n,3] float32, losses = [lam_a x assignment, lam_f x flow, total])."""
    X = _t64(pc_trans).requires_grad_(True)
    B = X.shape[0]
    src_idx = torch.as_tensor(np.asarray(src_idx)).long()
    assert 0 <= c <= B
    assert np.array_equal(np.asarray(pc_src, np.float32), np.asarray(pc_trans, np.float32)[:, src_idx.numpy()])
    matched32 = np.take_along_axis(np.asarray(tgt, np.float32), np.asarray(cols, np.int64)[..., None], axis=1)
    diff = X[:, src_idx] - _t64(matched32)
    ass = lam_a * (diff * diff).sum()                                              # run_robot.py:181-184
    g_ass, = torch.autograd.grad(ass, X)
    if mutate == "single_lambda":
        g_ass = g_ass * 0.5
    G, fl = g_ass, torch.zeros((), dtype=torch.float64)
    if gt is not None:
        cs = c if mutate != "cano_shift" else (c + 1 if c < B else c - 1)
        comp = _splice(X, _t64(cano), cs)
        prev = comp[:-1]
        if mutate == "flip_prev_sign":
            prev = 2.0 * prev.detach() - prev                                      # the value kept, the derivative negated
        pred = comp[1:] - prev
        d = pred - _t64(gt)
        f = (torch.where(d.abs() <= 1.0, 0.5 * d * d, d.abs() - 0.5) if robust else d * d).sum(-1)       # F.huber_loss, delta = 1
        m = torch.as_tensor(np.asarray(mask, bool))
        fl = lam_f * (torch.where(m, f, torch.zeros_like(f)) + smooth * torch.where(m, torch.zeros_like(f), (pred * pred).sum(-1))).sum()
        g_fl, = torch.autograd.grad(fl, X)
        if mutate == "drop_last_frame":
            g_fl = g_fl.clone()
            g_fl[B - 1] = 0.0
        G = G + g_fl
    return dict(G=G.numpy(), matched=matched32, losses=np.array([float(ass.detach()), float(fl.detach()), float((ass + fl).detach())]))


def kin_post_f32(pc_trans, cano, c, pc_src, tgt, cols, src_idx, lam_a, gt=None, mask=None, lam_f=1.0, robust=False, smooth=1e-2):
    """kin_post_ref's G in numpy float32, closed form, every operation rounded to float32."""
    f = np.float32
    X, cano = np.asarray(pc_trans, f), np.asarray(cano, f)
    B = X.shape[0]
    src_idx = np.asarray(src_idx, np.int64)
    matched = np.take_along_axis(np.asarray(tgt, f), np.asarray(cols, np.int64)[..., None], axis=1)
    G = np.zeros_like(X)
    G[:, src_idx] = (f(2.0) * f(lam_a)) * (X[:, src_idx] - matched)
    if gt is not None:
        comp = np.concatenate((X[:c], cano[None], X[c:]), axis=0)
        pred = comp[1:] - comp[:-1]
        d = pred - np.asarray(gt, f)
        gf = np.where(np.abs(d) <= f(1.0), d, np.sign(d)).astype(f) if robust else f(2.0) * d
        gp = np.where(np.asarray(mask, bool)[..., None], gf, f(smooth) * (f(2.0) * pred)).astype(f) * f(lam_f)
        gc = np.zeros_like(comp)
        gc[1:] += gp
        gc[:-1] -= gp
        G = G + np.concatenate((gc[:c], gc[c + 1:]), axis=0)
    return G


POST_N, POST_NS = 300, 77
POST_SHAPES = [(B, c) for B in (1, 2, 70) for c in sorted({0, 1, B - 1, B})]                 # (B, cano_idx)
POST_VARIANTS = [("assign_only", False, False), ("flow", True, False), ("flow_huber", True, True)]
POST_LAM_A, POST_LAM_F, POST_SMOOTH = 0.3, 0.7, 1e-2
MASK_MARGIN = 1e-5
POST_SEED = 11                             # of the seeds 0..11, those that keep every point of every case MASK_MARGIN off the mask threshold: 3, 4, 5, 6, 11


def ragged_lengths(rng, B):
    """Reference-set lengths from 3 (= k) to 200, both ends present from B = 2 on."""
    lens = rng.integers(3, 201, B)
    lens[0] = 3
    if B > 1:
        lens[1] = 200
    return [int(v) for v in lens]


def blend_targets(comp, refs, flows):
    """oracle.blend_anchor_motion of every frame pair on the spliced sequence -> (gt [B,N,3], mask [B,N], margin): margin =
    how close, relatively, any point's nearest reference comes to the mask's threshold max(fmax, 0.05)."""
    import oracle

    gts, masks, margin = [], [], np.inf
    for f, (r, fl) in enumerate(zip(refs, flows)):
        g, m = oracle.blend_anchor_motion(comp[f], r, fl, k=3)
        dist, idx = oracle.knn_cuda(r[None], comp[f][None], 3)
        dmin = np.maximum(dist[0].astype(np.float32), np.float32(1e-10)).min(-1)
        fn = (fl[idx[0]].astype(np.float32) ** 2)
        thr = np.maximum(((fn[..., 0] + fn[..., 1]) + fn[..., 2]).max(-1), np.float32(0.05)).astype(np.float64)
        assert np.array_equal(m, dmin <= thr)
        margin = min(margin, float((np.abs(dmin.astype(np.float64) - thr) / thr).min()))
        gts.append(g)
        masks.append(m)
    return np.stack(gts), np.stack(masks), margin


@functools.lru_cache(maxsize=None)
def make_post_case(B, c, seed=POST_SEED):
    """Inputs of reart_kin_post at pose_len B with the canonical frame at c: a cloud of POST_N points drifting through B + 1
    frames, POST_NS sampled points with a random permutation per frame as the optimum, ragged flow references next to the
    spliced frames (one of them ON a query point: the d < 1e-10 clamp) and the oracle's blended targets.  All float32."""
    rng = np.random.default_rng([seed, B, c])
    N, n = POST_N, POST_NS
    base = rng.uniform(-0.3, 0.3, (N, 3))
    drift = np.cumsum(rng.normal(0, 0.01, (B + 1, 1, 3)), axis=0) + np.cumsum(rng.normal(0, 0.004, (B + 1, N, 3)), axis=0)
    comp = (base[None] + drift).astype(np.float32)
    cano, pc_trans = comp[c].copy(), np.ascontiguousarray(np.delete(comp, c, axis=0))
    src_idx = np.sort(rng.permutation(N)[:n]).astype(np.int64)
    slot = np.full(N, -1, np.int32)
    slot[src_idx] = np.arange(n, dtype=np.int32)
    tgt = (pc_trans[:, rng.permutation(N)[:n]] + rng.normal(0, 0.01, (B, n, 3))).astype(np.float32)
    cols = np.stack([rng.permutation(n) for _ in range(B)]).astype(np.int32)
    lens = ragged_lengths(rng, B)
    refs, flows = [], []
    for f, m in enumerate(lens):
        sel = rng.permutation(N)[:m]
        refs.append((comp[f][sel] + rng.normal(0, 0.02, (m, 3))).astype(np.float32))
        flows.append(((comp[f + 1][sel] - comp[f][sel]) * 0.5 + rng.normal(0, 0.002, (m, 3))).astype(np.float32))
    refs[B // 2][1] = comp[B // 2][17]                           # an exact hit
    gt, mask, margin = blend_targets(comp, refs, flows)
    assert margin >= MASK_MARGIN, f"a point within {margin:.1e} of the mask's threshold: choose another seed"
    assert 0.05 < mask.mean() < 0.95 or B == 1, mask.mean()
    return dict(B=B, c=c, N=N, n=n, comp=comp, cano=cano, pc_trans=pc_trans, pc_src=np.ascontiguousarray(pc_trans[:, src_idx]),
                src_idx=src_idx, slot=slot, tgt=tgt, cols=cols, lens=lens, refs=refs, flows=flows, gt=gt, mask=mask, margin=margin)


def post_args(case, flow, robust):
    kw = dict(gt=case["gt"], mask=case["mask"], lam_f=POST_LAM_F, robust=robust, smooth=POST_SMOOTH) if flow else {}
    return (case["pc_trans"], case["cano"], case["c"], case["pc_src"], case["tgt"], case["cols"], case["src_idx"], POST_LAM_A), kw


@functools.lru_cache(maxsize=None)
def post_f32_spread():
    """The largest deviation of kin_post_f32 from kin_post_ref over every case the GPU test runs, relative to max|G|."""
    worst = 0.0
    for B, c in POST_SHAPES:
        case = make_post_case(B, c)
        for _, flow, robust in POST_VARIANTS:
            a, kw = post_args(case, flow, robust)
            G = kin_post_ref(*a, **kw)["G"]
            worst = max(worst, float(np.abs(kin_post_f32(*a, **kw).astype(np.float64) - G).max() / np.abs(G).max()))
    return worst


def post_g_tol():
    """The bound of reart_kin_post's G against kin_post_ref, relative to max|G|: 8 x what float32 rounding of the same
    expressions costs (summation orders and the kernel's own blend, which may differ from the oracle's by rtol 2e-6, enter)."""
    return 8.0 * post_f32_spread()


def check_post(G, matched, losses, ref, tol, what=""):
    """The comparison of the reart_kin_post test: G within tol of max|G|, the matched targets bit-equal (None: not asked for),
    the three losses within LOSS_TOL relative -> the measured ratio of G."""
    G = np.asarray(G, np.float64)
    assert G.shape == ref["G"].shape and np.isfinite(G).all(), what
    sp = float(np.abs(G - ref["G"]).max() / np.abs(ref["G"]).max())
    assert sp <= tol, f"{what}: dL/d pc_trans off by {sp:.2e} of max|G| (bound {tol:.2e}); worst frame {int(np.abs(G - ref['G']).max(axis=(1, 2)).argmax())}"
    if matched is not None:
        np.testing.assert_array_equal(np.asarray(matched), ref["matched"], err_msg=f"{what}: matched targets")
    if losses is not None:
        for i, name in enumerate(("assignment", "flow", "total")):
            a, b = float(losses[i]), float(ref["losses"][i])
            assert abs(a - b) <= LOSS_TOL * abs(b), f"{what}: {name} loss {a!r} against {b!r}"
    return sp
