"""The retargeting loop of reart_ik_fit (csrc/ik.hip; the reference's ik, utils/kinematic_utils.py:200-266) restated on the CPU
with the pieces of tests/kin_ref.py and torch.optim.Adam itself, and the inputs and bounds of tests/test_ik_ref_cpu.py and
tests/test_ik_fused_gpu.py.  Nothing of reart_amd is imported here.

  ik_loop_ref     per pose: n_iter x ( fk_ref, apply_parts, sum of squared distances, autograd backward,
                  torch.optim.Adam(lr 0.1, amsgrad=True).step() ) on CPU tensors of `dtype`; the decisions of the screw map
                  are taken on float32 copies (kin_ref.fk_decisions).  The M poses are one [M,E] parameter: the loss is a sum
                  over poses and Adam works element by element, so every row is the loop of that pose alone.
                  dtype=float64 is the reference, dtype=float32 what rounding alone costs (the `spread` of a case).

`mutate` plants one known error (kin_ref docstring), so that a test can show that the comparison rejects it:
  "no_amsgrad"           Adam without the running maximum of the second moment
  "no_bias_correction"   the two bias corrections of Adam left out
  "mean_loss"            the mean over n x 3 coordinates instead of their sum
  "skip_root_children"   the gradient of the edges under the root dropped

The bound of the GPU test: IK_TOL_FACTOR x spread, the multiple this project gives a kernel over the float32 restatement's own
deviation (kin_ref.post_g_tol).  The conditions a case has to meet for that to mean something: spread(theta) <= SPREAD_THETA_MAX
and spread(loss) <= SPREAD_LOSS_MAX (tests/test_ik_ref_cpu.py holds every case to them).
"""
import functools

import numpy as np
import torch

from tests import kin_ref

IK_TOL_FACTOR = 8.0
SPREAD_THETA_MAX = 1e-3      # rad, after the case's iterations
SPREAD_LOSS_MAX = 1e-5       # of loss[0], over the first LOSS_STEPS entries of the history
LOSS_STEPS = 10
LR = 1e-1
MUTATIONS = ("no_amsgrad", "no_bias_correction", "mean_loss", "skip_root_children")


def _fk(tree, A, Mo, TH):
    """[B,P,4,4] in the dtype of the operands: kin_ref.fk_ref for float64, the same evaluation for float32 (kin_ref.fk_case_f32)."""
    parent, edge_of, order = tree
    if TH.dtype == torch.float64:
        return kin_ref.fk_ref(parent, edge_of, order, A, Mo, TH, check=False)
    B, E = TH.shape
    no_rot, clamped = kin_ref.fk_decisions(A, TH)
    T = kin_ref.screw_ref(A[None].expand(B, E, 3), Mo[None].expand(B, E, 3), TH, torch.full_like(TH, 1e-6), no_rot, clamped)
    F = [None] * len(parent)
    for p in order:
        p = int(p)
        F[p] = torch.eye(4, dtype=TH.dtype).expand(B, 4, 4) if parent[p] < 0 else F[int(parent[p])] @ T[:, int(edge_of[p])]
    return torch.stack(F, 1)


def _plain_adam_step(p, g, st, t, lr, bias_correction, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam(amsgrad=True)'s step written out, for the mutation that torch has no switch for."""
    st["m"] = st["m"] + (1 - b1) * (g - st["m"])
    st["v"] = b2 * st["v"] + (1 - b2) * g * g
    st["vmax"] = torch.maximum(st["vmax"], st["v"])
    bc1, bc2 = (1 - b1 ** t, 1 - b2 ** t) if bias_correction else (1.0, 1.0)
    return p - (lr / bc1) * st["m"] / (st["vmax"].sqrt() / bc2 ** 0.5 + eps)


def ik_loop_ref(tree, axis, moment, src, part, tgt, n_iter, theta_init=None, dtype=torch.float64, mutate=None):
    """-> (theta [M,E], loss [M, n_iter + 1]) float64 numpy: loss[:, i] at the parameters before step i, loss[:, n_iter] at the
    returned theta.  tgt [M,n,3] (or [n,3]); theta_init [M,E] or None = float32(1e-6) everywhere; the optimiser starts at zero.
    Points whose label is outside [0, P) take no part."""
    assert mutate is None or mutate in MUTATIONS
    threads = torch.get_num_threads()
    torch.set_num_threads(1)            # one summation order on every machine: the float32 loop is a yardstick
    try:
        return _ik_loop(tree, axis, moment, src, part, tgt, n_iter, theta_init, dtype, mutate)
    finally:
        torch.set_num_threads(threads)


def _ik_loop(tree, axis, moment, src, part, tgt, n_iter, theta_init, dtype, mutate):
    parent = np.asarray(tree[0])
    P, E = len(parent), len(parent) - 1
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32), dtype=dtype)
    tgt = np.asarray(tgt, np.float32)
    tgt = tgt[None] if tgt.ndim == 2 else tgt
    part = np.asarray(part, np.int64)
    keep = (part >= 0) & (part < P)
    X, Y, lab = t(np.asarray(src, np.float32)[keep]), t(tgt[:, keep]), part[keep]
    M = Y.shape[0]
    A, Mo = t(np.asarray(axis, np.float32).reshape(E, 3)), t(np.asarray(moment, np.float32).reshape(E, 3))
    init = np.full((M, E), np.float32(1e-6), np.float32) if theta_init is None else np.asarray(theta_init, np.float32)
    TH = t(init).reshape(M, E).clone().requires_grad_(E > 0)
    under_root = [int(tree[1][c]) for c in range(P) if parent[c] >= 0 and parent[parent[c]] < 0]

    def losses(th):
        d = kin_ref.apply_parts(X, _fk(tree, A, Mo, th), lab) - Y
        per = (d * d).sum((1, 2))
        return per / (3 * X.shape[0]) if mutate == "mean_loss" else per

    hist = []
    if E == 0 or n_iter == 0:
        with torch.no_grad():
            l = losses(TH)
        hist = [l.double().numpy()] * (n_iter + 1)
        return TH.detach().double().numpy(), np.stack(hist, 1)
    opt = torch.optim.Adam([TH], lr=LR, amsgrad=(mutate != "no_amsgrad"))
    st = dict(m=torch.zeros_like(TH), v=torch.zeros_like(TH), vmax=torch.zeros_like(TH))
    for it in range(n_iter):
        per = losses(TH)
        hist.append(per.detach().double().numpy())
        opt.zero_grad()
        per.sum().backward()
        if mutate == "skip_root_children":
            TH.grad[:, under_root] = 0.0
        if mutate == "no_bias_correction":
            with torch.no_grad():
                TH.copy_(_plain_adam_step(TH, TH.grad, st, it + 1, LR, bias_correction=False))
        else:
            opt.step()
    with torch.no_grad():
        hist.append(losses(TH).double().numpy())
    return TH.detach().double().numpy(), np.stack(hist, 1)


# ------------------------------------------------------------------------------------------------------------ cases
# name -> (tree kind, P, points per part | explicit counts per owner, empty parts, M, n_iter, seed)
# Seeds: the first of 0..11 at which the case meets SPREAD_THETA_MAX and SPREAD_LOSS_MAX (tests/test_ik_ref_cpu.py checks it);
# rejected seeds are listed next to the case.
IK_CASES = {
    "P1_no_joint": ("chain", 1, 2, 0, 2, 200, 0),
    "P2_root_owns_nothing": ("chain", 2, [0, 3], 0, 1, 200, 0),
    "chain_P64": ("chain", 64, 3, 0, 2, 200, 1),                 # rejected: 0 (spread(theta) 1.03e-3; 200 steps do not settle a chain)
    "star_P64": ("star", 64, 3, 0, 2, 200, 0),
    "random_P33_empty5": ("random", 33, 3, 5, 5, 200, 0),
    "n1024_ragged_P7": ("random", 7, [600, 1, 85, 85, 85, 84, 84], 0, 2, 200, 0),
    "P5_n5_M300": ("random", 5, 1, 0, 300, 50, 0),
    "P5_n5_M4": ("random", 5, 1, 0, 4, 200, 0),
}
IK_SEED_SALT = {k: i for i, k in enumerate(IK_CASES)}
REF_CASES = ("P2_root_owns_nothing", "chain_P64", "star_P64", "random_P33_empty5", "n1024_ragged_P7")   # held to float64
WARM_CASE, WARM_ITERS = "chain_P64", 20                         # not settled after 200 steps: loss[0] is a scale
FWD_CASE = "random_P33_empty5"


@functools.lru_cache(maxsize=None)
def make_ik_case(name, seed=None):
    """float32 numpy inputs of one row of IK_CASES: tree (parent, edge_of, order), axis, moment [E,3], src [n,3], part [n],
    tgt [M,n,3] = the points carried by ground-truth angles theta_star with |theta_star| in [0.2, 1.0]: clear of every
    threshold of the screw map, and an optimum with loss 0."""
    kind, P, k, empty, M, n_iter, s = IK_CASES[name]
    rng = np.random.default_rng([77, IK_SEED_SALT[name], s if seed is None else seed])
    E = P - 1
    parent, edge_of, order, owners = kin_ref.random_tree(rng, P, kind, empty=empty)
    if isinstance(k, list):
        counts = np.zeros(P, np.int64)
        if k[0] == 0:                                            # the root owns nothing, the rest by order
            counts[order[1:]] = k[1:]
        else:
            counts[rng.permutation(P)] = k
    else:
        counts = np.zeros(P, np.int64)
        counts[owners] = k
    part = rng.permutation(np.repeat(np.arange(P), counts)).astype(np.int64)
    n = len(part)
    axis = rng.normal(size=(E, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    moment = rng.normal(0, 0.3, (E, 3))
    src = rng.uniform(-0.3, 0.3, (n, 3))
    theta_star = rng.uniform(0.2, 1.0, (M, E)) * rng.choice([-1.0, 1.0], (M, E))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    axis, moment, src, theta_star = f32(axis), f32(moment), f32(src), f32(theta_star)
    tree = (parent, edge_of, order)
    with torch.no_grad():
        t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)
        tgt = kin_ref.apply_parts(t64(src), _fk(tree, t64(axis.reshape(E, 3)), t64(moment.reshape(E, 3)), t64(theta_star)), part)
    if E == 0:                                                   # nothing to fit: targets off the points, a loss to report
        tgt = tgt + t64(rng.normal(0, 0.1, (M, n, 3)))
    return dict(name=name, tree=tree, P=P, E=E, n=n, M=M, n_iter=n_iter, axis=axis, moment=moment, src=src, part=part,
                tgt=f32(tgt.numpy()), theta_star=theta_star, counts=counts)


def pointless_edges(case):
    """Edges whose subtree (the child part and everything under it) owns no point: their angle never gets a gradient."""
    parent, edge_of, _ = case["tree"]
    own = case["counts"].astype(np.int64).copy()
    sub = own.copy()
    for c in range(case["P"]):
        q = int(parent[c])
        while q >= 0:
            sub[q] += own[c]
            q = int(parent[q])
    return sorted(int(edge_of[c]) for c in range(case["P"]) if parent[c] >= 0 and sub[c] == 0)


@functools.lru_cache(maxsize=None)
def case_ref(name, dtype="float64", mutate=None, seed=None):
    """(theta, loss) of ik_loop_ref on a case, computed once per process."""
    c = make_ik_case(name, seed)
    return ik_loop_ref(c["tree"], c["axis"], c["moment"], c["src"], c["part"], c["tgt"], c["n_iter"],
                       dtype=getattr(torch, dtype), mutate=mutate)


@functools.lru_cache(maxsize=None)
def warm_ref(dtype="float64"):
    """The warm start: WARM_ITERS steps from the float32 image of the float64 200-step result of WARM_CASE, Adam from zero."""
    c = make_ik_case(WARM_CASE)
    init = case_ref(WARM_CASE)[0].astype(np.float32)
    return init, ik_loop_ref(c["tree"], c["axis"], c["moment"], c["src"], c["part"], c["tgt"], WARM_ITERS, theta_init=init,
                             dtype=getattr(torch, dtype))


def deviation(theta, loss, ref):
    """(max |theta - theta_ref|, max over the first LOSS_STEPS entries of |loss - loss_ref| / loss_ref[0]) against ref = (theta, loss)."""
    th, ls = np.asarray(theta, np.float64), np.asarray(loss, np.float64)
    d_th = float(np.abs(th - ref[0]).max()) if th.size else 0.0
    k = min(LOSS_STEPS, ref[1].shape[1])
    d_ls = float((np.abs(ls[:, :k] - ref[1][:, :k]) / ref[1][:, :1]).max())
    return d_th, d_ls


def spread(name, seed=None):
    """What float32 rounding of the same loop costs on a case: deviation of the float32 loop from the float64 one."""
    return deviation(*case_ref(name, "float32", seed=seed), case_ref(name, "float64", seed=seed))


def warm_spread():
    return deviation(*warm_ref("float32")[1], warm_ref("float64")[1])


def check_fit(theta, loss, ref, sp, what=""):
    """The comparison of the GPU test: theta within IK_TOL_FACTOR x spread(theta), the first LOSS_STEPS losses within
    IK_TOL_FACTOR x spread(loss) of loss_ref[0] -> the measured deviations (printed by the caller before this asserts)."""
    d_th, d_ls = deviation(theta, loss, ref)
    assert np.isfinite(np.asarray(theta)).all() and np.isfinite(np.asarray(loss)).all(), what
    assert d_th <= IK_TOL_FACTOR * sp[0], f"{what}: theta off by {d_th:.3e} rad, bound {IK_TOL_FACTOR:g} x {sp[0]:.3e}"
    assert d_ls <= IK_TOL_FACTOR * sp[1], f"{what}: loss history off by {d_ls:.3e} of loss[0], bound {IK_TOL_FACTOR:g} x {sp[1]:.3e}"
    return d_th, d_ls
