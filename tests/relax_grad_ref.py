"""float64 restatement of one iteration of the relaxation loop (run_robot.py:154-221; oracle/step.py, reart_relax_step) with
torch autograd: the losses and the gradients of the five parameter tensors, W1 | b1 | W2 | p6d | pt (the order of
RelaxEngine.adam_m), that the fused step reduces before Adam -- ``+ wd * param`` included when weight decay is on.

Every discrete decision is taken from the fp32 iteration on the same inputs, i.e. from the C oracle:
  * the hard part of the straight-through Gumbel softmax (oracle.base_forward),
  * the ReLU activity of the seg head (its pre-activation in the oracle's fp32 operation order),
  * the Chamfer neighbours in both directions (oracle.knn_points on the fp32 forward output),
  * the blended flow target and its mask (oracle.blend_anchor_motion; the reference computes them under no_grad).
Huber's branch is not a decision: its loss and gradient are continuous at |d| = 1.

``mutate`` injects one known error, so that a test can show that its comparison rejects it:
  ("scale", name)     the gradient of tensor `name` times 1.001
  "huber_quadratic"   Huber's quadratic branch everywhere (the linear branch dropped)
  "swap_weights"      blend weights from the other distance (Euclidean <-> squared)
  "end_frame_shift"   each non-canonical end frame of the complete sequence (index 0 or B) also takes the flow term of
                      the pair next to it, i.e. the one shifted by one frame (a clamped frame index left unguarded)
  "double_lambda"     lambda_flow (lambda_assign in the assignment loss) applied twice
  "double_smooth"     smooth_weight applied twice
  "drop_tau"          1 / tau dropped from the gradient of the logits (the forward unchanged)

``make_case`` builds the inputs of the configurations both tests run.
Test infrastructure for tests/test_relax_grad_ref_cpu.py and tests/test_step_grad_gpu.py."""
import numpy as np
import torch
import torch.nn.functional as F

PARAMS = ("W1", "b1", "W2", "p6d", "pt")
ORACLE_GRADS = dict(W1="gW1", b1="gb1", W2="gW2", p6d="g6d", pt="gt")
# per tensor: max |g - g_ref| <= TOL * max |g_ref|.  Bound of the fp32 oracle against this restatement
# (tests/test_relax_grad_ref_cpu.py), and the tolerance of the fused kernels (tests/test_step_grad_gpu.py).
# Below 1e-3 with room to spare: a tensor scaled by 1.001 moves its largest entry by 1e-3 of max |g|.
TOL = 2e-4


def relu_active(cano, W1, b1):
    """[N,H] bool: h > 0 with the pre-activation in the oracle's fp32 order (oracle/model.c seg_logits:
    fmaf(W1[j,2], x2, fmaf(W1[j,1], x1, W1[j,0] * x0)) + b1[j]).  The products of two floats are exact in float64, so
    float64 sum then float32 rounding is fmaf up to a double rounding, which cannot change the sign."""
    x = np.asarray(cano, np.float32)
    W1, b1 = np.asarray(W1, np.float32), np.asarray(b1, np.float32)
    acc = x[:, 0:1] * W1[None, :, 0]
    acc = (x[:, 1:2].astype(np.float64) * W1[None, :, 1] + acc).astype(np.float32)
    acc = (x[:, 2:3].astype(np.float64) * W1[None, :, 2] + acc).astype(np.float32)
    return (acc + b1[None]) > 0


def rotation_6d_to_matrix(d6):
    """screw_se3/geo_utils.py:632-651; rows b1, b2, b3"""
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = F.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


def relax_grad_ref(cano, pcs, params, gumbel, tau, cano_idx, refs=None, ref_flows=None, lambda_flow=1.0, robust=False,
                   smooth_weight=1e-2, euclidean=True, weight_decay=0.0, assign=None, mutate=None):
    """One iteration at `params` (dict of fp32 arrays W1 [H,3], b1 [H], W2 [P,H], p6d [B,P,6], pt [B,P,3]) with the
    injected Gumbel noise [N,P] at temperature `tau` (the fp32 value the step uses).  assign = (src [n], tgt [B,n],
    lambda_assign) replaces the Chamfer loss, as in RelaxOracle.step.  ->
    dict(recon, flow (lambda included), grads {name: float64 array}, fw (the oracle's fp32 forward), stats)."""
    import oracle

    o64 = lambda a: torch.as_tensor(np.asarray(a, np.float32), dtype=torch.float64)
    tau = float(np.float32(tau))
    cano32, pcs32 = np.asarray(cano, np.float32), np.asarray(pcs, np.float32)
    fw = oracle.base_forward(cano32, params["W1"], params["b1"], params["W2"], params["p6d"], params["pt"], gumbel, tau)
    X32 = fw["out"]
    B, N = X32.shape[:2]
    P = params["W2"].shape[0]
    prm = {k: o64(params[k]).requires_grad_(True) for k in PARAMS}
    x, Y = o64(cano32), o64(pcs32)

    # seg head, straight-through Gumbel softmax (networks/model.py:42-58)
    pre = x @ prm["W1"].T + prm["b1"]
    h = pre * torch.from_numpy(relu_active(cano32, params["W1"], params["b1"])).to(torch.float64)
    s = h @ prm["W2"].T                                                       # [N,P]
    z = (s + o64(gumbel)) / tau
    if mutate == "drop_tau":                                                  # value unchanged, d z / d s = 1
        z = z + (s - s.detach()) * (1.0 - 1.0 / tau)
    y = z.softmax(-1)
    hard = F.one_hot(torch.from_numpy(fw["hard_idx"].astype(np.int64)), P).to(torch.float64)
    weight = hard - y.detach() + y
    # rigid motion of every part, blended by the weights (networks/model.py:60-68)
    R = rotation_6d_to_matrix(prm["p6d"])                                     # [B,P,3,3]
    pc = torch.einsum("bpij,nj->bpni", R, x) + prm["pt"][:, :, None, :]       # [B,P,N,3]
    X = torch.einsum("np,bpni->bni", weight, pc)                              # [B,N,3]

    bi = torch.arange(B)[:, None]
    if assign is not None:
        src, tgt, lam = assign
        lam = float(np.float32(lam)) * (float(np.float32(lam)) if mutate == "double_lambda" else 1.0)
        src = torch.as_tensor(np.asarray(src, np.int64))
        tgt = torch.as_tensor(np.asarray(tgt, np.int64))
        recon = lam * ((X[:, src] - Y[bi, tgt]) ** 2).sum()
    else:
        # recon_loss (networks/loss.py:24-29): neighbours of the fp32 clouds, distances in float64
        _, i1 = oracle.knn_points(X32, pcs32)
        _, i2 = oracle.knn_points(pcs32, X32)
        i1, i2 = torch.from_numpy(i1[..., 0]), torch.from_numpy(i2[..., 0])
        recon = ((X - Y[bi, i1]) ** 2).sum() + ((Y - X[bi, i2]) ** 2).sum()

    flow = torch.zeros((), dtype=torch.float64)
    stats = {}
    if refs is not None:
        # run_robot.py:194-209: pairs (f, f + 1) of the complete sequence, canonical frame inserted at cano_idx
        c = cano_idx
        comp32 = np.concatenate([X32[:c], cano32[None], X32[c:]], axis=0)
        eu = (not euclidean) if mutate == "swap_weights" else euclidean
        bl = [oracle.blend_anchor_motion(comp32[f], refs[f], ref_flows[f], 3, eu) for f in range(B)]
        gt = torch.from_numpy(np.stack([b[0] for b in bl])).to(torch.float64)
        mask = torch.from_numpy(np.stack([b[1] for b in bl]))
        comp = torch.cat((X[:c], x[None], X[c:]), dim=0)
        pred = comp[1:] - comp[:-1]
        d = pred - gt
        if robust and mutate != "huber_quadratic":
            fterm = F.huber_loss(pred, gt, reduction="none", delta=1.0).sum(-1)
        elif robust:
            fterm = (0.5 * d * d).sum(-1)
        else:
            fterm = (d * d).sum(-1)
        sw = smooth_weight * (smooth_weight if mutate == "double_smooth" else 1.0)
        lf = lambda_flow * (lambda_flow if mutate == "double_lambda" else 1.0)
        m = mask.to(torch.float64)
        flow = lf * (m * fterm + sw * (1.0 - m) * (pred ** 2).sum(-1)).sum()
        if mutate == "end_frame_shift":
            with torch.no_grad():   # d flow / d pred
                gd = torch.where(d.abs() <= 1.0, d, d.sign()) if robust else 2.0 * d
                gpf = lf * (m[..., None] * gd + sw * (1.0 - m[..., None]) * 2.0 * pred)
            extra = torch.zeros((), dtype=torch.float64)
            if c != 0:       # complete frame 0 = X[0] takes + gpf[0] besides its own - gpf[0]
                extra = extra + (gpf[0] * X[0]).sum()
            if c != B:       # complete frame B = X[B - 1] takes - gpf[B - 1] besides its own + gpf[B - 1]
                extra = extra - (gpf[B - 1] * X[B - 1]).sum()
            flow = flow + (extra - extra.detach())
        with torch.no_grad():
            mk = mask[..., None].expand_as(d)
            stats["huber_frac"] = float((d.abs() > 1.0)[mk].double().mean()) if bool(mk.any()) else 0.0
            stats["smooth_frac"] = float((~mask).double().mean())

    (recon + flow).backward()
    grads = {k: prm[k].grad.numpy().copy() for k in PARAMS}
    if weight_decay:
        for k in PARAMS:    # torch.optim.Adam: grad.add(param, alpha=weight_decay), on the parameter before the step
            grads[k] = grads[k] + float(np.float32(weight_decay)) * np.asarray(params[k], np.float64)
    if isinstance(mutate, tuple) and mutate[0] == "scale":
        grads[mutate[1]] = grads[mutate[1]] * 1.001
    return dict(recon=float(recon.detach()), flow=float(flow.detach()), grads=grads, fw=fw, stats=stats)


def grad_spread(got, ref):
    """{name: max |got - ref| / max |ref|} over the five tensors (got: fp32 or float64 arrays of any layout)."""
    out = {}
    for k in PARAMS:
        g = np.asarray(got[k], np.float64).reshape(-1)
        r = np.asarray(ref[k], np.float64).reshape(-1)
        out[k] = float(np.abs(g - r).max() / max(np.abs(r).max(), 1e-30))
    return out


def check_grads(got, ref, tol=TOL, what=""):
    """The comparison of both tests: per tensor, max |got - ref| <= tol * max |ref|.  -> the spreads."""
    sp = grad_spread(got, ref)
    bad = {k: v for k, v in sp.items() if not v <= tol}
    assert not bad, f"{what}: gradient spread above {tol:g} of max|g| in {bad} (all: {sp})"
    return sp


def kernel_grads(adam_m, shapes, beta1=0.9):
    """The gradients the fused step reduced, from RelaxEngine.adam_m after one step from m = 0: the kernel's Adam leaves
    m = g * (1.0f - beta1f), rounded once, so m / (1.0f - beta1f) in fp32 is g within about one ulp.
    shapes: {name: shape} for the names of PARAMS."""
    m = np.asarray(adam_m, np.float32)
    one_minus = np.float32(1.0) - np.float32(beta1)
    out, o = {}, 0
    for k in PARAMS:
        n = int(np.prod(shapes[k]))
        out[k] = (m[o:o + n] / one_minus).reshape(shapes[k])
        o += n
    assert o == m.size, (o, m.size)
    return out


def oracle_grads(out, params, weight_decay=0.0):
    """RelaxOracle.step's gradients (before its Adam) in PARAMS order, ``+ wd * param`` in fp32 as the oracle adds it."""
    g = {k: np.asarray(out["grads"][ORACLE_GRADS[k]], np.float32) for k in PARAMS}
    if weight_decay:
        g = {k: (v + np.float32(weight_decay) * np.asarray(params[k], np.float32)).astype(np.float32) for k, v in g.items()}
    return g


# ------------------------------------------------------------------------------------ configurations
# One edge of the fused step each.  N: the point count on the GPU (64-point search groups, POST_FBS = 512 and
# CG_RANGE = 1024 are the block sizes it straddles); the CPU test runs the same inputs.
CASES = {
    "chamfer_P20_B3_N1025": dict(B=3, N=1025, P=20, cano_idx=1, flow=False),
    "flow_cano0_B4": dict(B=4, N=700, P=20, cano_idx=0),
    "flow_canoB_B4": dict(B=4, N=700, P=20, cano_idx=4),
    "B1_cano0": dict(B=1, N=300, P=20, cano_idx=0),
    "B1_cano1": dict(B=1, N=300, P=20, cano_idx=1),
    "huber_linear": dict(B=3, N=600, P=20, cano_idx=1, robust=True, flow_std=2.5),
    "squared_smooth": dict(B=3, N=600, P=20, cano_idx=2, knn_squared=True, far_refs=True),
    "assign_only": dict(B=3, N=500, P=12, cano_idx=1, flow=False, assign=0.3),
    "assign_flow": dict(B=3, N=500, P=12, cano_idx=1, assign=0.3),
    "weight_decay": dict(B=3, N=400, P=8, cano_idx=1, weight_decay=0.05),
    "P10_N513": dict(B=3, N=513, P=10, cano_idx=2),
    "P32_N63": dict(B=3, N=63, P=32, cano_idx=1),
    "P2_N1088": dict(B=2, N=1088, P=2, cano_idx=1),
    "bwd16": dict(B=4, N=577, P=20, cano_idx=2, tuning={"tune_bwd_pts": 16}),
    "bwd64": dict(B=4, N=577, P=20, cano_idx=2, tuning={"tune_bwd_pts": 64}),
    "fwd64": dict(B=4, N=577, P=20, cano_idx=2, tuning={"tune_fwd_pts": 64}),
}
LAMBDA_FLOW = 0.7


def random_params(rng, B, P, H=128):
    """Seg head and poses; parts start from distinct poses: with equal poses the loss does not depend on the
    segmentation and the seg-head gradient is rounding noise."""
    return dict(W1=rng.normal(0, 0.6, (H, 3)).astype(np.float32), b1=rng.normal(0, 0.1, H).astype(np.float32),
                W2=rng.normal(0, 0.2, (P, H)).astype(np.float32),
                p6d=(np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), (B, P, 1))
                     + rng.normal(0, 0.05, (B, P, 6))).astype(np.float32),
                pt=rng.normal(0, 0.01, (B, P, 3)).astype(np.float32))


def make_case(name, seed=0):
    """Inputs of CASES[name] -> dict(cano, pcs, params (fp32 arrays), refs, flows, cano_idx, kw (RelaxOracle and
    relax_grad_ref keywords), engine_kw (RelaxEngine keywords), assign, tuning)."""
    c = CASES[name]
    B, N, P = c["B"], c["N"], c["P"]
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    cano = rng.uniform(-0.3, 0.3, (N, 3)).astype(np.float32)
    pcs = (cano[None] + rng.normal(0, 0.02, (B, N, 3))).astype(np.float32)
    params = random_params(rng, B, P)
    refs = flows = None
    if c.get("flow", True):
        lens = [int(m) for m in rng.integers(N // 3, N + 1, B)]
        refs = [rng.uniform(-0.3, 0.3, (m, 3)).astype(np.float32) for m in lens]
        if c.get("far_refs"):     # references in the slab x < -0.2 only: points past x ~ 0.03 are farther than sqrt(0.05)
            for r in refs:
                r[:, 0] = rng.uniform(-0.3, -0.2, r.shape[0])
        flows = [rng.normal(0, c.get("flow_std", 0.02), r.shape).astype(np.float32) for r in refs]
    assign = None
    if c.get("assign"):
        n = N // 2
        assign = (rng.permutation(N)[:n], np.stack([rng.permutation(N)[:n] for _ in range(B)]), c["assign"])
    lam = LAMBDA_FLOW if refs is not None else 1.0
    kw = dict(lambda_flow=lam, robust=c.get("robust", False), smooth_weight=1e-2,
              euclidean=not c.get("knn_squared", False), weight_decay=c.get("weight_decay", 0.0))
    engine_kw = dict(lambda_flow=lam, use_robust_loss=kw["robust"], smooth_weight=1e-2,
                     knn_squared=c.get("knn_squared", False), weight_decay=kw["weight_decay"])
    return dict(cano=cano, pcs=pcs, params=params, refs=refs, flows=flows, cano_idx=c["cano_idx"], kw=kw,
                engine_kw=engine_kw, assign=assign, tuning=c.get("tuning"))


def gumbel(rng, N, P):
    return -np.log(rng.exponential(size=(N, P))).astype(np.float32)
