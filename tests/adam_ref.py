"""Float64 restatement of torch.optim.Adam's step (numpy only, nothing of the product): parameter groups, amsgrad, L2 weight
decay, maximize and a step count per tensor, with the fixed inputs and the criterion the optimiser tests share.

Per element, for a tensor at its 1-based step count `step`, with the options of its group:

    g = -g (maximize);  g = g + wd * p (wd != 0)
    m = m + (g - m) * (1 - beta1);  v = v * beta2 + ((1 - beta2) * g) * g;  vmax = max(vmax, v) (amsgrad)
    p = p - lr / (1 - beta1^step) * (m / (sqrt(v or vmax) / sqrt(1 - beta2^step) + eps))

A tensor without a gradient at a step is skipped and its state is untouched; state starts at zero at a tensor's first step.
`dtype=np.float32` evaluates the same expression with one float32 rounding per operation (the scalars formed in double and
rounded once): what a correct float32 implementation may look like.  `mutate` plants one known error, so that a test can show
that the criterion rejects it:
    no_amsgrad_max        the denominator uses v although amsgrad is on
    decoupled_decay       p *= 1 - lr * wd instead of g += wd * p
    step_off_by_one       bias corrections of step + 1
    no_eps                eps left out of the denominator
    no_bias_correction2   sqrt(v) not divided by sqrt(1 - beta2^step)
    ignore_maximize       the gradient is not negated

The criterion (tests of reart_amd.optim.Adam): D = max |p - p_float64| over all elements after the last step, for the
implementation under test and for torch.optim.Adam(foreach=False) on the same device and float32 inputs; D_test <= 2 * D_torch.
Both are float32 evaluations of one formula and may differ by contraction and by a multiplication with a reciprocal in place
of a division by a host scalar, each an ulp of an intermediate; a wrong formula is at least 60 times torch's deviation."""
import numpy as np

MUTATIONS = ("no_amsgrad_max", "decoupled_decay", "step_off_by_one", "no_eps", "no_bias_correction2", "ignore_maximize")
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)      # around the 256-thread block: one element, tails, exact blocks, several blocks
STEPS = 6
GRID = [(a, w, m) for a in (False, True) for w in (0.0, 1e-2) for m in (False, True)]      # amsgrad x weight decay x maximize


def group(lr, weight_decay=0.0, amsgrad=False, maximize=False, betas=(0.9, 0.999), eps=1e-8):
    return dict(lr=lr, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, betas=betas, eps=eps)


def gradients(rng, sizes, steps=STEPS):
    """N(0, 1) times 10^U(-8, 1) per element: eps matters for some entries, and with amsgrad the running maximum differs
    from v for some.  -> [steps][tensor] float32."""
    return [[(rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 1, n)).astype(np.float32) for n in sizes] for _ in range(steps)]


def case(amsgrad, weight_decay, maximize, seed=0, sizes=SIZES):
    """The fixed inputs: eight parameters in two groups (the first three: lr 1e-2, no decay; the other five: lr 1e-3 and
    `weight_decay`), six steps.  -> (params [tensor] float32, groups, group_of [tensor], grads [step][tensor] float32)."""
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    groups = [group(1e-2, 0.0, amsgrad, maximize), group(1e-3, weight_decay, amsgrad, maximize)]
    group_of = [0 if k < 3 else 1 for k in range(len(sizes))]
    return params, groups, group_of, gradients(rng, sizes)


def adam_ref(params, groups, group_of, grads, state=None, dtype=np.float64, mutate=None):
    """`grads`: [step][tensor], None where a tensor has no gradient at that step.  `state`: {tensor index: dict(step, m, v,
    vmax)} carried from an earlier call (modified and returned).  -> (params [tensor] of `dtype`, state)."""
    assert mutate is None or mutate in MUTATIONS
    f = dtype
    p = [np.asarray(x).astype(f) for x in params]
    state = {} if state is None else state
    for step_grads in grads:
        for k, g in enumerate(step_grads):
            if g is None:
                continue
            o = groups[group_of[k]]
            st = state.setdefault(k, dict(step=0, m=np.zeros_like(p[k]), v=np.zeros_like(p[k]), vmax=np.zeros_like(p[k])))
            for name in ("m", "v", "vmax"):
                st[name] = st[name].astype(f)
            st["step"] += 1
            step = st["step"] + (1 if mutate == "step_off_by_one" else 0)
            beta1, beta2 = o["betas"]
            step_size = f(o["lr"] / (1.0 - beta1 ** step))
            bc2_sqrt = f((1.0 - beta2 ** step) ** 0.5)
            w1, w2, b2, eps, wd = f(1.0 - beta1), f(1.0 - beta2), f(beta2), f(o["eps"]), f(o["weight_decay"])
            g = np.asarray(g).astype(f)
            if o["maximize"] and mutate != "ignore_maximize":
                g = -g
            if o["weight_decay"] != 0:
                if mutate == "decoupled_decay":
                    p[k] = p[k] * f(1.0 - o["lr"] * o["weight_decay"])
                else:
                    g = g + wd * p[k]
            st["m"] = st["m"] + (g - st["m"]) * w1
            st["v"] = st["v"] * b2 + (w2 * g) * g
            second = st["v"]
            if o["amsgrad"]:
                st["vmax"] = np.maximum(st["vmax"], st["v"])
                if mutate != "no_amsgrad_max":
                    second = st["vmax"]
            root = np.sqrt(second)
            denom = root if mutate == "no_bias_correction2" else root / bc2_sqrt
            if mutate != "no_eps":
                denom = denom + eps
            with np.errstate(divide="ignore", invalid="ignore"):
                p[k] = p[k] - step_size * (st["m"] / denom)
            assert p[k].dtype == f and st["m"].dtype == f and st["v"].dtype == f
    return p, state


def deviation(got, ref):
    """max |got - ref| over all elements of all tensors, in double."""
    return max((float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) for a, b in zip(got, ref) if np.size(b)),
               default=0.0)


def criterion(d_test, d_torch):
    return d_test <= 2.0 * d_torch


def run_torch(make_optimizer, params, groups, group_of, grads, device="cpu", dtype=None, views=None, on_step=None):
    """The same inputs through a torch-style optimiser class on `device`: `make_optimizer(param_groups)` -> optimiser.
    `views(k, array)` -> the tensor that holds parameter k (default: a tensor of its own); gradients likewise with
    `views(k, array, grad=True)`.  `on_step(t, optimiser, tensors)` runs after step t (0-based).
    -> (params [tensor] numpy, optimiser, tensors)."""
    import torch

    dtype = dtype or torch.float32
    put = views or (lambda k, a, grad=False: torch.from_numpy(np.array(a)).to(device=device, dtype=dtype))
    tensors = [put(k, a).requires_grad_(True) for k, a in enumerate(params)]
    opt = make_optimizer([dict(params=[t for t, j in zip(tensors, group_of) if j == i], **o) for i, o in enumerate(groups)])
    for i, step_grads in enumerate(grads):
        for k, (t, g) in enumerate(zip(tensors, step_grads)):
            t.grad = None if g is None else put(k, g, grad=True)
        opt.step()
        if on_step is not None:
            on_step(i, opt, tensors)
    return [t.detach().cpu().numpy() for t in tensors], opt, tensors
