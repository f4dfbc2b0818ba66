"""``reart_amd.optim.Adam`` (reart_adam_groups) on the GPU against the float64 restatement of tests/adam_ref.py.

The criterion throughout: D = max |p - p_float64| over all elements after the last step; D of the optimiser under test is at most
twice D of torch.optim.Adam(foreach=False) on the same device with the same float32 inputs (adam_ref docstring: both are float32
evaluations of one formula; any wrong formula, table or block map is at least 60 times torch's deviation).  Both figures, and
the number of elements whose bits differ from torch's two paths, are printed per case; bit equality is reported, not asserted."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

from tests import adam_ref as ar

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FULL = (True, 1e-2, True)       # amsgrad, weight decay and maximize all on


@functools.lru_cache(maxsize=None)
def _reference(amsgrad, wd, maximize):
    """(case, float64 restatement, torch foreach=False, torch foreach=True, D_torch) of a grid case, computed once."""
    case = ar.case(amsgrad, wd, maximize)
    ref, _ = ar.adam_ref(*case)
    single, _, _ = ar.run_torch(lambda g: torch.optim.Adam(g, foreach=False), *case, device="cuda:0")
    multi, _, _ = ar.run_torch(lambda g: torch.optim.Adam(g, foreach=True), *case, device="cuda:0")
    return case, ref, single, multi, ar.deviation(single, ref)


def _native(groups):
    from reart_amd.optim import Adam

    return Adam(groups)


def _differing(a, b):
    return sum(int(np.count_nonzero(x.view(np.int32) != y.view(np.int32))) for x, y in zip(a, b))


@pytest.mark.parametrize("amsgrad,wd,maximize", ar.GRID)
def test_parity_grid(dev, amsgrad, wd, maximize):
    case, ref, single, multi, d_torch = _reference(amsgrad, wd, maximize)
    launches = []
    got, opt, _ = ar.run_torch(_native, *case, device=dev, on_step=lambda i, o, t: launches.append((o.last_path, o.last_launches)))
    d_fused = ar.deviation(got, ref)
    n = sum(ar.SIZES)
    print(f"amsgrad {amsgrad} wd {wd} maximize {maximize}: D_fused {d_fused:.3e} D_torch {d_torch:.3e}; elements of {n} whose bits "
          f"differ from foreach=False {_differing(got, single)}, from foreach=True {_differing(got, multi)}")
    assert launches == [("native", 1)] * ar.STEPS
    assert d_torch > 0 and ar.criterion(d_fused, d_torch), (d_fused, d_torch)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_views_aligned_to_four_bytes_only(dev, offset):
    """Parameters and gradients are contiguous slices that start `offset` elements past a 16-byte boundary, between guard
    elements; the guards keep their bits, and so does every gradient (weight decay and maximize happen in registers)."""
    case, ref, _, _, d_torch = _reference(*FULL)
    guard, buffers = np.float32(12345.678), []

    def view(k, a, grad=False):
        buf = torch.full((len(a) + 12,), float(guard), device=dev)
        assert buf.data_ptr() % 16 == 0
        s = buf[4 + offset:4 + offset + len(a)]
        s.copy_(torch.from_numpy(np.array(a)))
        buffers.append((buf, 4 + offset, len(a), np.array(a) if grad else None))
        return s

    got, opt, tensors = ar.run_torch(_native, *case, device=dev, views=view)
    assert opt.last_path == "native" and opt.last_launches == 1
    assert all(t.data_ptr() % 16 == 4 * offset for t in tensors)
    d_fused = ar.deviation(got, ref)
    print(f"offset {offset}: D_fused {d_fused:.3e} D_torch {d_torch:.3e}")
    assert ar.criterion(d_fused, d_torch), (d_fused, d_torch)
    for buf, start, n, grad in buffers:
        host = buf.cpu().numpy()
        outside = np.concatenate([host[:start], host[start + n:]])
        assert np.array_equal(outside.view(np.int32), np.full_like(outside, guard).view(np.int32))
        if grad is not None:
            assert np.array_equal(host[start:start + n].view(np.int32), grad.view(np.int32))


def test_more_tensors_than_one_call_takes(dev):
    """2 x capacity + 3 parameters of 0 to 5 elements in one group: three calls; the criterion; and the same bits as the same
    parameters stepped eight to an optimiser."""
    from reart_amd import _lib

    count = 2 * _lib.ADAM_MAX_TENSORS + 3
    sizes = [k % 6 for k in range(count)]
    rng = np.random.default_rng(5)
    params = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    groups, group_of, grads = [ar.group(1e-3, 1e-2, True, False)], [0] * count, ar.gradients(rng, sizes)
    case = (params, groups, group_of, grads)
    ref, _ = ar.adam_ref(*case)
    d_torch = ar.deviation(ar.run_torch(lambda g: torch.optim.Adam(g, foreach=False), *case, device=dev)[0], ref)
    got, opt, _ = ar.run_torch(_native, *case, device=dev)
    assert opt.last_path == "native" and opt.last_launches == 3
    d_fused = ar.deviation(got, ref)
    print(f"{count} tensors: D_fused {d_fused:.3e} D_torch {d_torch:.3e}")
    assert d_torch > 0 and ar.criterion(d_fused, d_torch), (d_fused, d_torch)
    for lo in range(0, count, 8):
        part, opt8, _ = ar.run_torch(_native, params[lo:lo + 8], groups, group_of[lo:lo + 8], [g[lo:lo + 8] for g in grads], device=dev)
        assert opt8.last_launches == 1
        for a, b in zip(part, got[lo:lo + 8]):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_parameters_without_a_gradient(dev):
    """Tensor 1 never has a gradient: untouched, no state.  Tensor 4 gets its first at the third step: its step count reads 1
    when the others read 3, and it is checked against the restatement with that count."""
    params, groups, group_of, grads = ar.case(*FULL)
    for t, step_grads in enumerate(grads):
        step_grads[1] = None
        if t < 2:
            step_grads[4] = None
    case = (params, groups, group_of, grads)
    ref, state = ar.adam_ref(*case)
    assert 1 not in state and state[4]["step"] == ar.STEPS - 2
    d_torch = ar.deviation(ar.run_torch(lambda g: torch.optim.Adam(g, foreach=False), *case, device=dev)[0], ref)
    seen = {}

    def after(i, opt, tensors):
        assert opt.last_path == "native" and opt.last_launches == 1
        if i == 2:
            seen.update({k: float(opt.state[t]["step"]) for k, t in enumerate(tensors) if t in opt.state})

    got, opt, tensors = ar.run_torch(_native, *case, device=dev, on_step=after)
    assert seen == {k: (1.0 if k == 4 else 3.0) for k in range(len(params)) if k != 1}
    assert tensors[1] not in opt.state and np.array_equal(got[1].view(np.int32), params[1].view(np.int32))
    assert float(opt.state[tensors[4]]["step"]) == ar.STEPS - 2 and opt.state[tensors[4]]["step"].device.type == "cpu"
    d_fused, d_late = ar.deviation(got, ref), ar.deviation([got[4]], [ref[4]])
    print(f"D_fused {d_fused:.3e} (the late tensor alone {d_late:.3e}) D_torch {d_torch:.3e}")
    assert d_torch > 0 and ar.criterion(d_fused, d_torch), (d_fused, d_torch)


def _advance(opt, tensors, grads, dev):
    for step_grads in grads:
        for t, g in zip(tensors, step_grads):
            t.grad = torch.from_numpy(g).to(dev)
        opt.step()


@pytest.mark.parametrize("first", ["native", "torch"])
def test_state_goes_to_torch_and_back(dev, first):
    """Three steps with one optimiser, its state_dict loaded into the other, three more steps: six steps of the restatement."""
    from reart_amd.optim import Adam

    case, ref, _, _, d_torch = _reference(*FULL)
    params, groups, group_of, grads = case
    classes = {"native": Adam, "torch": lambda g: torch.optim.Adam(g, foreach=False)}
    tensors = [torch.from_numpy(p.copy()).to(dev).requires_grad_(True) for p in params]
    make = lambda name: classes[name]([dict(params=[t for t, j in zip(tensors, group_of) if j == i], **o) for i, o in enumerate(groups)])
    a, b = make(first), make("torch" if first == "native" else "native")
    _advance(a, tensors, grads[:3], dev)
    sa = copy.deepcopy(a.state_dict())                       # load_state_dict shares the tensors it is given
    b.load_state_dict(a.state_dict())
    _advance(b, tensors, grads[3:], dev)
    native = a if first == "native" else b
    assert native.last_path == "native" and native.last_launches == 1
    d = ar.deviation([t.detach().cpu().numpy() for t in tensors], ref)
    print(f"{first} first: D {d:.3e} D_torch {d_torch:.3e}")
    assert ar.criterion(d, d_torch), (d, d_torch)
    # the same keys, shapes, dtypes and devices as torch's state
    sb = b.state_dict()
    assert sa["param_groups"] == sb["param_groups"] and sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        assert list(sa["state"][k]) == list(sb["state"][k]) == ["step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"]
        for name, v in sa["state"][k].items():
            w = sb["state"][k][name]
            assert (v.shape, v.dtype, v.device) == (w.shape, w.dtype, w.device), (k, name)
        assert float(sa["state"][k]["step"]) == 3.0 and float(sb["state"][k]["step"]) == 6.0


@pytest.mark.parametrize("what", ["float64", "transposed", "capturable"])
def test_other_inputs_take_torchs_step(dev, what):
    """One parameter outside the native path's contract, or a group switch it does not cover: the whole step is torch's."""
    from reart_amd.optim import Adam

    def build(cls):
        g = torch.Generator(device=dev).manual_seed(3)
        r = lambda *s, **kw: torch.randn(*s, device=dev, generator=g, **kw)
        plain, odd = r(40).requires_grad_(True), r(6, 7, dtype=torch.float64 if what == "float64" else torch.float32)
        odd = (odd.t() if what == "transposed" else odd).requires_grad_(True)
        opt = cls([plain, odd], lr=1e-2, amsgrad=True, weight_decay=1e-2, capturable=what == "capturable")
        for _ in range(3):
            plain.grad, odd.grad = r(40), r(*odd.shape, dtype=odd.dtype)
            opt.step()
        return opt, plain, odd

    opt, plain, odd = build(Adam)
    _, plain_t, odd_t = build(torch.optim.Adam)
    assert opt.last_path == "torch" and opt.last_launches == 0
    assert (what == "transposed") == (not odd.is_contiguous())
    assert torch.equal(plain, plain_t) and torch.equal(odd, odd_t)


def test_state_the_kernel_cannot_index_takes_torchs_step(dev):
    """A moment that is not laid out like its parameter (set by hand here: a transposed buffer) sends the step to torch."""
    from reart_amd.optim import Adam

    def build(cls):
        g = torch.Generator(device=dev).manual_seed(5)
        p = torch.randn(6, 7, device=dev, generator=g).requires_grad_(True)
        opt = cls([p], lr=1e-2, amsgrad=True)
        paths = []
        for i in range(3):
            p.grad = torch.randn(6, 7, device=dev, generator=g)
            if i == 1:
                opt.state[p]["exp_avg"] = opt.state[p]["exp_avg"].t().contiguous().t()
                assert not opt.state[p]["exp_avg"].is_contiguous()
            opt.step()
            paths.append(getattr(opt, "last_path", None))
        return p, paths

    p, paths = build(Adam)
    p_t, _ = build(lambda g, **kw: torch.optim.Adam(g, foreach=False, **kw))
    assert paths == ["native", "torch", "torch"]
    # Only the first step differs between the two runs (native against torch's).  Per step each run rounds p - u once, so the
    # runs part by at most one float32 spacing of p per step, plus the difference of the two u, 2 ulp(lr) = 2e-9 per step and
    # far below a spacing here: three steps, three spacings of the largest |p|; four leaves room for the u terms.
    p, p_t = p.detach(), p_t.detach()
    assert float((p - p_t).abs().max()) <= 4 * float(np.spacing(np.float32(p_t.abs().max().item())))


def _operator_loop(dev, fused_adam, kinematic, n_iter=3):
    """tests/test_chamfer_loss_gpu.py::_loop with the optimiser switch; parameters after every iteration."""
    import functools as ft

    from reart_amd import run_robot as rr

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    flag = ["--fused_adam"] if fused_adam else []
    if kinematic:
        from tests.test_kinematic_engine_gpu import _model

        k = np.load(os.path.join(HERE, "golden", "kinematic.npz"))
        cano, rng = t(k["cano_pc"]), np.random.default_rng(3)
        with torch.no_grad():
            pcs = _model(dev, k, cano)(cano)[0]
        pcs = (pcs + t(rng.normal(0, 0.004, tuple(pcs.shape)).astype(np.float32))).contiguous()
        comp = torch.cat((pcs[:2], cano[None], pcs[2:]), dim=0)
        sel = [torch.from_numpy(rng.permutation(cano.shape[0])[:300 + 7 * f]).to(dev) for f in range(pcs.shape[0])]
        refs, flows = [comp[f][s] for f, s in enumerate(sel)], [(comp[f + 1][s] - comp[f][s]) * 0.5 for f, s in enumerate(sel)]
        a = rr.build_parser().parse_args(["--model", "kinematic", "--use_flow_loss", "--cano_idx", "2"] + flag)
        model, tau = _model(dev, k, cano), None
    else:
        from reart_amd.networks.model import BaseModel
        from reart_amd.synthetic import make_sequence, split_canonical
        from reart_amd.utils.model_utils import tau_cosine

        seq = make_sequence(T=4, n_parts=4, pts_per_part=128, with_flow=True)
        cano, pcs = split_canonical(seq["complete"].astype(np.float32), 2)
        cano, pcs = t(cano), t(pcs)
        refs, flows = [t(r.astype(np.float32)) for r in seq["ref_loc"]], [t(f.astype(np.float32)) for f in seq["ref_flow"]]
        a = rr.build_parser().parse_args(["--model", "base", "--use_flow_loss", "--cano_idx", "2"] + flag)
        torch.manual_seed(4)
        model = BaseModel(num_parts=a.num_parts, pose_len=pcs.shape[0]).to(dev)
        tau = ft.partial(tau_cosine, max_iter=a.n_iter, end_temp=a.end_tau, start_temp=a.start_tau)
    loop = rr.OperatorLoop(a, model, cano, pcs, refs, flows, tau)
    torch.manual_seed(9)                                         # the Gumbel draws of the model's forward
    rows, params = [], []
    for i in range(n_iter):
        losses = loop.iteration(i)
        rows.append({name: float(v.detach()) for name, v in losses.items()})
        params.append([p.detach().clone() for g in loop.optimizer.param_groups for p in g["params"]])
    return loop, rows, params


@pytest.mark.parametrize("kinematic", [False, True], ids=["base", "kinematic"])
def test_operator_loop_with_fused_adam(dev, kinematic):
    """Three iterations of OperatorLoop (T = 4, 4 parts x 128 points, flow loss; the kinematic case on the model of
    tests/test_kinematic_engine_gpu.py) with --fused_adam and without it, generators seeded alike.  Iteration 0 starts from
    the same parameters and noise, so its losses are equal.  One Adam step from zero moments moves an entry by
    lr * g / (|g| + eps), at most lr, and both runs hold the same gradients: the parameters after iteration 0 agree within
    2 ulp of the entry's group's lr.  (For an entry with |p| >> lr that leaves no room at all: p - u is rounded to the grid of
    p, whose spacing exceeds 2 ulp(lr), so the two runs must agree in every bit there.  The kernel's roundings are those of the
    multi-tensor kernels torch.optim.Adam uses by default on the GPU, csrc/adam.hip; with one rounding per operation instead,
    1 of 2560 entries of W2 and 5 of 135 of the kinematic model were beyond the bound, by one spacing of the entry, up to
    64 ulp(lr).)
    Later iterations are printed and only asserted to be finite."""
    from reart_amd.optim import Adam

    loop_on, rows_on, p_on = _operator_loop(dev, True, kinematic)
    loop_off, rows_off, p_off = _operator_loop(dev, False, kinematic)
    assert type(loop_on.optimizer) is Adam and loop_on.optimizer.last_path == "native" and loop_on.optimizer.last_launches == 1
    assert type(loop_off.optimizer) is torch.optim.Adam
    for i, (on, off) in enumerate(zip(rows_on, rows_off)):
        print(f"iteration {i}: fused {on} torch {off}")
    assert rows_on[0] == rows_off[0]
    lrs = [g["lr"] for g in loop_on.optimizer.param_groups for _ in g["params"]]
    worst = 0.0
    for a, b, lr in zip(p_on[0], p_off[0], lrs):
        ulp = float(np.spacing(np.float32(lr)))
        diff = (a.double() - b.double()).abs()
        worst = max(worst, float(diff.max()) / ulp)
        print(f"after iteration 0: {tuple(a.shape)} lr {lr}: max |difference| {float(diff.max()):.3e} = {float(diff.max()) / ulp:.2f} ulp(lr), "
              f"{int((diff > 2 * ulp).sum())} of {a.numel()} entries beyond 2 ulp(lr), {int((a != b).sum())} differ at all")
    assert worst <= 2.0, worst
    for i in range(len(p_on)):
        print(f"after iteration {i}: {sum(int((a != b).sum()) for a, b in zip(p_on[i], p_off[i]))} entries differ in any bit")
    for ps in (p_on[-1], p_off[-1]):
        assert all(torch.isfinite(p).all() for p in ps)
    assert all(np.isfinite(v) for row in rows_on + rows_off for v in row.values())


def test_ik_single_with_fused_adam(dev, monkeypatch):
    """The model and samples of tests/test_ik_gpu.py: the retarget error with reart_amd.optim.Adam is within 1 % of the error
    with torch.optim.Adam, the bound that test uses for the same optimiser on another device; every step is native."""
    from reart_amd.knn_cuda import KNN
    from reart_amd.networks.model import KinematicModel
    from reart_amd.optim import Adam
    from reart_amd.utils.kinematic_utils import JointTree, ik_single

    eligible, plain_check = [], Adam._with_grad
    monkeypatch.setattr(Adam, "_with_grad", lambda self: eligible.append(plain_check(self)) or eligible[-1])

    K, G = np.load(os.path.join(HERE, "golden", "kinematic.npz")), np.load(os.path.join(HERE, "golden", "ik_nao.npz"))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    parent, edge_of = K["parent"], K["edge_of_part"]
    edges = sorted(((int(edge_of[c]), c, int(parent[c])) for c in range(len(parent)) if parent[c] >= 0))
    tree = JointTree([[c, p] for _, c, p in edges], int(K["order"][0]))
    model = KinematicModel(pose_len=9, seg_part=t(K["seg_part"]), cano_pc=t(K["cano_pc"]), knn=KNN(k=1, transpose_mode=True),
                           edge_index={f"{c}_{p}": e for e, c, p in edges}, paths_to_base=tree.paths_to_base,
                           reverse_topo=K["order"].tolist(), axis_list=t(K["axis"]), moment_list=t(K["moment"]),
                           theta_list=t(K["theta"])).to(dev)
    for s in range(3):
        novel = dict(sparse_cano_pc=G[f"sparse_cano_{s}"], sparse_novel_pc=G[f"sparse_novel_{s}"], novel_pc=G[f"novel_pc_{s}"])
        plain, _ = ik_single(model, t(K["cano_pc"]), novel, dev)
        fused, kw = ik_single(model, t(K["cano_pc"]), novel, dev, fused_adam=True)
        print(f"sample {s}: retarget error {fused:.5f} with fused_adam, {plain:.5f} without")
        assert kw["theta_list"].shape == (1, 9)
        assert abs(fused - plain) <= 1e-2 * plain, (s, fused, plain)
    assert len(eligible) == 3 * 200 and all(w is not None and len(w[0][1]) == 1 for w in eligible)
