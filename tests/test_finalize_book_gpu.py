"""The end-of-iteration bookkeeping as one workgroup of the finalize launch (csrc/model.hip: base_bwd_finalize_book) and the
Adam step sizes in two workspace slots -- written for the NEXT step by that workgroup, promoted by the backward block launch
of the next iteration, seeded in both slots by reart_relax_prepare.  What can go wrong is an ordering or a slot mistake, and
it shows where the same iterations are cut differently into launch sequences: eager steps, graphs of odd and even lengths, a
second prepare in mid-run, the batched planes, the long model path and the step without a search launch.  Every comparison
is byte for byte except the temperature against the host's cosine (1e-6, the bound tests/test_step_gpu.py holds it to)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N_ITER, START_TAU, END_TAU = 50, 5.0, 1.0


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _data(N, T, seed, flow=True):
    rng = np.random.default_rng(seed)
    B = T - 1
    cano = rng.uniform(-0.3, 0.3, (N, 3)).astype(np.float32)
    pcs = (cano[None] + rng.normal(0, 0.02, (B, N, 3))).astype(np.float32)
    refs = flows = None
    if flow:
        refs = [rng.uniform(-0.3, 0.3, (max(3, N // 2) + 7 * i, 3)).astype(np.float32) for i in range(B)]
        flows = [rng.normal(0, 0.02, r.shape).astype(np.float32) for r in refs]
    return dict(cano=cano, pcs=pcs, refs=refs, flows=flows, B=B, N=N)


def _engine(dev, d, P, H=128, seed=0, cano_idx=1, **kw):
    """A fresh model (the same initial weights for the same seed) and its engine."""
    from reart_amd.networks.blocks import MLPConv1d
    from reart_amd.networks.model import BaseModel
    from reart_amd.relax import RelaxEngine

    torch.manual_seed(seed)
    model = BaseModel(num_parts=P, pose_len=d["B"])
    if H != 128:
        model.seg_head = MLPConv1d(3, (H, P), bn=False, gn=False, last_activation="none")
    model = model.to(dev)
    refs = None if d["refs"] is None else [t(r, dev) for r in d["refs"]]
    flows = None if d["flows"] is None else [t(f, dev) for f in d["flows"]]
    eng = RelaxEngine(t(d["cano"], dev), t(d["pcs"], dev), model, cano_idx, refs, flows, n_iter=N_ITER, start_tau=START_TAU,
                      end_tau=END_TAU, lambda_flow=0.7, seed=5, **kw)
    return eng


def _state(eng):
    it, log = eng.loss_log()
    out = [p.detach().cpu().numpy().copy() for p in eng.params]
    out += [log.cpu().numpy(), eng.tau.cpu().numpy(), eng.iter.cpu().numpy(), eng.last_losses().cpu().numpy()]
    return out


def _same(a, b, what):
    names = ("W1", "b1", "W2", "p6d", "pt", "loss_log", "tau", "iter", "last_losses")
    for k, x, y in zip(names, a, b):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {k} differs"


def _graph_of(eng, k):
    """k iterations captured WITHOUT a warm-up iteration (the kernels are loaded: an eager engine has run in this process),
    so that graph lengths and eager steps add up to the iteration count exactly."""
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for _ in range(k):
            eng._enqueue()
    eng._graph, eng._steps_per_graph = g, k


def _check_scalars(eng, n):
    """n eager iterations, one at a time: iter, the next temperature and the loss row's temperature after each."""
    from reart_amd.utils.model_utils import tau_cosine

    for k in range(int(eng.iter.item()) + 1, int(eng.iter.item()) + n + 1):
        used = eng.tau.cpu().numpy()[0]
        eng.step()
        assert int(eng.iter.item()) == k
        want = tau_cosine(k + 1, N_ITER, END_TAU, START_TAU)
        got = float(eng.tau.item())
        print(f"iteration {k}: tau {got!r}, host {want!r}")
        assert abs(got - want) < 1e-6, (k, got, want)
        row = eng.last_losses().cpu().numpy()
        assert row[3].tobytes() == used.tobytes(), (k, row, used)       # the temperature this iteration USED
        assert np.isfinite(row).all() and row[0] > 0


_EAGER7 = {}


def _eager7(dev):
    """T = 6, N = 512 with flow, seven eager steps (checked against the host on the way): the reference of the splits."""
    if "state" not in _EAGER7:
        d = _data(512, 6, 11)
        eng = _engine(dev, d, 20)
        _check_scalars(eng, 7)
        _EAGER7["data"], _EAGER7["state"] = d, _state(eng)
    return _EAGER7["data"], _EAGER7["state"]


def test_scalars_against_the_host_over_seven_iterations(dev):
    d, state = _eager7(dev)
    assert int(state[7][0]) == 7 and state[5].shape == (7, 4)
    assert np.isfinite(state[5]).all() and all(np.isfinite(x).all() for x in state[:5])


@pytest.mark.parametrize("glen,replays,eager", [(7, 1, 0), (2, 3, 1), (3, 2, 1)])
def test_split_invariance(dev, glen, replays, eager):
    """Seven iterations as one graph of 7, as a graph of 2 replayed three times plus one eager step, as a graph of 3
    replayed twice plus one eager step: what seven eager steps leave.  With an odd graph length the same graph node runs
    at both parities of the iteration count, so a slot chosen by parity or a promotion that is skipped breaks here."""
    d, ref = _eager7(dev)
    eng = _engine(dev, d, 20)
    _graph_of(eng, glen)
    eng.step(glen * replays + eager)
    assert (eng.graph_replays, eng.eager_steps) == (replays, eager)
    _same(_state(eng), ref, f"graph of {glen} x {replays} + {eager} eager")


def test_adam_step_count_survives_a_second_prepare(dev):
    """Three iterations from a fresh prepare; and two iterations, a second reart_relax_prepare (iter = 2 is caller state and
    stays), one more.  prepare seeds BOTH step-size slots with step 3's, so the block launch that follows promotes the
    right values whatever the bookkeeping workgroup of iteration 2 had left."""
    from reart_amd import _lib
    from reart_amd.relax import _lib_fns

    d = _data(512, 6, 11)
    a = _engine(dev, d, 20)
    a.step(3)
    b = _engine(dev, d, 20)
    b.step(2)
    torch.cuda.synchronize()
    rc = _lib_fns().reart_relax_prepare(ctypes.byref(b.cfg), ctypes.byref(b._bufs), _lib.ptr(b.workspace), b.workspace.numel(),
                                        _lib.stream())
    _lib.check(rc, "reart_relax_prepare")
    assert int(b.iter.item()) == 2
    b.step(1)
    _same(_state(b), _state(a), "prepare at it = 2")


# finalize grid: ceil((4 (P H + 4 H) rounded up to 64 + 64 B P) / 256) body workgroups + the bookkeeping one
#   N = 100, P = 8, H = 32, T = 4: 4 * 384 = 1536 | 64 * 24 = 1536 -> 12 body workgroups exactly, the 13th is the book
#   N = 33, P = 10, H = 64, T = 3: 4 * 896 = 3584 | 64 * 20 = 1280 -> 19 body workgroups exactly
#   N = 33, P = 5, H = 24, T = 3: 4 * 216 = 864 -> 896 | 64 * 10 = 640 -> 1536 / 256 = 6; weight quads end inside a wave
UNEVEN = [(100, 8, 32, 4), (33, 10, 64, 3), (33, 5, 24, 3)]


@pytest.mark.parametrize("N,P,H,T", UNEVEN)
def test_uneven_shapes_eager_graph_and_batch(dev, N, P, H, T):
    from reart_amd.relax import RelaxBatch

    ds = [_data(N, T, 100 + k) for k in range(3)]
    solo = []
    for k, d in enumerate(ds):
        e = _engine(dev, d, P, H, seed=k)
        e.step(3)
        solo.append(_state(e))
        assert int(solo[-1][7][0]) == 3 and all(np.isfinite(x).all() for x in solo[-1])
    g = _engine(dev, ds[0], P, H, seed=0)
    _graph_of(g, 3)
    g.step(3)
    assert (g.graph_replays, g.eager_steps) == (1, 0)
    _same(_state(g), solo[0], "graph of 3")
    engines = [_engine(dev, d, P, H, seed=k) for k, d in enumerate(ds)]
    RelaxBatch(engines).step(3)
    for k, e in enumerate(engines):
        _same(_state(e), solo[k], f"batch instance {k}")


def test_long_model_path(dev):
    """pose_len 59 at 20 parts is the first the in-LDS backward does not take (tests/test_long_sequence_gpu.py: _BWD_LAST);
    N = 33: two 32-point workgroups, the second with one point.  The long block kernel promotes the step sizes too."""
    from reart_amd import _lib

    P, B, N = 20, 59, 33
    assert _lib.lib().reart_base_path(P, B, 128, 1) == 1
    d = _data(N, B + 1, 21)
    a = _engine(dev, d, P, cano_idx=30)
    _check_scalars(a, 2)
    b = _engine(dev, d, P, cano_idx=30)
    _graph_of(b, 2)
    b.step(2)
    assert (b.graph_replays, b.eager_steps) == (1, 0)
    _same(_state(b), _state(a), "long path, graph of 2")


def test_assignment_loss_step_without_a_search_launch(dev):
    """Assignment loss and no flow loss: the iteration has no search launch (forward, consumers, backward, finalize)."""
    N, T = 100, 4
    d = _data(N, T, 31, flow=False)
    rng = np.random.default_rng(32)
    src = rng.permutation(N)[:60]
    tgt = np.stack([rng.permutation(N)[:60] for _ in range(T - 1)])
    runs = []
    for mode in ("eager", "graph"):
        e = _engine(dev, d, 8)
        e.set_assignment(torch.from_numpy(src), torch.from_numpy(tgt), 0.3)
        assert e.cfg.use_assign == 1 and e.cfg.use_flow == 0
        if mode == "eager":
            _check_scalars(e, 2)
        else:
            _graph_of(e, 2)
            e.step(2)
            assert (e.graph_replays, e.eager_steps) == (1, 0)
        runs.append(_state(e))
        assert runs[-1][5][:, 0].min() > 0 and (runs[-1][5][:, 1] == 0).all()      # an assignment loss, no flow loss
    _same(runs[1], runs[0], "assignment step, graph of 2")
