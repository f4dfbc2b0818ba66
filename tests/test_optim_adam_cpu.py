"""CPU-side checks of reart_amd.optim.Adam: the yardstick of the GPU tests (tests/adam_ref.py) against torch.optim.Adam in
float64, the criterion against planted errors, the deferral to torch on host tensors, the --fused_adam flag, and the C ABI of
reart_adam_groups (limit, refusals before any device work)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import adam_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG = 0, -1


@pytest.mark.parametrize("amsgrad,wd,maximize", ar.GRID)
def test_restatement_equals_torch_in_float64(amsgrad, wd, maximize):
    case = ar.case(amsgrad, wd, maximize)
    want, _, _ = ar.run_torch(lambda g: torch.optim.Adam(g, foreach=False), *case, dtype=torch.float64)
    got, _ = ar.adam_ref(*case)
    d = ar.deviation(got, want)
    print(f"amsgrad {amsgrad} wd {wd} maximize {maximize}: restatement - torch float64 {d:.3e}")
    assert d <= 1e-14


def test_restatement_with_a_late_first_gradient_equals_torch_in_float64():
    """One tensor never has a gradient, one gets its first at the third step: own step counts, state created at first use."""
    params, groups, group_of, grads = ar.case(True, 1e-2, False)
    for t, step_grads in enumerate(grads):
        step_grads[1] = None
        if t < 2:
            step_grads[4] = None
    want, opt, tensors = ar.run_torch(lambda g: torch.optim.Adam(g, foreach=False), params, groups, group_of, grads, dtype=torch.float64)
    got, state = ar.adam_ref(params, groups, group_of, grads)
    assert ar.deviation(got, want) <= 1e-14
    assert 1 not in state and state[4]["step"] == ar.STEPS - 2 and state[0]["step"] == ar.STEPS
    assert tensors[1] not in opt.state and float(opt.state[tensors[4]]["step"]) == ar.STEPS - 2


def _cpu_deviations(case):
    ref, _ = ar.adam_ref(*case)
    torch32, _, _ = ar.run_torch(lambda g: torch.optim.Adam(g, foreach=False), *case)
    return ref, ar.deviation(torch32, ref)


@pytest.mark.parametrize("amsgrad,wd,maximize", ar.GRID)
def test_criterion_passes_the_float32_restatement(amsgrad, wd, maximize):
    case = ar.case(amsgrad, wd, maximize)
    ref, d_torch = _cpu_deviations(case)
    d_f32 = ar.deviation(ar.adam_ref(*case, dtype=np.float32)[0], ref)
    print(f"amsgrad {amsgrad} wd {wd} maximize {maximize}: D_float32 {d_f32:.3e} D_torch {d_torch:.3e}")
    assert 0 < d_torch < 1e-6
    assert ar.criterion(d_f32, d_torch)


@pytest.mark.parametrize("mutate", ar.MUTATIONS)
def test_criterion_rejects_a_planted_error(mutate):
    """amsgrad, weight decay and maximize all on, so that every mutant has something to get wrong."""
    case = ar.case(True, 1e-2, True)
    ref, d_torch = _cpu_deviations(case)
    d_bad = ar.deviation(ar.adam_ref(*case, dtype=np.float32, mutate=mutate)[0], ref)
    print(f"{mutate}: D {d_bad:.3e} against D_torch {d_torch:.3e} ({d_bad / d_torch:.0f} x)")
    assert not ar.criterion(d_bad, d_torch)
    assert d_bad >= 50 * d_torch


@pytest.mark.parametrize("amsgrad,wd,maximize", [(False, 0.0, False), (True, 1e-2, True)])
def test_host_tensors_take_torchs_step(amsgrad, wd, maximize):
    from reart_amd.optim import Adam

    case = ar.case(amsgrad, wd, maximize)
    want, opt_t, tens_t = ar.run_torch(lambda g: torch.optim.Adam(g), *case)
    got, opt, tens = ar.run_torch(lambda g: Adam(g), *case)
    assert opt.last_path == "torch" and opt.last_launches == 0
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    for a, b in zip(tens, tens_t):
        assert opt.state[a].keys() == opt_t.state[b].keys()
        for k in opt.state[a]:
            assert torch.equal(opt.state[a][k], opt_t.state[b][k]), k
    sd, sd_t = opt.state_dict(), opt_t.state_dict()
    assert sd["param_groups"] == sd_t["param_groups"] and sd["state"].keys() == sd_t["state"].keys()


def test_closure_and_hooks_run_once_on_the_torch_path():
    from reart_amd.optim import Adam

    torch.optim.Adam([torch.zeros(1, requires_grad=True)])          # torch's own class has been instantiated: its step is hooked
    p = torch.ones(3, requires_grad=True)
    opt = Adam([p], lr=0.1)
    calls = []
    opt.register_step_post_hook(lambda *a: calls.append("post"))

    def closure():
        opt.zero_grad()
        loss = (p * p).sum()
        loss.backward()
        calls.append("closure")
        return loss

    loss = opt.step(closure)
    assert float(loss.detach()) == 3.0 and calls == ["closure", "post"] and opt.last_path == "torch"
    assert float(opt.state[p]["step"]) == 1.0


def test_parser_flag():
    from reart_amd.run_robot import build_parser

    assert build_parser().parse_args([]).fused_adam is False
    assert build_parser().parse_args(["--fused_adam"]).fused_adam is True


def test_limit_and_record_match_the_header():
    from reart_amd import _lib
    from reart_amd.optim import AdamTensor

    hdr = open(os.path.join(ROOT, "include", "reart_hip.h")).read()
    assert int(re.search(r"#define\s+REART_ADAM_MAX_TENSORS\s+(\d+)", hdr).group(1)) == _lib.ADAM_MAX_TENSORS == 32
    body = hdr[hdr.index("typedef struct reart_adam_tensor {"):hdr.index("} reart_adam_tensor;")]
    fields = []
    for typ, names in re.findall(r"\b((?:const )?float|int)\s+([a-zA-Z_0-9,\s\*]+);", body):
        for nm in names.split(","):
            fields.append((nm.strip().lstrip("*"), ctypes.c_void_p if "*" in nm else (ctypes.c_float if "float" in typ else ctypes.c_int)))
    assert fields == list(AdamTensor._fields_)
    assert ctypes.sizeof(AdamTensor) == 64
    assert _lib.PROTOTYPES["reart_adam_groups"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                                                    ctypes.c_double, ctypes.c_void_p])


def test_entry_refuses_before_any_device_work():
    from reart_amd import _lib
    from reart_amd.optim import AdamTensor

    fn = _lib.lib().reart_adam_groups
    d = 4096     # a non-null dummy address: these calls are refused, or launch nothing

    def call(count=1, table=True, betas=(0.9, 0.999), **over):
        recs = (AdamTensor * _lib.ADAM_MAX_TENSORS)()
        for r in recs:
            r.param = r.grad = r.exp_avg = r.exp_avg_sq = d
            r.n, r.step_size, r.bias_correction2_sqrt = 10, 1e-3, 0.5
        for k, v in over.items():
            setattr(recs[max(count, 1) - 1], k, v)          # the LAST record: every record is checked
        return fn(recs if table else None, count, betas[0], betas[1], 1e-8, None)

    assert call(count=0) == OK and call(count=0, table=False) == OK
    assert call(table=False) == INVALID_ARG
    assert call(count=-1) == INVALID_ARG and call(count=_lib.ADAM_MAX_TENSORS + 1) == INVALID_ARG
    for count in (1, 5, _lib.ADAM_MAX_TENSORS):
        assert call(count=count, n=-1) == INVALID_ARG
        for null in ("param", "grad", "exp_avg", "exp_avg_sq"):
            assert call(count=count, **{null: None}) == INVALID_ARG, null
        for bc in (0.0, -0.5, float("nan"), float("inf")):
            assert call(count=count, bias_correction2_sqrt=bc) == INVALID_ARG, bc
    # empty records are legal, with null pointers too, and a call of empty records launches nothing
    recs = (AdamTensor * 3)()
    for r in recs:
        r.bias_correction2_sqrt = 0.5
    assert fn(recs, 3, 0.9, 0.999, 1e-8, None) == OK
