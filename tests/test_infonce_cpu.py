"""The yardstick of the descriptor InfoNCE tests, checked without a GPU (tests/infonce_ref.py): the float64 restatement
against torch's float64 autograd of the cross-entropy composition, the derived bounds against an honest float32 model (they
must hold) and against four planted errors (they must not), the share of rows on which `top` is compared, and the host-tensor
error of correspondence_targets."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import infonce_ref as nr


@pytest.fixture(scope="module")
def restated():
    out = {}
    for c in nr.CASES:
        r = nr.restate(c, g=1.0)
        out[c["name"]] = (r, nr.bounds(c, r))
    return out


@pytest.mark.parametrize("c", nr.CASES, ids=nr.CASE_IDS)
def test_restatement_equals_torch_float64_autograd(c, restated):
    r, _ = restated[c["name"]]
    f1 = torch.from_numpy(c["f1"]).double().requires_grad_(True)
    f2 = torch.from_numpy(c["f2"]).double().requires_grad_(True)
    live, used, col = nr.used_rows(c)
    keep = torch.from_numpy(used[..., None] & live[:, None, :])
    logits = torch.bmm(f1, f2.transpose(1, 2)) / r["tau"]
    logits = torch.where(keep, logits, torch.full_like(logits, -np.inf))
    logits = torch.where(torch.from_numpy(used)[..., None], logits, torch.zeros_like(logits))     # ignored rows: any finite row
    target = torch.from_numpy(np.where(used, col, -100))
    total = F.cross_entropy(logits.reshape(-1, c["N2"]), target.reshape(-1), ignore_index=-100, reduction="sum")
    count = int(used.sum())
    loss = total / count if count else total * 0.0
    loss.backward()

    def close(a, b):
        b = np.asarray(b, np.float64)
        scale = max(1.0, float(np.abs(b).max()) if b.size else 1.0)
        np.testing.assert_allclose(np.asarray(a, np.float64), b, rtol=1e-12, atol=1e-12 * scale)

    close(r["loss"], loss.item())
    close(r["dF1"], f1.grad.numpy())
    close(r["dF2"], f2.grad.numpy())
    per_row = F.cross_entropy(logits.detach().reshape(-1, c["N2"]), target.reshape(-1), ignore_index=-100, reduction="none")
    close(r["row_loss"], per_row.reshape(c["B"], c["N1"]).numpy())
    lse = torch.logsumexp(logits.detach(), 2).numpy()
    close(r["lse"], np.where(used, lse, 0.0))
    assert r["count"] == count
    assert (r["top"][used] == logits.detach().argmax(2).numpy()[used]).all() and (r["top"][~used] == -1).all()


@pytest.mark.parametrize("order", [dict(tile=32, reverse=False), dict(tile=7, reverse=True), dict(tile=100000, reverse=False)],
                         ids=["tile32", "tile7_descending", "one_tile"])
@pytest.mark.parametrize("c", nr.CASES, ids=nr.CASE_IDS)
def test_honest_float32_model_is_inside_every_bound(c, order, restated):
    r, b = restated[c["name"]]
    w = nr.worst(nr.model32(c, g=1.0, **order), r, b)
    assert nr.inside(w), w


@pytest.mark.parametrize("plant", nr.PLANTS)
def test_planted_errors_leave_the_bounds(plant, restated):
    touched = 0
    for c in nr.CASES:
        if not nr.touches(c, plant):
            continue
        touched += 1
        r, b = restated[c["name"]]
        w = nr.worst(nr.model32(c, g=1.0, plant=plant), r, b)
        assert not nr.inside(w), (c["name"], plant, w)
    assert touched >= 3


@pytest.mark.parametrize("c", nr.CASES, ids=nr.CASE_IDS)
def test_top_is_compared_on_95_percent_of_the_used_rows(c, restated):
    r, b = restated[c["name"]]
    assert nr.top_share(c, r, b) >= 0.95


def test_upstream_scale_enters_restatement_and_bounds_linearly():
    c = nr.CASES[3]
    r1, r3 = nr.restate(c, g=1.0), nr.restate(c, g=-2.5)
    np.testing.assert_allclose(r3["dF1"], -2.5 * r1["dF1"], rtol=1e-14)
    np.testing.assert_allclose(nr.bounds(c, r3)["dF2"], 2.5 * nr.bounds(c, r1)["dF2"], rtol=1e-14)


def test_case_table_covers_the_edges():
    got = {k: {c[k] for c in nr.CASES} for k in ("N1", "N2", "C", "B", "tau")}
    assert {1, 31, 32, 33, 127, 129, 300} <= got["N1"]
    assert {1, 2, 33, 64, 65, 257, 1000} <= got["N2"]
    assert {1, 3, 63, 64, 65, 256} <= got["C"]
    assert {1, 3} <= got["B"] and {1.0, 0.07} <= got["tau"]
    assert any((c["pos"] == -1).any() and (c["pos"] == c["N2"]).any() for c in nr.CASES)
    assert any(nr.restate(c)["count"] == 0 for c in nr.CASES)
    assert any(np.abs(nr.restate(c)["S"][np.isfinite(nr.restate(c)["S"])]).max() > 8e3 for c in nr.CASES if c["name"] == "huge_logits")
    c = next(c for c in nr.CASES if c["name"] == "max_in_last_tile")
    assert (nr.restate(c)["top"] == c["N2"] - 1).all() and (c["N2"] - 1) % nr.TILE == 0


def test_correspondence_targets_refuses_host_tensors():
    from reart_amd.utils.flow_utils import correspondence_targets

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        correspondence_targets(torch.zeros(1, 4, 3), torch.zeros(1, 5, 3), 0.1)
    with pytest.raises(ValueError):
        correspondence_targets(torch.zeros(1, 4, 3), torch.zeros(2, 5, 3), 0.1)


def test_class_validates_before_anything_is_launched():
    from reart_amd.networks.loss import DescriptorInfoNCE

    f1, f2, pos = torch.zeros(1, 4, 8), torch.zeros(1, 5, 8), torch.zeros(1, 4, dtype=torch.int64)
    with pytest.raises(ValueError):
        DescriptorInfoNCE(tau=0.0)
    op = DescriptorInfoNCE()
    with pytest.raises(TypeError):
        op(f1.double(), f2, pos)
    with pytest.raises(TypeError):
        op(f1, f2, pos.int())
    with pytest.raises(TypeError):
        op(f1, f2, pos, torch.zeros(1, 5))
    with pytest.raises(ValueError):
        op(f1, f2[:, :, :7], pos)
    with pytest.raises(ValueError):
        op(f1, f2, pos[:, :3])
    with pytest.raises(ValueError):
        op(f1, f2, pos, torch.zeros(1, 4, dtype=torch.bool))
    with pytest.raises(NotImplementedError):
        op(torch.zeros(1, 2, 257), torch.zeros(1, 2, 257), torch.zeros(1, 2, dtype=torch.int64))
    with pytest.raises(NotImplementedError):
        op(torch.zeros(1, 65537, 1), torch.zeros(1, 2, 1), torch.zeros(1, 65537, dtype=torch.int64))
    with pytest.raises(NotImplementedError):
        op(torch.zeros(1025, 1, 1), torch.zeros(1025, 1, 1), torch.zeros(1025, 1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op(f1, f2, pos)
