"""Shared by tests/test_infonce_cpu.py and tests/test_infonce_gpu.py: a float64 restatement of the descriptor InfoNCE operator
(csrc/infonce.hip; networks.loss.DescriptorInfoNCE) on the float32 operands, the case table, and error bounds that hold for
ANY order of summation, derived from the number formats alone.

Operator.  s_ij = <f1_i, f2_j> / tau; a column is live unless col_mask says 0; a row is used when its pos lies in [0, N2) and
that column is live.  For used rows lse_i = log sum_live exp(s_ij), row_loss_i = lse_i - s_i,pos(i), top_i = the lowest live
column attaining the maximum; unused rows 0, 0, -1.  count = used rows of the batch, loss = sum(row_loss) / count (0 when
count = 0).  p_ij = exp(s_ij - lse_i) on live columns of used rows, p' = p - [j = pos(i)],
dF1_i = g / (count tau) sum_j p'_ij f2_j, dF2_j = g / (count tau) sum_i p'_ij f1_i.

Bounds (u = 2^-24, the unit round-off of float32; |x| of a descriptor is its Euclidean norm):
  e_i    = (C + 2) 2u max_j |f1_i| |f2_j| / tau            a float32 logit: a C-term dot product in any order is within
           C u |f1_i| |f2_j| (Cauchy-Schwarz on sum |a_k| |b_k|), the scaling by 1 / tau costs at most 2 u more; twice that.
  lse    : e_i + (N2 + 8) u + 2u |lse_i|                   every term of the sum is off by at most e_i in the exponent, the
           sum of N2 positive terms by N2 u relative in any order, exp, rescaling and log by the 8 u, the result's rounding.
  eps_i  = e_i + (the lse bound) + 4 u                     relative error of p_ij = exp(s_ij - lse_i).
  row_loss: the lse bound + e_i.
  dF1_ic : [eps_i sum_j p_ij |f2_jc| + (N2 + 2) 2u sum_j |p'_ij| |f2_jc|] |g| / (count tau)
  dF2_jc : [sum_i eps_i p_ij |f1_ic| + (N1 + 2) 2u sum_i |p'_ij| |f1_ic|] |g| / (count tau)
  loss   : the mean of the used rows' bounds + one ulp of the loss.
  Underflow: the relative bound eps_i cannot hold for a p_ij below float32's smallest normal number 2^-126 (it is stored as a
  subnormal or as 0, as is a product p f of that size), so each of the N2 (N1) terms of a gradient entry carries an absolute
  2^-125 |f| |g| / (count tau) more: nothing next to any entry that is not itself of that size.
The 4 u of eps_i is the exponential's share: it assumes exp(a - b) within 4 u RELATIVE of the exact exponential of the two
float32 numbers a and b.  The kernel meets it by construction (nce_exp_diff in csrc/infonce.hip): the difference is formed
exactly in double and split into a float32 head and tail, e^(head + tail) = expf(head) (1 + tail); the device library's expf
is within 1 ulp = 2 u, the closing fmaf rounds once (1 u), tail^2 < u^2: 3 u.  A plain expf(a - b) would NOT meet it: the
rounded difference is off by u |a - b|, which the exponential turns into a relative error of u |a - b|, unbounded in the
logits' magnitude; the float32 numpy model below splits the difference the same way.
Unused rows, masked columns and a call without used rows are exact: 0, -1, 0.

`top` is compared only on rows whose two largest float64 logits (over live columns) differ by more than the sum of their
bounds, 2 e_i; at least 95 % of the used rows of every case qualify (the CPU test asserts it; the seeds are chosen for it)."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -125   # per gradient term: a probability and its product with a descriptor entry, each below the normal range
TILE = 32          # the kernel's streamed tile: the cases are built around its edges

# ---------------------------------------------------------------------------------------------------------------- cases
def _case(name, B, N1, N2, C, tau, seed, spread=2.0, **kw):
    """Descriptors N(0, a^2) with a chosen so that the logits have a standard deviation of `spread` (a soft row
    distribution: every column matters to lse), positives uniform over the columns."""
    rng = np.random.default_rng(seed)
    a = np.sqrt(spread * tau / np.sqrt(C))
    f1 = (rng.standard_normal((B, N1, C)) * a).astype(np.float32)
    f2 = (rng.standard_normal((B, N2, C)) * a).astype(np.float32)
    pos = rng.integers(0, N2, size=(B, N1)).astype(np.int64)
    c = dict(name=name, B=B, N1=N1, N2=N2, C=C, tau=tau, f1=f1, f2=f2, pos=pos, mask=None, rng=rng)
    c.update(kw)
    return c


def _build_cases():
    cases = []
    cases.append(_case("one", 1, 1, 1, 1, 1.0, 1))
    cases.append(_case("n31_m2_c3", 1, 31, 2, 3, 0.07, 2))
    c = _case("n32_m33_c63_unused", 3, 32, 33, 63, 1.0, 3)
    c["pos"][0, 5] = -1; c["pos"][1, 0] = 33; c["pos"][2, 31] = -7; c["pos"][1, 17] = 1 << 40
    cases.append(c)
    cases.append(_case("n33_m64_c64", 1, 33, 64, 64, 0.07, 4))
    c = _case("n127_m65_c65_empty_element", 3, 127, 65, 65, 0.07, 5)
    c["pos"][1, :] = -1                                  # a batch element with no used row
    cases.append(c)
    c = _case("n129_m257_c256_shared", 1, 129, 257, 256, 1.0, 6)
    c["pos"][0, 20:60] = 200                             # 40 rows share one positive
    cases.append(c)
    c = _case("n300_m1000_c64_masked", 3, 300, 1000, 64, 0.07, 7)
    m = np.ones((3, 1000), np.uint8)
    m[:, c["rng"].permutation(1000)[:333]] = 0           # a third of the columns, some positives among them
    m[2, :] = 0                                          # every column of one element
    c["mask"] = m
    cases.append(c)
    c = _case("no_used_row", 1, 33, 33, 3, 1.0, 8)
    c["pos"][:] = -1
    cases.append(c)
    c = _case("huge_logits", 1, 129, 257, 64, 0.07, 9, spread=3000.0)      # |s| reaches 10^4: exp(s) overflows float32
    c["pos"][0, 0] = 256
    cases.append(c)
    c = _case("max_in_last_tile", 1, 33, 65, 64, 0.07, 10)                 # column 64 alone in the last tile holds every maximum
    c["f1"][0, :, 0] = np.abs(c["f1"][0, :, 0]) + 0.2
    c["f2"][0, 64, :] = 0.0
    c["f2"][0, 64, 0] = 8.0
    cases.append(c)
    cases.append(_case("many_clouds_unsplit", 520, 5, 70, 3, 1.0, 11))     # enough row tiles that the columns are not split
    c = _case("n300_m257_c1_mask_bool", 1, 300, 257, 1, 1.0, 12)
    m = np.ones((1, 257), np.uint8)
    m[0, ::3] = 0
    c["mask"] = m
    cases.append(c)
    for c in cases:
        del c["rng"]
    return cases


CASES = _build_cases()
CASE_IDS = [c["name"] for c in CASES]


# ---------------------------------------------------------------------------------------------------------- restatement
def used_rows(c):
    B, N1, N2 = c["B"], c["N1"], c["N2"]
    live = np.ones((B, N2), bool) if c["mask"] is None else c["mask"].astype(bool)
    inr = (c["pos"] >= 0) & (c["pos"] < N2)
    col = np.where(inr, c["pos"], 0)
    used = inr & np.take_along_axis(live, col, 1)
    return live, used, col


def restate(c, g=1.0):
    """float64 on the float32 operands (tau as the float32 the entry point receives)."""
    f1, f2 = c["f1"].astype(np.float64), c["f2"].astype(np.float64)
    tau = float(np.float32(c["tau"]))
    live, used, col = used_rows(c)
    S = np.einsum("bic,bjc->bij", f1, f2) / tau
    with np.errstate(invalid="ignore", divide="ignore"):
        Sm = np.where(live[:, None, :], S, -np.inf)
        m = Sm.max(2)
        m0 = np.where(np.isfinite(m), m, 0.0)
        lse_all = m0 + np.log(np.exp(Sm - m0[..., None]).sum(2))
    lse = np.where(used, lse_all, 0.0)
    spos = np.take_along_axis(S, col[..., None], 2)[..., 0]
    row_loss = np.where(used, lse - spos, 0.0)
    top = np.where(used, Sm.argmax(2), -1).astype(np.int64)              # argmax: the first, i.e. lowest, maximum
    count = int(used.sum())
    loss = row_loss.sum() / count if count else 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        P = np.where(used[..., None] & live[:, None, :], np.exp(Sm - np.where(used, lse, 0.0)[..., None]), 0.0)
    Pp = P.copy()
    bb, ii = np.nonzero(used)
    Pp[bb, ii, col[bb, ii]] -= 1.0
    k = g / (count * tau) if count else 0.0
    dF1 = k * np.einsum("bij,bjc->bic", Pp, f2)
    dF2 = k * np.einsum("bij,bic->bjc", Pp, f1)
    return dict(loss=loss, row_loss=row_loss, lse=lse, top=top, count=count, dF1=dF1, dF2=dF2, S=Sm, P=P, Pp=Pp, used=used, live=live,
                tau=tau, g=g)


def bounds(c, r):
    """The header's bounds for the restatement `r` of case `c`: a dict of arrays shaped like the outputs, plus `top_ok`."""
    f1, f2 = c["f1"].astype(np.float64), c["f2"].astype(np.float64)
    N1, N2, C, tau, g, count = c["N1"], c["N2"], c["C"], r["tau"], abs(r["g"]), r["count"]
    used, live = r["used"], r["live"]
    n1, n2 = np.sqrt((f1 * f1).sum(2)), np.sqrt((f2 * f2).sum(2))
    n2max = np.where(live, n2, 0.0).max(1) if N2 else np.zeros(c["B"])
    e = (C + 2) * 2 * U * n1 * n2max[:, None] / tau
    lse_b = e + (N2 + 8) * U + 2 * U * np.abs(r["lse"])
    eps = e + lse_b + 4 * U
    row_b = lse_b + e
    k = g / (count * tau) if count else 0.0
    a1, a2 = np.abs(f1), np.abs(f2)
    dF1_b = k * (eps[..., None] * np.einsum("bij,bjc->bic", r["P"], a2) + (N2 + 2) * 2 * U * np.einsum("bij,bjc->bic", np.abs(r["Pp"]), a2)
                 + TINY * a2.sum(1)[:, None, :])
    dF2_b = k * (np.einsum("bij,bic->bjc", r["P"] * eps[..., None], a1) + (N1 + 2) * 2 * U * np.einsum("bij,bic->bjc", np.abs(r["Pp"]), a1)
                 + TINY * a1.sum(1)[:, None, :])
    zero = np.zeros_like(e)
    loss_b = (np.where(used, row_b, 0.0).sum() / count + 2 * U * abs(r["loss"])) if count else 0.0
    # top: the two largest logits apart by more than their two bounds together
    if N2 >= 2:
        two = np.sort(r["S"], axis=2)[:, :, -2:]
        with np.errstate(invalid="ignore"):
            gap = two[..., 1] - two[..., 0]
        top_ok = used & ~(gap <= 2 * e)                                  # -inf second (one live column): qualifies
    else:
        top_ok = used.copy()
    return dict(loss=loss_b, row_loss=np.where(used, row_b, zero), lse=np.where(used, lse_b, zero), dF1=dF1_b, dF2=dF2_b, top_ok=top_ok)


def top_share(c, r, b):
    n = int(r["used"].sum())
    return 1.0 if n == 0 else float(b["top_ok"].sum()) / n


def worst(out, r, b, keys=("loss", "row_loss", "lse", "dF1", "dF2")):
    """Largest |out - restatement| / bound per output present in `out` (0 where both error and bound are 0, inf where only the
    bound is), plus `top`: mismatches on qualifying rows + wrong entries on unused rows, and `count`: |difference|."""
    w = {}
    for key in keys:
        if out.get(key) is None:
            continue
        err = np.abs(np.asarray(out[key], np.float64) - r[key])
        bd = np.broadcast_to(np.asarray(b[key], np.float64), err.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0.0, 0.0, np.where(bd > 0.0, err / bd, np.inf))
        q = np.where(np.isnan(q), np.inf, q)
        w[key] = float(q.max()) if q.size else 0.0
    if out.get("top") is not None:
        t = np.asarray(out["top"])
        w["top"] = int((t[b["top_ok"]] != r["top"][b["top_ok"]]).sum() + (t[~r["used"]] != -1).sum())
    if out.get("count") is not None:
        w["count"] = abs(int(out["count"]) - r["count"])
    return w


def inside(w):
    return all(v <= 1.0 for k, v in w.items() if k not in ("top", "count")) and w.get("top", 0) == 0 and w.get("count", 0) == 0


# ------------------------------------------------------------------------------------- a float32 model, and planted errors
def _exp_diff32(a, b):
    """exp(a - b) for float32 arrays as the kernel takes it: exact difference, float32 head and tail."""
    d = a.astype(np.float64) - b.astype(np.float64)
    hi = d.astype(np.float32)
    lo = (d - hi.astype(np.float64)).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(hi)
        return (e + e * lo).astype(np.float32)


PLANTS = ("no_rescale", "drop_last_tile", "no_delta_dF2", "div_N1")


def model32(c, g=1.0, tile=TILE, reverse=False, plant=None):
    """An honest float32 implementation (online maximum over column tiles of `tile`, ascending or descending), or one with a
    planted error."""
    f1, f2, pos = c["f1"], c["f2"], c["pos"]
    B, N1, N2 = c["B"], c["N1"], c["N2"]
    tau = np.float32(c["tau"])
    inv = np.float32(1.0) / tau
    live, used, col = used_rows(c)
    S = (np.einsum("bic,bjc->bij", f1, f2).astype(np.float32) * inv).astype(np.float32)
    m = np.full((B, N1), -np.inf, np.float32)
    s = np.zeros((B, N1), np.float32)
    arg = np.full((B, N1), -1, np.int64)
    spos = np.zeros((B, N1), np.float32)
    starts = list(range(0, N2, tile))
    if plant == "drop_last_tile" and N2 % tile:
        starts = starts[:-1]
    if reverse:
        starts = starts[::-1]
    for j0 in starts:
        j1 = min(N2, j0 + tile)
        lv = live[:, None, j0:j1]
        with np.errstate(invalid="ignore"):
            T = np.where(lv, S[:, :, j0:j1], np.float32(-np.inf))
            tm, ta = T.max(2), T.argmax(2) + j0
            has = lv.any(2) & np.ones((B, N1), bool)
            better = has & ((tm > m) | (arg < 0) | ((tm == m) & (ta < arg)))
            mn = np.where(has & (tm > m), tm, m)
            if plant != "no_rescale":
                s = np.where(np.isfinite(m) & (mn > m), s * _exp_diff32(m, mn), s)
            m = mn
            arg = np.where(better, ta, arg)
            mm = np.where(np.isfinite(m), m, np.float32(0))
            s = s + np.where(lv, _exp_diff32(T, np.broadcast_to(mm[..., None], T.shape)), np.float32(0)).sum(2, dtype=np.float32)
        hit = (col >= j0) & (col < j1)
        spos = np.where(hit, np.take_along_axis(S, col[..., None], 2)[..., 0], spos)
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = np.where(used, (m.astype(np.float64) + np.log(s.astype(np.float64))), 0.0).astype(np.float32)
        row_loss = np.where(used, m.astype(np.float64) + np.log(s.astype(np.float64)) - spos, 0.0).astype(np.float32)
    top = np.where(used, arg, -1)
    count = int(used.sum())
    denom = B * N1 if plant == "div_N1" else count
    loss = np.float32(row_loss.astype(np.float64).sum() / denom) if count else np.float32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        P = np.where(used[..., None] & live[:, None, :], _exp_diff32(S, np.broadcast_to(lse[..., None], S.shape)), np.float32(0))
    P1 = P.copy()
    bb, ii = np.nonzero(used)
    P1[bb, ii, col[bb, ii]] -= np.float32(1)
    P2 = P if plant == "no_delta_dF2" else P1
    k = np.float32(g / (float(denom) * float(tau))) if count else np.float32(0)
    dF1 = (np.einsum("bij,bjc->bic", P1, f2).astype(np.float32) * k).astype(np.float32)
    dF2 = (np.einsum("bij,bic->bjc", P2, f1).astype(np.float32) * k).astype(np.float32)
    return dict(loss=loss, row_loss=row_loss, lse=lse, top=top, count=count, dF1=dF1, dF2=dF2)


def touches(c, plant):
    """Whether a planted error can change an output of this case at all."""
    _, used, col = used_rows(c)
    count, N2 = int(used.sum()), c["N2"]
    if count == 0:
        return False
    if plant == "no_rescale":
        return N2 > TILE
    if plant == "drop_last_tile":
        return N2 % TILE != 0
    if plant == "div_N1":
        return count != c["B"] * c["N1"]
    return True
