"""Cases and references for the front end over its documented range (no GPU code is imported here): the PointNet++ layer
kernel ``reart_mlp_layer`` (csrc/gemm.hip), ball query and 3-NN interpolation (csrc/pointnet.hip, csrc/gemm.hip) and the
descriptor matching ``reart_match_smnn`` (csrc/smnn.hip).

Layer cases are held to a float64 evaluation of relu(X W + b) and the group maximum, on the float32 operands the kernel
multiplies, with a bound that is derived and not measured:

    |kernel - f64|  <=  (Cin + 2) * 2^-23 * (|X| |W| + |b|)        per element, evaluated in float64.

A float32 sum of Cin products plus the bias is Cin multiplications and Cin additions; with a relative error of at most
u per operation its result is within ((1 + u)^(Cin + 1) - 1) (|X| |W| + |b|) of the exact one in ANY order of summation
(Higham, Accuracy and Stability of Numerical Algorithms, 3.1).  u = 2^-24 for round-to-nearest and below 2^-23 for a matrix
unit that truncates, and (1 + 2^-23)^(Cin + 1) - 1 < (Cin + 2) 2^-23 for every Cin of interest (Cin < 2^20).  ReLU and the
maximum are exact and 1-Lipschitz: a pooled output takes the largest bound of its group.

The other three tables are compared element for element: ball query and 3-NN with the oracle's restatements (their
arithmetic is part of the contract), the matching with float64 direct differences on inputs that are admitted only if no
decision is within 1e-5 of its threshold.
"""
import functools
import math
from collections import namedtuple

import numpy as np

EPS = 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------------
# reart_mlp_layer
# ---------------------------------------------------------------------------------------------------------------------
def pick(Cin, Cout, pool_k):
    """The instantiation mlp_gemm_kernel<NB, BK, ANY> that ``reart_mlp_layer`` launches, restated from its launcher."""
    NB = 1 if Cout <= 32 else 2 if Cout <= 64 else 3 if Cout <= 96 else 7 if 192 < Cout <= 224 else 2
    BK = 8 if Cin <= 8 else 16
    return NB, BK, pool_k not in (0, 1, 32, 64, 128)


TRIPLES = [(nb, bk, any_) for nb in (1, 2, 3, 7) for bk in (8, 16) for any_ in (False, True)]

# form: "plain" (contiguous X), "strided" (ldx > Cin at a base offset of `off` floats), "gather_fx" ([F | xyz - centre]),
# "gather_xf" ([xyz | F]); opt: the form's own parameters
LayerCase = namedtuple("LayerCase", "rows Cin Cout pool_k relu form opt")


def _plain(rows, Cin, Cout, pool_k=0, relu=True):
    return LayerCase(rows, Cin, Cout, pool_k, relu, "plain", {})


def _strided(rows, Cin, Cout, off, ldx, pool_k=0, relu=True, bias=True):
    return LayerCase(rows, Cin, Cout, pool_k, relu, "strided", dict(off=off, ldx=ldx, bias=bias))


def _gather(form, D, K, B, S, Npts, Cout, centres, relu=True):
    return LayerCase(B * S * K, D + 3, Cout, K, relu, form, dict(D=D, B=B, S=S, Npts=Npts, centres=centres))


LAYER_CASES = [
    # un-pooled, plain: rows 1, 127, 128, 129, 300 x every Cin and Cout of interest x all eight (NB, BK)
    _plain(1, 1, 1), _plain(127, 3, 32), _plain(128, 8, 33), _plain(129, 9, 64), _plain(300, 16, 65), _plain(300, 17, 96),
    _plain(129, 131, 100), _plain(127, 8, 193), _plain(300, 17, 224), _plain(129, 9, 225), _plain(128, 3, 256),
    _plain(300, 6, 65), _plain(129, 16, 1, pool_k=1),
    # pooled inside the waves' rows (32, 64, 128)
    _plain(96, 17, 20, 32, relu=False), _plain(256, 5, 100, 64), _plain(384, 131, 193, 128),
    # ANY = true, NB = 1: whole groups inside a tile (24, 2), one group above 128 rows with a short last chunk (130, 200)
    _plain(264, 6, 32, 24, relu=False), _plain(130, 17, 1, 2), _plain(260, 3, 20, 130), _plain(400, 16, 32, 200),
    # NB = 2
    _plain(300, 8, 64, 100), _plain(264, 9, 225, 24), _plain(2000, 1, 33, 1000, relu=False), _plain(768, 131, 100, 384),
    _plain(260, 17, 256, 130), _plain(256, 8, 33, 2),
    # NB = 3
    _plain(200, 3, 65, 100), _plain(258, 16, 96, 2), _plain(400, 8, 96, 200, relu=False), _plain(1000, 17, 65, 1000),
    # NB = 7
    _plain(48, 8, 193, 24), _plain(300, 9, 224, 100), _plain(130, 6, 224, 130), _plain(600, 131, 193, 200),
    _plain(384, 16, 224, 384), _plain(260, 131, 224, 2, relu=False),
    # ldx > Cin, odd (aligned and unaligned rows alternate), at base offsets of 0, 1, 2, 3 floats; bias = NULL
    _strided(129, 16, 33, 0, 19, bias=False), _strided(130, 17, 65, 1, 21), _strided(128, 8, 32, 2, 9, pool_k=32),
    _strided(200, 5, 100, 3, 7, pool_k=100, bias=False), _strided(127, 16, 96, 0, 20),
    _strided(260, 131, 224, 1, 133, pool_k=130, relu=False, bias=False), _strided(300, 9, 256, 2, 11, bias=False),
    # gathered [F | xyz - centre]: D = 0, 1, 4, 5, 12, 131 (12: a thread's 8-element run straddles the F / xyz boundary)
    _gather("gather_fx", 0, 32, 2, 3, 20, 32, True), _gather("gather_fx", 1, 24, 2, 7, 33, 64, False),
    _gather("gather_fx", 4, 64, 2, 3, 50, 96, True), _gather("gather_fx", 5, 16, 3, 9, 41, 193, True),
    _gather("gather_fx", 12, 128, 1, 3, 77, 100, True), _gather("gather_fx", 12, 130, 2, 2, 90, 65, False),
    _gather("gather_fx", 131, 32, 2, 5, 60, 225, True),
    # gathered [xyz | F] (sample_and_group_all's order), centres present and NULL
    _gather("gather_xf", 0, 200, 3, 1, 200, 32, False), _gather("gather_xf", 1, 32, 2, 5, 40, 33, True),
    _gather("gather_xf", 4, 100, 2, 2, 64, 224, False), _gather("gather_xf", 5, 64, 1, 3, 30, 1, True),
    _gather("gather_xf", 12, 2, 2, 65, 50, 96, False), _gather("gather_xf", 131, 1000, 2, 1, 1000, 256, False),
    _gather("gather_xf", 131, 128, 1, 2, 99, 64, True),
]


@functools.lru_cache(maxsize=None)
def layer_data(i):
    """The inputs of case i (float32, fixed by i) and ``Xop``: the [rows, Cin] float32 operand the kernel multiplies -- for
    a gathered case the features and xyz - centre, subtracted in float32 here as the kernel subtracts it."""
    c = LAYER_CASES[i]
    rng = np.random.default_rng(1000 + i)
    d = {}
    # asymmetric weights: a transposed fragment layout cannot pass
    d["W"] = (rng.normal(size=(c.Cin, c.Cout)) + np.arange(c.Cout)[None, :] * 0.01).astype(np.float32)
    b = rng.normal(size=c.Cout).astype(np.float32)
    if not c.relu and c.pool_k > 1:
        b[::2] -= np.float32(6.0 * math.sqrt(c.Cin) + 6.0)       # every other column: the group maxima are negative
    d["b"] = b if c.opt.get("bias", True) else None
    if c.form == "plain":
        d["X"] = rng.normal(size=(c.rows, c.Cin)).astype(np.float32)
        d["Xop"] = d["X"]
    elif c.form == "strided":
        off, ldx = c.opt["off"], c.opt["ldx"]
        d["buf"] = rng.normal(size=off + c.rows * ldx).astype(np.float32)
        d["Xop"] = np.ascontiguousarray(d["buf"][off:].reshape(c.rows, ldx)[:, :c.Cin])
    else:
        D, B, S, Npts, K = c.opt["D"], c.opt["B"], c.opt["S"], c.opt["Npts"], c.pool_k
        d["F"] = rng.normal(size=(B * Npts, D)).astype(np.float32) if D else None
        d["Q"] = rng.normal(size=(B * Npts, 3)).astype(np.float32)
        d["C"] = rng.normal(size=(B * S, 3)).astype(np.float32) if c.opt["centres"] else None
        d["idx"] = rng.integers(0, Npts, (B, S, K)).astype(np.int64)
        bb = np.arange(B)[:, None, None]
        q = d["Q"].reshape(B, Npts, 3)[bb, d["idx"]]
        if d["C"] is not None:
            q = q - d["C"].reshape(B, S, 1, 3)                    # float32 - float32: the kernel's operand
        parts = [q]
        if D:
            f = d["F"].reshape(B, Npts, D)[bb, d["idx"]]
            parts = [f, q] if c.form == "gather_fx" else [q, f]
        d["Xop"] = np.ascontiguousarray(np.concatenate(parts, axis=-1).reshape(c.rows, c.Cin).astype(np.float32))
    return d


def out_rows(c):
    return c.rows // c.pool_k if c.pool_k > 1 else c.rows


@functools.lru_cache(maxsize=None)
def layer_ref(i):
    """(float64 result, per-element bound) of case i; see the module docstring for the bound."""
    c, d = LAYER_CASES[i], layer_data(i)
    X, W = d["Xop"].astype(np.float64), d["W"].astype(np.float64)
    b = np.zeros(c.Cout) if d["b"] is None else d["b"].astype(np.float64)
    y = X @ W + b
    bound = (c.Cin + 2) * EPS * (np.abs(X) @ np.abs(W) + np.abs(b))
    if c.relu:
        y = np.maximum(y, 0.0)
    if c.pool_k > 1:
        y = y.reshape(-1, c.pool_k, c.Cout).max(axis=1)
        bound = bound.reshape(-1, c.pool_k, c.Cout).max(axis=1)
    y.setflags(write=False)
    bound.setflags(write=False)
    return y, bound


FAULTS = ("bias32", "drop_k", "live128")


def layer_emulate(i, fault=None):
    """The layer in float32 numpy, honest (fault = None) or with one planted error of the kind a kernel could make:
    ``bias32``: accumulators n >= 1 of a column block take the bias of column - 32; ``drop_k``: the last k is dropped when
    Cin is no multiple of the K step; ``live128``: the running maximum of a group above 128 rows takes all 128 rows of
    its short last chunk (the next group's rows, or relu(b) beyond the last row, where the kernel's tile holds zeros)."""
    c, d = LAYER_CASES[i], layer_data(i)
    NB, BK, ANY = pick(c.Cin, c.Cout, c.pool_k)
    X, W = d["Xop"], d["W"]
    b = np.zeros(c.Cout, np.float32) if d["b"] is None else d["b"]
    if fault == "drop_k" and c.Cin % BK:
        X, W = X[:, :-1], W[:-1]
    if fault == "bias32":
        col = np.arange(c.Cout)
        b = np.where((col % (32 * NB)) >= 32, b[np.maximum(col - 32, 0)], b)
    y = (np.matmul(X, W, dtype=np.float32) if X.shape[1] else np.zeros((c.rows, c.Cout), np.float32)) + b[None, :]
    act = (lambda v: np.maximum(v, np.float32(0))) if c.relu else (lambda v: v)
    y = act(y)
    if c.pool_k > 1:
        if fault == "live128" and ANY and c.pool_k > 128:
            span = -(-c.pool_k // 128) * 128
            ypad = np.concatenate([y, np.tile(act(b)[None, :], (128, 1))])
            y = np.stack([ypad[g * c.pool_k:g * c.pool_k + span].max(axis=0) for g in range(c.rows // c.pool_k)])
        else:
            y = y.reshape(-1, c.pool_k, c.Cout).max(axis=1)
    return y.astype(np.float32)


def layer_ratio(i, got):
    """max |got - f64| / bound over the elements of case i (inf where the bound is zero and the result is not exact)."""
    ref, bound = layer_ref(i)
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


# ---------------------------------------------------------------------------------------------------------------------
# ball query
# ---------------------------------------------------------------------------------------------------------------------
BallCase = namedtuple("BallCase", "N nsample S")
BALL_B, BALL_RADIUS, BALL_MARGIN = 3, 0.5, 1e-3
BALL_CASES = [BallCase(*t_) for t_ in (
    (1, 1, 1), (1, 2, 3), (63, 2, 5), (63, 64, 3), (64, 1, 130), (64, 64, 1), (64, 65, 5), (65, 64, 3), (65, 200, 1),
    (129, 2, 5), (129, 65, 130), (129, 200, 3), (700, 64, 5), (700, 65, 3), (700, 200, 130), (700, 1, 1))]


def ball_step_index(nsample):
    """The point index at which ``nsample`` hits are complete exactly at the end of a 64-point step of the wave."""
    return 64 * -(-nsample // 64) - 1


@functools.lru_cache(maxsize=None)
def ball_data(i):
    """(xyz [B,N,3], centres [B,S,3]) of case i.  A cloud is a cluster A of min(nsample, N) points within 0.09 of the origin
    -- its nsample-th member at an index = 63 mod 64 where N allows it -- up to two points E near (0.7, 0, 0), and the rest on
    a jittered lattice of pitch 0.8 far away.  Centres cycle through: the origin (A alone: full exactly at a step), (0.3, 0, 0)
    (A and E: overflow), a far corner (empty), a lattice point (itself), the middle of two lattice points (those two).  Every
    squared distance is more than 15 % of r^2 = 0.25 away from r^2."""
    c = BALL_CASES[i]
    rng = np.random.default_rng(2000 + i)
    xyz = np.empty((BALL_B, c.N, 3), np.float32)
    ctr = np.empty((BALL_B, c.S, 3), np.float32)
    lattice = np.stack(np.meshgrid(*[np.arange(9)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.8 + 2.0
    for b in range(BALL_B):
        nA, t_ = min(c.nsample, c.N), ball_step_index(c.nsample)
        if t_ < c.N:
            a_idx = np.concatenate([np.sort(rng.choice(t_, nA - 1, replace=False)), [t_]]).astype(np.int64)
        else:
            a_idx = np.sort(rng.choice(c.N, nA, replace=False))
        rest = rng.permutation(np.setdiff1d(np.arange(c.N), a_idx))
        e_idx, bg_idx = rest[:2], rest[2:]
        xyz[b, a_idx] = rng.uniform(-0.05, 0.05, (len(a_idx), 3))
        xyz[b, e_idx] = np.array([0.7, 0.0, 0.0]) + rng.uniform(-0.05, 0.05, (len(e_idx), 3))
        cells = rng.permutation(len(lattice))[:len(bg_idx)]
        xyz[b, bg_idx] = lattice[cells] + rng.uniform(-0.01, 0.01, (len(bg_idx), 3))
        far = np.array([-5.0, -5.0, -5.0])
        for s in range(c.S):
            kind = (s + b) % 5
            if kind == 0:
                p = np.zeros(3)
            elif kind == 1:
                p = np.array([0.3, 0.0, 0.0])
            elif kind == 3 and len(bg_idx):
                p = xyz[b, bg_idx[s % len(bg_idx)]].astype(np.float64)
            elif kind == 4 and len(bg_idx):
                cell = lattice[cells[s % len(bg_idx)]]
                p = cell + np.array([0.4, 0.0, 0.0])              # between this cell and its +x neighbour (present or not)
            else:
                p = far
            ctr[b, s] = p
    xyz.setflags(write=False)
    ctr.setflags(write=False)
    return xyz, ctr


def ball_classes(i):
    """Per ball of case i, from float64 distances: (count, empty, overflow, exact_step) arrays [B,S]; exact_step: the
    nsample-th hit has an index = 63 mod 64, so the wave's early exit falls exactly on a step."""
    c = BALL_CASES[i]
    xyz, ctr = ball_data(i)
    d2 = ((ctr.astype(np.float64)[:, :, None, :] - xyz.astype(np.float64)[:, None, :, :]) ** 2).sum(-1)
    hit = d2 < BALL_RADIUS ** 2
    count = hit.sum(-1)
    exact = np.zeros(count.shape, bool)
    for b in range(hit.shape[0]):
        for s in range(hit.shape[1]):
            k = np.nonzero(hit[b, s])[0]
            exact[b, s] = len(k) >= c.nsample and k[c.nsample - 1] % 64 == 63
    rel = np.abs(d2 - BALL_RADIUS ** 2).min() / BALL_RADIUS ** 2
    return count, count == 0, count > c.nsample, exact, float(rel)


# ---------------------------------------------------------------------------------------------------------------------
# 3-NN interpolation
# ---------------------------------------------------------------------------------------------------------------------
TnnCase = namedtuple("TnnCase", "B N S2 D")
TNN_CASES = [TnnCase(*t_) for t_ in (
    (1, 1, 3, 1), (3, 255, 4, 256), (1, 256, 1023, 257), (3, 257, 1024, 1), (1, 255, 1025, 1), (1, 257, 2048, 256),
    (3, 1, 2049, 257), (1, 256, 2049, 1), (1, 257, 3, 257), (3, 256, 4, 1))]


@functools.lru_cache(maxsize=None)
def tnn_data(i):
    """(fine xyz1 [B,N,3], coarse xyz2 [B,S2,3], points2 [B,S2,D]): the smaller cloud is a subset of the larger (every such
    pair meets at a "zero" distance, which the expanded form leaves as +-1e-7 of noise), and one coarse point that is also
    a fine point is stored twice (two neighbours at the same distance: the lower index comes first)."""
    c = TNN_CASES[i]
    rng = np.random.default_rng(3000 + i)
    if c.N >= c.S2:
        fine = rng.uniform(-1, 1, (c.B, c.N, 3)).astype(np.float32)
        coarse = np.stack([fine[b, rng.permutation(c.N)[:c.S2]] for b in range(c.B)])
        coarse[:, c.S2 - 1] = coarse[:, 0]
    else:
        coarse = rng.uniform(-1, 1, (c.B, c.S2, 3)).astype(np.float32)
        fine = np.empty((c.B, c.N, 3), np.float32)
        for b in range(c.B):
            perm = rng.permutation(c.S2)
            coarse[b, perm[c.N]] = coarse[b, perm[0]]             # a copy of a point the fine cloud takes
            fine[b] = coarse[b, perm[:c.N]]
    pts = rng.normal(size=(c.B, c.S2, c.D)).astype(np.float32)
    for a in (fine, coarse, pts):
        a.setflags(write=False)
    return fine, coarse, pts


# ---------------------------------------------------------------------------------------------------------------------
# descriptor matching
# ---------------------------------------------------------------------------------------------------------------------
SmnnCase = namedtuple("SmnnCase", "N1 N2 E th")
SMNN_MARGIN = 1e-5
SMNN_CASES = [SmnnCase(n1, n2, E, th) for (n1, n2) in ((2, 2), (63, 65), (64, 64), (65, 130), (300, 77)) for E in (1, 3)
              for th in (0.9, 0.5, -1.0)]


def _smnn_draw(c, seed):
    rng = np.random.default_rng(seed)
    d1 = np.empty((c.E, c.N1, 64), np.float32)
    d2 = np.empty((c.E, c.N2, 64), np.float32)
    plants = []
    for e in range(c.E):
        M = max(c.N1, c.N2)
        base, perm = rng.normal(size=(M, 64)), rng.permutation(M)
        d1[e] = base[:c.N1] + 0.15 * rng.normal(size=(c.N1, 64))
        d2[e] = base[perm[:c.N2]] + 0.15 * rng.normal(size=(c.N2, 64))
        j = int(np.nonzero(perm[:c.N2] < c.N1)[0][0])             # desc2 row j is the partner of desc1 row p
        p = int(perm[j])
        j2 = (j + 1 + c.N2 // 3) % c.N2
        i2 = (p + 1 + c.N1 // 3) % c.N1
        d2[e, j2] = d2[e, j]                                      # stored twice: row p sees a ratio of exactly 1
        d1[e, i2] = d2[e, j]                                      # equal to both copies: 0 / 0
        plants.append((p, i2, j, j2))
    return d1, d2, plants


def smnn_reference(d1, d2, th):
    """float64, direct differences, lowest index on ties -> (keep [E,N1] bool, tgt [E,N1] int64, margin): keep[i] iff
    j = nn(i) has nn(j) == i and, for th >= 0, both ratios (nearest / second nearest Euclidean distance) are <= th -- a NaN
    ratio (0 / 0) fails that comparison, as it does in the reference's.  margin: how close a ratio that is not an exact tie
    of the best two (ratio exactly 1, or 0 / 0) comes to th and to 1."""
    E, N1, _ = d1.shape
    keep = np.zeros((E, N1), bool)
    tgt = np.zeros((E, N1), np.int64)
    margin = np.inf

    def top2(a, b):
        m = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
        i0 = m.argmin(1)                                          # the first minimum: lowest index
        rows = np.arange(m.shape[0])
        v0 = m[rows, i0]
        m[rows, i0] = np.inf
        v1 = m.min(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return i0, np.sqrt(v0) / np.sqrt(v1), v0 == v1

    for e in range(E):
        a, b = d1[e].astype(np.float64), d2[e].astype(np.float64)
        iA, rA, tieA = top2(a, b)
        iB, rB, tieB = top2(b, a)
        for r, tie in ((rA, tieA), (rB, tieB)):
            free = r[~tie]
            if len(free):
                margin = min(margin, float((1.0 - free).min()))
                if th >= 0:
                    margin = min(margin, float(np.abs(free - th).min()))
        mutual = iB[iA] == np.arange(N1)
        with np.errstate(invalid="ignore"):
            ok = np.ones(N1, bool) if th < 0 else (rA <= th) & (rB[iA] <= th)
        keep[e], tgt[e] = mutual & ok, iA
    return keep, tgt, margin


@functools.lru_cache(maxsize=None)
def smnn_data(i):
    """(desc1 [E,N1,64], desc2 [E,N2,64], plants, keep, tgt, margin) of case i: the first seed whose draw is admitted -- every
    ratio other than the planted ones at least SMNN_MARGIN away from th and from 1 (a condition on the inputs alone)."""
    c = SMNN_CASES[i]
    for seed in range(4000 + 100 * i, 4000 + 100 * i + 100):
        d1, d2, plants = _smnn_draw(c, seed)
        keep, tgt, margin = smnn_reference(d1, d2, c.th)
        if margin >= SMNN_MARGIN:
            for a in (d1, d2, keep, tgt):
                a.setflags(write=False)
            return d1, d2, plants, keep, tgt, margin
    raise AssertionError(f"no admitted draw for {c}")
