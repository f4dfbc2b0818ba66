"""Cases and a float64 restatement for the first-order backward of the PointNet++ front end (no GPU code is imported here):
``reart_mlp_layer_backward`` and ``reart_three_interpolate_backward`` (csrc/pointnet_grad.hip).

The layer is A = relu?(X W + b), Y = the max over groups of pool_k rows of A (or A).  The restatement takes its DECISIONS -- the
ReLU mask A > 0 and, per (group, column), the lowest row whose A equals the group's maximum (with ReLU a maximum of 0 selects
nothing) -- from the float32 A it is given, and computes dWt, dbias, dX, dF and dpoints2 in float64 on the float32 operands the
kernel multiplies (the convention of ``pointnet_range_ref.layer_ref``).  dZ is exact: a copy of dY or a zero.

Bounds, per element, derived and not measured; they hold for ANY order of summation (Higham 3.1, as in pointnet_range_ref:
a float32 sum of n products is within ((1 + u)^n - 1) sum |products| of the exact one, u < 2^-23 for a truncating matrix unit):

    |dWt   - f64| <= (rows + 2) 2^-23 (|X|^T |dZ|)
    |dbias - f64| <= rows 2^-23 sum_r |dZ|
    |dX    - f64| <= (Cout + 2) 2^-23 (|dZ| |Wt|^T)                       (the forward's bound: dX is a forward layer on dZ)
    |dF    - f64| <= sum over the point's m records of dX's bound + m 2^-23 sum |dX|
    |dP2   - f64| <= (m + 2) 2^-23 sum |w dOut|                            (m pairs name the coarse point)
"""
import functools
from collections import namedtuple

import numpy as np

from tests import pointnet_range_ref as R

EPS = R.EPS
ROW_CHUNK = 256           # REART_MLP_GRAD_ROW_CHUNK; tests/test_pointnet_grad_cpu.py holds it to reart_amd._lib

# name: None for the cases of pointnet_range_ref.LAYER_CASES (taken as they are), else the new case's name
GradCase = namedtuple("GradCase", "name c")


def _new_cases():
    C = ROW_CHUNK
    return [
        # rows = the row chunk of the dWt kernel, chunk - 1, chunk + 1, 2 chunk + 1
        GradCase("chunk", R._plain(C, 9, 33)), GradCase("chunk-1", R._plain(C - 1, 16, 65)),
        GradCase("chunk+1", R._plain(C + 1, 17, 32)), GradCase("2chunk+1", R._plain(2 * C + 1, 5, 100)),
        GradCase("2chunk+1-pooled", R._plain(2 * C + 2, 8, 33, 2)),
        # one row stored twice in every group, no other tie: the LOWER copy is selected
        GradCase("tie-relu", R._plain(96, 6, 40, 24)), GradCase("tie-linear", R._plain(128, 9, 33, 32, relu=False)),
        # every pre-activation of group 1 negative under ReLU: the group's gradients are exactly 0
        GradCase("dead-group", R._plain(72, 5, 33, 24)),
        # gathered: point 0 in every group, point 1 in none
        GradCase("everywhere-nowhere", R._gather("gather_fx", 5, 16, 2, 6, 30, 33, True)),
        # gathered: an index repeated inside a group (ball query's padding)
        GradCase("padded", R._gather("gather_xf", 4, 24, 2, 5, 40, 65, True)),
        GradCase("padded-fx", R._gather("gather_fx", 12, 32, 1, 4, 50, 32, True)),
    ]


GRAD_CASES = [GradCase(None, c) for c in R.LAYER_CASES] + _new_cases()
NEW_NAMES = ("chunk", "chunk-1", "chunk+1", "2chunk+1", "2chunk+1-pooled", "tie-relu", "tie-linear", "dead-group",
             "everywhere-nowhere", "padded", "padded-fx")


def case_id(i):
    g = GRAD_CASES[i]
    return "%d-%s-%dx%dx%d-k%d-%s" % ((i, g.name or "range") + tuple(g.c[:4]) + (g.c.form,))


def _operand(c, d):
    """Xop of a gathered case from its parts (as pointnet_range_ref.layer_data forms it)."""
    D, B, S, Npts, K = c.opt["D"], c.opt["B"], c.opt["S"], c.opt["Npts"], c.pool_k
    bb = np.arange(B)[:, None, None]
    q = d["Q"].reshape(B, Npts, 3)[bb, d["idx"]]
    if d["C"] is not None:
        q = q - d["C"].reshape(B, S, 1, 3)
    parts = [q]
    if D:
        f = d["F"].reshape(B, Npts, D)[bb, d["idx"]]
        parts = [f, q] if c.form == "gather_fx" else [q, f]
    return np.ascontiguousarray(np.concatenate(parts, axis=-1).reshape(c.rows, c.Cin).astype(np.float32))


@functools.lru_cache(maxsize=None)
def grad_data(i):
    """The inputs of case i: those of pointnet_range_ref.layer_data for its own cases, built here for the new ones, plus the
    upstream gradient ``dY`` [out rows, Cout] (float32, fixed by i)."""
    g = GRAD_CASES[i]
    c = g.c
    if g.name is None:
        d = dict(R.layer_data(i))
    else:
        rng = np.random.default_rng(7000 + i)
        d = {"W": (rng.normal(size=(c.Cin, c.Cout)) + np.arange(c.Cout)[None, :] * 0.01).astype(np.float32),
             "b": rng.normal(size=c.Cout).astype(np.float32)}
        if c.form == "plain":
            X = rng.normal(size=(c.rows, c.Cin)).astype(np.float32)
            if g.name.startswith("tie"):
                X3 = X.reshape(-1, c.pool_k, c.Cin)
                X3[:, c.pool_k - 3] = X3[:, 5]                     # row 5 of every group again at pool_k - 3: equal bits in A
            if g.name == "dead-group":
                X[c.pool_k:2 * c.pool_k] = 0.0                     # group 1: A = relu(b) with b < 0
                d["b"] = -np.abs(d["b"]) - np.float32(0.5)
                X[:c.pool_k] *= np.float32(8.0)                    # the other groups keep live columns
                X[2 * c.pool_k:] *= np.float32(8.0)
            d["X"] = d["Xop"] = X
        else:
            D, B, S, Npts, K = c.opt["D"], c.opt["B"], c.opt["S"], c.opt["Npts"], c.pool_k
            d["F"] = rng.normal(size=(B * Npts, D)).astype(np.float32)
            d["Q"] = rng.normal(size=(B * Npts, 3)).astype(np.float32)
            d["C"] = rng.normal(size=(B * S, 3)).astype(np.float32)
            if g.name == "everywhere-nowhere":
                idx = rng.integers(2, Npts, (B, S, K))
                idx[:, :, 3] = 0
            else:                                                  # a ball with few hits: the first hit fills the rest
                idx = np.stack([np.stack([np.sort(rng.choice(Npts, K, replace=False)) for _ in range(S)]) for _ in range(B)])
                fill = rng.integers(1, K // 2, (B, S))
                for b in range(B):
                    for s in range(S):
                        idx[b, s, fill[b, s]:] = idx[b, s, 0]
            d["idx"] = idx.astype(np.int64)
            d["Xop"] = _operand(c, d)
    d["dY"] = np.random.default_rng(8000 + i).normal(size=(R.out_rows(c), c.Cout)).astype(np.float32)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def forward_A(i):
    """The un-pooled activation in float32 numpy (what a CPU test takes the decisions from)."""
    c, d = GRAD_CASES[i].c, grad_data(i)
    b = np.zeros(c.Cout, np.float32) if d["b"] is None else d["b"]
    a = np.matmul(d["Xop"], d["W"], dtype=np.float32) + b[None, :]
    return np.maximum(a, np.float32(0)) if c.relu else a


def select(c, A, last_tie=False, mask_ge=False):
    """The decisions -> bool [rows, Cout]: dZ = dY[group] where True, 0 elsewhere.  ``last_tie`` / ``mask_ge``: planted errors."""
    live = (A >= 0 if mask_ge else A > 0) if c.relu else np.ones(A.shape, bool)
    if c.pool_k <= 1:
        return live
    A3 = A.reshape(-1, c.pool_k, c.Cout)
    if last_tie:
        sel = c.pool_k - 1 - np.argmax(A3[:, ::-1], axis=1)
    else:
        sel = np.argmax(A3, axis=1)                                # the first maximum: the lowest row
    hot = np.arange(c.pool_k)[None, :, None] == sel[:, None, :]
    return (hot & live.reshape(A3.shape)).reshape(A.shape)         # a selected row with A = 0 under ReLU: nothing


def dz_of(c, A, dY, **fault):
    up = np.repeat(dY, c.pool_k, axis=0) if c.pool_k > 1 else dY
    return np.where(select(c, A, **fault), up, np.float32(0)).astype(np.float32)


def feature_columns(c):
    D = c.opt["D"]
    return slice(0, D) if c.form == "gather_fx" else slice(3, 3 + D)


def scatter_rows(c, idx, vals, skip_first=False):
    """sum of vals[r] over the rows r that name point (b, p), ascending -> [B * Npts, cols]; also the count per point."""
    B, Npts = c.opt["B"], c.opt["Npts"]
    gp = (np.arange(B)[:, None, None] * Npts + idx).reshape(-1)
    out = np.zeros((B * Npts, vals.shape[1]), vals.dtype)
    cnt = np.zeros(B * Npts, np.int64)
    seen = np.zeros(B * Npts, bool)
    for r in range(len(gp)):
        if skip_first and not seen[gp[r]]:
            seen[gp[r]] = True
            continue
        out[gp[r]] += vals[r]
        cnt[gp[r]] += 1
    return out, cnt


def grad_ref(i, A):
    """float64 results and per-element bounds of case i with the decisions taken from the float32 ``A`` [rows, Cout]:
    dict of name -> (value, bound) for dWt, dbias, dX and (gathered, D > 0) dF; plus "dZ" -> float32 array."""
    c, d = GRAD_CASES[i].c, grad_data(i)
    dZ32 = dz_of(c, A, d["dY"])
    X, W, dZ = d["Xop"].astype(np.float64), d["W"].astype(np.float64), dZ32.astype(np.float64)
    out = {"dZ": dZ32}
    out["dWt"] = (X.T @ dZ, (c.rows + 2) * EPS * (np.abs(X).T @ np.abs(dZ)))
    out["dbias"] = (dZ.sum(0), c.rows * EPS * np.abs(dZ).sum(0))
    dX, bX = dZ @ W.T, (c.Cout + 2) * EPS * (np.abs(dZ) @ np.abs(W).T)
    out["dX"] = (dX, bX)
    if c.form.startswith("gather") and c.opt["D"]:
        cols = feature_columns(c)
        val, cnt = scatter_rows(c, d["idx"], dX[:, cols])
        bsum, _ = scatter_rows(c, d["idx"], bX[:, cols])
        asum, _ = scatter_rows(c, d["idx"], np.abs(dX[:, cols]))
        out["dF"] = (val, bsum + cnt[:, None] * EPS * asum)
    return out


def grad_emulate(i, A, fault=None):
    """The backward in float32 numpy, honest (fault = None) or with ONE planted error: ``last_tie`` (the last tied row selected),
    ``mask_ge`` (A >= 0 passes the ReLU), ``drop_chunk`` (the last row chunk missing from dWt), ``skip_first`` (the first record
    of every point missing from the scatter)."""
    c, d = GRAD_CASES[i].c, grad_data(i)
    dZ = dz_of(c, A, d["dY"], last_tie=fault == "last_tie", mask_ge=fault == "mask_ge")
    keep = c.rows
    if fault == "drop_chunk":
        keep = (-(-c.rows // ROW_CHUNK) - 1) * ROW_CHUNK
    out = {"dWt": np.matmul(d["Xop"][:keep].T, dZ[:keep], dtype=np.float32), "dbias": dZ.sum(0, dtype=np.float32),
           "dX": np.matmul(dZ, d["W"].T, dtype=np.float32)}
    if c.form.startswith("gather") and c.opt["D"]:
        out["dF"] = scatter_rows(c, d["idx"], out["dX"][:, feature_columns(c)], skip_first=fault == "skip_first")[0]
    return out


FAULTS = ("last_tie", "mask_ge", "drop_chunk", "skip_first")


def ratio(got, ref, bound):
    """max |got - f64| / bound (inf where the bound is zero and the result is not exact)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def worst_ratio(i, A, got):
    """The largest ratio over the outputs present in ``got`` (dX of a gathered case is not an output: its dF is)."""
    ref = grad_ref(i, A)
    c = GRAD_CASES[i].c
    worst = 0.0
    for k, v in got.items():
        if k == "dX" and c.form.startswith("gather"):
            continue
        worst = max(worst, ratio(v, *ref[k]))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# interpolation backward
# ---------------------------------------------------------------------------------------------------------------------
FAR_CASE, FAR_INDEX = R.TnnCase(2, 130, 6, 33), 2      # the new case: coarse point 2 lies far away, no fine point selects it
TNN_CASES = list(R.TNN_CASES) + [FAR_CASE]
INTERP_COL0, INTERP_PAD = 4, 3      # dOut: columns col0 .. col0 + D of a tensor INTERP_PAD columns wider behind them


@functools.lru_cache(maxsize=None)
def interp_data(i):
    """(fine, coarse, dOut [B*N, col0 + D + pad]): the clouds of pointnet_range_ref.tnn_data(i) as they are; for the new case
    five fine points and, at FAR_INDEX, a point far away from every fine point."""
    c = TNN_CASES[i]
    if i < len(R.TNN_CASES):
        fine, coarse, _ = R.tnn_data(i)
    else:
        rng = np.random.default_rng(3900)
        fine = rng.uniform(-1, 1, (c.B, c.N, 3)).astype(np.float32)
        coarse = np.ascontiguousarray(fine[:, :c.S2]).copy()
        coarse[:, FAR_INDEX] = 50.0
    dOut = np.random.default_rng(9000 + i).normal(size=(c.B * c.N, INTERP_COL0 + c.D + INTERP_PAD)).astype(np.float32)
    for a in (fine, coarse, dOut):
        a.setflags(write=False)
    return fine, coarse, dOut


def interp_weights(dist3):
    """The forward's weights from the three squared distances, float32 operation for operation (interp3_kernel)."""
    w = np.float32(1.0) / (dist3.astype(np.float32) + np.float32(1e-8))
    ws = (w[..., 0] + w[..., 1]) + w[..., 2]
    return (w / ws[..., None]).astype(np.float32)


def interp_ref(idx3, w, dOut, S2, skip_first=False, dtype=np.float64):
    """dpoints2 [B,S2,D] and its bound from idx3 [B,N,3], w [B,N,3] (float32) and dOut [B*N, D] (the window only)."""
    B, N, _ = idx3.shape
    D = dOut.shape[1]
    val = np.zeros((B, S2, D), dtype)
    mag = np.zeros((B, S2, D), np.float64)
    cnt = np.zeros((B, S2), np.int64)
    seen = np.zeros((B, S2), bool)
    g = dOut.reshape(B, N, D)
    for b in range(B):
        for n in range(N):
            for j in range(3):
                s = idx3[b, n, j]
                if skip_first and not seen[b, s]:
                    seen[b, s] = True
                    continue
                val[b, s] += (w[b, n, j].astype(dtype) * g[b, n].astype(dtype)).astype(dtype)
                mag[b, s] += np.abs(w[b, n, j].astype(np.float64) * g[b, n].astype(np.float64))
                cnt[b, s] += 1
    return val, (cnt[:, :, None] + 2) * EPS * mag, cnt


# ---------------------------------------------------------------------------------------------------------------------
# the modules: float64 restatement with the decisions of a float32 forward (torch on the CPU, the oracle's sampling)
# ---------------------------------------------------------------------------------------------------------------------
class Restatement:
    """The layer classes and the extractor as tensor expressions, evaluated twice side by side: in float32 (which decides every
    ReLU and every group maximum, as the kernels do) and in float64 with those decisions (which carries the autograd graph to
    the float64 copies of the parameters and of the incoming features).  Channel-last throughout.  ``margin``: the smallest
    pooled top-two gap between distinct values, or selected pre-activation, relative to its layer's largest activation."""

    def __init__(self, sd):
        import torch

        self.torch = torch
        self.p32 = {k: torch.tensor(np.asarray(v)) for k, v in sd.items()}
        self.p64 = {k: (v.double().requires_grad_(not k.endswith(("running_mean", "running_var"))) if v.dtype == torch.float32 else v)
                    for k, v in self.p32.items()}
        self.margin = np.inf

    def fold(self, conv, bn, p):
        w = p[conv + ".weight"]
        w = w.reshape(w.shape[0], -1)
        s = p[bn + ".weight"] / self.torch.sqrt(p[bn + ".running_var"] + 1e-5)
        return (w * s[:, None]).t(), (p[conv + ".bias"] - p[bn + ".running_mean"]) * s + p[bn + ".bias"]

    def stack(self, x32, x64, names, pool_k=0):
        """[rows, Cin] twice -> [rows (/pool_k), C] twice."""
        torch = self.torch
        for conv, bn in names:
            W32, b32 = self.fold(conv, bn, self.p32)
            W64, b64 = self.fold(conv, bn, self.p64)
            z32, z64 = x32 @ W32 + b32, x64 @ W64 + b64
            live = z32 > 0
            x32, x64 = torch.where(live, z32, torch.zeros_like(z32)), torch.where(live, z64, torch.zeros_like(z64))
        if pool_k > 1:
            C = x32.shape[1]
            A3 = x32.reshape(-1, pool_k, C)
            sel = torch.from_numpy(np.argmax(A3.numpy(), axis=1))                     # the first maximum
            y32 = torch.gather(A3, 1, sel[:, None, :])[:, 0]
            top = y32.numpy()
            if (top > 0).any():
                a = A3.numpy()
                below = np.where(a < top[:, None, :], a, -np.inf).max(axis=1)         # the largest value that is not the top's
                z3 = z32.reshape(-1, pool_k, C).numpy()
                zsel = np.take_along_axis(z3, sel.numpy()[:, None, :], 1)[:, 0]
                pos = top > 0
                m = min(float((top - below)[pos].min()), float(np.abs(zsel)[pos].min())) / float(top.max())
                self.margin = min(self.margin, m)
            x32, x64 = y32, torch.gather(x64.reshape(-1, pool_k, C), 1, sel[:, None, :])[:, 0]
        return x32, x64

    @staticmethod
    def _idx(points, idx):
        B = points.shape[0]
        return points[np.arange(B).reshape((B,) + (1,) * (idx.ndim - 1)), idx]

    def grouped(self, xyz, f32, f64, new_xyz, idx, names, xyz_first):
        """xyz [B,N,3] numpy; features [B,N,D] twice or None; centres [B,S,3] numpy or None; idx [B,S,K] -> [B,S,C] twice."""
        torch = self.torch
        B, S, K = idx.shape
        g = self._idx(xyz, idx)
        if new_xyz is not None:
            g = g - new_xyz[:, :, None, :]
        g = torch.from_numpy(np.ascontiguousarray(g, np.float32))
        tidx = torch.from_numpy(idx)
        parts32, parts64 = [g], [g.double()]
        if f32 is not None:
            bb = torch.arange(B)[:, None, None]
            a, b = f32[bb, tidx], f64[bb, tidx]
            parts32, parts64 = ([g, a], [g.double(), b]) if xyz_first else ([a, g], [b, g.double()])
        x32, x64 = torch.cat(parts32, -1).reshape(B * S * K, -1), torch.cat(parts64, -1).reshape(B * S * K, -1)
        y32, y64 = self.stack(x32, x64, names, K)
        return y32.reshape(B, S, -1), y64.reshape(B, S, -1)

    def sa_msg(self, prefix, xyz, f32, f64, npoint, radii, nsamples, n_layers, start):
        import oracle

        fps = oracle.fps(xyz, npoint, start=start, cuda_mode=False)
        new_xyz = self._idx(xyz, fps)
        o32, o64 = [], []
        for i, (radius, K) in enumerate(zip(radii, nsamples)):
            idx = oracle.ball_query(radius, K, xyz, new_xyz, cuda_mode=False)
            names = [(f"{prefix}conv_blocks.{i}.{j}", f"{prefix}bn_blocks.{i}.{j}") for j in range(n_layers)]
            a, b = self.grouped(xyz, f32, f64, new_xyz, idx, names, xyz_first=False)
            o32.append(a)
            o64.append(b)
        return new_xyz, self.torch.cat(o32, -1), self.torch.cat(o64, -1)

    def sa(self, prefix, xyz, f32, f64, npoint, radius, nsample, n_layers, start, group_all):
        import oracle

        names = [(f"{prefix}mlp_convs.{j}", f"{prefix}mlp_bns.{j}") for j in range(n_layers)]
        B, N, _ = xyz.shape
        if group_all:
            idx = np.broadcast_to(np.arange(N)[None, None, :], (B, 1, N)).copy()
            return (np.zeros((B, 1, 3), np.float32),) + self.grouped(xyz, f32, f64, None, idx, names, xyz_first=True)
        fps = oracle.fps(xyz, npoint, start=start, cuda_mode=False)
        new_xyz = self._idx(xyz, fps)
        idx = oracle.ball_query(radius, nsample, xyz, new_xyz, cuda_mode=False)
        return (new_xyz,) + self.grouped(xyz, f32, f64, new_xyz, idx, names, xyz_first=True)

    def fp(self, prefix, xyz1, xyz2, p1_32, p1_64, p2_32, p2_64, n_layers):
        import oracle

        torch = self.torch
        B, N, _ = xyz1.shape
        if xyz2.shape[1] == 1:
            i32, i64 = p2_32.expand(B, N, -1), p2_64.expand(B, N, -1)
        else:
            dist3, idx3 = oracle.three_nn_expanded(xyz1, xyz2)
            w = torch.from_numpy(interp_weights(dist3))
            tidx, bb = torch.from_numpy(idx3), torch.arange(B)[:, None]
            g32, g64 = [p2_32[bb, tidx[:, :, j]] for j in range(3)], [p2_64[bb, tidx[:, :, j]] for j in range(3)]
            i32 = (g32[0] * w[:, :, 0:1] + g32[1] * w[:, :, 1:2]) + g32[2] * w[:, :, 2:3]
            wd = w.double()
            i64 = g64[0] * wd[:, :, 0:1] + g64[1] * wd[:, :, 1:2] + g64[2] * wd[:, :, 2:3]
        if p1_32 is not None:
            i32, i64 = torch.cat([p1_32, i32], -1), torch.cat([p1_64, i64], -1)
        names = [(f"{prefix}mlp_convs.{j}", f"{prefix}mlp_bns.{j}") for j in range(n_layers)]
        y32, y64 = self.stack(i32.reshape(B * N, -1), i64.reshape(B * N, -1), names)
        return y32.reshape(B, N, -1), y64.reshape(B, N, -1)

    def extractor(self, pts, starts):
        """PointNet2Msg2(64): pts [B,N,3] numpy -> [B,N,64] twice."""
        torch = self.torch
        B, N, _ = pts.shape
        f32 = torch.from_numpy(pts)
        f64 = f32.double()
        l1_xyz, a1, b1 = self.sa_msg("sa1.", pts, f32, f64, 512, [0.05, 0.1, 0.2], [32, 64, 128], 3, starts[0])
        l2_xyz, a2, b2 = self.sa_msg("sa2.", l1_xyz, a1, b1, 128, [0.2, 0.4], [64, 128], 3, starts[1])
        _, a3, b3 = self.sa("sa3.", l2_xyz, a2, b2, None, None, None, 3, None, True)
        a2n, b2n = self.fp("fp3.", l2_xyz, l2_xyz[:, :1], a2, b2, a3, b3, 2)
        a1n, b1n = self.fp("fp2.", l1_xyz, l2_xyz, a1, b1, a2n, b2n, 2)
        s32 = torch.cat([f32, f32], -1)
        a0n, b0n = self.fp("fp1.", pts, l1_xyz, s32, s32.double(), a1n, b1n, 2)
        y32, y64 = self.stack(a0n.reshape(B * N, -1), b0n.reshape(B * N, -1), [("conv1", "bn1")])
        return y32.reshape(B, N, -1), y64.reshape(B, N, -1)
