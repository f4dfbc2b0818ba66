"""Reference statements for the warm Chamfer operators on batches whose clouds differ in length (``x_lengths`` /
``y_lengths``): a padded batch is its trimmed clouds, one dense problem each; padding rows are (distance 0, index 0,
gradient 0).  Built on chamfer_loss_ref.py / chamfer_points_ref.py per element.  numpy only; not a test module."""
import numpy as np

from tests import chamfer_loss_ref, chamfer_points_ref


# (P1, P2, ((lx, ly) per element)): the smallest shapes that cross the 16-target boxes, the rows of 16 lanes, the 64-query
# groups, the 256-point consumer ranges and the choice of 1 ... 4 search waves; full, tiny, empty and mixed elements
CASES = {
    "A": (300, 270, ((300, 270), (1, 2), (0, 90), (257, 0), (64, 256), (17, 15))),
    "B": (1500, 1000, ((1500, 1000), (1000, 70), (65, 999))),
    "C1": (1, 1, ((1, 1),)),
    "C0": (1, 1, ((1, 0),)),
    "C2": (1, 1, ((0, 1),)),
}


def make_case(name, fill=0.0):
    """(x [N,P1,3], y [N,P2,3] float32 uniform in [-0.4, 0.4]^3 with the padding rows set to ``fill``, lx, ly), seeded."""
    P1, P2, lens = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) * 7 + 11)
    N = len(lens)
    x = rng.uniform(-0.4, 0.4, (N, P1, 3)).astype(np.float32)
    y = rng.uniform(-0.4, 0.4, (N, P2, 3)).astype(np.float32)
    lx, ly = [l[0] for l in lens], [l[1] for l in lens]
    for n in range(N):
        x[n, lx[n]:] = fill
        y[n, ly[n]:] = fill
    return x, y, lx, ly


def trim(c, lengths):
    """Padded batch [N,P,...] -> list of the N live prefixes [l_n,...]."""
    return [np.ascontiguousarray(c[n, :int(l)]) for n, l in enumerate(lengths)]


def nearest32(q, t):
    """One cloud against one cloud under the library's float32 contract, ((dx*dx)+(dy*dy))+(dz*dz) without contraction, ties to
    the lowest index -> (d [Pq] float32, idx [Pq] int64); an empty target cloud gives (0, 0)."""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    if t.shape[0] == 0 or q.shape[0] == 0:
        return np.zeros(q.shape[0], np.float32), np.zeros(q.shape[0], np.int64)
    df = q[:, None, :] - t[None, :, :]
    sq = df * df
    d = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    idx = d.argmin(-1)                              # first minimum = lowest index
    return d[np.arange(q.shape[0]), idx], idx.astype(np.int64)


def knn_ragged(x, y, lx, ly):
    """(d [N,P1] float32, idx [N,P1] int64) of x's live points among y's live points; padding rows, and every row of an
    element whose y is empty, are (0, 0)."""
    N, P1 = x.shape[0], x.shape[1]
    d, i = np.zeros((N, P1), np.float32), np.zeros((N, P1), np.int64)
    for n, (a, b) in enumerate(zip(trim(x, lx), trim(y, ly))):
        d[n, :a.shape[0]], i[n, :a.shape[0]] = nearest32(a, b)
    return d, i


def loss(d_xy, d_yx, lx, ly):
    """float32(sum in float64 of the live rows' float32 distances of both directions)."""
    total = np.float64(0.0)
    for n in range(d_xy.shape[0]):
        total += np.asarray(d_xy[n, :lx[n]], np.float64).sum() + np.asarray(d_yx[n, :ly[n]], np.float64).sum()
    return np.float32(total)


def _blank(P):
    z3 = np.zeros((P, 3), np.float64)
    return {"grad": z3.copy(), "own": z3.copy(), "scat": z3.copy(), "mag": z3.copy(), "cnt": np.zeros((P,), np.int64)}


def gradients(x, y, lx, ly, i_xy, i_yx, g_xy=None, g_yx=None, points=False):
    """The float64 gradient terms of chamfer_loss_ref.gradients (``points``: chamfer_points_ref.gradients with the upstreams
    g_xy / g_yx, None = dropped) evaluated per element on the trimmed clouds and written back into padded arrays
    -> dict per cloud ("x", "y") of grad, own, scat, mag [N,P,3] and cnt [N,P]; padding rows, and elements with an empty
    cloud, are zero."""
    N = x.shape[0]
    out = {name: {k: np.stack([_blank(c.shape[1])[k] for _ in range(N)]) for k in ("grad", "own", "scat", "mag", "cnt")}
           for name, c in (("x", x), ("y", y))}
    for n in range(N):
        a, b = int(lx[n]), int(ly[n])
        if a == 0 or b == 0:
            continue
        xa, yb = x[n:n + 1, :a], y[n:n + 1, :b]
        ixy, iyx = i_xy[n:n + 1, :a], i_yx[n:n + 1, :b]
        if points:
            g = chamfer_points_ref.gradients(xa, yb, ixy, iyx, None if g_xy is None else g_xy[n:n + 1, :a],
                                             None if g_yx is None else g_yx[n:n + 1, :b])
        else:
            g = chamfer_loss_ref.gradients(xa, yb, ixy, iyx)
        for name, l in (("x", a), ("y", b)):
            for k, v in g[name].items():
                out[name][k][n, :l] = v[0]
    return out


def frame_formula(set1, set2, reduction):
    """The reference's compute_chamfer_list (utils/eval_utils.py:39-66) in float64 by brute force: per frame the sum (or,
    for "mean", the mean over that frame's own points) of the squared nearest-neighbour distances of each direction, added;
    then summed / averaged over frames, or the per-frame values for any other reduction."""
    per = []
    for a, b in zip(set1, set2):
        d12 = chamfer_loss_ref.nearest(a[None], b[None])[0][0]
        d21 = chamfer_loss_ref.nearest(b[None], a[None])[0][0]
        per.append(d12.mean() + d21.mean() if reduction == "mean" else d12.sum() + d21.sum())
    per = np.stack(per)
    if reduction == "mean":
        return per.mean()
    return per.sum() if reduction == "sum" else per
