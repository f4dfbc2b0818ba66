"""Float64 restatement of the per-point Chamfer distances' gradients for per-point upstream gradients, for the tests of
``ChamferPoints`` (modelled on chamfer_loss_ref.py, whose ``nearest``, ``counts`` and ``cluster_case`` it uses).  numpy
only; not a test module."""
import numpy as np

from tests.chamfer_loss_ref import cluster_case, counts, nearest  # noqa: F401  (re-exported for the tests)


def value(x, y, w, v):
    """sum_i w_i d_xy[i] + sum_j v_j d_yx[j] in float64 (brute-force neighbours)."""
    return (np.asarray(w, np.float64) * nearest(x, y)[0]).sum() + (np.asarray(v, np.float64) * nearest(y, x)[0]).sum()


def gradients(x, y, i_xy, i_yx, g_xy, g_yx):
    """The two formulas in float64 from the float32 inputs, the given neighbour indices and the upstream gradients
    (None: that direction's terms are dropped, its indices are not read):
        grad_x[n,i] = 2 g_xy[n,i] (x_i - y_{i_xy[i]}) + 2 sum_{j: i_yx[j] = i} g_yx[n,j] (x_i - y_j)
        grad_y[n,j] = 2 g_yx[n,j] (y_j - x_{i_yx[j]}) + 2 sum_{i: i_xy[i] = j} g_xy[n,i] (y_j - x_i)
    -> dict per cloud ("x", "y") of: grad [N,P,3]; own [N,P,3] = the first term; scat [N,P,3] = the second term;
    mag [N,P,3] = sum of |2 g (difference)| over the second term's addends; cnt [N,P] = the number of those addends."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = {}
    for name, own, oth, i_own, g_own, i_oth, g_oth in (("x", x, y, i_xy, g_xy, i_yx, g_yx), ("y", y, x, i_yx, g_yx, i_xy, g_xy)):
        N, P, _ = own.shape
        first, scat, mag = np.zeros_like(own), np.zeros_like(own), np.zeros_like(own)
        cnt = np.zeros((N, P), np.int64)
        if g_own is not None:
            g = np.asarray(g_own, np.float64)[..., None]
            first = 2.0 * g * (own - np.take_along_axis(oth, np.asarray(i_own)[..., None].repeat(3, -1), 1))
        if g_oth is not None:
            g = np.asarray(g_oth, np.float64)
            i_oth = np.asarray(i_oth)
            for n in range(N):
                diff = 2.0 * g[n][:, None] * (own[n][i_oth[n]] - oth[n])      # addend of every point of the other cloud
                np.add.at(scat[n], i_oth[n], diff)
                np.add.at(mag[n], i_oth[n], np.abs(diff))
            cnt = counts(i_oth, P)
        out[name] = {"grad": first + scat, "own": first, "scat": scat, "mag": mag, "cnt": cnt}
    return out
