"""Float64 restatement of the bidirectional K = 1 Chamfer sum and its gradients (networks/loss.py:24-29 through
utils/chamfer.py:78-123), for the tests of ``ChamferLoss``.  numpy only; not a test module."""
import numpy as np


def nearest(a, b):
    """Brute force in float64: for every a[n,i] the lowest index of the nearest b[n,j] -> (d [N,Pa], idx [N,Pa])."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = ((a[:, :, None, :] - b[:, None, :, :]) ** 2).sum(-1)
    idx = d.argmin(-1)
    return np.take_along_axis(d, idx[..., None], -1)[..., 0], idx


def counts(idx, P):
    """How many points chose each of the P targets: idx [N,Pq] -> [N,P]."""
    out = np.zeros((idx.shape[0], P), np.int64)
    for n in range(idx.shape[0]):
        np.add.at(out[n], idx[n], 1)
    return out


def gradients(x, y, i_xy, i_yx):
    """The two formulas in float64 from the float32 inputs and the given neighbour indices:
        grad_x[n,i] = 2 (x_i - y_nn(i)) + 2 sum_{j: nn_yx(j) = i} (x_i - y_j)
        grad_y[n,j] = 2 (y_j - x_nn_yx(j)) + 2 sum_{i: nn(i) = j} (y_j - x_i)
    -> dict per cloud ("x", "y") of: grad [N,P,3]; own [N,P,3] = the first term; scat [N,P,3] = the second term;
    mag [N,P,3] = sum of |2 (difference)| over the second term's addends; cnt [N,P] = the number of those addends."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = {}
    for name, own, oth, i_own, i_oth in (("x", x, y, i_xy, i_yx), ("y", y, x, i_yx, i_xy)):
        N, P, _ = own.shape
        first = 2.0 * (own - np.take_along_axis(oth, i_own[..., None].repeat(3, -1), 1))
        scat, mag = np.zeros_like(own), np.zeros_like(own)
        for n in range(N):
            diff = 2.0 * (own[n][i_oth[n]] - oth[n])          # addend of every point of the other cloud
            np.add.at(scat[n], i_oth[n], diff)
            np.add.at(mag[n], i_oth[n], np.abs(diff))
        out[name] = {"grad": first + scat, "own": first, "scat": scat, "mag": mag, "cnt": counts(i_oth, P)}
    return out


def loss(d_xy, d_yx):
    """float32(sum of the float32 distances in float64)."""
    return np.float32(np.asarray(d_xy, np.float64).sum() + np.asarray(d_yx, np.float64).sum())


def cluster_case(n_cluster=1000, n_far=7, seed=3):
    """The case that stresses the fixed-point range: n_cluster y points around ONE x point, the other x points far away."""
    rng = np.random.default_rng(seed)
    x = np.empty((1, 1 + n_far, 3), np.float32)
    x[0, 0] = (0.25, -0.5, 0.125)
    x[0, 1:] = x[0, 0] + rng.choice([-1.0, 1.0], (n_far, 3)) * rng.uniform(5.0, 9.0, (n_far, 3))
    y = (x[0, 0] + rng.normal(0, 1e-2, (1, n_cluster, 3))).astype(np.float32)
    return x, y
