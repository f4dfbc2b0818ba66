"""numpy restatement of the K-nearest search contract (include/reart_hip.h, reart_knn_points_idx / _f64) in the dtype of
its inputs: d = ((d0*d0) + (d1*d1)) + ... with dc = p1[c] - p2[c], summed in ascending c, every operation one rounding
(numpy ufuncs never fuse); neighbours ascending by (distance, index); rows at or past lengths1[n] and slots at or past
lengths2[n] are zero.  Test infrastructure for the float64 search, which the float32 C oracle does not cover."""
import numpy as np


def knn_ref(p1, p2, K, lengths1=None, lengths2=None, rows=None, chunk=128):
    """p1 [N,P1,D], p2 [N,P2,D] of one float dtype -> (dists [N,R,K] in that dtype, idx [N,R,K] int64) for the query
    rows `rows` (default: all P1, R = P1)."""
    assert p1.dtype == p2.dtype
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    rows = np.arange(P1) if rows is None else np.asarray(rows)
    dists = np.zeros((N, len(rows), K), p1.dtype)
    idx = np.zeros((N, len(rows), K), np.int64)
    for n in range(N):
        n1 = P1 if lengths1 is None else max(0, min(int(lengths1[n]), P1))
        n2 = P2 if lengths2 is None else max(0, min(int(lengths2[n]), P2))
        kk = min(K, n2)
        if kk == 0:
            continue
        tT = np.ascontiguousarray(p2[n, :n2].T)                    # [D, n2]: contiguous per-dimension rows
        for s in range(0, len(rows), chunk):
            r = rows[s:s + chunk]
            pos = s + np.nonzero(r < n1)[0]
            if len(pos) == 0:
                continue
            qT = np.ascontiguousarray(p1[n, rows[pos]].T)         # [D, m]
            acc = np.zeros((len(pos), n2), p1.dtype)
            for c in range(D):
                diff = qT[c][:, None] - tT[c][None, :]
                acc = acc + diff * diff
            j = np.broadcast_to(np.arange(n2), acc.shape)
            order = np.lexsort((j, acc), axis=-1)[:, :kk]
            dists[n, pos, :kk] = np.take_along_axis(acc, order, -1)
            idx[n, pos, :kk] = order
    return dists, idx
