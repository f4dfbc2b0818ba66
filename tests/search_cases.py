"""Hostile geometry for the exact box-pruned searches (csrc/prune.hip) and a plain model of their filter.

``case(name)`` gives float32 ``(queries [P1,3], targets [P2,3])`` from a fixed numpy generator, both clouds already stored
in ``reart_amd.relax.kd_order`` order: boxes of 16 stored targets are then tight and the pruning is active also on the
entries that do no sorting of their own.  The sizes sit on the kernel's structural edges -- boxes of 16 targets with half
boxes / blocks of 8, query groups of 64, S = 1 .. 4 slices by the target count, a coarse round of 64 S boxes (a second
round beyond 1024 S targets).

    case         queries                                     targets                          what it is for
    lattice      every 3rd lattice point + 0.025,            12^3 lattice, step 0.05 (1728)   exact ties between distinct targets in
                 every 5th lattice point (922)                                                different boxes and slices; exact hits
    sphere       300 near the centre, 300 in [-1,1]^3,       3000 on a sphere of radius 0.3   every target nearly equidistant; queries
                 50 in [5,9]^3                                                                far outside every box
    cluster      800 in [-1.2,1.2]^3                         2000 from N(0, 1e-3) + 100       one part of the tree holds almost all
                                                             outliers                         boxes
    sheet        700 in [-0.4,0.4]^3                         2500 with z = 0                  boxes of zero extent along one axis
    line         513                                         1025 on the x axis               zero extent along two axes; P1 and P2 one
                                                                                              past a multiple of 64 / 16
    coincident   130                                         300 copies of one point          every distance tied; nothing prunable; S = 4
    jump         1000: targets + N(0, 2e-3), every 5th       4112 uniform in [-0.4,0.4]^3     the loop's situation (a fifth of the queries
                 re-drawn uniformly                                                           have jumped); second coarse round of one box
    big          uniform x 2^40 (700)                        uniform x 2^40 (1500)            squared distances near 1e22
    offset       uniform + 2^20 (700)                        uniform + 2^20 (1500)            coordinates quantised by their own magnitude:
                                                                                              coincident and tied targets nobody wrote down
    tiny60       uniform x 2^-60 (700)                       uniform x 2^-60 (1500)           squares near the bottom of the normal range
    tiny70       uniform x 2^-70 (700)                       uniform x 2^-70 (1500)           squares are denormal numbers: distances
                                                                                              quantised to a few values
    small_P1xP2  P1 = 1, 3, 64, 65 in turn                   P2 = 1, 2, 3, 8, 9, 16, 17, 63,  fewer targets than K, one box, one half box,
                                                             129, 193                         each S

The model functions are float32 with the kernel's order of operations, ``(dx dx + dy dy) + dz dz`` and
``e = max(lo - q, q - hi, 0)``; numpy rounds every operation once (no fused multiply-add) and keeps denormal numbers.
A slot for which no target exists (P2 < K) holds distance 0 and index 0, as ``oracle.knn_points`` leaves it."""
import functools

import numpy as np

BOX = 16                    # targets per box (NN_BOX)
OFFSET_E = 20               # the `offset` case adds 2^OFFSET_E: an ulp of 2^-3 over clouds 0.8 wide (2^19: 37 % ties at K = 1)
SMALL = tuple(zip((1, 3, 64, 65, 1, 3, 64, 65, 3, 65), (1, 2, 3, 8, 9, 16, 17, 63, 129, 193)))      # (P1, P2)


def _uniform(rng, n, lo=-0.4, hi=0.4):
    return rng.uniform(lo, hi, (n, 3))


def _lattice(rng):
    lat = np.stack(np.meshgrid(*[np.arange(12) * 0.05] * 3, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([lat[::3] + 0.025, lat[::5]]), lat


def _sphere(rng):
    surf = rng.normal(size=(3000, 3))
    surf /= np.linalg.norm(surf, axis=-1, keepdims=True)
    return np.concatenate([rng.uniform(-0.05, 0.05, (300, 3)), rng.uniform(-1, 1, (300, 3)), rng.uniform(5, 9, (50, 3))]), surf * 0.3


def _cluster(rng):
    return rng.uniform(-1.2, 1.2, (800, 3)), np.concatenate([rng.normal(0, 1e-3, (2000, 3)), rng.uniform(-1, 1, (100, 3))])


def _sheet(rng):
    return rng.uniform(-0.4, 0.4, (700, 3)), np.concatenate([rng.uniform(-0.3, 0.3, (2500, 2)), np.zeros((2500, 1))], -1)


def _line(rng):
    t = np.zeros((1025, 3))
    t[:, 0] = rng.uniform(-0.4, 0.4, 1025)
    q = rng.uniform(-0.4, 0.4, (513, 3))
    q[::4, 1:] = 0.0                               # a quarter of the queries on the line itself
    return q, t


def _coincident(rng):
    p = rng.uniform(-0.4, 0.4, (1, 3))
    return rng.uniform(-0.4, 0.4, (130, 3)), np.repeat(p, 300, 0)


def _jump(rng):
    t = _uniform(rng, 4112)
    q = t[rng.integers(0, 4112, 1000)] + rng.normal(0, 2e-3, (1000, 3))
    q[::5] = _uniform(rng, 200)
    return q, t


def _scaled(scale, rng):
    return _uniform(rng, 700) * scale, _uniform(rng, 1500) * scale


def _offset(rng):
    return _uniform(rng, 700) + 2.0 ** OFFSET_E, _uniform(rng, 1500) + 2.0 ** OFFSET_E


def _small(p1, p2, rng):
    return _uniform(rng, p1), _uniform(rng, p2)


_TABLE = {"lattice": _lattice, "sphere": _sphere, "cluster": _cluster, "sheet": _sheet, "line": _line,
          "coincident": _coincident, "jump": _jump, "big": functools.partial(_scaled, 2.0 ** 40), "offset": _offset,
          "tiny60": functools.partial(_scaled, 2.0 ** -60), "tiny70": functools.partial(_scaled, 2.0 ** -70)}
_TABLE.update({f"small_{p1}x{p2}": functools.partial(_small, p1, p2) for p1, p2 in SMALL})
NAMES = tuple(_TABLE)


def _stored(c):
    """float32, in the leaf order of its own k-d tree."""
    import torch

    from reart_amd.relax import kd_order

    c = np.ascontiguousarray(c, dtype=np.float32)
    return np.ascontiguousarray(c[kd_order(torch.from_numpy(c)).numpy()])


@functools.lru_cache(maxsize=None)
def case(name, seed=0):
    """(queries [P1,3], targets [P2,3]) float32 in k-d leaf order, read-only.  ``seed`` draws another instance of the case."""
    rng = np.random.default_rng([NAMES.index(name), seed, 2024])
    q, t = (_stored(c) for c in _TABLE[name](rng))
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t


# ---- the plain model --------------------------------------------------------------------------------------------------
def sqdist(q, t):
    """[P1,3] x [P2,3] -> [P1,P2] float32, ``(dx dx + dy dy) + dz dz``."""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    dx, dy, dz = (q[:, None, a] - t[None, :, a] for a in range(3))
    return (dx * dx + dy * dy) + dz * dz


def brute(q, t, K):
    """(dists [P1,K] float32 ascending, idx [P1,K] int64): a stable sort on the full distance matrix."""
    d = sqdist(q, t)
    n = min(K, d.shape[1])
    order = np.argsort(d, axis=1, kind="stable")[:, :n]
    dists, idx = np.zeros((d.shape[0], K), np.float32), np.zeros((d.shape[0], K), np.int64)
    dists[:, :n], idx[:, :n] = np.take_along_axis(d, order, 1), order
    return dists, idx


def boxes(t):
    """(lo [nb,3], hi [nb,3]): the corners of every 16 stored targets (the last box may be short)."""
    t = np.asarray(t, np.float32)
    nb = (t.shape[0] + BOX - 1) // BOX
    pad = np.concatenate([t, np.repeat(t[-1:], nb * BOX - t.shape[0], 0)]).reshape(nb, BOX, 3)
    return pad.min(1), pad.max(1)


def lower_bound(q, lo, hi):
    """[P1,3] x [nb,3] -> [P1,nb] float32: the point-to-box bound of the precise filter."""
    q = np.asarray(q, np.float32)
    ex, ey, ez = (np.maximum(np.maximum(lo[None, :, a] - q[:, None, a], q[:, None, a] - hi[None, :, a]), np.float32(0))
                  for a in range(3))
    return (ex * ex + ey * ey) + ez * ez


def kth(q, t, K):
    """[P1] the K-th smallest distance of every query (the last one there is when P2 < K)."""
    d = np.sort(sqdist(q, t), axis=1)
    return d[:, min(K, d.shape[1]) - 1]


def tie_fraction(q, t, K):
    """Share of the queries for which more than one target attains the K-th distance."""
    return float(((sqdist(q, t) == kth(q, t, K)[:, None]).sum(1) > 1).mean())


def prunable(q, t, K):
    """Share of the (query, box) pairs with ``lower_bound > K-th distance``: what an ideal seed lets the filter drop."""
    return float((lower_bound(q, *boxes(t)) > kth(q, t, K)[:, None]).mean())


def violations(q, t):
    """Number of (query, target) pairs with ``lower_bound(query, box of target) > distance`` in float32."""
    lb = lower_bound(q, *boxes(t))
    return int((lb[:, np.arange(t.shape[0]) // BOX] > sqdist(q, t)).sum())
