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
A slot for which no target exists (P2 < K) holds distance 0 and index 0, as ``oracle.knn_points`` leaves it.

``large_case(name)`` gives the cases of a second table, ``LARGE``, by the same conventions; they reach what the sizes
above cannot: a third and later coarse round, box numbers above 4096, target indices above 65 535, more than 2^20 distance
evaluations by one cold wave.  ``NAMES`` does not contain them.

    case          queries                                    targets                          what it is for
    round3        1000, as `jump`                            8208 uniform (2 x 4096 + 16)     third coarse round of one box at S = 4; nine
                                                                                              rounds at S = 1
    coincident8k  130 uniform                                8208 copies of one point         every distance tied, nothing prunable: every
                                                                                              wave scans or queues every box of three rounds
    lattice27k    every 7th cell centre, every 11th          30^3 lattice, step 0.05          exact ties between distinct targets in different
                  lattice point (6313)                                                        boxes, slices and coarse rounds (7 at S = 4)
    scan70k       the targets permuted + N(0, 2e-3), every   70 000 on a closed bumpy         indices above 65 535, box numbers above 4096,
                  5th re-drawn uniformly (70 000)            surface + N(0, 1e-3)             18 coarse rounds at S = 4, more than 2^20
                                                                                              evaluations per cold wave; free of ties
    fanin70k      chamfer_loss_ref.cluster_case(70 000):     its 8 x points                   70 000 addends in one target's fixed-point sum
                  the 70 000 y points

The model functions above build full P1 x P2 matrices; for the large cases use ``brute_chunked`` / ``kth_chunked`` / ``blocks``
(256 queries at a time) or pass the rows of ``sample(name)`` -- no matrix above 64 M entries (``MAX_ENTRIES``)."""
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


def stored(c):
    """float32, in the leaf order of its own k-d tree."""
    import torch

    from reart_amd.relax import kd_order

    c = np.ascontiguousarray(c, dtype=np.float32)
    return np.ascontiguousarray(c[kd_order(torch.from_numpy(c)).numpy()])


@functools.lru_cache(maxsize=None)
def case(name, seed=0):
    """(queries [P1,3], targets [P2,3]) float32 in k-d leaf order, read-only.  ``seed`` draws another instance of the case."""
    rng = np.random.default_rng([NAMES.index(name), seed, 2024])
    q, t = (stored(c) for c in _TABLE[name](rng))
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


# ---- the large cases --------------------------------------------------------------------------------------------------
MAX_ENTRIES = 64 * 2 ** 20      # no model matrix above this many entries
BLOCK = 256                     # queries per block of the chunked forms


def _round3(rng, seed=0):
    t = _uniform(rng, 8208)
    q = t[rng.integers(0, 8208, 1000)] + rng.normal(0, 2e-3, (1000, 3))
    q[::5] = _uniform(rng, 200)
    return q, t


def _coincident8k(rng, seed=0):
    p = rng.uniform(-0.4, 0.4, (1, 3))
    return rng.uniform(-0.4, 0.4, (130, 3)), np.repeat(p, 8208, 0)


def _lattice27k(rng, seed=0):
    lat = np.stack(np.meshgrid(*[np.arange(30) * 0.05] * 3, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([lat[::7] + 0.025, lat[::11]]), lat


def _scan70k(rng, seed=0, n=70000):
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    t = u * (0.3 + 0.05 * np.sin(7 * u[:, :1]) * np.cos(5 * u[:, 1:2])) + rng.normal(0, 1e-3, (n, 3))
    q = t[rng.permutation(n)] + rng.normal(0, 2e-3, (n, 3))
    q[::5] = _uniform(rng, q[::5].shape[0])
    return q, t


def _fanin70k(rng, seed=0):      # the only construction that draws from a generator of its own
    from tests.chamfer_loss_ref import cluster_case

    x, y = cluster_case(n_cluster=70000, seed=3 + seed)
    return y[0], x[0]


#         case: (first word of the generator's seed, construction(rng, seed))
LARGE = {"round3": (101, _round3), "coincident8k": (102, _coincident8k), "lattice27k": (103, _lattice27k),
         "scan70k": (100, _scan70k), "fanin70k": (104, _fanin70k)}
LARGE_NAMES = tuple(LARGE)
ROUNDS3 = ("round3", "coincident8k", "lattice27k", "scan70k")       # the cases that claim a third coarse round at S = 4


@functools.lru_cache(maxsize=None)
def large_case(name, seed=0):
    """As ``case``, for the table ``LARGE``."""
    key, make = LARGE[name]
    rng = np.random.default_rng([key, seed, 2024])
    q, t = (stored(c) for c in make(rng, seed))
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t


def sample(P1, n=512):
    """``n`` fixed rows out of P1 (all of them when P1 <= n), ascending."""
    return np.arange(P1) if P1 <= n else np.sort(np.random.default_rng(P1).choice(P1, n, replace=False))


def coarse_rounds(P2, S):
    """(boxes, coarse rounds of 64 S boxes) of P2 targets."""
    nbox = (P2 + BOX - 1) // BOX
    return nbox, (nbox + 64 * S - 1) // (64 * S)


def blocks(q, t):
    """(first row, float32 distances [<= 256, P2]) of every block of 256 queries; the rows are the caller's to overwrite."""
    assert BLOCK * t.shape[0] <= MAX_ENTRIES
    for r in range(0, q.shape[0], BLOCK):
        yield r, sqdist(q[r:r + BLOCK], t)


def brute_chunked(q, t, K):
    """``brute`` without the full matrix: per block of 256 queries, K times the first minimum of the row (the lowest index
    among equal distances), which is then struck out -- the first K entries of the stable sort."""
    n = min(K, t.shape[0])
    dists, idx = np.zeros((q.shape[0], K), np.float32), np.zeros((q.shape[0], K), np.int64)
    for r, d in blocks(q, t):
        rows = np.arange(d.shape[0])
        for k in range(n):
            j = d.argmin(1)
            dists[r:r + d.shape[0], k], idx[r:r + d.shape[0], k] = d[rows, j], j
            d[rows, j] = np.inf
    return dists, idx


def kth_chunked(q, t, K):
    """``kth`` without the full matrix -> (K-th distance [P1], number of targets at exactly that distance [P1])."""
    n = min(K, t.shape[0])
    out, cnt = np.zeros(q.shape[0], np.float32), np.zeros(q.shape[0], np.int64)
    for r, d in blocks(q, t):
        out[r:r + d.shape[0]] = np.partition(d, n - 1, axis=1)[:, n - 1]
        cnt[r:r + d.shape[0]] = (d == out[r:r + d.shape[0], None]).sum(1)
    return out, cnt


def tie_fraction_chunked(q, t, K):
    """``tie_fraction`` without the full matrix."""
    return float((kth_chunked(q, t, K)[1] > 1).mean())


def violations_chunked(q, t):
    """``violations`` without the full matrices."""
    lo, hi = boxes(t)
    box_of = np.arange(t.shape[0]) // BOX
    return sum(int((lower_bound(q[r:r + BLOCK], lo, hi)[:, box_of] > d).sum()) for r, d in blocks(q, t))
