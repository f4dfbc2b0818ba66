"""Restatement of reart_connection_select / reart_connection_term (csrc/connection_term.hip; networks/loss.py
compute_connection_loss :60-78 of the reference) in numpy.  It imports nothing of reart_amd and reads nothing outside the
repository.

The SELECTION is restated in float32 with the kernel's rounding, d = ((dx*dx) + (dy*dy)) + (dz*dz), every operation rounded
once, and its rules: the neighbour of a source is the lowest target index attaining the minimum; the k sources of an edge are
the k smallest keys (bits of d, source index), ascending.  It is exact: the tables of the kernel must equal it.
VALUE and GRADIENT are restated in float64 on the float32 inputs.

`assert_tie_free` is what makes a case comparable with the composition compute_connection_loss(..., ChamferDistance(), k),
whose search and topk leave ties open: for every selected source the nearest and the second-nearest target distance differ, and
the k-th and the (k+1)-th source key have distinct distances.  `case()` asserts it for every case marked `compose`, so a bad
seed fails in the CPU test."""
import functools
import os

import numpy as np

from tests.structure_loss_ref import GRAD_TOL, VALUE_TOL  # noqa: F401  (the bounds of both tests)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sqdist(a, b):
    """[n,3] x [m,3] float32 -> [n,m] float32 in the kernel's order of operations."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = a[:, None, :] - b[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _edge(cano, seg, a, b, P, k):
    """-> (valid, source indices [na], their distance [na] float32, their neighbour [na], the full matrix or None)"""
    none = (False, None, None, None, None)
    if not (0 <= a < P and 0 <= b < P):
        return none
    A, B = np.flatnonzero(seg == a), np.flatnonzero(seg == b)
    if len(A) < k or len(B) < 1:
        return none
    D = sqdist(cano[A], cano[B])
    nn = D.argmin(1)                                     # first minimum: B ascends, the lowest index
    return True, A, D[np.arange(len(A)), nn], B[nn], D


def select(cano, seg, pairs, P, k):
    """-> dict(src [E,k] int32, tgt [E,k] int32, dist [E,k] float32, valid [E] bool)"""
    cano, seg = np.asarray(cano, np.float32), np.asarray(seg, np.int64)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    E = len(pairs)
    out = dict(src=np.zeros((E, k), np.int32), tgt=np.zeros((E, k), np.int32), dist=np.zeros((E, k), np.float32),
               valid=np.zeros(E, bool))
    for e, (a, b) in enumerate(pairs):
        ok, A, d, t, _ = _edge(cano, seg, int(a), int(b), P, k)
        if not ok:
            continue
        order = np.lexsort((A, d.view(np.uint32)))[:k]   # keys (bits of d, i): d >= +0, so bit order is value order
        out["src"][e], out["tgt"][e], out["dist"][e], out["valid"][e] = A[order], t[order], d[order], True
    return out


def assert_tie_free(cano, seg, pairs, P, k):
    """-> the smallest gaps met (second neighbour, (k+1)-th key), for the record."""
    cano, seg = np.asarray(cano, np.float32), np.asarray(seg, np.int64)
    gap_nn, gap_k = np.inf, np.inf
    for e, (a, b) in enumerate(np.asarray(pairs, np.int64).reshape(-1, 2)):
        ok, A, d, _, D = _edge(cano, seg, int(a), int(b), P, k)
        assert ok, f"edge {e}: invalid, the composition raises"
        order = np.lexsort((A, d.view(np.uint32)))
        if D.shape[1] > 1:
            two = np.partition(D[order[:k]], 1, axis=1)[:, :2]
            assert (two[:, 0] < two[:, 1]).all(), f"edge {e}: a selected source has two nearest targets"
            gap_nn = min(gap_nn, float((two[:, 1] - two[:, 0]).min()))
        if len(A) > k:
            assert d[order[k - 1]] < d[order[k]], f"edge {e}: the k-th and the (k+1)-th source are equally far"
            gap_k = min(gap_k, float(d[order[k]] - d[order[k - 1]]))
    return gap_nn, gap_k


def term(pc, src, tgt, valid, k, weight=1.0):
    """float64 -> dict(loss, edge_cost [E], grad [T,N,3])"""
    p = np.asarray(pc, np.float32).astype(np.float64)
    src, tgt, valid = np.asarray(src, np.int64), np.asarray(tgt, np.int64), np.asarray(valid, bool)
    E = len(valid)
    cost, grad = np.zeros(E), np.zeros_like(p)
    for e in np.flatnonzero(valid):
        diff = p[:, src[e]] - p[:, tgt[e]]               # [T,k,3]
        cost[e] = (diff * diff).sum() / k
        g = (2.0 * weight / k) * diff
        for r in range(k):                               # indices repeat: add one row at a time
            grad[:, src[e, r]] += g[:, r]
            grad[:, tgt[e, r]] -= g[:, r]
    return dict(loss=weight * cost.sum(), edge_cost=cost, grad=grad)


def connection_term(cano, seg, pairs, P, pc, k, weight=1.0):
    s = select(cano, seg, pairs, P, k)
    return dict(term(pc, s["src"], s["tgt"], s["valid"], k, weight), **s)


def compare(got, ref, what=""):
    """Tables and `valid` equal; value within VALUE_TOL relative, edge costs within VALUE_TOL of the largest; the gradient
    tensor within GRAD_TOL of its largest reference entry -> the measured ratios."""
    for key in ("src", "tgt", "valid"):
        if got.get(key) is not None:
            assert np.array_equal(np.asarray(got[key]).astype(np.int64), np.asarray(ref[key]).astype(np.int64)), f"{what}: {key}"
    out = {}
    if got.get("loss") is not None:
        out["loss"] = abs(got["loss"] - ref["loss"]) / abs(ref["loss"]) if ref["loss"] else abs(got["loss"])
        assert out["loss"] <= VALUE_TOL, f"{what}: value {got['loss']!r} against {ref['loss']!r}: {out['loss']:.2e}"
    if got.get("edge_cost") is not None and len(ref["edge_cost"]):
        top = float(np.abs(ref["edge_cost"]).max())
        out["edge_cost"] = float(np.abs(np.asarray(got["edge_cost"], np.float64) - ref["edge_cost"]).max()) / (top if top else 1.0)
        assert out["edge_cost"] <= VALUE_TOL, f"{what}: edge costs off by {out['edge_cost']:.2e}"
    if got.get("grad") is not None:
        g, r = np.asarray(got["grad"], np.float64), ref["grad"]
        assert g.shape == r.shape and np.isfinite(g).all(), what
        top = float(np.abs(r).max())
        out["grad"] = float(np.abs(g - r).max()) / top if top else float(np.abs(g).max())
        assert out["grad"] <= GRAD_TOL, f"{what}: gradient off by {out['grad']:.2e} of max|g| = {top:.3g}"
    return out


# ------------------------------------------------------------------------------------------------------------ cases
def make_case(N, T, k, sizes, edges, outside=(), seed=0, num_parts=None):
    """A random cloud whose part p has sizes[p] points, scattered over the index range; the points left over carry the labels
    of `outside` in turn (labels no part has).  Frames: the cloud plus noise."""
    rng = np.random.default_rng([seed, N, T, k])
    labels = np.concatenate([np.full(s, p, np.int64) for p, s in enumerate(sizes)] + [np.zeros(0, np.int64)])
    rest = N - len(labels)
    assert rest >= 0 and (rest == 0 or len(outside)), (N, len(labels))
    labels = np.concatenate([labels, np.resize(np.asarray(outside, np.int64), rest)]) if rest else labels
    seg = np.empty(N, np.int64)
    seg[rng.permutation(N)] = labels
    cano = rng.uniform(-0.5, 0.5, (N, 3)).astype(np.float32)
    pc = (cano[None] + rng.normal(0.0, 0.05, (T, N, 3))).astype(np.float32)
    return dict(cano=cano, seg=seg, pairs=np.asarray(edges, np.int32).reshape(-1, 2), pc=pc, k=k,
                P=num_parts if num_parts is not None else len(sizes))


def _chain(P):
    return [(p, p + 1) for p in range(P - 1)]


OUT = (-1, 64, 1000, -7, 1 << 40)       # labels outside [0, P) for every P <= 64
# name -> (make_case arguments, compose: comparable with the composition, i.e. every edge valid and tie-free)
CASES = {
    # |src| = k, k+1, 63, 64, 65, 257, 1025, 1500 and |tgt| = 1, 64, 65, 10, 1025; part 6 spills a workgroup of sources and an
    # LDS tile of targets, is a source of two edges and the target of another; N = 4097
    "k10_sizes": (dict(N=4097, T=2, k=10, sizes=(10, 11, 63, 64, 65, 257, 1025, 1, 1025, 1500),
                       edges=[(0, 7), (1, 3), (2, 4), (3, 6), (4, 0), (5, 8), (6, 8), (6, 7), (9, 6)], outside=OUT), True),
    # a chain of P - 1 edges, every inner part source of one edge and target of the next; |src| = k = 1 and k + 1 = 2
    "k1_chain": (dict(N=1500, T=65, k=1, sizes=(1, 2, 63, 64, 65, 257, 1025, 23), edges=_chain(8)), True),
    # k = 64: |src| = k, k + 1 = 65, 257, 1025; all 64 pairs of (4, 5) share one target point
    "k64": (dict(N=4097, T=1, k=64, sizes=(64, 65, 63, 257, 1025, 1, 1025), edges=[(0, 5), (1, 2), (3, 4), (4, 6), (6, 1), (4, 5)],
                 outside=OUT), True),
    "T1024": (dict(N=300, T=1024, k=10, sizes=(100, 100, 100), edges=[(0, 1), (1, 2)]), True),
    "E1": (dict(N=1500, T=2, k=10, sizes=(700, 800), edges=[(1, 0)]), True),
    "E0": (dict(N=1500, T=2, k=10, sizes=(700, 800), edges=[], num_parts=2), False),
    # a star around part 0, an edge listed twice, (a, b) with (b, a), a self edge
    "star_twice_both_self": (dict(N=1500, T=2, k=10, sizes=(300, 200, 250, 150, 350, 250),
                                  edges=[(0, 1), (0, 2), (3, 0), (0, 4), (1, 2), (1, 2), (2, 4), (4, 2), (5, 5)]), False),
    # |src| = k - 1, an empty target part (2), a part number no point carries (5), labels outside [0, P)
    "invalid_edges": (dict(N=512, T=2, k=10, sizes=(9, 100, 0, 100, 50), num_parts=6, outside=OUT,
                           edges=[(0, 1), (1, 2), (1, 3), (5, 1), (3, 5), (3, 4), (4, 1)]), False),
    # the limit: 65 536 points, 64 parts of about 1024
    "N65536_P64": (dict(N=65536, T=1, k=10, sizes=(), outside=tuple(range(64)), num_parts=64, edges=_chain(64), seed=1), False),
}


@functools.lru_cache(maxsize=None)
def case(name):
    args, compose = CASES[name]
    c = make_case(**args)
    if compose:
        assert_tie_free(c["cano"], c["seg"], c["pairs"], c["P"], c["k"])
    return c


@functools.lru_cache(maxsize=None)
def case_ref(name, weight=1.0):
    c = case(name)
    return connection_term(c["cano"], c["seg"], c["pairs"], c["P"], c["pc"], c["k"], weight)


def tie_case():
    """The tie rules on exact coordinates, part 0 -> part 1 with k = 3, and the self edge (0, 0).
    Part 1: points 1 and 4 coincide (the neighbour is 1), point 6 lies far off.  Part 0: points 0 and 2 are mirror images about
    the coincident pair (equal distances 0.25: 0 before 2), point 3 at 1.0, point 5 at distance 0.0625 comes first, point 7 far."""
    cano = np.zeros((8, 3), np.float32)
    seg = np.array([0, 1, 0, 0, 1, 0, 1, 0], np.int64)
    cano[1] = cano[4] = (0.0, 0.0, 0.0)
    cano[6] = (8.0, 0.0, 0.0)
    cano[0], cano[2], cano[3], cano[5], cano[7] = (0.5, 0, 0), (-0.5, 0, 0), (0, 1.0, 0), (0, 0, 0.25), (0, -4.0, 0)
    pc = (cano[None] * np.array([1.0, 1.5], np.float32)[:, None, None] + np.float32(0.125)).astype(np.float32)
    pc[1, 4] += np.float32(0.5)
    expect = dict(src=np.array([[5, 0, 2], [0, 2, 3]], np.int32), tgt=np.array([[1, 1, 1], [0, 2, 3]], np.int32),
                  dist=np.array([[0.0625, 0.25, 0.25], [0, 0, 0]], np.float32), valid=np.array([True, True]))
    return dict(cano=cano, seg=seg, pairs=np.array([(0, 1), (0, 0)], np.int32), pc=pc, k=3, P=2), expect


# ---------------------------------------------------------------------------------------------------------- goldens
def golden_case():
    """The reference's own run on tests/golden/structure.npz: (case, golden entries of loss_terms.npz)."""
    z, g = np.load(os.path.join(GOLD, "structure.npz")), np.load(os.path.join(GOLD, "loss_terms.npz"))
    c = dict(cano=z["cano"], seg=z["new_seg"], pairs=np.asarray(z["new_conn"], np.int32), pc=z["pred"], k=int(g["conn_k"]),
             P=int(z["new_conn"].max()) + 1)
    return c, {k: g["conn_" + k] for k in ("loss", "src", "tgt", "rows", "grad_rows")}


def pair_sets(src, tgt):
    """per edge the sorted (src, tgt) pairs: the selection as a set"""
    return [sorted(zip(s.tolist(), t.tolist())) for s, t in zip(np.asarray(src), np.asarray(tgt))]
