"""Plain numpy restatement of the float32, D = 3 K-nearest search and its backward (include/reart_hip.h:
reart_knn_points_idx, reart_knn_cuda, reart_knn_points_backward), and the case table of the K = 1 ... 16 tests.

Forward contract: d = ((dx*dx) + (dy*dy)) + (dz*dz) with dc = p1[c] - p2[c], every operation one fp32 rounding (numpy's
elementwise operations never contract to FMA); neighbours ascending by (distance, index) -- a stable argsort of the
distances; rows at or past lengths1[n] and slots at or past lengths2[n] are zero.  The Euclidean form takes the fp32 sqrt
of the squared distances.

Two float64 checks come with every result:
  * d64: the float64 sum of squares of the contract's fp32 differences, for every returned pair.  The fp32 value is that
    sum after three roundings of non-negative terms (a product, then two sums, on the longest chain), each of relative
    size below 2^-24, so |d32 - d64| <= 3 * 2^-24 * d64 (EPS_SQ).  The sqrt adds one rounding and halves the error of its
    argument: 4 * 2^-24 (EPS_EUCLID) is kept for the Euclidean form.
  * set_ok: d32 of every returned pair <= d32 of every other pair, hence d64(other) * (1 + EPS_SQ) >= d64(returned) *
    (1 - EPS_SQ): the returned set is the float64 K-nearest set up to pairs closer together than that bound.

The `mutate=` switches make the restatement wrong in one specific way each (MUTATIONS, BACKWARD_MUTATIONS); they exist so
that tests/test_knn_ref_cpu.py can show that the case table tells every one of them from the truth.  Several of them need
the launch plan of csrc/knn.hip (slice count S, slice length L, the list length KK that K is rounded up to), restated in
`plan`; the CPU test checks that restatement against the library's own workspace query.

Backward contract: v = (2 g) * diff in fp32, grad_p1[n, i] = sum of v over k ascending, grad_p2[n, j] = minus the sum of v
over its pairs in ascending (i, k), pairs with i >= lengths1[n] or k >= min(K, lengths2[n]) left out.  The float64 form also
returns, per entry, the number of addends and sum |v|: the fp32 form differs from it by at most (addends + 2) * 2^-23 *
sum |v| (two roundings in each v -- the difference and the product -- and one per addition, 2^-24 each, with a factor 2
to spare for the second-order terms).

CASES: name -> builder of dict(p1, p2, lengths1, lengths2, Ks); every array is seeded per case and read-only.  N, P1, P2:
  one            1, 1, 1        K > P2 for every K > 1
  s1_last        2, 65, 254     largest P2 with one slice; query tail lanes
  s2_first       2, 63, 255     first P2 with S = 2        s4_first   1, 130, 509    S = 4
  s8_first       1, 64, 1017    S = 8                      s16_first  1, 130, 2033   S = 16
  empty_slice    1, 64, 2049    L = 144: the 16th slice starts at 2160 and holds padding only
  copies         1, 500, 1200   400 targets stored three times (L = 160: the copies fall in different slices), 200 queries
                                are exact hits
  collisions     1, 300, 600    coordinates 1024 + k * 2^-13, k in 0 .. 5: distinct targets collide in fp32 distance
  block_ties     1, 64, 400     S = 2, L = 208: one copy of the point the queries sit at and around in every block of 8,
                                26 tied blocks in the first slice -- added to the table so that a tie between blocks
                                is also decided at the list lengths 16 > 8 (`block_tie_later` at K = 9 ... 16)
  origin         2, 100, 300    queries at and around (0, 0, 0): a zero pad value would win there
  ragged         4, 200, 700    lengths1 = [200, 17, 0, 64], lengths2 = [700, 5, 1, 333]
  ragged_sliced  2, 70, 2049    lengths2 = [2049, 9]: fifteen slices of padding for the second element
  wide_s1        128, 4096, 300 waves = 8192 -> S = 1 with P2 > 254 (K in {2, 16} only)
  wide_s2        64, 4096, 600  waves = 4096 -> S = 2 where a small launch has S = 4 (K = 5 only)
The two wide cases keep the sizes the table gives: the C oracle needs well under a second for either on 16 CPUs."""
import collections
import functools

import numpy as np

MAX_K = 16
EPS_SQ = 3.0 * 2.0 ** -24
EPS_EUCLID = 4.0 * 2.0 ** -24
F32 = np.float32

MUTATIONS = ("merge_le", "block_tie_later", "fma", "pad_zero", "ignore_lengths2", "keep_rows", "fill_kk",
             "drop_short_last", "no_sqrt", "sqrt_fill")
BACKWARD_MUTATIONS = ("ki_order", "k_past_lengths2", "rows_past_lengths1")

KnnResult = collections.namedtuple("KnnResult", "dists idx d64 set_ok")
KnnGrad = collections.namedtuple("KnnGrad", "grad_p1 grad_p2 abs_p1 abs_p2 n_p1 n_p2")


# ---- the launch plan of csrc/knn.hip (knn_round_k, knn_pick_split, knn_plan) ----------------------------------------------
def round_k(K):
    return next(o for o in (1, 2, 3, 4, 8, 16) if K <= o)


def plan(N, P1, P2, K=1):
    """-> (S slices, L targets per slice, KK list length)."""
    waves, S = N * -(-P1 // 64), 1
    while waves * S < 8192 and S < 16:
        S *= 2
    while S > 1 and -(-P2 // S) < 128:
        S //= 2
    L = -(-(-(-P2 // S)) // 16) * 16
    return S, L, round_k(K)


def plan_workspace_bytes(N, P1, P2, K):
    """What reart_knn_points_workspace_bytes must return for that plan: the SoA image and, for S > 1, the partial lists."""
    S, L, KK = plan(N, P1, P2, K)
    al = lambda b: -(-b // 256) * 256
    return al(N * 3 * L * S * 4) + (2 * al(S * N * P1 * KK * 4) if S > 1 else 0)


# ---- forward --------------------------------------------------------------------------------------------------------------
def _diffs(q, t):
    return [q[:, None, c] - t[None, :, c] for c in range(3)]         # fp32, one rounding each


def _dist32(dx, dy, dz, fma=False):
    if not fma:
        return (dx * dx + dy * dy) + dz * dz
    # fma(dz, dz, fma(dy, dy, dx * dx)): the products of two fp32 numbers are exact in float64
    s = (dx * dx).astype(np.float64)
    s = (s + dy.astype(np.float64) * dy.astype(np.float64)).astype(F32).astype(np.float64)
    return (s + dz.astype(np.float64) * dz.astype(np.float64)).astype(F32)


class KnnRef:
    """The ranked neighbour lists of one problem, computed once; `at(K)` cuts the K-column result out of them."""

    def __init__(self, p1, p2, lengths1=None, lengths2=None, mutate=None, checks=True):
        assert mutate is None or mutate in MUTATIONS, mutate
        assert p1.dtype == F32 and p2.dtype == F32 and p1.shape[2] == 3 and p2.shape[2] == 3
        self.p1, self.p2, self.mutate, self.checks = p1, p2, mutate, checks
        self.N, self.P1, self.P2 = p1.shape[0], p1.shape[1], p2.shape[1]
        clamp = lambda l, P: [P] * self.N if l is None else [max(0, min(int(v), P)) for v in l]
        self.n1, self.n2 = clamp(lengths1, self.P1), clamp(lengths2, self.P2)
        if mutate == "ignore_lengths2":
            self.n2 = [self.P2] * self.N
        self.S, self.L, _ = plan(self.N, self.P1, self.P2)
        self._lists = {}

    def _ranked(self, n, KK):
        """-> (ld f32 [rows, 16], li i64 [rows, 16], l64 f64 [rows, 16], rest64 f64 [rows]): the 16 best pairs of every row
        ascending by (distance, index), (+INF, 0) where there are fewer; their float64 distances; the smallest float64
        distance among all other pairs.  KK matters to `block_tie_later` only."""
        key = (n, KK if self.mutate == "block_tie_later" else 0)
        if key in self._lists:
            return self._lists[key]
        m, L, S = self.mutate, self.L, self.S
        rows = self.P1 if m == "keep_rows" else self.n1[n]
        n2 = self.n2[n]
        t = self.p2[n, :n2]
        if m == "pad_zero":                             # the padding of the SoA image takes part as points at the origin
            t = np.concatenate([t, np.zeros((L * S - n2, 3), F32)])
        if m == "drop_short_last" and n2 > 0:           # the slice that holds the last target, if it holds under 16
            first = (n2 - 1) // L * L
            if n2 - first < 16:
                t = t[:first]
        nc = t.shape[0]
        dx, dy, dz = _diffs(self.p1[n, :rows], t)
        D = _dist32(dx, dy, dz, fma=(m == "fma"))
        j = np.broadcast_to(np.arange(nc), D.shape)
        if m == "merge_le":                             # among equal distances a later slice goes first
            order = np.lexsort((j, -(j // L), D), axis=-1)
        elif m == "block_tie_later":                    # per slice the KK best blocks of 8 by (minimum, LATER block first)
            pad = np.full((rows, L * S - nc), np.inf, F32)
            Dp = np.concatenate([D, pad], axis=1)
            bm = Dp.reshape(rows, S, L // 8, 8).min(-1)
            bid = np.broadcast_to(np.arange(L // 8), bm.shape)
            best = np.lexsort((-bid, bm), axis=-1)[..., :KK]
            keep = np.zeros(bm.shape, bool)
            np.put_along_axis(keep, best, True, axis=-1)
            keep = np.repeat(keep.reshape(rows, S * (L // 8)), 8, axis=1)[:, :nc]
            order = np.argsort(np.where(keep, D, F32(np.inf)), axis=-1, kind="stable")
            D = np.where(keep, D, F32(np.inf))
        else:
            order = np.argsort(D, axis=-1, kind="stable")
        top = order[:, :MAX_K]
        ld = np.full((rows, MAX_K), np.inf, F32)
        li = np.zeros((rows, MAX_K), np.int64)
        l64 = np.full((rows, MAX_K), np.inf)
        rest64 = np.full((rows,), np.inf)
        w = top.shape[1]
        ld[:, :w] = np.take_along_axis(D, top, -1)
        li[:, :w] = np.where(np.isfinite(ld[:, :w]), top, 0)
        if self.checks:
            D64 = dx.astype(np.float64) ** 2 + dy.astype(np.float64) ** 2 + dz.astype(np.float64) ** 2
            l64[:, :w] = np.take_along_axis(D64, top, -1)
            if nc > w:
                np.put_along_axis(D64, top, np.inf, -1)
                rest64 = D64.min(-1)
        self._lists[key] = (ld, li, l64, rest64)
        return self._lists[key]

    def at(self, K, euclidean=False):
        assert 1 <= K <= MAX_K
        m, KK = self.mutate, round_k(K)
        dists = np.zeros((self.N, self.P1, K), F32)
        idx = np.zeros((self.N, self.P1, K), np.int64)
        d64 = np.zeros((self.N, self.P1, K))
        set_ok = np.ones((self.N, self.P1), bool)
        for n in range(self.N):
            ld, li, l64, rest64 = self._ranked(n, KK)
            rows = ld.shape[0]
            valid = min(K, self.n2[n])
            if m == "fill_kk" and K < KK:               # the clamp forgotten: every written slot keeps its list entry
                valid = K
            d = ld[:, :valid]
            if euclidean and m != "no_sqrt":
                d = np.sqrt(d)
            dists[n, :rows, :valid] = d
            idx[n, :rows, :valid] = li[:, :valid]
            if m == "sqrt_fill" and euclidean:          # the sqrt of the list entry, +INF, where zero belongs
                dists[n, :rows, valid:] = np.sqrt(ld[:, valid:K])
            d64[n, :rows, :valid] = l64[:, :valid]
            if self.checks and valid > 0 and rows > 0:
                other = np.minimum(l64[:, valid:].min(-1, initial=np.inf), rest64)
                set_ok[n, :rows] = other * (1 + EPS_SQ) >= l64[:, :valid].max(-1) * (1 - EPS_SQ)
        return KnnResult(dists, idx, d64, set_ok)


def knn_ref(p1, p2, lengths1, lengths2, K, euclidean=False, mutate=None):
    """p1 [N,P1,3], p2 [N,P2,3] float32, lengths [N] or None -> KnnResult(dists f32 [N,P1,K], idx i64 [N,P1,K], d64, set_ok).
    A sweep over K builds one KnnRef and calls `at` instead."""
    return KnnRef(p1, p2, lengths1, lengths2, mutate=mutate).at(K, euclidean=euclidean)


def check_float64(res, euclidean=False, what=""):
    """The two float64 checks of a KnnResult (module docstring)."""
    ref = np.sqrt(res.d64) if euclidean else res.d64
    eps = EPS_EUCLID if euclidean else EPS_SQ
    err = np.abs(res.dists.astype(np.float64) - ref)
    assert (err <= eps * ref).all(), (what, float((err / np.maximum(ref, 1e-300)).max()), eps)
    assert res.set_ok.all(), (what, np.argwhere(~res.set_ok)[:4].tolist())


# ---- backward -------------------------------------------------------------------------------------------------------------
def knn_backward_ref(p1, p2, idx, grad_dists, lengths1=None, lengths2=None, dtype=np.float32, mutate=None):
    """-> KnnGrad.  dtype float32: the documented order of additions, every operation one fp32 rounding (abs_* and n_* are
    None).  dtype float64: the same sums in float64 with abs_p1 / abs_p2 = sum |v| and n_p1 / n_p2 = addends per entry."""
    assert mutate is None or mutate in BACKWARD_MUTATIONS, mutate
    dt = np.dtype(dtype)
    N, P1, _ = p1.shape
    P2, K = p2.shape[1], idx.shape[2]
    g1, g2 = np.zeros(p1.shape, dt), np.zeros(p2.shape, dt)
    want = dt == np.float64
    a1, a2 = (np.zeros(p1.shape), np.zeros(p2.shape)) if want else (None, None)
    c1, c2 = (np.zeros(p1.shape[:2], np.int64), np.zeros(p2.shape[:2], np.int64)) if want else (None, None)
    for n in range(N):
        n1 = P1 if lengths1 is None or mutate == "rows_past_lengths1" else max(0, min(int(lengths1[n]), P1))
        n2 = P2 if lengths2 is None else max(0, min(int(lengths2[n]), P2))
        kk = K if mutate == "k_past_lengths2" else min(K, n2)
        if n1 == 0 or kk == 0:
            continue
        j = idx[n, :n1, :kk]
        x, y = p1[n, :n1].astype(dt), p2[n].astype(dt)
        v = (dt.type(2) * grad_dists[n, :n1, :kk].astype(dt))[..., None] * (x[:, None, :] - y[j])     # [n1, kk, 3]
        for k in range(kk):                                                                           # k ascending
            g1[n, :n1] = g1[n, :n1] + v[:, k]
        # buckets: the pairs e = (i, k) of a target in ascending (i, k); round r adds the r-th pair of every bucket
        ii, kq = np.divmod(np.arange(n1 * kk), kk)
        jf, vf = j.reshape(-1), v.reshape(-1, 3)
        by_target = np.lexsort((ii, kq, jf)) if mutate == "ki_order" else np.argsort(jf, kind="stable")
        js = jf[by_target]
        start = np.searchsorted(js, js, side="left")
        rank = np.arange(js.size) - start
        for r in range(int(rank.max()) + 1):
            sel = by_target[rank == r]
            g2[n, jf[sel]] = g2[n, jf[sel]] - vf[sel]
        if want:
            a1[n, :n1] = np.abs(v).sum(1)
            c1[n, :n1] = kk
            np.add.at(a2[n], jf, np.abs(vf))
            np.add.at(c2[n], jf, 1)
    return KnnGrad(g1, g2, a1, a2, c1, c2)


def backward_bound(n_addends, abs_sum):
    """Per-entry bound between the fp32 and the float64 form (module docstring)."""
    return (n_addends[..., None] + 2) * 2.0 ** -23 * abs_sum


# ---- the case table -------------------------------------------------------------------------------------------------------
ALL_K = tuple(range(1, MAX_K + 1))


def _uniform(seed, N, P1, P2, scale=0.35):
    rng = np.random.default_rng(seed)
    return rng.uniform(-scale, scale, (N, P1, 3)).astype(F32), rng.uniform(-scale, scale, (N, P2, 3)).astype(F32)


def _plain(seed, N, P1, P2, Ks=ALL_K):
    def build():
        a, b = _uniform(seed, N, P1, P2)
        return dict(p1=a, p2=b, lengths1=None, lengths2=None, Ks=Ks)
    return build


def _copies():
    rng = np.random.default_rng(108)
    base = rng.uniform(-1, 1, (1, 400, 3)).astype(F32)
    b = np.concatenate([base, base, base], axis=1)
    a = rng.uniform(-1, 1, (1, 500, 3)).astype(F32)
    a[0, 150:350] = base[0, rng.permutation(400)[:200]]                   # exact hits: distance 0, three times each
    return dict(p1=a, p2=b, lengths1=None, lengths2=None, Ks=ALL_K)


def _collisions():
    rng = np.random.default_rng(109)
    lat = lambda n: (1024.0 + rng.integers(0, 6, (1, n, 3)) * 2.0 ** -13).astype(F32)
    return dict(p1=lat(300), p2=lat(600), lengths1=None, lengths2=None, Ks=ALL_K)


def _block_ties():
    rng = np.random.default_rng(115)
    c = np.array([0.25, -0.125, 0.5], F32)
    b = rng.uniform(-1, 1, (1, 400, 3)).astype(F32)
    near = np.linalg.norm(b[0] - c, axis=1) < 0.3
    b[0, near] += np.array([0.0, 0.0, -1.0], F32)                         # every other target is far from c
    b[0, 3::8] = c                                                        # one copy of c in every block of 8
    a = (c + rng.uniform(-0.01, 0.01, (1, 64, 3))).astype(F32)
    a[0, :8] = c
    return dict(p1=a, p2=b, lengths1=None, lengths2=None, Ks=ALL_K)


def _origin():
    a, b = _uniform(110, 2, 100, 300)
    rng = np.random.default_rng(1110)
    a[:, :10] = 0.0
    a[:, 10:30] = rng.uniform(-1e-3, 1e-3, (2, 20, 3)).astype(F32)
    return dict(p1=a, p2=b, lengths1=None, lengths2=None, Ks=ALL_K)


def _ragged():
    a, b = _uniform(111, 4, 200, 700)
    return dict(p1=a, p2=b, lengths1=np.array([200, 17, 0, 64], np.int64), lengths2=np.array([700, 5, 1, 333], np.int64),
                Ks=ALL_K)


def _ragged_sliced():
    a, b = _uniform(112, 2, 70, 2049)
    return dict(p1=a, p2=b, lengths1=None, lengths2=np.array([2049, 9], np.int64), Ks=ALL_K)


CASES = {
    "one": _plain(101, 1, 1, 1),
    "s1_last": _plain(102, 2, 65, 254),
    "s2_first": _plain(103, 2, 63, 255),
    "s4_first": _plain(104, 1, 130, 509),
    "s8_first": _plain(105, 1, 64, 1017),
    "s16_first": _plain(106, 1, 130, 2033),
    "empty_slice": _plain(107, 1, 64, 2049),
    "copies": _copies,
    "collisions": _collisions,
    "block_ties": _block_ties,
    "origin": _origin,
    "ragged": _ragged,
    "ragged_sliced": _ragged_sliced,
    "wide_s1": _plain(113, 128, 4096, 300, Ks=(2, 16)),
    "wide_s2": _plain(114, 64, 4096, 600, Ks=(5,)),
}
WIDE = ("wide_s1", "wide_s2")
SMALL = tuple(c for c in CASES if c not in WIDE)
# (S, L) each case is in the table for
EXPECT_PLAN = {"one": (1, 16), "s1_last": (1, 256), "s2_first": (2, 128), "s4_first": (4, 128), "s8_first": (8, 128),
               "s16_first": (16, 128), "empty_slice": (16, 144), "copies": (8, 160), "collisions": (4, 160),
               "block_ties": (2, 208),
               "origin": (2, 160), "ragged": (4, 176), "ragged_sliced": (16, 144), "wide_s1": (1, 304), "wide_s2": (2, 304)}


@functools.lru_cache(maxsize=None)
def make_case(name):
    case = CASES[name]()
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    case["name"] = name
    return case


def cases_for(K, names=None):
    return [make_case(c) for c in (names or CASES) if K in make_case(c)["Ks"]]
