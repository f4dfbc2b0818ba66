"""CPU: the numpy restatement tests/knn_ref.py of the float32 D = 3 K-nearest search and its backward is right -- equal to
the C oracle bit for bit on every case of its table at every K = 1 ... 16, and inside its own float64 bounds -- and the case
table discriminates: every injected error (knn_ref.MUTATIONS, BACKWARD_MUTATIONS) changes the result of at least one
(case, K).  The rejecting cases are printed (run with -s).  The two wide cases exist for the launch size of the GPU kernels;
here their first two batch elements are compared, at their own K."""
import numpy as np
import pytest

from tests import knn_ref as R


@pytest.fixture(scope="module")
def refs():
    """name -> KnnRef, built once per case (the wide cases cut to two batch elements)."""
    out = {}
    for name in R.CASES:
        c = R.make_case(name)
        cut = (lambda a: a if a is None else a[:2]) if name in R.WIDE else (lambda a: a)
        out[name] = dict(c, p1=cut(c["p1"]), p2=cut(c["p2"]), lengths1=cut(c["lengths1"]), lengths2=cut(c["lengths2"]))
        out[name]["ref"] = R.KnnRef(out[name]["p1"], out[name]["p2"], out[name]["lengths1"], out[name]["lengths2"])
    return out


@pytest.fixture(scope="module")
def truth(oracle, refs):
    """(name, K) -> the oracle's (dists, idx), computed once."""
    return {(name, K): oracle.knn_points(c["p1"], c["p2"], c["lengths1"], c["lengths2"], K=K)
            for name, c in refs.items() for K in c["Ks"]}


def test_case_table_hits_the_slice_counts_it_names():
    """Each case's (S, L) in the restated plan is the one the table gives, and the restated plan is the library's: its
    workspace query (host code, no device) returns exactly the bytes of that plan, for every list length KK."""
    from reart_amd import _lib

    L = _lib.lib()
    assert set(R.EXPECT_PLAN) == set(R.CASES)
    for name in R.CASES:
        c = R.make_case(name)
        N, P1, P2 = c["p1"].shape[0], c["p1"].shape[1], c["p2"].shape[1]
        assert R.plan(N, P1, P2)[:2] == R.EXPECT_PLAN[name], name
        for K in R.ALL_K:
            assert L.reart_knn_points_workspace_bytes(N, P1, P2, K) == R.plan_workspace_bytes(N, P1, P2, K), (name, K)
    # the steps of the slice count for a small launch, and S = 1 whatever P2 is once waves reach 8192
    assert [R.plan(1, 64, p)[0] for p in (254, 255, 508, 509, 1016, 1017, 2032, 2033)] == [1, 2, 2, 4, 4, 8, 8, 16]
    assert R.plan(128, 4096, 100000)[0] == 1
    # empty_slice: the last slice starts past the last target; ragged_sliced: nine targets sit in the first of 16 slices
    assert 15 * 144 > 2049 > 14 * 144
    # copies: the three copies of a target lie in three different slices
    assert len({0 // 160, 400 // 160, 800 // 160}) == 3 and 399 // 160 != 799 // 160 != 1199 // 160


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_equals_the_oracle(oracle, refs, truth, name):
    c = refs[name]
    for K in c["Ks"]:
        d_ref, i_ref = truth[name, K]
        res = c["ref"].at(K)
        np.testing.assert_array_equal(res.idx, i_ref, err_msg=f"{name} K={K}")
        np.testing.assert_array_equal(res.dists.view(np.uint32), d_ref.view(np.uint32), err_msg=f"{name} K={K}")
        R.check_float64(res, what=f"{name} K={K}")
        # zero fill, asserted and not excluded: rows past lengths1, slots past lengths2
        n1 = c["lengths1"] if c["lengths1"] is not None else [c["p1"].shape[1]] * len(c["p1"])
        n2 = c["lengths2"] if c["lengths2"] is not None else [c["p2"].shape[1]] * len(c["p1"])
        for n in range(len(c["p1"])):
            assert not res.dists[n, n1[n]:].any() and not res.idx[n, n1[n]:].any()
            assert not res.dists[n, :, n2[n]:].any() and not res.idx[n, :, n2[n]:].any()
        if c["lengths1"] is None and c["lengths2"] is None and K <= c["p2"].shape[1]:
            d_e, i_e = oracle.knn_cuda(c["p2"], c["p1"], K, euclidean=True)
            e = c["ref"].at(K, euclidean=True)
            np.testing.assert_array_equal(e.idx, i_e)
            ulp = np.abs(e.dists.view(np.int32).astype(np.int64) - d_e.view(np.int32).astype(np.int64))
            assert ulp.max() <= 1, (name, K, int(ulp.max()))
            R.check_float64(e, euclidean=True, what=f"{name} K={K} euclidean")
            d_s, i_s = oracle.knn_cuda(c["p2"], c["p1"], K, euclidean=False)
            np.testing.assert_array_equal(d_s, d_ref)
            np.testing.assert_array_equal(i_s, i_ref)


def test_knn_ref_function_is_the_class(refs):
    c = refs["ragged"]
    a = R.knn_ref(c["p1"], c["p2"], c["lengths1"], c["lengths2"], 5, euclidean=True)
    b = c["ref"].at(5, euclidean=True)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_lengths2_zero_is_all_zero(oracle):
    """A lengths2 entry of 0 with P2 > 0: the header's answer is all zero, in the restatement and in the oracle."""
    c = R.make_case("s1_last")
    l2 = np.array([0, 254], np.int64)
    for K in (1, 2, 5, 16):
        res = R.knn_ref(c["p1"], c["p2"], None, l2, K)
        d, i = oracle.knn_points(c["p1"], c["p2"], None, l2, K=K)
        assert not res.dists[0].any() and not res.idx[0].any() and res.dists[1, :, :K].all()
        np.testing.assert_array_equal(res.dists, d)
        np.testing.assert_array_equal(res.idx, i)


def _grad_out(name, K, shape):
    return np.random.default_rng(1000 * K + len(name)).normal(size=shape).astype(np.float32)


@pytest.mark.parametrize("name", list(R.SMALL))
def test_backward_restatement_equals_the_oracle(oracle, refs, truth, name):
    c = refs[name]
    for K in c["Ks"]:
        _, idx = truth[name, K]
        g = _grad_out(name, K, idx.shape)
        g1_ref, g2_ref = oracle.knn_points_backward(c["p1"], c["p2"], idx, g, c["lengths1"], c["lengths2"])
        f32 = R.knn_backward_ref(c["p1"], c["p2"], idx, g, c["lengths1"], c["lengths2"])
        np.testing.assert_array_equal(f32.grad_p1.view(np.uint32), g1_ref.view(np.uint32), err_msg=f"{name} K={K}")
        np.testing.assert_array_equal(f32.grad_p2.view(np.uint32), g2_ref.view(np.uint32), err_msg=f"{name} K={K}")
        f64 = R.knn_backward_ref(c["p1"], c["p2"], idx, g, c["lengths1"], c["lengths2"], dtype=np.float64)
        assert (np.abs(f32.grad_p1 - f64.grad_p1) <= R.backward_bound(f64.n_p1, f64.abs_p1)).all(), (name, K)
        assert (np.abs(f32.grad_p2 - f64.grad_p2) <= R.backward_bound(f64.n_p2, f64.abs_p2)).all(), (name, K)
        assert f64.n_p2.sum() == f64.n_p1.sum(), (name, K)                     # every pair lands in exactly one bucket


def _differs(a, b):
    return not (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]))


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_case_table_rejects_forward_mutation(refs, truth, mutate):
    euclid = mutate in ("no_sqrt", "sqrt_fill")
    hits = []
    for name in R.SMALL:
        c = refs[name]
        bad = R.KnnRef(c["p1"], c["p2"], c["lengths1"], c["lengths2"], mutate=mutate, checks=False)
        for K in c["Ks"]:
            d_ref, i_ref = truth[name, K]
            if euclid:          # the Euclidean form of the truth: the fp32 sqrt of the oracle's squared distances, zeros kept
                d_ref = np.sqrt(d_ref)
            got = bad.at(K, euclidean=euclid)
            if _differs((got.dists, got.idx), (d_ref, i_ref)):
                hits.append((name, K))
    per_case = {}
    for name, K in hits:
        per_case.setdefault(name, []).append(K)
    print(f"\n[{mutate}] rejected by {len(hits)} (case, K): " + "; ".join(f"{n} K={ks}" for n, ks in per_case.items()))
    assert hits, f"no (case, K) of the table tells `{mutate}` from the truth: add a case"


@pytest.mark.parametrize("mutate", R.BACKWARD_MUTATIONS)
def test_case_table_rejects_backward_mutation(oracle, refs, truth, mutate):
    hits = []
    for name in R.SMALL:
        c = refs[name]
        for K in (1, 3, 5, 8, 16):
            _, idx = truth[name, K]
            g = _grad_out(name, K, idx.shape)
            ref = oracle.knn_points_backward(c["p1"], c["p2"], idx, g, c["lengths1"], c["lengths2"])
            bad = R.knn_backward_ref(c["p1"], c["p2"], idx, g, c["lengths1"], c["lengths2"], mutate=mutate)
            if not (np.array_equal(bad.grad_p1.view(np.uint32), ref[0].view(np.uint32))
                    and np.array_equal(bad.grad_p2.view(np.uint32), ref[1].view(np.uint32))):
                hits.append((name, K))
    per_case = {}
    for name, K in hits:
        per_case.setdefault(name, []).append(K)
    print(f"\n[{mutate}] rejected by {len(hits)} (case, K): " + "; ".join(f"{n} K={ks}" for n, ks in per_case.items()))
    assert hits, f"no (case, K) of the table tells `{mutate}` from the truth: add a case"
