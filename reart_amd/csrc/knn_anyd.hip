// reart_amd/csrc/knn_anyd.hip -- K-nearest-neighbour search for points of any dimension D (1 <= D <= REART_MAX_D) and
// any K (1 <= K <= REART_MAX_K_LIST), float32 or float64 (gfx950).
//
// float32: D = 3 keeps the kernels of knn.hip / knn_list.hip; this file serves the other D of knn_points,
// chamferdist._C.knn_points_idx and knn_cuda.KNN (DESIGN.md "K-NN, any D").  float64: every D, D = 3 included, of
// chamferdist._C.knn_points_idx / knn_points (DESIGN.md "K-NN, float64").  The backward (float32 only, as upstream's)
// is knn_bwd_kernel of knn.hip.
//
// Design:
//   * Targets are transposed once into a +INF padded SoA image [N][D][Ppad] (Ppad = P2 rounded up to 64),
//     queries into groups of Q: [N][ceil(P1/Q)][D][Q].  One wave serves one group of Q queries and streams the
//     targets 64 per step in ascending j: lane l holds target j0 + l, reads its D coordinates with coalesced
//     loads, and uses each one for all Q queries.  The Q coordinates of one dimension are wave-uniform and
//     contiguous (scalar loads).  In float32 two queries share one packed-fp32 instruction per operation; gfx950
//     has no packed fp64 VALU, so in float64 every query costs its own v_add_f64 / v_mul_f64 / v_add_f64 per
//     dimension (ka_add).
//   * Each query keeps its K best targets as a sorted key list in LDS (knn_keys.h): 8 B keys in float32, 16 B
//     KeyF64 in float64; Q is sized by that LDS.  A step whose keys are all at or above a query's K-th key costs
//     that query one ballot; otherwise the wave sorts the candidates and merges them into that query's list.
//   * Rounding contract (the oracle's sqdist): d = (((a0-b0)*(a0-b0)) + ((a1-b1)*(a1-b1))) + ..., in the element
//     type, every operation correctly rounded, ascending dimension, no FMA (-ffp-contract=off, no fma builtins).
//     The packed operations round every lane exactly as the scalar ones, and starting the sum from +0 changes
//     nothing (+0 + x = x for x >= +0).  No matrix cores: an MFMA rounds as an fma chain.
#include "common.h"
#include "internal.h"
#include "knn_keys.h"
#include <math.h>

#define KA_DC 16                      // target coordinates a lane holds per chunk of the distance loop

// ---------------------------------------------------------------------------------
// AoS [N][P][D] -> [N][G][D][R] with row j = g * R + r; rows j >= min(len[b], P) hold `pad`.
// Job 0: the targets (G = 1, R = Ppad, pad +INF), job 1: the query groups (R = Q, pad 0).
// ---------------------------------------------------------------------------------
template <class T>
struct KaImageJob {
    const T *src;
    const int64_t *len;               // nullable
    T *dst;
    int P, G, R;
    T pad;
};

template <class T>
__global__ __launch_bounds__(256) void knn_anyd_image_kernel(KaImageJob<T> j0, KaImageJob<T> j1, int D) {
    const KaImageJob<T> jb = blockIdx.z ? j1 : j0;
    const int b = blockIdx.y;
    const size_t per = (size_t)jb.G * D * jb.R;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    const int r = (int)(e % jb.R);
    const int c = (int)((e / jb.R) % D);
    const int g = (int)(e / ((size_t)jb.R * D));
    const int j = g * jb.R + r;
    int n = jb.len ? (int)jb.len[b] : jb.P;
    n = n < jb.P ? n : jb.P;
    jb.dst[(size_t)b * per + e] = j < n ? jb.src[((size_t)b * jb.P + j) * D + c] : jb.pad;
}

// ---------------------------------------------------------------------------------
// What the two element types do differently: the key, and how the squared distances of one target to the Q queries
// of a group are summed.  float32 keeps two queries per f2 and adds them with packed instructions, float64 keeps one
// sum per query.  ka_add takes the Q query coordinates of one dimension and the target's.  The sums are a plain array
// handed to free functions: as members of a struct the same source compiles to other instructions in the D % 16 tail.
// ---------------------------------------------------------------------------------
template <class T>
struct KaType;
template <>
struct KaType<float> {
    typedef u64 Key;
    typedef f2 Sum;
};
template <>
struct KaType<double> {
    typedef KeyF64 Key;
    typedef double Sum;
};

template <int Q>
__device__ __forceinline__ void ka_add(f2 (&s)[Q / 2], const float *qc, float t) {
    const f2 tt = f2{t, t};
#pragma unroll
    for (int p = 0; p < Q / 2; ++p) {
        const f2 dq = ((const f2 *)qc)[p] - tt;
        s[p] = s[p] + dq * dq;
    }
}
template <int Q>
__device__ __forceinline__ void ka_add(double (&s)[Q], const double *qc, double t) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const double dq = qc[q] - t;
        s[q] = s[q] + dq * dq;
    }
}

// the key of query q's distance to target j
template <int Q>
__device__ __forceinline__ u64 ka_key(const f2 (&s)[Q / 2], int q, unsigned j) {
    const float d = (q & 1) ? s[q / 2].y : s[q / 2].x;
    return ((u64)__float_as_uint(d) << 32) | j;
}
template <int Q>
__device__ __forceinline__ KeyF64 ka_key(const double (&s)[Q], int q, unsigned j) {
    return KeyF64{(u64)__double_as_longlong(s[q]), j, 0u};
}

// a key's distance as it is written out (euclidean: knn_cuda's sqrt, float32 only) and its target index
__device__ __forceinline__ float ka_dist(u64 key, int euclidean) {
    float dd = __uint_as_float((unsigned)(key >> 32));
    if (euclidean) dd = sqrtf(dd);
    return dd;
}
__device__ __forceinline__ double ka_dist(KeyF64 key, int) { return __longlong_as_double((long long)key.d); }
__device__ __forceinline__ int64_t ka_index(u64 key) { return (int64_t)(unsigned)key; }
__device__ __forceinline__ int64_t ka_index(KeyF64 key) { return (int64_t)key.j; }

// ---------------------------------------------------------------------------------
// Search: one wave per group of Q queries.  NE = list entries per lane (K <= 64 * NE).  euclidean: float32 only, the
// float64 entry passes 0.  The arguments stay separate: as members of one struct the compiler loads them later and in
// other groups, and that reschedules up to a fifth of a kernel's instructions (profiles/knn_unify_resources.txt).
// ---------------------------------------------------------------------------------
template <class T, int Q, int NE>
__global__ __launch_bounds__(64) void knn_anyd_kernel(const T *__restrict__ qimg, const T *__restrict__ tsoa,
                                                      const int64_t *__restrict__ lenq, const int64_t *__restrict__ lent,
                                                      int P1, int P2, int D, int Ppad, int G, int K, int euclidean,
                                                      int items, T *__restrict__ dists, int64_t *__restrict__ idx) {
    typedef typename KaType<T>::Key Key;
    typedef typename KaType<T>::Sum Sum;
    constexpr int NS = Q * sizeof(T) / sizeof(Sum);                    // sums of a group
    extern __shared__ __attribute__((aligned(16))) unsigned char s_lds[];
    Key *s_keys = (Key *)s_lds;       // Q lists of K keys, then 64 sorted candidates
    const int w = reart_xcd_remap(blockIdx.x, items);
    if (w < 0) return;
    const int lane = threadIdx.x;
    const int b = w / G, i0 = (w % G) * Q;
    int n1 = lenq ? (int)lenq[b] : P1;
    n1 = n1 < P1 ? n1 : P1;
    int n2 = lent ? (int)lent[b] : P2;
    n2 = n2 < P2 ? n2 : P2;
    const int nv = n1 - i0 < 0 ? 0 : (n1 - i0 < Q ? n1 - i0 : Q);     // queries of the group with a list
    Key *cand = s_keys + (size_t)Q * K;
    for (int e = lane; e < Q * K; e += 64) s_keys[e] = kl_none<Key>();
    reart_wave_sync();

    Key thr[Q];                       // each list's K-th key (all-ones while it is not full)
#pragma unroll
    for (int q = 0; q < Q; ++q) thr[q] = kl_none<Key>();
    const T *qg = qimg + (size_t)w * D * Q;                            // [D][Q] of this group, wave-uniform
    const T *tb = tsoa + (size_t)b * D * Ppad + lane;
    const int nsteps = nv ? n2 : 0;
    const int Dc = D - D % KA_DC;
    for (int j0 = 0; j0 < nsteps; j0 += 64) {
        const T *tp = tb + j0;        // < Ppad: the image is padded to a multiple of 64
        Sum s[NS];
#pragma unroll
        for (int p = 0; p < NS; ++p) s[p] = Sum{};
        for (int c0 = 0; c0 < Dc; c0 += KA_DC) {
            T t[KA_DC];
#pragma unroll
            for (int u = 0; u < KA_DC; ++u) t[u] = tp[(size_t)(c0 + u) * Ppad];
#pragma unroll
            for (int u = 0; u < KA_DC; ++u) ka_add<Q>(s, qg + (size_t)(c0 + u) * Q, t[u]);
        }
        for (int c = Dc; c < D; ++c) ka_add<Q>(s, qg + (size_t)c * Q, tp[(size_t)c * Ppad]);
        const unsigned j = (unsigned)(j0 + lane);
        const bool in = (int)j < n2;
        Key key[Q];
        bool acc[Q];
        unsigned pend = 0;            // queries with candidates in this step (wave-uniform)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            key[q] = ka_key<Q>(s, q, j);
            acc[q] = in && q < nv && key[q] < thr[q];
            if (__ballot(acc[q])) pend |= 1u << q;
        }
        while (pend) {
            const int q = __builtin_ctz(pend);
            pend &= pend - 1;
            Key kq = key[0];
            bool aq = acc[0];
#pragma unroll
            for (int r = 1; r < Q; ++r)
                if (q == r) { kq = key[r]; aq = acc[r]; }
            const int c = __popcll(__ballot(aq));
            const Key v = kl_sort64(kl_sel(aq, kq, kl_none<Key>()), lane);   // candidates in lanes [0, c)
            const Key nt = kl_merge<NE>(s_keys + (size_t)q * K, cand, K, v, c, lane);
#pragma unroll
            for (int r = 0; r < Q; ++r)
                if (q == r) thr[r] = nt;
        }
    }

    const int valid = K < n2 ? K : n2;
    const int nrow = P1 - i0 < Q ? P1 - i0 : Q;
    for (int q = 0; q < nrow; ++q) {
        const Key *lst = s_keys + (size_t)q * K;
        T *od = dists + ((size_t)b * P1 + i0 + q) * K;
        int64_t *oi = idx + ((size_t)b * P1 + i0 + q) * K;
        const int vq = q < nv ? valid : 0;
        for (int e = lane; e < K; e += 64) {
            const Key key = lst[e];
            const bool ok = e < vq;
            const T dd = ka_dist(key, euclidean);
            od[e] = ok ? dd : (T)0;
            oi[e] = ok ? ka_index(key) : (int64_t)0;
        }
    }
}

// ---------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------
struct KnnAnydPlan {
    int Q, NE, Ppad, G;
    size_t off_q, lds, total;
};

#ifndef KA_MIN_WAVES_LIST
#define KA_MIN_WAVES_LIST 4096        // K > 1: waves wanted per launch (4 per SIMD) before Q shrinks
#endif

// Q queries per wave: as many as the list LDS allows (<= REART_LDS_DEFAULT_CAP; with the 16 B keys of float64
// K = 1024 gets Q = 2) while the launch keeps enough waves; a target coordinate a lane loads serves Q queries.
// K = 1 is distance-bound: one wave per SIMD (256 CUs x 4) is enough.  K > 1 merges on most early steps, and a merge
// is a chain of dependent cross-lane and LDS operations that only other waves can hide, so it wants
// KA_MIN_WAVES_LIST.  elem, key: bytes per coordinate and per list key.
static int knn_anyd_plan(int N, int P1, int P2, int D, int K, size_t elem, size_t key, KnnAnydPlan *pl) {
    if (N <= 0 || P1 <= 0 || P2 <= 0 || D < 1 || D > REART_MAX_D || K < 1 || K > REART_MAX_K_LIST)
        return REART_ERR_UNSUPPORTED;
    const long want = K > 1 ? KA_MIN_WAVES_LIST : 1024;
    int Q = 8;
    while (Q > 2 && key * ((size_t)Q * K + 64) > REART_LDS_DEFAULT_CAP) Q >>= 1;
    while (Q > 2 && (long)N * reart_div_up(P1, Q) < want) Q >>= 1;
    if ((long)N * reart_div_up(P1, Q) > (1L << 30)) return REART_ERR_UNSUPPORTED;
    pl->Q = Q;
    pl->NE = K <= 64 ? 1 : K <= 128 ? 2 : K <= 256 ? 4 : K <= 512 ? 8 : 16;
    pl->Ppad = (int)reart_align_up((size_t)P2, 64);
    pl->G = reart_div_up(P1, Q);
    pl->off_q = reart_align_up((size_t)N * D * pl->Ppad * elem, 256);
    pl->total = pl->off_q + reart_align_up((size_t)N * pl->G * D * Q * elem, 256);
    pl->lds = key * ((size_t)Q * K + 64);
    return REART_OK;
}

extern "C" size_t reart_knn_points_workspace_bytes_d(int N, int P1, int P2, int D, int K) {
    if (D == 3) return reart_knn_points_workspace_bytes(N, P1, P2, K);
    KnnAnydPlan pl;
    return knn_anyd_plan(N, P1, P2, D, K, sizeof(float), sizeof(u64), &pl) == REART_OK ? pl.total : 0;
}

extern "C" size_t reart_knn_points_workspace_bytes_f64(int N, int P1, int P2, int D, int K) {
    KnnAnydPlan pl;
    return knn_anyd_plan(N, P1, P2, D, K, sizeof(double), sizeof(KeyF64), &pl) == REART_OK ? pl.total : 0;
}

// q [N,P1,D] queries, t [N,P2,D] targets; N, P1, P2 >= 1, 1 <= D <= REART_MAX_D, 1 <= K <= REART_MAX_K_LIST
template <class T>
int reart_knn_anyd_run(const T *q, const T *t, const int64_t *lenq, const int64_t *lent, int N, int P1, int P2, int D,
                       int K, int euclidean, T *dists, int64_t *idx, void *workspace, size_t workspace_bytes,
                       hipStream_t st) {
    typedef void (*Kernel)(const T *, const T *, const int64_t *, const int64_t *, int, int, int, int, int, int, int, int,
                           T *, int64_t *);
#define KA_ROW(Q) {knn_anyd_kernel<T, Q, 1>, knn_anyd_kernel<T, Q, 2>, knn_anyd_kernel<T, Q, 4>, \
                   knn_anyd_kernel<T, Q, 8>, knn_anyd_kernel<T, Q, 16>}
    static const Kernel kernels[3][5] = {KA_ROW(2), KA_ROW(4), KA_ROW(8)};   // [log2 Q - 1][log2 NE]
#undef KA_ROW
    KnnAnydPlan pl;
    const int rc = knn_anyd_plan(N, P1, P2, D, K, sizeof(T), sizeof(typename KaType<T>::Key), &pl);
    if (rc != REART_OK) return rc;
    if (!workspace || workspace_bytes < pl.total) return REART_ERR_INVALID_ARG;
    T *tsoa = (T *)workspace, *qimg = (T *)((char *)workspace + pl.off_q);
    // the query image takes no lengths: its padding rows are zeros, and the search masks them by lenq
    const KaImageJob<T> jt = {t, lent, tsoa, P2, 1, pl.Ppad, (T)INFINITY};
    const KaImageJob<T> jq = {q, nullptr, qimg, P1, pl.G, pl.Q, (T)0};
    const size_t per = (size_t)D * (pl.Ppad > pl.G * pl.Q ? pl.Ppad : pl.G * pl.Q);
    hipLaunchKernelGGL(knn_anyd_image_kernel<T>, dim3((unsigned)((per + 255) / 256), N, 2), dim3(256), 0, st, jt, jq, D);
    REART_CHECK_LAUNCH();
    const int items = N * pl.G;
    hipLaunchKernelGGL(kernels[__builtin_ctz(pl.Q) - 1][__builtin_ctz(pl.NE)], dim3(reart_xcd_grid(items)), dim3(64),
                       pl.lds, st, (const T *)qimg, (const T *)tsoa, lenq, lent, P1, P2, D, pl.Ppad, pl.G, K, euclidean,
                       items, dists, idx);
    REART_CHECK_LAUNCH();
    return REART_OK;
}

template int reart_knn_anyd_run<float>(const float *, const float *, const int64_t *, const int64_t *, int, int, int,
                                       int, int, int, float *, int64_t *, void *, size_t, hipStream_t);
template int reart_knn_anyd_run<double>(const double *, const double *, const int64_t *, const int64_t *, int, int, int,
                                        int, int, int, double *, int64_t *, void *, size_t, hipStream_t);
