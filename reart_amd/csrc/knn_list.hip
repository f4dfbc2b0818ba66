// reart_amd/csrc/knn_list.hip -- K-nearest-neighbour search for 16 < K <= REART_MAX_K_LIST (gfx950).
//
// The K <= 16 kernels of knn.hip keep each query's list in registers; this file serves the larger K of
// knn_points(K=...) and knn_cuda.KNN(k) (DESIGN.md "K-NN, large K").
//
// Design:
//   * One wave per query, four queries per workgroup.  The query's K best targets so far are a sorted
//     list of K 64-bit keys in LDS, key = (bits of the fp32 distance) << 32 | j (knn_keys.h).
//   * Targets stream 64 per step in ascending j from the SoA image soa_kernel builds (one coalesced load
//     per coordinate).  A lane's target is a candidate when its key is below the list's K-th key, which
//     every lane reads from the same LDS word.  A step without candidates costs one ballot; otherwise the
//     wave sorts its <= 64 candidates (bitonic, across lanes) and merges them into the list (kl_merge).
//   * Rounding contract as knn.hip: d = ((dx*dx)+(dy*dy))+(dz*dz), fp32, no FMA (-ffp-contract=off).
//     The result is the list order, so it does not depend on scheduling: no atomics, no cross-wave state.
#include "common.h"
#include "internal.h"
#include "knn_keys.h"
#include <math.h>

#define KL_BS 256                     // four waves, four queries per workgroup
#define KL_WAVES (KL_BS / 64)

struct KnnListArgs {
    const float *q;                   // [N,P1,3] queries
    const float *tsoa;                // [N,3,Ppad] SoA targets
    const int64_t *lenq, *lent;       // nullable
    int N, P1, P2, Ppad, K, euclidean;
    float *dists;                     // [N,P1,K]
    int64_t *idx;                     // [N,P1,K]
};

// NE = list entries per lane (K <= 64 * NE)
template <int NE>
__global__ __launch_bounds__(KL_BS) void knn_list_kernel(KnnListArgs a) {
    extern __shared__ u64 s_keys[];   // per wave: list [K], sorted candidates [64]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long w = (long)blockIdx.x * KL_WAVES + wv;   // query (b, i) = (w / P1, w % P1)
    if (w >= (long)a.N * a.P1) return;                 // whole wave
    const int K = a.K;
    const int b = (int)(w / a.P1), i = (int)(w % a.P1);
    u64 *lst = s_keys + (size_t)wv * (K + 64);
    u64 *cand = lst + K;
    const int n1 = a.lenq ? (int)a.lenq[b] : a.P1;
    int n2 = a.lent ? (int)a.lent[b] : a.P2;
    n2 = n2 < a.P2 ? n2 : a.P2;
    float *od = a.dists + (size_t)w * K;
    int64_t *oi = a.idx + (size_t)w * K;
    if (i >= n1) {
        for (int e = lane; e < K; e += 64) { od[e] = 0.f; oi[e] = 0; }
        return;
    }
#pragma unroll
    for (int u = 0; u < NE; ++u)
        if (lane + 64 * u < K) lst[lane + 64 * u] = ~0ull;
    reart_wave_sync();

    const float *qp = a.q + (size_t)w * 3;
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    const float *tx = a.tsoa + (size_t)b * 3 * a.Ppad, *ty = tx + a.Ppad, *tz = ty + a.Ppad;
    u64 thr = ~0ull;                  // the list's K-th key (all-ones while it is not full)
    for (int j0 = 0; j0 < n2; j0 += 64) {
        const int j = j0 + lane;      // < Ppad: the image is padded to a multiple of 64
        const float d = reart_sqdist3(qx, qy, qz, tx[j], ty[j], tz[j]);
        const u64 key = ((u64)__float_as_uint(d) << 32) | (unsigned)j;
        const bool acc = j < n2 && key < thr;
        const u64 m = __ballot(acc);
        if (!m) continue;
        const int c = __popcll(m);
        const u64 v = kl_sort64(acc ? key : ~0ull, lane);   // candidates in lanes [0, c)
        thr = kl_merge<NE>(lst, cand, K, v, c, lane);
    }

    const int valid = K < n2 ? K : n2;
#pragma unroll
    for (int u = 0; u < NE; ++u) {
        const int e = lane + 64 * u;
        if (e < K) {
            const u64 key = lst[e];
            const bool ok = e < valid;
            float dd = __uint_as_float((unsigned)(key >> 32));
            if (a.euclidean) dd = sqrtf(dd);
            od[e] = ok ? dd : 0.0f;
            oi[e] = ok ? (int64_t)(unsigned)key : (int64_t)0;
        }
    }
}

// ---------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------
static int kl_ppad(int P2) { return (int)reart_align_up((size_t)P2, 64); }

size_t reart_knn_list_workspace_bytes(int N, int P1, int P2, int K) {
    if (N <= 0 || P1 <= 0 || P2 <= 0 || K <= REART_MAX_K || K > REART_MAX_K_LIST) return 0;
    return reart_align_up((size_t)N * 3 * kl_ppad(P2) * sizeof(float), 256);
}

template <int NE>
static void knn_list_launch(const KnnListArgs &a, size_t lds, hipStream_t st) {
    const long queries = (long)a.N * a.P1;
    hipLaunchKernelGGL(knn_list_kernel<NE>, dim3((unsigned)((queries + KL_WAVES - 1) / KL_WAVES)), dim3(KL_BS), lds,
                       st, a);
}

// q [N,P1,3] queries, t [N,P2,3] targets, P1, P2 >= 1, REART_MAX_K < K <= REART_MAX_K_LIST
int reart_knn_list_run(const float *q, const float *t, const int64_t *lenq, const int64_t *lent, int N, int P1,
                       int P2, int K, int euclidean, float *dists, int64_t *idx, void *workspace,
                       size_t workspace_bytes, hipStream_t st) {
    const size_t need = reart_knn_list_workspace_bytes(N, P1, P2, K);
    if (!need) return REART_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < need) return REART_ERR_INVALID_ARG;
    const int Ppad = kl_ppad(P2);
    SoaArgs sa;
    sa.job[0].src = t; sa.job[0].len = lent; sa.job[0].dst = (float *)workspace;
    sa.job[0].P = P2; sa.job[0].Ppad = Ppad;
    sa.job[1] = sa.job[0];
    int rc = reart_soa_launch(sa, Ppad, N, 1, st);
    if (rc != REART_OK) return rc;
    KnnListArgs a;
    a.q = q; a.tsoa = (const float *)workspace; a.lenq = lenq; a.lent = lent;
    a.N = N; a.P1 = P1; a.P2 = P2; a.Ppad = Ppad; a.K = K; a.euclidean = euclidean;
    a.dists = dists; a.idx = idx;
    const size_t lds = sizeof(u64) * (size_t)KL_WAVES * (K + 64);   // <= 34 KiB at K = 1024
    if (K <= 64) knn_list_launch<1>(a, lds, st);
    else if (K <= 128) knn_list_launch<2>(a, lds, st);
    else if (K <= 256) knn_list_launch<4>(a, lds, st);
    else if (K <= 512) knn_list_launch<8>(a, lds, st);
    else knn_list_launch<16>(a, lds, st);
    REART_CHECK_LAUNCH();
    return REART_OK;
}
