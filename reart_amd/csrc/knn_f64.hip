// reart_amd/csrc/knn_f64.hip -- K-nearest-neighbour search over float64 point clouds, any D (1 <= D <= REART_MAX_D)
// and any K (1 <= K <= REART_MAX_K_LIST) (gfx950).
//
// Serves chamferdist._C.knn_points_idx / knn_points on float64 clouds (DESIGN.md "K-NN, float64"); the float32
// searches of knn.hip / knn_list.hip / knn_dim.hip are separate and unchanged.  There is no float64 backward: the
// upstream backward is float-only, and the autograd wrapper casts to float32 before it.
//
// Design (the any-D search of knn_dim.hip in double):
//   * Targets are transposed once into a +INF padded SoA image [N][D][Ppad] of doubles (Ppad = P2 rounded up to 64),
//     queries into groups of Q: [N][ceil(P1/Q)][D][Q].  One wave serves one group of Q queries and streams the
//     targets 64 per step in ascending j: lane l holds target j0 + l, reads its D coordinates with coalesced loads,
//     and uses each one for all Q queries (the Q query coordinates of one dimension are wave-uniform).  gfx950 has
//     no packed fp64 VALU, so every query costs its own v_add_f64 / v_mul_f64 / v_add_f64 per dimension.
//   * Each query keeps its K best targets as a sorted list of KeyF64 (distance bits, index) in LDS (knn_keys.h),
//     16 B per entry; Q is sized by that LDS.  A step whose keys are all at or above a query's K-th key costs that
//     query one ballot; otherwise the wave sorts the candidates and merges them into that query's list.
//   * Rounding contract: d = (((a0-b0)*(a0-b0)) + ((a1-b1)*(a1-b1))) + ..., fp64, every operation correctly
//     rounded, ascending dimension, no FMA (-ffp-contract=off, no fma builtins).  Starting the sum from +0 changes
//     nothing (+0 + x = x for x >= +0).  No matrix cores: v_mfma_f64_* rounds as an fma chain.
#include "common.h"
#include "knn_keys.h"
#include <math.h>

#define KF_DC 16                      // target coordinates a lane holds per chunk of the distance loop

// ---------------------------------------------------------------------------------
// AoS [N][P][D] -> [N][G][D][R] with row j = g * R + r; rows j >= min(len[b], P) hold `pad`.
// Job 0: the targets (G = 1, R = Ppad, pad +INF), job 1: the query groups (R = Q, pad 0).
// ---------------------------------------------------------------------------------
struct F64ImageJob {
    const double *src;
    const int64_t *len;               // nullable
    double *dst;
    int P, G, R;
    double pad;
};

__global__ __launch_bounds__(256) void knn_f64_image_kernel(F64ImageJob j0, F64ImageJob j1, int D) {
    const F64ImageJob jb = blockIdx.z ? j1 : j0;
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
// Search: one wave per group of Q queries.  NE = list entries per lane (K <= 64 * NE).
// ---------------------------------------------------------------------------------
template <int Q, int NE>
__global__ __launch_bounds__(64) void knn_f64_kernel(const double *__restrict__ qimg, const double *__restrict__ tsoa,
                                                     const int64_t *__restrict__ lenq, const int64_t *__restrict__ lent,
                                                     int P1, int P2, int D, int Ppad, int G, int K, int items,
                                                     double *__restrict__ dists, int64_t *__restrict__ idx) {
    extern __shared__ KeyF64 s_keyd[];   // Q lists of K keys, then 64 sorted candidates
    const int w = reart_xcd_remap(blockIdx.x, items);
    if (w < 0) return;
    const int lane = threadIdx.x;
    const int b = w / G, i0 = (w % G) * Q;
    int n1 = lenq ? (int)lenq[b] : P1;
    n1 = n1 < P1 ? n1 : P1;
    int n2 = lent ? (int)lent[b] : P2;
    n2 = n2 < P2 ? n2 : P2;
    const int nv = n1 - i0 < 0 ? 0 : (n1 - i0 < Q ? n1 - i0 : Q);     // queries of the group with a list
    KeyF64 *cand = s_keyd + (size_t)Q * K;
    for (int e = lane; e < Q * K; e += 64) s_keyd[e] = kl_none<KeyF64>();
    kl_wave_sync();

    KeyF64 thr[Q];                    // each list's K-th key (all-ones while it is not full)
#pragma unroll
    for (int q = 0; q < Q; ++q) thr[q] = kl_none<KeyF64>();
    const double *qg = qimg + (size_t)w * D * Q;                       // [D][Q] of this group, wave-uniform
    const double *tb = tsoa + (size_t)b * D * Ppad + lane;
    const int nsteps = nv ? n2 : 0;
    const int Dc = D - D % KF_DC;
    for (int j0 = 0; j0 < nsteps; j0 += 64) {
        const double *tp = tb + j0;   // < Ppad: the image is padded to a multiple of 64
        double s[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) s[q] = 0.0;
        for (int c0 = 0; c0 < Dc; c0 += KF_DC) {
            double t[KF_DC];
#pragma unroll
            for (int u = 0; u < KF_DC; ++u) t[u] = tp[(size_t)(c0 + u) * Ppad];
#pragma unroll
            for (int u = 0; u < KF_DC; ++u) {
                const double *qc = qg + (size_t)(c0 + u) * Q;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const double dq = qc[q] - t[u];
                    s[q] = s[q] + dq * dq;
                }
            }
        }
        for (int c = Dc; c < D; ++c) {
            const double tv = tp[(size_t)c * Ppad];
            const double *qc = qg + (size_t)c * Q;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const double dq = qc[q] - tv;
                s[q] = s[q] + dq * dq;
            }
        }
        const unsigned j = (unsigned)(j0 + lane);
        const bool in = (int)j < n2;
        KeyF64 key[Q];
        bool acc[Q];
        unsigned pend = 0;            // queries with candidates in this step (wave-uniform)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            key[q] = KeyF64{(u64)__double_as_longlong(s[q]), j, 0u};
            acc[q] = in && q < nv && key[q] < thr[q];
            if (__ballot(acc[q])) pend |= 1u << q;
        }
        while (pend) {
            const int q = __builtin_ctz(pend);
            pend &= pend - 1;
            KeyF64 kq = key[0];
            bool aq = acc[0];
#pragma unroll
            for (int r = 1; r < Q; ++r)
                if (q == r) { kq = key[r]; aq = acc[r]; }
            const int c = __popcll(__ballot(aq));
            const KeyF64 v = kl_sort64(kl_sel(aq, kq, kl_none<KeyF64>()), lane);  // candidates in lanes [0, c)
            const KeyF64 nt = kl_merge<NE>(s_keyd + (size_t)q * K, cand, K, v, c, lane);
#pragma unroll
            for (int r = 0; r < Q; ++r)
                if (q == r) thr[r] = nt;
        }
    }

    const int valid = K < n2 ? K : n2;
    const int nrow = P1 - i0 < Q ? P1 - i0 : Q;
    for (int q = 0; q < nrow; ++q) {
        const KeyF64 *lst = s_keyd + (size_t)q * K;
        double *od = dists + ((size_t)b * P1 + i0 + q) * K;
        int64_t *oi = idx + ((size_t)b * P1 + i0 + q) * K;
        const int vq = q < nv ? valid : 0;
        for (int e = lane; e < K; e += 64) {
            const KeyF64 key = lst[e];
            const bool ok = e < vq;
            od[e] = ok ? __longlong_as_double((long long)key.d) : 0.0;
            oi[e] = ok ? (int64_t)key.j : (int64_t)0;
        }
    }
}

// ---------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------
struct KnnF64Plan {
    int Q, NE, Ppad, G;
    size_t off_q, lds, total;
};

#ifndef KF_MIN_WAVES_LIST
#define KF_MIN_WAVES_LIST 4096        // K > 1: waves wanted per launch (4 per SIMD) before Q shrinks
#endif

// Q queries per wave, as in knn_dim_plan: as many as the list LDS allows (<= REART_LDS_DEFAULT_CAP; 16 B per key, so
// K = 1024 gets Q = 2) while the launch keeps enough waves.
static int knn_f64_plan(int N, int P1, int P2, int D, int K, KnnF64Plan *pl) {
    if (N <= 0 || P1 <= 0 || P2 <= 0 || D < 1 || D > REART_MAX_D || K < 1 || K > REART_MAX_K_LIST)
        return REART_ERR_UNSUPPORTED;
    const long want = K > 1 ? KF_MIN_WAVES_LIST : 1024;
    int Q = 8;
    while (Q > 2 && sizeof(KeyF64) * ((size_t)Q * K + 64) > REART_LDS_DEFAULT_CAP) Q >>= 1;
    while (Q > 2 && (long)N * reart_div_up(P1, Q) < want) Q >>= 1;
    if ((long)N * reart_div_up(P1, Q) > (1L << 30)) return REART_ERR_UNSUPPORTED;
    pl->Q = Q;
    pl->NE = K <= 64 ? 1 : K <= 128 ? 2 : K <= 256 ? 4 : K <= 512 ? 8 : 16;
    pl->Ppad = (int)reart_align_up((size_t)P2, 64);
    pl->G = reart_div_up(P1, Q);
    pl->off_q = reart_align_up((size_t)N * D * pl->Ppad * sizeof(double), 256);
    pl->total = pl->off_q + reart_align_up((size_t)N * pl->G * D * Q * sizeof(double), 256);
    pl->lds = sizeof(KeyF64) * ((size_t)Q * K + 64);
    return REART_OK;
}

extern "C" size_t reart_knn_points_workspace_bytes_f64(int N, int P1, int P2, int D, int K) {
    KnnF64Plan pl;
    return knn_f64_plan(N, P1, P2, D, K, &pl) == REART_OK ? pl.total : 0;
}

template <int Q, int NE>
static void knn_f64_launch(const KnnF64Plan &pl, const double *qimg, const double *tsoa, const int64_t *lenq,
                           const int64_t *lent, int N, int P1, int P2, int D, int K, double *dists, int64_t *idx,
                           hipStream_t st) {
    const int items = N * pl.G;
    hipLaunchKernelGGL((knn_f64_kernel<Q, NE>), dim3(reart_xcd_grid(items)), dim3(64), pl.lds, st, qimg, tsoa, lenq,
                       lent, P1, P2, D, pl.Ppad, pl.G, K, items, dists, idx);
}

template <int Q>
static void knn_f64_launch_q(const KnnF64Plan &pl, const double *qimg, const double *tsoa, const int64_t *lenq,
                             const int64_t *lent, int N, int P1, int P2, int D, int K, double *dists, int64_t *idx,
                             hipStream_t st) {
    switch (pl.NE) {
        case 1: knn_f64_launch<Q, 1>(pl, qimg, tsoa, lenq, lent, N, P1, P2, D, K, dists, idx, st); break;
        case 2: knn_f64_launch<Q, 2>(pl, qimg, tsoa, lenq, lent, N, P1, P2, D, K, dists, idx, st); break;
        case 4: knn_f64_launch<Q, 4>(pl, qimg, tsoa, lenq, lent, N, P1, P2, D, K, dists, idx, st); break;
        case 8: knn_f64_launch<Q, 8>(pl, qimg, tsoa, lenq, lent, N, P1, P2, D, K, dists, idx, st); break;
        default: knn_f64_launch<Q, 16>(pl, qimg, tsoa, lenq, lent, N, P1, P2, D, K, dists, idx, st); break;
    }
}

extern "C" int reart_knn_points_idx_f64(const double *p1, const double *p2, const int64_t *lengths1,
                                        const int64_t *lengths2, int N, int P1, int P2, int D, int K, double *dists,
                                        int64_t *idx, void *workspace, size_t workspace_bytes, void *stream) {
    if (N < 0 || P1 < 0 || P2 < 0 || K < 1 || D < 1) return REART_ERR_INVALID_ARG;
    if (D > REART_MAX_D || K > REART_MAX_K_LIST) return REART_ERR_UNSUPPORTED;
    if (N == 0 || P1 == 0) return REART_OK;
    if (!dists || !idx) return REART_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (P2 == 0) {  // nothing to search: zero padded outputs (utils/chamfer.py:163-170)
        if (hipMemsetAsync(dists, 0, sizeof(double) * (size_t)N * P1 * K, st) != hipSuccess ||
            hipMemsetAsync(idx, 0, sizeof(int64_t) * (size_t)N * P1 * K, st) != hipSuccess)
            return REART_ERR_LAUNCH;
        return REART_OK;
    }
    if (!p1 || !p2) return REART_ERR_INVALID_ARG;
    KnnF64Plan pl;
    const int rc = knn_f64_plan(N, P1, P2, D, K, &pl);
    if (rc != REART_OK) return rc;
    if (!workspace || workspace_bytes < pl.total) return REART_ERR_INVALID_ARG;
    double *tsoa = (double *)workspace, *qimg = (double *)((char *)workspace + pl.off_q);
    const F64ImageJob jt = {p2, lengths2, tsoa, P2, 1, pl.Ppad, (double)INFINITY};
    const F64ImageJob jq = {p1, nullptr, qimg, P1, pl.G, pl.Q, 0.0};
    const size_t per = (size_t)D * (pl.Ppad > pl.G * pl.Q ? pl.Ppad : pl.G * pl.Q);
    hipLaunchKernelGGL(knn_f64_image_kernel, dim3((unsigned)((per + 255) / 256), N, 2), dim3(256), 0, st, jt, jq, D);
    REART_CHECK_LAUNCH();
    switch (pl.Q) {
        case 8: knn_f64_launch_q<8>(pl, qimg, tsoa, lengths1, lengths2, N, P1, P2, D, K, dists, idx, st); break;
        case 4: knn_f64_launch_q<4>(pl, qimg, tsoa, lengths1, lengths2, N, P1, P2, D, K, dists, idx, st); break;
        default: knn_f64_launch_q<2>(pl, qimg, tsoa, lengths1, lengths2, N, P1, P2, D, K, dists, idx, st); break;
    }
    REART_CHECK_LAUNCH();
    return REART_OK;
}
