// reart_amd/csrc/knn_dim.hip -- K-nearest-neighbour search and its backward for points of any dimension
// D != 3, 1 <= D <= REART_MAX_D (gfx950).
//
// D = 3 keeps the kernels of knn.hip / knn_list.hip; this file serves the other D of knn_points,
// chamferdist._C.knn_points_idx / knn_points_backward and knn_cuda.KNN (DESIGN.md "K-NN, any D").
//
// Design:
//   * Targets are transposed once into a +INF padded SoA image [N][D][Ppad] (Ppad = P2 rounded up to 64),
//     queries into groups of Q: [N][ceil(P1/Q)][D][Q].  One wave serves one group of Q queries and streams the
//     targets 64 per step in ascending j: lane l holds target j0 + l, reads its D coordinates with coalesced
//     loads, and uses each one for all Q queries.  The Q coordinates of one dimension are wave-uniform and
//     contiguous (scalar loads), so two queries share one packed-fp32 instruction per operation.
//   * Each query keeps its K best targets as a sorted key list in LDS (knn_keys.h).  A step whose keys are all
//     at or above a query's K-th key costs that query one ballot; otherwise the wave sorts the candidates and
//     merges them into that query's list.
//   * Rounding contract (the oracle's sqdist): d = (((a0-b0)*(a0-b0)) + ((a1-b1)*(a1-b1))) + ..., fp32,
//     ascending dimension, no FMA (-ffp-contract=off).  The packed operations round every lane exactly as the
//     scalar ones, and starting the sum from +0 changes nothing (+0 + x = x for x >= +0).  No matrix cores: an
//     MFMA rounds as an fma chain.
#include "common.h"
#include "internal.h"
#include "blocksort.h"
#include "knn_keys.h"
#include <math.h>

#define KD_DC 16                      // target coordinates a lane holds per chunk of the distance loop

// ---------------------------------------------------------------------------------
// AoS [N][P][D] -> [N][G][D][R] with row j = g * R + r; rows j >= min(len[b], P) hold `pad`.
// Job 0: the targets (G = 1, R = Ppad, pad +INF), job 1: the query groups (R = Q, pad 0).
// ---------------------------------------------------------------------------------
struct DimImageJob {
    const float *src;
    const int64_t *len;               // nullable
    float *dst;
    int P, G, R;
    float pad;
};

__global__ __launch_bounds__(256) void knn_dim_image_kernel(DimImageJob j0, DimImageJob j1, int D) {
    const DimImageJob jb = blockIdx.z ? j1 : j0;
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
__global__ __launch_bounds__(64) void knn_dim_kernel(const float *__restrict__ qimg, const float *__restrict__ tsoa,
                                                     const int64_t *__restrict__ lenq, const int64_t *__restrict__ lent,
                                                     int P1, int P2, int D, int Ppad, int G, int K, int euclidean,
                                                     int items, float *__restrict__ dists, int64_t *__restrict__ idx) {
    extern __shared__ u64 s_keys[];   // Q lists of K keys, then 64 sorted candidates
    const int w = reart_xcd_remap(blockIdx.x, items);
    if (w < 0) return;
    const int lane = threadIdx.x;
    const int b = w / G, i0 = (w % G) * Q;
    int n1 = lenq ? (int)lenq[b] : P1;
    n1 = n1 < P1 ? n1 : P1;
    int n2 = lent ? (int)lent[b] : P2;
    n2 = n2 < P2 ? n2 : P2;
    const int nv = n1 - i0 < 0 ? 0 : (n1 - i0 < Q ? n1 - i0 : Q);     // queries of the group with a list
    u64 *cand = s_keys + (size_t)Q * K;
    for (int e = lane; e < Q * K; e += 64) s_keys[e] = ~0ull;
    kl_wave_sync();

    u64 thr[Q];                       // each list's K-th key (all-ones while it is not full)
#pragma unroll
    for (int q = 0; q < Q; ++q) thr[q] = ~0ull;
    const float *qg = qimg + (size_t)w * D * Q;                        // [D][Q] of this group, wave-uniform
    const float *tb = tsoa + (size_t)b * D * Ppad + lane;
    const int nsteps = nv ? n2 : 0;
    const int Dc = D - D % KD_DC;
    for (int j0 = 0; j0 < nsteps; j0 += 64) {
        const float *tp = tb + j0;    // < Ppad: the image is padded to a multiple of 64
        f2 s[Q / 2];
#pragma unroll
        for (int p = 0; p < Q / 2; ++p) s[p] = f2{0.f, 0.f};
        for (int c0 = 0; c0 < Dc; c0 += KD_DC) {
            float t[KD_DC];
#pragma unroll
            for (int u = 0; u < KD_DC; ++u) t[u] = tp[(size_t)(c0 + u) * Ppad];
#pragma unroll
            for (int u = 0; u < KD_DC; ++u) {
                const f2 tt = f2{t[u], t[u]};
                const f2 *qc = (const f2 *)(qg + (size_t)(c0 + u) * Q);
#pragma unroll
                for (int p = 0; p < Q / 2; ++p) {
                    const f2 dq = qc[p] - tt;
                    s[p] = s[p] + dq * dq;
                }
            }
        }
        for (int c = Dc; c < D; ++c) {
            const float tv = tp[(size_t)c * Ppad];
            const f2 tt = f2{tv, tv};
            const f2 *qc = (const f2 *)(qg + (size_t)c * Q);
#pragma unroll
            for (int p = 0; p < Q / 2; ++p) {
                const f2 dq = qc[p] - tt;
                s[p] = s[p] + dq * dq;
            }
        }
        const unsigned j = (unsigned)(j0 + lane);
        const bool in = (int)j < n2;
        u64 key[Q];
        bool acc[Q];
        unsigned pend = 0;            // queries with candidates in this step (wave-uniform)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float d = (q & 1) ? s[q / 2].y : s[q / 2].x;
            key[q] = ((u64)__float_as_uint(d) << 32) | j;
            acc[q] = in && q < nv && key[q] < thr[q];
            if (__ballot(acc[q])) pend |= 1u << q;
        }
        while (pend) {
            const int q = __builtin_ctz(pend);
            pend &= pend - 1;
            u64 kq = key[0];
            bool aq = acc[0];
#pragma unroll
            for (int r = 1; r < Q; ++r)
                if (q == r) { kq = key[r]; aq = acc[r]; }
            const int c = __popcll(__ballot(aq));
            const u64 v = kl_sort64(aq ? kq : ~0ull, lane);            // candidates in lanes [0, c)
            const u64 nt = kl_merge<NE>(s_keys + (size_t)q * K, cand, K, v, c, lane);
#pragma unroll
            for (int r = 0; r < Q; ++r)
                if (q == r) thr[r] = nt;
        }
    }

    const int valid = K < n2 ? K : n2;
    const int nrow = P1 - i0 < Q ? P1 - i0 : Q;
    for (int q = 0; q < nrow; ++q) {
        const u64 *lst = s_keys + (size_t)q * K;
        float *od = dists + ((size_t)b * P1 + i0 + q) * K;
        int64_t *oi = idx + ((size_t)b * P1 + i0 + q) * K;
        const int vq = q < nv ? valid : 0;
        for (int e = lane; e < K; e += 64) {
            const u64 key = lst[e];
            const bool ok = e < vq;
            float dd = __uint_as_float((unsigned)(key >> 32));
            if (euclidean) dd = sqrtf(dd);
            od[e] = ok ? dd : 0.0f;
            oi[e] = ok ? (int64_t)(unsigned)key : (int64_t)0;
        }
    }
}

// ---------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------
struct KnnDimPlan {
    int Q, NE, Ppad, G;
    size_t off_q, lds, total;
};

#ifndef KD_MIN_WAVES_LIST
#define KD_MIN_WAVES_LIST 4096        // K > 1: waves wanted per launch (4 per SIMD) before Q shrinks
#endif

// Q queries per wave: as many as the list LDS allows (<= REART_LDS_DEFAULT_CAP) while the launch keeps enough waves;
// a target coordinate a lane loads serves Q queries.  K = 1 is distance-bound: one wave per SIMD (256 CUs x 4) is
// enough.  K > 1 merges on most early steps, and a merge is a chain of dependent cross-lane and LDS operations that
// only other waves can hide, so it wants KD_MIN_WAVES_LIST.
static int knn_dim_plan(int N, int P1, int P2, int D, int K, KnnDimPlan *pl) {
    if (N <= 0 || P1 <= 0 || P2 <= 0 || D < 1 || D > REART_MAX_D || K < 1 || K > REART_MAX_K_LIST)
        return REART_ERR_UNSUPPORTED;
    const long want = K > 1 ? KD_MIN_WAVES_LIST : 1024;
    int Q = 8;
    while (Q > 2 && sizeof(u64) * ((size_t)Q * K + 64) > REART_LDS_DEFAULT_CAP) Q >>= 1;
    while (Q > 2 && (long)N * reart_div_up(P1, Q) < want) Q >>= 1;
    if ((long)N * reart_div_up(P1, Q) > (1L << 30)) return REART_ERR_UNSUPPORTED;
    pl->Q = Q;
    pl->NE = K <= 64 ? 1 : K <= 128 ? 2 : K <= 256 ? 4 : K <= 512 ? 8 : 16;
    pl->Ppad = (int)reart_align_up((size_t)P2, 64);
    pl->G = reart_div_up(P1, Q);
    pl->off_q = reart_align_up((size_t)N * D * pl->Ppad * sizeof(float), 256);
    pl->total = pl->off_q + reart_align_up((size_t)N * pl->G * D * Q * sizeof(float), 256);
    pl->lds = sizeof(u64) * ((size_t)Q * K + 64);
    return REART_OK;
}

extern "C" size_t reart_knn_points_workspace_bytes_d(int N, int P1, int P2, int D, int K) {
    if (D == 3) return reart_knn_points_workspace_bytes(N, P1, P2, K);
    KnnDimPlan pl;
    return knn_dim_plan(N, P1, P2, D, K, &pl) == REART_OK ? pl.total : 0;
}

template <int Q, int NE>
static void knn_dim_launch(const KnnDimPlan &pl, const float *qimg, const float *tsoa, const int64_t *lenq,
                           const int64_t *lent, int N, int P1, int P2, int D, int K, int euclidean, float *dists,
                           int64_t *idx, hipStream_t st) {
    const int items = N * pl.G;
    hipLaunchKernelGGL((knn_dim_kernel<Q, NE>), dim3(reart_xcd_grid(items)), dim3(64), pl.lds, st, qimg, tsoa, lenq,
                       lent, P1, P2, D, pl.Ppad, pl.G, K, euclidean, items, dists, idx);
}

template <int Q>
static void knn_dim_launch_q(const KnnDimPlan &pl, const float *qimg, const float *tsoa, const int64_t *lenq,
                             const int64_t *lent, int N, int P1, int P2, int D, int K, int euclidean, float *dists,
                             int64_t *idx, hipStream_t st) {
    switch (pl.NE) {
        case 1: knn_dim_launch<Q, 1>(pl, qimg, tsoa, lenq, lent, N, P1, P2, D, K, euclidean, dists, idx, st); break;
        case 2: knn_dim_launch<Q, 2>(pl, qimg, tsoa, lenq, lent, N, P1, P2, D, K, euclidean, dists, idx, st); break;
        case 4: knn_dim_launch<Q, 4>(pl, qimg, tsoa, lenq, lent, N, P1, P2, D, K, euclidean, dists, idx, st); break;
        case 8: knn_dim_launch<Q, 8>(pl, qimg, tsoa, lenq, lent, N, P1, P2, D, K, euclidean, dists, idx, st); break;
        default: knn_dim_launch<Q, 16>(pl, qimg, tsoa, lenq, lent, N, P1, P2, D, K, euclidean, dists, idx, st); break;
    }
}

// q [N,P1,D] queries, t [N,P2,D] targets; N, P1, P2 >= 1, 1 <= D <= REART_MAX_D, 1 <= K <= REART_MAX_K_LIST
int reart_knn_dim_run(const float *q, const float *t, const int64_t *lenq, const int64_t *lent, int N, int P1, int P2,
                      int D, int K, int euclidean, float *dists, int64_t *idx, void *workspace, size_t workspace_bytes,
                      hipStream_t st) {
    KnnDimPlan pl;
    const int rc = knn_dim_plan(N, P1, P2, D, K, &pl);
    if (rc != REART_OK) return rc;
    if (!workspace || workspace_bytes < pl.total) return REART_ERR_INVALID_ARG;
    float *tsoa = (float *)workspace, *qimg = (float *)((char *)workspace + pl.off_q);
    const DimImageJob jt = {t, lent, tsoa, P2, 1, pl.Ppad, INFINITY};
    const DimImageJob jq = {q, nullptr, qimg, P1, pl.G, pl.Q, 0.f};
    const size_t per = (size_t)D * (pl.Ppad > pl.G * pl.Q ? pl.Ppad : pl.G * pl.Q);
    hipLaunchKernelGGL(knn_dim_image_kernel, dim3((unsigned)((per + 255) / 256), N, 2), dim3(256), 0, st, jt, jq, D);
    REART_CHECK_LAUNCH();
    switch (pl.Q) {
        case 8: knn_dim_launch_q<8>(pl, qimg, tsoa, lenq, lent, N, P1, P2, D, K, euclidean, dists, idx, st); break;
        case 4: knn_dim_launch_q<4>(pl, qimg, tsoa, lenq, lent, N, P1, P2, D, K, euclidean, dists, idx, st); break;
        default: knn_dim_launch_q<2>(pl, qimg, tsoa, lenq, lent, N, P1, P2, D, K, euclidean, dists, idx, st); break;
    }
    REART_CHECK_LAUNCH();
    return REART_OK;
}

// ---------------------------------------------------------------------------------
// Backward for D != 3: knn_bwd_kernel of knn.hip with a loop over the D components.  Every component sums in
// the order of the D = 3 kernel and the oracle: grad_p1 over k ascending, grad_p2 over the target's bucket of
// (i, k) pairs in ascending order (counting sort), v = (2g) * diff, no float atomics.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_BS) void knn_bwd_dim_kernel(
    const float *__restrict__ p1, const float *__restrict__ p2, const int64_t *__restrict__ len1,
    const int64_t *__restrict__ len2, const int64_t *__restrict__ idx, const float *__restrict__ gd, int P1, int P2,
    int D, int K, int nbits, float *__restrict__ g1, float *__restrict__ g2, int *__restrict__ ws) {
    __shared__ int s_cnt[RS_DIG * RS_BS];
    __shared__ int s_wave[RS_BS / 64];
    const int n = blockIdx.x, tid = threadIdx.x;
    int n1 = len1 ? (int)len1[n] : P1;
    int n2 = len2 ? (int)len2[n] : P2;
    n1 = n1 < P1 ? n1 : P1;
    n2 = n2 < P2 ? n2 : P2;
    const int kk = K < n2 ? K : n2;
    p1 += (size_t)n * P1 * D; p2 += (size_t)n * P2 * D;
    idx += (size_t)n * P1 * K; gd += (size_t)n * P1 * K;
    g1 += (size_t)n * P1 * D; g2 += (size_t)n * P2 * D;
    int *cnt = ws + (size_t)n * (2 * (size_t)P2 + 2 * (size_t)P1 * K);  // [P2]
    int *off = cnt + P2;                                                 // [P2]
    int *bufA = off + P2, *bufB = bufA + (size_t)P1 * K;                 // [P1*K] each

    for (int j = tid; j < P2; j += RS_BS) cnt[j] = 0;
    __syncthreads();
    // grad_p1 and bucket counts (integer atomics: order-independent result)
    for (int i = tid; i < P1; i += RS_BS) {
        const float *x = p1 + (size_t)i * D;
        float *o = g1 + (size_t)i * D;
        if (i < n1) {
            for (int c = 0; c < D; ++c) {
                float a = 0.f;
                for (int k = 0; k < kk; ++k) {
                    const int j = (int)idx[(size_t)i * K + k];
                    a += (2.0f * gd[(size_t)i * K + k]) * (x[c] - p2[(size_t)j * D + c]);
                }
                o[c] = a;
            }
            for (int k = 0; k < kk; ++k) atomicAdd(&cnt[(int)idx[(size_t)i * K + k]], 1);
        } else {
            for (int c = 0; c < D; ++c) o[c] = 0.f;
        }
    }
    __syncthreads();
    // exclusive scan of cnt -> off
    const int chunk = (P2 + RS_BS - 1) / RS_BS;
    const int c0 = tid * chunk < P2 ? tid * chunk : P2, c1 = (c0 + chunk < P2) ? c0 + chunk : P2;
    int tot = 0;
    for (int j = c0; j < c1; ++j) tot += cnt[j];
    int run = block_excl_scan(tot, s_wave, nullptr);
    for (int j = c0; j < c1; ++j) { off[j] = run; run += cnt[j]; }
    // valid (i,k) pairs, id e = i*kk + k, stably sorted by target index
    const int M = n1 * kk;
    const int *sorted = block_stable_sort_ids(M, nbits, bufA, bufB, s_cnt, s_wave, [&](int e) {
        return (int)idx[(size_t)(e / kk) * K + (e % kk)];
    });
    for (int j = tid; j < P2; j += RS_BS) {
        const int o = off[j], cj = cnt[j];
        const float *y = p2 + (size_t)j * D;
        for (int c = 0; c < D; ++c) {
            float a = 0.f;
            for (int m = 0; m < cj; ++m) {
                const int e = sorted[o + m];
                const int i = e / kk, k = e % kk;
                a -= (2.0f * gd[(size_t)i * K + k]) * (p1[(size_t)i * D + c] - y[c]);
            }
            g2[(size_t)j * D + c] = a;
        }
    }
}

// N, P1, P2 >= 1, 1 <= D <= REART_MAX_D; workspace as knn_bwd_kernel's
int reart_knn_dim_backward_launch(const float *p1, const float *p2, const int64_t *lengths1, const int64_t *lengths2,
                                  const int64_t *idx, const float *grad_dists, int N, int P1, int P2, int D, int K,
                                  float *grad_p1, float *grad_p2, int *workspace, hipStream_t st) {
    hipLaunchKernelGGL(knn_bwd_dim_kernel, dim3(N), dim3(RS_BS), 0, st, p1, p2, lengths1, lengths2, idx, grad_dists,
                       P1, P2, D, K, reart_bits_for(P2), grad_p1, grad_p2, workspace);
    REART_CHECK_LAUNCH();
    return REART_OK;
}
