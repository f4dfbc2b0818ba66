// reart_amd/csrc/structure_term.hip -- the screw-consistency term of the reference (networks/loss.py structure_loss :32-57)
// and the reverse mode of the relative transform (utils/graph_utils.py compute_relative_trans :162-175) for gfx950.
//
// structure.hip's screw_fit_kernel answers the same questions once, at the end of a run: one workgroup, a thread per edge,
// sequential over the frames.  Inside an iteration the work is T x E independent screw decompositions joined per edge by a
// handful of sums over the frames, and a gradient that every part collects from its incident edges:
//   st_edge_kernel     one workgroup per edge, its lanes striding the frames (one wave up to T = 64, four beyond).  Pass 1
//                      decomposes every frame and reduces the masked sums of axis / moment, |theta| and |d| inside the
//                      workgroup (reart_wave_sum_d, then LDS); pass 2 builds the constant target of every frame, its cost and
//                      dL/dM, and -- with `pairs` -- carries dL/dM to the two ends of the edge, written per (frame, edge,
//                      end) into the workspace.
//   st_gather_kernel   one workgroup per (part, run of 16 frames): the part's incidence list (edge, end) is compacted from
//                      `pairs` into LDS in ascending edge order, then a thread owns one entry of one 4x4 and adds the
//                      list's contributions in that order.  Workgroup (0, 0) also adds the edge costs (reart_loss_sum_d,
//                      common.h, the connection term's as well: in double, a fixed order, one rounding).
// No atomics, no host synchronisation, no allocation, no memset: every output entry has one writer.  Two launches with
// `pairs`, two without (edge kernel + the loss sum).
#include "common.h"
#include "internal.h"
#include "screw_dev.h"
#include <math.h>

#define ST_MAX_P 64       // parts, as the kinematic entries
#define ST_MAX_E 4096     // edges: the incidence list of a part, 2 E ints, stays in LDS
#define ST_GT 16          // frames per workgroup of the gather kernel
#define ST_NRED 16        // sums of pass 1

static bool st_shape_ok(int T, int P, int E) {
    return T >= 1 && T <= REART_MAX_POSE_LEN && P >= 1 && P <= ST_MAX_P && E >= 0 && E <= ST_MAX_E;
}
// the edges' costs in double [E], then (ends: a gradient through the pairs is wanted) the two ends' rows per (frame, edge) [T][E][24]
struct StWs { double *cost_d; float *ends; };
static size_t st_ws_layout(int T, int E, bool ends, void *workspace, StWs *w) {
    reart_arena ws(workspace);
    w->cost_d = ws.take<double>(E > 0 ? E : 1);
    w->ends = ends ? ws.take<float>(24 * (size_t)T * (size_t)E) : nullptr;
    return ws.off;
}

// frob_cost(M, G) with its derivative: err = M inv(G) - I (rows 0..2), cost = |err|^2, dM = scale * err * inv(G)^T.
__device__ __forceinline__ float frob_cost_grad(const float *M, const float *G, float scale, float *dM) {
    float gi[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) gi[4 * i + j] = G[4 * j + i];
        gi[4 * i + 3] = (-G[i] * G[3] + -G[4 + i] * G[7]) + -G[8 + i] * G[11];
    }
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float er[4];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            er[j] = ((M[4 * i] * gi[j] + M[4 * i + 1] * gi[4 + j]) + M[4 * i + 2] * gi[8 + j]) - (i == j ? 1.f : 0.f);
            acc += er[j] * er[j];
        }
        er[3] = ((M[4 * i] * gi[3] + M[4 * i + 1] * gi[7]) + M[4 * i + 2] * gi[11]) + M[4 * i + 3];
        acc += er[3] * er[3];
        // M's row i meets inv(G)'s rows 0..2 in columns 0..2 and its constant row (0 0 0 1) in column 3
#pragma unroll
        for (int j = 0; j < 3; ++j)
            dM[4 * i + j] = scale * (((er[0] * gi[4 * j] + er[1] * gi[4 * j + 1]) + er[2] * gi[4 * j + 2]) + er[3] * gi[4 * j + 3]);
        dM[4 * i + 3] = scale * er[3];
    }
    return acc;
}

// reverse mode of rel_transform: M = [Ra^T Rb | Ra^T (tb - ta)], dM (3x4) -> gA, gB (3x4 each, rows 0..2 of the two ends)
__device__ __forceinline__ void rel_transform_bwd(const float *A, const float *B, const float *dM, float *gA, float *gB) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float dt = B[4 * k + 3] - A[4 * k + 3];
        float tb = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            gA[4 * k + i] = (((dM[4 * i] * B[4 * k] + dM[4 * i + 1] * B[4 * k + 1]) + dM[4 * i + 2] * B[4 * k + 2])) + dM[4 * i + 3] * dt;
            gB[4 * k + i] = (A[4 * k] * dM[i] + A[4 * k + 1] * dM[4 + i]) + A[4 * k + 2] * dM[8 + i];
            tb += A[4 * k + i] * dM[4 * i + 3];
        }
        gA[4 * k + 3] = -tb;
        gB[4 * k + 3] = tb;
    }
}

struct StArgs {
    const float *trans;      // [T,P,4,4]; pairs == nullptr: the relative motions [T,E,4,4]
    const int32_t *pairs;    // [E,2] (src, tgt)
    int T, P, E;
    float weight;
    float *edge_cost;        // [E]  (nullable)
    uint8_t *prismatic;      // [E]  (nullable)
    double *cost_d;          // [E]  workspace: the edge costs as the loss adds them
    float *ends;             // [T,E,2,12] workspace: rows 0..2 of the gradient of the src and the tgt transform (pairs, grad)
    float *grad_rel;         // [T,E,4,4] the gradient itself (no pairs, grad)
};

// the relative motion of (frame t, edge e); with pairs also the two ends' rows 0..2
__device__ __forceinline__ void st_load(const StArgs &a, int t, int e, int ia, int ib, float *Al, float *Bl, float *M) {
    if (a.pairs) {
        const float *A = a.trans + ((size_t)t * a.P + ia) * 16;
        const float *B = a.trans + ((size_t)t * a.P + ib) * 16;
#pragma unroll
        for (int i = 0; i < 12; ++i) { Al[i] = A[i]; Bl[i] = B[i]; }
        rel_transform(Al, Bl, M);
    } else {
        const float *R = a.trans + ((size_t)t * a.E + e) * 16;
#pragma unroll
        for (int i = 0; i < 12; ++i) M[i] = R[i];
    }
}

// sum over the workgroup of n doubles per thread, in a fixed tree -> every thread reads the totals from s_out
template <int BS, int N>
__device__ __forceinline__ void st_block_sum(double *v, double (*s_part)[ST_NRED], double *s_out) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = reart_wave_sum_d(v[i]);
    __syncthreads();                      // s_part / s_out of an earlier sum have been read
    if ((tid & 63) == 0)
#pragma unroll
        for (int i = 0; i < N; ++i) s_part[tid >> 6][i] = v[i];
    __syncthreads();
    if (tid < N) {
        double tot = s_part[0][tid];
        for (int w = 1; w < BS / 64; ++w) tot += s_part[w][tid];
        s_out[tid] = tot;
    }
    __syncthreads();
}

// One workgroup per edge; thread tid owns the frames tid, tid + BS, ... (FPT of them at most).
template <int BS, int FPT>
__global__ __launch_bounds__(BS) void st_edge_kernel(StArgs a) {
    __shared__ double s_part[BS / 64][ST_NRED];
    __shared__ double s_tot[ST_NRED];
    const int e = blockIdx.x, tid = threadIdx.x;
    int ia = 0, ib = 0;
    bool valid = true;
    if (a.pairs) {
        ia = a.pairs[2 * e];
        ib = a.pairs[2 * e + 1];
        valid = ia >= 0 && ia < a.P && ib >= 0 && ib < a.P;     // an index outside [0,P) is the caller's error: no access
    }
    // ---- pass 1: screw parameters of the own frames; sums 0..5 all frames, 6..11 non-unit frames, 12 their count,
    //      13 |theta|, 14 |d|
    float th[FPT], dd[FPT];
    double acc[ST_NRED];
#pragma unroll
    for (int i = 0; i < ST_NRED; ++i) acc[i] = 0.0;
#pragma unroll
    for (int k = 0; k < FPT; ++k) {
        const int t = tid + k * BS;
        th[k] = 0.f; dd[k] = 0.f;
        if (valid && t < a.T) {
            float Al[12], Bl[12], M[12], l[3], m[3];
            st_load(a, t, e, ia, ib, Al, Bl, M);
            transform_to_screw(M, l, m, th[k], dd[k]);
            const bool unit = ((fabsf(th[k]) <= 1e-5f) || (fabsf(th[k] - PI_F) <= 1e-5f)) && (dd[k] <= 1e-5f);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                acc[c] += (double)l[c];
                acc[3 + c] += (double)m[c];
                if (!unit) { acc[6 + c] += (double)l[c]; acc[9 + c] += (double)m[c]; }
            }
            if (!unit) acc[12] += 1.0;
            acc[13] += (double)fabsf(th[k]);
            acc[14] += (double)fabsf(dd[k]);
        }
    }
    st_block_sum<BS, ST_NRED>(acc, s_part, s_tot);
    const double nkeep = s_tot[12];
    const bool plain = a.E <= 1 || nkeep == 0.0;
    float ml[3], mm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ml[c] = (float)(plain ? s_tot[c] / (double)a.T : s_tot[6 + c] / nkeep);
        mm[c] = (float)(plain ? s_tot[3 + c] / (double)a.T : s_tot[9 + c] / nkeep);
    }
    const bool pris = (float)(s_tot[14] / (double)a.T) > (float)(s_tot[13] / (double)a.T);
    // ---- pass 2: target, cost and gradient of the own frames
    const float scale = 2.0f * a.weight;
    float csum = 0.f;
#pragma unroll
    for (int k = 0; k < FPT; ++k) {
        const int t = tid + k * BS;
        if (t >= a.T) continue;
        float Al[12], Bl[12], M[12], G[12], dM[12];
        if (valid) {
            st_load(a, t, e, ia, ib, Al, Bl, M);
            screw_fwd(ml, mm, pris ? 1e-6f : th[k], pris ? dd[k] : 1e-6f, G);
            csum += frob_cost_grad(M, G, scale, dM);
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i) { Al[i] = 0.f; Bl[i] = 0.f; dM[i] = 0.f; }
        }
        if (a.ends) {
            float gA[12], gB[12];
            rel_transform_bwd(Al, Bl, dM, gA, gB);
            float4 *o = (float4 *)(a.ends + ((size_t)t * a.E + e) * 24);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                o[i] = make_float4(gA[4 * i], gA[4 * i + 1], gA[4 * i + 2], gA[4 * i + 3]);
                o[3 + i] = make_float4(gB[4 * i], gB[4 * i + 1], gB[4 * i + 2], gB[4 * i + 3]);
            }
        }
        if (a.grad_rel) {
            float4 *o = (float4 *)(a.grad_rel + ((size_t)t * a.E + e) * 16);
#pragma unroll
            for (int i = 0; i < 3; ++i) o[i] = make_float4(dM[4 * i], dM[4 * i + 1], dM[4 * i + 2], dM[4 * i + 3]);
            o[3] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    double c1[1] = {(double)csum};
    st_block_sum<BS, 1>(c1, s_part, s_tot);
    if (tid == 0) {
        a.cost_d[e] = s_tot[0];
        if (a.edge_cost) a.edge_cost[e] = (float)s_tot[0];
        if (a.prismatic) a.prismatic[e] = (valid && pris) ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void st_loss_kernel(const double *cost_d, int E, float weight, float *loss) {
    __shared__ double s_w[4];
    reart_loss_sum_d<256>(cost_d, E, weight, loss, s_w);
}

// grad[t,p] = sum over the edges that end in p, ascending edge number, src end before tgt end; row 3 = 0.
// Workgroup (p, run of ST_GT frames); with `loss`, workgroup (0, 0) adds the edge costs as well.
__global__ __launch_bounds__(256) void st_gather_kernel(const float *__restrict__ ends, const int32_t *__restrict__ pairs, int T, int P,
                                                        int E, float *__restrict__ grad, const double *__restrict__ cost_d,
                                                        float weight, float *__restrict__ loss) {
    __shared__ int s_list[2 * ST_MAX_E];       // 2 * edge + end
    __shared__ int s_cnt[257];
    __shared__ double s_w[4];
    const int p = blockIdx.x, t0 = blockIdx.y * ST_GT, tid = threadIdx.x;
    const int chunk = (E + 255) / 256, k0 = min(E, tid * chunk), k1 = min(E, k0 + chunk);
    int c = 0;
    for (int k = k0; k < k1; ++k) c += (pairs[2 * k] == p) + (pairs[2 * k + 1] == p);
    s_cnt[tid + 1] = c;
    if (tid == 0) s_cnt[0] = 0;
    __syncthreads();
    if (tid == 0)
        for (int i = 1; i <= 256; ++i) s_cnt[i] += s_cnt[i - 1];
    __syncthreads();
    int w = s_cnt[tid];
    for (int k = k0; k < k1; ++k) {
        if (pairs[2 * k] == p) s_list[w++] = 2 * k;
        if (pairs[2 * k + 1] == p) s_list[w++] = 2 * k + 1;
    }
    __syncthreads();
    const int n = s_cnt[256], t = t0 + (tid >> 4), ent = tid & 15;
    if (t < T) {
        float sum = 0.f;
        if (ent < 12) {
            const float *base = ends + (size_t)t * E * 24 + ent;
            for (int q = 0; q < n; ++q) sum += base[(size_t)s_list[q] * 12];
        }
        grad[((size_t)t * P + p) * 16 + ent] = sum;
    }
    if (loss && blockIdx.x == 0 && blockIdx.y == 0) reart_loss_sum_d<256>(cost_d, E, weight, loss, s_w);
}

// grad_rel [T,E,4,4] -> the two ends' rows per (frame, edge); rows 0..2 of the upstream only
__global__ __launch_bounds__(256) void st_rel_bwd_kernel(const float *__restrict__ trans, const int32_t *__restrict__ pairs, int T,
                                                         int P, int E, const float *__restrict__ grad_rel, float *__restrict__ ends) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)T * E) return;
    const int t = (int)(i / E), e = (int)(i % E);
    const int ia = pairs[2 * e], ib = pairs[2 * e + 1];
    float gA[12], gB[12];
    if (ia >= 0 && ia < P && ib >= 0 && ib < P) {
        const float *A = trans + ((size_t)t * P + ia) * 16, *B = trans + ((size_t)t * P + ib) * 16, *g = grad_rel + i * 16;
        float Al[12], Bl[12], dM[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) { Al[k] = A[k]; Bl[k] = B[k]; dM[k] = g[k]; }
        rel_transform_bwd(Al, Bl, dM, gA, gB);
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) { gA[k] = 0.f; gB[k] = 0.f; }
    }
    float4 *o = (float4 *)(ends + i * 24);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[k] = make_float4(gA[4 * k], gA[4 * k + 1], gA[4 * k + 2], gA[4 * k + 3]);
        o[3 + k] = make_float4(gB[4 * k], gB[4 * k + 1], gB[4 * k + 2], gB[4 * k + 3]);
    }
}

static void st_launch_edges(const StArgs &a, hipStream_t st) {
    if (a.T <= 64) hipLaunchKernelGGL((st_edge_kernel<64, 1>), dim3(a.E), dim3(64), 0, st, a);
    else if (a.T <= 256) hipLaunchKernelGGL((st_edge_kernel<256, 1>), dim3(a.E), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((st_edge_kernel<256, REART_MAX_POSE_LEN / 256>), dim3(a.E), dim3(256), 0, st, a);
}

extern "C" size_t reart_structure_term_workspace_bytes(int T, int P, int E) {
    StWs w;
    return st_shape_ok(T, P, E) ? st_ws_layout(T, E, true, nullptr, &w) : 0;
}

extern "C" int reart_structure_term(const float *trans, int T, int P, const int32_t *pairs, int E, float weight, float *loss,
                                    float *edge_cost, uint8_t *prismatic, float *grad, void *workspace, size_t workspace_bytes,
                                    void *stream) {
    if (!trans || !loss || T <= 0 || P <= 0 || E < 0) return REART_ERR_INVALID_ARG;
    if (!st_shape_ok(T, pairs ? P : 1, E)) return REART_ERR_UNSUPPORTED;
    StWs w;
    if (!workspace || workspace_bytes < st_ws_layout(T, E, pairs && grad && E > 0, workspace, &w)) return REART_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (E > 0) {
        StArgs a{trans, pairs, T, P, E, weight, edge_cost, prismatic, w.cost_d, w.ends, pairs ? nullptr : grad};
        st_launch_edges(a, st);
    }
    if (pairs && grad)    // E == 0: every list is empty, the gradient is written as zeros
        hipLaunchKernelGGL(st_gather_kernel, dim3(P, reart_div_up(T, ST_GT)), dim3(256), 0, st, w.ends, pairs, T, P, E, grad, w.cost_d,
                           weight, loss);
    else
        hipLaunchKernelGGL(st_loss_kernel, dim3(1), dim3(256), 0, st, w.cost_d, E, weight, loss);
    REART_CHECK_LAUNCH();
    return REART_OK;
}

extern "C" size_t reart_rel_trans_backward_workspace_bytes(int T, int P, int E) {      // one block: the two ends' rows
    return st_shape_ok(T, P, E) ? reart_align_up(sizeof(float) * 24 * (size_t)T * (size_t)(E > 0 ? E : 1), 256) : 0;
}

extern "C" int reart_rel_trans_backward(const float *trans, int T, int P, const int32_t *pairs, int E, const float *grad_rel,
                                        float *grad_trans, void *workspace, size_t workspace_bytes, void *stream) {
    if (!trans || !grad_trans || T <= 0 || P <= 0 || E < 0 || (E > 0 && (!pairs || !grad_rel))) return REART_ERR_INVALID_ARG;
    if (!st_shape_ok(T, P, E)) return REART_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < reart_rel_trans_backward_workspace_bytes(T, P, E)) return REART_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    float *ws_ends = (float *)workspace;
    if (E > 0) {
        const size_t n = (size_t)T * E;
        hipLaunchKernelGGL(st_rel_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, trans, pairs, T, P, E, grad_rel,
                           ws_ends);
    }
    hipLaunchKernelGGL(st_gather_kernel, dim3(P, reart_div_up(T, ST_GT)), dim3(256), 0, st, ws_ends, pairs, T, P, E, grad_trans,
                       (const double *)nullptr, 0.f, (float *)nullptr);
    REART_CHECK_LAUNCH();
    return REART_OK;
}
