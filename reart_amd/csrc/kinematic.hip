// reart_amd/csrc/kinematic.hip -- screw-joint forward kinematics for gfx950.
//
// Replaces, fused, the per-iteration Python of the reference's projection model:
//   fk                                         utils/kinematic_utils.py:151-198
//   screw_param_to_exponential_coordinates     screw_se3/screw_utils.py:6-23
//   transform_from_exponential_coordinates     screw_se3/screw_utils.py:27-30
//   se3_exp_map (+ _so3_exp_map, _se3_V_matrix) screw_se3/geo_utils.py:90-222
// and their autograd backward.  The reference walks the joint tree in a Python loop issuing
// dozens of tiny bmm / boolean-mask ops per part (each mask = a host sync on a GPU); here one
// thread per frame evaluates the whole tree (P <= 64 parts, a few hundred flops) in one launch.
//
// Reproduced on purpose: clamp on the SQUARED rotation norm at 1e-4; the
// no-rotation test |theta| < 1e-6 is strict and in fp32 (branch-free select here); revolute
// joints carry d = 1e-6 when no distance list is given.
#include "common.h"
#include "internal.h"
#include <math.h>

#define FK_MAXP 64
#include "screw_dev.h"

// FK[c] = FK[parent(c)] * T_rel(c), parts visited root -> leaf (`order`)
__global__ __launch_bounds__(64) void fk_fwd_kernel(const int *__restrict__ parent,
                                                    const int *__restrict__ edge_of_part,
                                                    const int *__restrict__ order, int P,
                                                    const float *__restrict__ axis,
                                                    const float *__restrict__ moment,
                                                    const float *__restrict__ theta,
                                                    const float *__restrict__ distance, int B, int E,
                                                    float *__restrict__ trans) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= B) return;
    for (int oi = 0; oi < P; ++oi) {
        const int c = order[oi];
        float *F = trans + 16 * ((size_t)t * P + c);
        F[12] = 0.f; F[13] = 0.f; F[14] = 0.f; F[15] = 1.f;
        if (parent[c] < 0) {
#pragma unroll
            for (int i = 0; i < 12; ++i) F[i] = (i % 5 == 0) ? 1.f : 0.f;
            continue;
        }
        const int e = edge_of_part[c];
        float Tr[12];
        screw_fwd(axis + 3 * e, moment + 3 * e, theta[(size_t)t * E + e],
                  distance ? distance[(size_t)t * E + e] : 1e-6f, Tr);
        const float *Fp = trans + 16 * ((size_t)t * P + parent[c]);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // row i of the parent (4th column multiplies the implicit [0 0 0 1] row of T_rel)
                float acc = Fp[4 * i] * Tr[j];
                acc = fmaf(Fp[4 * i + 1], Tr[4 + j], acc);
                acc = fmaf(Fp[4 * i + 2], Tr[8 + j], acc);
                if (j == 3) acc = fmaf(Fp[4 * i + 3], 1.0f, acc);
                F[4 * i + j] = acc;
            }
    }
}

extern "C" int reart_fk_forward(const int32_t *parent, const int32_t *edge_of_part, const int32_t *order,
                                int P, const float *axis, const float *moment, const float *theta,
                                const float *distance, int B, int E, float *trans, void *stream) {
    if (P < 1 || P > FK_MAXP || B < 0 || E < 0) return REART_ERR_INVALID_ARG;      // the limit of reart_fk_backward: a model is refused
    if (B == 0) return REART_OK;                                                  // before its first forward, not at its first backward
    if (!parent || !edge_of_part || !order || !trans) return REART_ERR_INVALID_ARG;
    // a single part has no joint: its empty axis / moment / theta may be NULL (the kernel writes the root's identity only)
    if (E == 0 ? P != 1 : (!axis || !moment || !theta)) return REART_ERR_INVALID_ARG;
    hipLaunchKernelGGL(fk_fwd_kernel, dim3(reart_div_up(B, 64)), dim3(64), 0, (hipStream_t)stream, parent,
                       edge_of_part, order, P, axis, moment, theta, distance, B, E, trans);
    REART_CHECK_LAUNCH();
    return REART_OK;
}

// ---------------------------------------------------------------------------------------
// backward.
//  (1) gpose[t,p] (3x4) = sum_{n: part_n = p} [ G[t,n] x_n^T | G[t,n] ]   -- one workgroup per
//      frame; thread c in 0..11 owns one matrix entry for ALL parts in LDS and walks the points in
//      ascending order (deterministic, no atomics).
//  (2) per frame: leaves -> root  gFK[parent] += gFK[c] T_rel^T, gT_rel = FK[parent]^T gFK[c],
//      then screw_bwd; per-frame axis/moment contributions go to a [B,E,6] scratch.
//  (3) axis/moment gradients = sum over frames in ascending order.
// ---------------------------------------------------------------------------------------
// Two launches since round 6.  As ONE workgroup per frame the 21 slices' serial walks each waited for their own loads, trip by
// trip (68 us per launch at 9 x 4096: the longest kernel between two assignment re-solves).  Now a workgroup per (frame, slice):
// the slice's points -- part labels, gradients, coordinates -- come into LDS in one coalesced batch, twelve threads walk them in
// the SAME ascending order, and a second launch adds the slices in ascending order: the same additions in the same order.
// (PG_SLICES: internal.h)
__global__ __launch_bounds__(256) void pose_grad_kernel(const float *__restrict__ x,
                                                        const int64_t *__restrict__ part,
                                                        const float *__restrict__ G, int N, int P,
                                                        float *__restrict__ partial /* [B][PG_SLICES][P*12] */) {
    extern __shared__ float s_pg[];  // acc [P*12] | g [per*3] | xx [per*3] | pp [per] (ints)
    const int slice = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const int per = (N + PG_SLICES - 1) / PG_SLICES;
    const int n0 = slice * per, n1 = (n0 + per < N) ? n0 + per : N, cnt = n1 > n0 ? n1 - n0 : 0;
    float *acc = s_pg, *sg = acc + P * 12, *sx = sg + per * 3;
    int *sp = (int *)(sx + per * 3);
    for (int e = tid; e < cnt * 3; e += 256) { sg[e] = G[3 * ((size_t)t * N + n0) + e]; sx[e] = x[3 * (size_t)n0 + e]; }
    for (int e = tid; e < cnt; e += 256) sp[e] = (int)part[n0 + e];
    for (int e = tid; e < P * 12; e += 256) acc[e] = 0.f;
    __syncthreads();
    if (tid < 12) {
        const int c = tid, gi = c < 9 ? c / 3 : c - 9, xi = c % 3;
        for (int k = 0; k < cnt; ++k) {
            const float g = sg[3 * k + gi];
            acc[sp[k] * 12 + c] += c < 9 ? g * sx[3 * k + xi] : g;
        }
    }
    __syncthreads();
    float *out = partial + ((size_t)t * PG_SLICES + slice) * P * 12;
    for (int e = tid; e < P * 12; e += 256) out[e] = acc[e];
}

// (also clears frame t's rows of the joint gradients fk_bwd_kernel accumulates into -- [B,E] theta, [B,E] distance (nullable),
// [B,E,6] axis/moment terms: three fill launches of their own otherwise, each a 5 us slot of the iteration)
// partial == NULL: no points (the sums are zero).  g_trans [B,P,4,4] (nullable): an upstream on the forward's `trans`; its rows
// 0..2 join the points' sums here, after the last slice, and walk the tree with them; its row 3 (constants) is not read.
__global__ __launch_bounds__(256) void pose_grad_sum_kernel(const float *__restrict__ partial, int P, float *__restrict__ gpose, int E,
                                                            float *__restrict__ g_theta, float *__restrict__ g_dist, float *__restrict__ g_lm,
                                                            const float *__restrict__ g_trans) {
    const int t = blockIdx.x;
    for (int e = threadIdx.x; e < 6 * E; e += 256) {
        g_lm[(size_t)t * 6 * E + e] = 0.f;
        if (e < E) { g_theta[(size_t)t * E + e] = 0.f; if (g_dist) g_dist[(size_t)t * E + e] = 0.f; }
    }
    for (int e = threadIdx.x; e < P * 12; e += 256) {
        float sum = 0.f;
        if (partial)
            for (int s = 0; s < PG_SLICES; ++s) sum += partial[((size_t)t * PG_SLICES + s) * P * 12 + e];
        const int p = e / 12, cc = e % 12;
        // gpose layout 3x4 row-major: entry (i,j) for cc<9 is R[i][j] (i = cc/3, j = cc%3), cc>=9 is t[cc-9]
        const int i = cc < 9 ? cc / 3 : cc - 9, j = cc < 9 ? cc % 3 : 3;
        if (g_trans) sum += g_trans[16 * ((size_t)t * P + p) + 4 * i + j];
        gpose[12 * ((size_t)t * P + p) + 4 * i + j] = sum;
    }
}

__global__ __launch_bounds__(64) void fk_bwd_kernel(const int *__restrict__ parent,
                                                    const int *__restrict__ edge_of_part,
                                                    const int *__restrict__ order, int P,
                                                    const float *__restrict__ axis,
                                                    const float *__restrict__ moment,
                                                    const float *__restrict__ theta,
                                                    const float *__restrict__ distance, int B, int E,
                                                    const float *__restrict__ trans,
                                                    float *__restrict__ gpose /* in/out [B,P,3,4] */,
                                                    float *__restrict__ g_theta, float *__restrict__ g_dist,
                                                    float *__restrict__ g_lm /* [B,E,6] */) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= B) return;
    for (int oi = P - 1; oi >= 0; --oi) {
        const int c = order[oi];
        if (parent[c] < 0) continue;
        const int e = edge_of_part[c], pa = parent[c];
        const float th = theta[(size_t)t * E + e];
        const float dd = distance ? distance[(size_t)t * E + e] : 1e-6f;
        float Tr[12];
        screw_fwd(axis + 3 * e, moment + 3 * e, th, dd, Tr);
        const float *gF = gpose + 12 * ((size_t)t * P + c);
        float *gFp = gpose + 12 * ((size_t)t * P + pa);
        const float *Fp = trans + 16 * ((size_t)t * P + pa);
        float gTr[12];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // gT_rel[i][j] = sum_k Fp[k][i] gF[k][j]   (rows 0..2 of the parent rotation)
                gTr[4 * i + j] = fmaf(Fp[8 + i], gF[8 + j], fmaf(Fp[4 + i], gF[4 + j], Fp[i] * gF[j]));
            }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            // gFp[i][k] += sum_j gF[i][j] Tr_full[k][j], Tr_full row 3 = [0 0 0 1]
#pragma unroll
            for (int k = 0; k < 3; ++k)
                gFp[4 * i + k] += fmaf(gF[4 * i + 3], Tr[4 * k + 3],
                                       fmaf(gF[4 * i + 2], Tr[4 * k + 2],
                                            fmaf(gF[4 * i + 1], Tr[4 * k + 1], gF[4 * i] * Tr[4 * k])));
            gFp[4 * i + 3] += gF[4 * i + 3];
        }
        float gl[3] = {0.f, 0.f, 0.f}, gm[3] = {0.f, 0.f, 0.f}, gth, gd;
        screw_bwd(axis + 3 * e, moment + 3 * e, th, dd, gTr, gl, gm, &gth, &gd);
        g_theta[(size_t)t * E + e] = gth;
        if (g_dist) g_dist[(size_t)t * E + e] = gd;
        float *o = g_lm + 6 * ((size_t)t * E + e);
        o[0] = gl[0]; o[1] = gl[1]; o[2] = gl[2]; o[3] = gm[0]; o[4] = gm[1]; o[5] = gm[2];
    }
}

__global__ __launch_bounds__(256) void lm_reduce_kernel(const float *__restrict__ g_lm, int B, int E,
                                                        float *__restrict__ g_axis, float *__restrict__ g_moment) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= E * 6) return;
    const int e = o / 6, c = o % 6;
    float acc = 0.f;
    for (int t = 0; t < B; ++t) acc += g_lm[6 * ((size_t)t * E + e) + c];
    if (c < 3) g_axis[3 * e + c] = acc;
    else g_moment[3 * e + c - 3] = acc;
}

struct FkBwdWs { float *gpose, *g_lm, *pg_partial; };
static size_t fk_bwd_ws_layout(int P, int B, int E, void *workspace, FkBwdWs *w) {
    reart_arena ws(workspace);
    w->gpose = ws.take<float>(12 * (size_t)B * P);
    w->g_lm = ws.take<float>(6 * (size_t)B * (E > 0 ? E : 1));
    w->pg_partial = ws.take<float>(12 * (size_t)B * P * PG_SLICES);      // the slices' partial pose gradients
    return ws.off;
}
extern "C" size_t reart_fk_backward_workspace_bytes(int P, int B, int E) {
    FkBwdWs w;
    return (P <= 0 || B <= 0 || E < 0) ? 0 : fk_bwd_ws_layout(P, B, E, nullptr, &w);
}

int reart_pose_grad_launch(const float *x, const int64_t *part, const float *G, int N, int P, int B, float *partial, hipStream_t st) {
    const int pg_per = (N + PG_SLICES - 1) / PG_SLICES;
    const size_t lds = sizeof(float) * ((size_t)P * 12 + 7 * (size_t)pg_per);
    if (lds > REART_LDS_DEFAULT_CAP &&
        hipFuncSetAttribute((const void *)pose_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return REART_ERR_LAUNCH;
    hipLaunchKernelGGL(pose_grad_kernel, dim3(PG_SLICES, B), dim3(256), lds, st, x, part, G, N, P, partial);
    return REART_OK;
}

extern "C" int reart_fk_backward(const float *x, const int64_t *part, const float *G, int N,
                                 const int32_t *parent, const int32_t *edge_of_part, const int32_t *order,
                                 int P, const float *axis, const float *moment, const float *theta,
                                 const float *distance, int B, int E, const float *trans,
                                 float *g_axis, float *g_moment, float *g_theta, float *g_distance,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    if (B != 0 && (!x || !part || !G)) return REART_ERR_INVALID_ARG;            // this entry takes no empty cloud without them
    return reart_fk_backward_launch(x, part, G, N, parent, edge_of_part, order, P, axis, moment, theta, distance, B, E, trans,
                                    nullptr, g_axis, g_moment, g_theta, g_distance, workspace, workspace_bytes, (hipStream_t)stream);
}

int reart_fk_backward_launch(const float *x, const int64_t *part, const float *G, int N, const int32_t *parent,
                             const int32_t *edge_of_part, const int32_t *order, int P, const float *axis, const float *moment,
                             const float *theta, const float *distance, int B, int E, const float *trans, const float *g_trans,
                             float *g_axis, float *g_moment, float *g_theta, float *g_distance, void *workspace,
                             size_t workspace_bytes, hipStream_t st) {
    if (P < 1 || P > FK_MAXP || B < 0 || E < 0 || N < 0) return REART_ERR_INVALID_ARG;
    if (B == 0) return REART_OK;
    if ((N > 0 && (!x || !part || !G)) || !parent || !edge_of_part || !order || !trans || !workspace) return REART_ERR_INVALID_ARG;
    if (E == 0 && P == 1) return REART_OK;                     // a single part: no joint, every joint gradient is empty
    if (!axis || !moment || !theta || !g_axis || !g_moment || !g_theta) return REART_ERR_INVALID_ARG;
    FkBwdWs w;
    if (workspace_bytes < fk_bwd_ws_layout(P, B, E, workspace, &w)) return REART_ERR_INVALID_ARG;
    if (N > 0) {
        const int rc = reart_pose_grad_launch(x, part, G, N, P, B, w.pg_partial, st);
        if (rc != REART_OK) return rc;
    }
    hipLaunchKernelGGL(pose_grad_sum_kernel, dim3(B), dim3(256), 0, st, N > 0 ? w.pg_partial : (const float *)nullptr, P, w.gpose, E,
                       g_theta, g_distance, w.g_lm, g_trans);
    hipLaunchKernelGGL(fk_bwd_kernel, dim3(reart_div_up(B, 64)), dim3(64), 0, st, parent, edge_of_part, order, P,
                       axis, moment, theta, distance, B, E, trans, w.gpose, g_theta, g_distance, w.g_lm);
    if (E > 0)
        hipLaunchKernelGGL(lm_reduce_kernel, dim3(reart_div_up(E * 6, 256)), dim3(256), 0, st, w.g_lm, B, E, g_axis,
                           g_moment);
    REART_CHECK_LAUNCH();
    return REART_OK;
}
