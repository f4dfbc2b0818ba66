// reart_amd/csrc/transform_grad.hip -- first-order gradients through the transforms a model returns, for gfx950.
//
// In the reference every transform is an ordinary autograd tensor: trans_list of BaseModel.forward is
// rotation_6d_to_matrix(proposal_6d) | proposal_t (networks/model.py:60-68), that of KinematicModel.forward is fk(...)
// (:151-159), compute_pc_transform is a bmm plus a one-hot sum (utils/model_utils.py:54-67), and the canonical cloud is a
// tensor like any other.  The operators of this library cover the losses of the reference's drivers (G = dL/d pc_trans ->
// parameters); the entries below add what a loss on the transforms themselves, on compute_pc_transform of predicted poses
// or on a learnable cloud needs:
//   reart_rotation_6d_to_matrix_backward   Gram-Schmidt backward (r6d_backward of model_dev.h, one thread per row)
//   reart_compute_pc_transform_backward    g_cano = sum_b R[b,part_n]^T G[b,n]; g_pose = the per-part sums of pose_grad_kernel
//   reart_fk_backward_trans                reart_fk_backward + an upstream on `trans` + the gradient of the cloud
//   reart_pose_trans_backward              BaseModel: upstream on trans_list -> proposal_6d / proposal_t
//   reart_base_backward_cano               BaseModel: gradient of the canonical cloud (rigid + straight-through term)
// All float32, all deterministic: a thread owns its output and adds in ascending frame / part / hidden-unit order, the sums
// over a part's points are those of pose_grad_kernel (kinematic.hip: slices walked in ascending point order, then added in
// ascending slice order); no atomics.  No entry synchronises with the host or allocates; arguments are refused before the
// first launch.
//
// Traffic: the two per-point kernels read G [B,N,3] once, a thread its own 12 bytes of each frame (a wave 768 contiguous
// bytes), yT / hT as [P,N] / [H,N] rows (lane <-> point: coalesced).  The pose rows [B,P] every point of a workgroup may
// ask for are staged in LDS a run of frames at a time (rows 0..2 of each 4x4, 12 floats), so a thread's part-dependent row
// is an LDS read, not a gather from global memory.
#include "common.h"
#include "internal.h"
#include "model_dev.h"

#define TG_BS 128                 // threads (= points) per workgroup of the per-point kernels
#define TG_POSE_FLOATS 12288      // rigid_t_kernel: LDS floats of one run of frames (48 KiB: a single frame at P = 1024)
#define TG_CANO_POSE_FLOATS 3072  // base_cano_kernel: the same next to its weights (12 KiB: 8 frames at P = 32)
#define TG_MAX_P 1024             // parts of reart_compute_pc_transform_backward: one frame's rows must fit in LDS
#define TG_MAX_PB 32              // parts of the relaxation model (reart_base_forward)
#define TG_MAX_H 256              // hidden units reart_base_backward_cano holds in LDS

// rows 0..2 of the pose rows [row0, row0 + nrows) -> s [nrows][12]; `stride` = floats per row in global memory (16 or 12)
__device__ __forceinline__ void stage_pose_rows(float *s, const float *__restrict__ pose, int stride, size_t row0, int nrows) {
    for (int e = threadIdx.x; e < nrows * 12; e += TG_BS) s[e] = pose[(row0 + e / 12) * stride + e % 12];
}

// ----------------------------------------------------------------------------------------------- 6D -> matrix, backward
__global__ __launch_bounds__(256) void r6d_bwd_kernel(const float *__restrict__ d6, const float *__restrict__ gR, int n,
                                                      float *__restrict__ g6) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float d[6], g[9], o[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) d[c] = d6[6 * (size_t)i + c];
#pragma unroll
    for (int c = 0; c < 9; ++c) g[c] = gR[9 * (size_t)i + c];
    r6d_backward(d, g, o);
#pragma unroll
    for (int c = 0; c < 6; ++c) g6[6 * (size_t)i + c] = o[c];
}

extern "C" int reart_rotation_6d_to_matrix_backward(const float *d6, const float *gR, int n, float *g6, void *stream) {
    if (n < 0) return REART_ERR_INVALID_ARG;
    if (n == 0) return REART_OK;
    if (!d6 || !gR || !g6) return REART_ERR_INVALID_ARG;
    hipLaunchKernelGGL(r6d_bwd_kernel, dim3(reart_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, d6, gR, n, g6);
    REART_CHECK_LAUNCH();
    return REART_OK;
}

// BaseModel's trans_list = [R(p6d) | pt]: rows 0..2 of the upstream g_trans [n,4,4] -> g6d [n,6], gt [n,3] (row 3 holds
// constants: ignored).  accumulate: onto what reart_base_backward left there.
__global__ __launch_bounds__(256) void pose_trans_bwd_kernel(const float *__restrict__ p6d, const float *__restrict__ g_trans, int n,
                                                             float *__restrict__ g6d, float *__restrict__ gt, int accumulate) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float d[6], g[9], o[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) d[c] = p6d[6 * (size_t)i + c];
#pragma unroll
    for (int c = 0; c < 9; ++c) g[c] = g_trans[16 * (size_t)i + 4 * (c / 3) + c % 3];
    r6d_backward(d, g, o);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        float *dst = g6d + 6 * (size_t)i + c;
        *dst = accumulate ? *dst + o[c] : o[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float *dst = gt + 3 * (size_t)i + c;
        const float v = g_trans[16 * (size_t)i + 4 * c + 3];
        *dst = accumulate ? *dst + v : v;
    }
}

extern "C" int reart_pose_trans_backward(const float *p6d, const float *g_trans, int n, float *g6d, float *gt, int accumulate,
                                         void *stream) {
    if (n < 0) return REART_ERR_INVALID_ARG;
    if (n == 0) return REART_OK;
    if (!p6d || !g_trans || !g6d || !gt) return REART_ERR_INVALID_ARG;
    hipLaunchKernelGGL(pose_trans_bwd_kernel, dim3(reart_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, p6d, g_trans, n,
                       g6d, gt, accumulate != 0);
    REART_CHECK_LAUNCH();
    return REART_OK;
}

// ------------------------------------------------------------------------------------ hard-label rigid apply, backward
// out[n] = sum_b R[b,part_n]^T G[b,n], b ascending; one thread per point, `tb` frames of pose rows in LDS at a time.
// A label outside [0,P) has no row: its point gets zero.
__global__ __launch_bounds__(TG_BS) void rigid_t_kernel(const float *__restrict__ pose, int stride, const int64_t *__restrict__ part,
                                                        const float *__restrict__ G, int N, int P, int B, int tb,
                                                        float *__restrict__ out) {
    extern __shared__ float s_rt[];   // [tb][P][12]
    const int n = blockIdx.x * TG_BS + threadIdx.x;
    const bool live = n < N;
    const int64_t pl = live ? part[n] : 0;
    const bool ok = live && pl >= 0 && pl < P;
    const int p = ok ? (int)pl : 0;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int t0 = 0; t0 < B; t0 += tb) {
        const int nt = B - t0 < tb ? B - t0 : tb;
        __syncthreads();              // the previous run of frames has been read
        stage_pose_rows(s_rt, pose, stride, (size_t)t0 * P, nt * P);
        __syncthreads();
        if (ok) {
#pragma unroll 4
            for (int u = 0; u < nt; ++u) {
                const float *g = G + 3 * ((size_t)(t0 + u) * N + n);
                const float g0 = g[0], g1 = g[1], g2 = g[2];
                const float *T = s_rt + 12 * (u * P + p);
                a0 = fmaf(T[8], g2, fmaf(T[4], g1, fmaf(T[0], g0, a0)));
                a1 = fmaf(T[9], g2, fmaf(T[5], g1, fmaf(T[1], g0, a1)));
                a2 = fmaf(T[10], g2, fmaf(T[6], g1, fmaf(T[2], g0, a2)));
            }
        }
    }
    if (live) {
        out[3 * (size_t)n] = a0;
        out[3 * (size_t)n + 1] = a1;
        out[3 * (size_t)n + 2] = a2;
    }
}

static void rigid_t_launch(const float *pose, int stride, const int64_t *part, const float *G, int N, int P, int B, float *out,
                          hipStream_t st) {
    int tb = TG_POSE_FLOATS / (P * 12);               // >= 1: the callers hold P <= TG_MAX_P
    if (tb > B) tb = B;
    hipLaunchKernelGGL(rigid_t_kernel, dim3(reart_div_up(N, TG_BS)), dim3(TG_BS), sizeof(float) * 12 * (size_t)tb * P, st, pose,
                       stride, part, G, N, P, B, tb, out);
}

// the slices' partial sums of pose_grad_kernel -> rows 0..2 of g_pose [B,P,4,4] in ascending slice order, row 3 = 0
__global__ __launch_bounds__(256) void pose_grad_sum44_kernel(const float *__restrict__ partial, int P, float *__restrict__ g_pose) {
    const int t = blockIdx.x;
    for (int e = threadIdx.x; e < P * 16; e += 256) {
        const int p = e >> 4, i = (e >> 2) & 3, j = e & 3;
        float sum = 0.f;
        if (i < 3) {
            const int cc = j < 3 ? 3 * i + j : 9 + i;         // pose_grad_kernel's entry: G x^T (9) | G (3)
            for (int s = 0; s < PG_SLICES; ++s) sum += partial[((size_t)t * PG_SLICES + s) * P * 12 + p * 12 + cc];
        }
        g_pose[16 * (size_t)t * P + e] = sum;
    }
}

extern "C" size_t reart_compute_pc_transform_backward_workspace_bytes(int N, int P, int B) {
    if (N < 0 || P < 1 || P > TG_MAX_P || B <= 0) return 0;
    return reart_align_up(sizeof(float) * 12 * (size_t)B * P * PG_SLICES, 256);
}

extern "C" int reart_compute_pc_transform_backward(const float *cano, const float *pose, const int64_t *part, const float *G,
                                                   int N, int P, int B, float *g_cano, float *g_pose, void *workspace,
                                                   size_t workspace_bytes, void *stream) {
    if (N < 0 || P < 1 || P > TG_MAX_P || B < 0) return REART_ERR_INVALID_ARG;
    if (B == 0 && N == 0) return REART_OK;
    if (N > 0 && B > 0 && (!cano || !pose || !part || !G)) return REART_ERR_INVALID_ARG;
    if (g_pose && B > 0 && (!workspace || workspace_bytes < reart_compute_pc_transform_backward_workspace_bytes(N, P, B)))
        return REART_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (g_cano && N > 0) {
        if (B == 0) {
            if (hipMemsetAsync(g_cano, 0, sizeof(float) * 3 * (size_t)N, st) != hipSuccess) return REART_ERR_LAUNCH;
        } else {
            rigid_t_launch(pose, 16, part, G, N, P, B, g_cano, st);
        }
    }
    if (g_pose && B > 0) {
        if (N == 0) {
            if (hipMemsetAsync(g_pose, 0, sizeof(float) * 16 * (size_t)B * P, st) != hipSuccess) return REART_ERR_LAUNCH;
        } else {
            const int rc = reart_pose_grad_launch(cano, part, G, N, P, B, (float *)workspace, st);
            if (rc != REART_OK) return rc;
            hipLaunchKernelGGL(pose_grad_sum44_kernel, dim3(B), dim3(256), 0, st, (const float *)workspace, P, g_pose);
        }
    }
    REART_CHECK_LAUNCH();
    return REART_OK;
}

// --------------------------------------------------------------------------------- fk backward with the two extras
extern "C" int reart_fk_backward_trans(const float *x, const int64_t *part, const float *G, int N, const int32_t *parent,
                                       const int32_t *edge_of_part, const int32_t *order, int P, const float *axis,
                                       const float *moment, const float *theta, const float *distance, int B, int E,
                                       const float *trans, const float *g_trans, float *g_axis, float *g_moment, float *g_theta,
                                       float *g_distance, float *g_x, void *workspace, size_t workspace_bytes, void *stream) {
    const int rc = reart_fk_backward_launch(x, part, G, N, parent, edge_of_part, order, P, axis, moment, theta, distance, B, E,
                                            trans, g_trans, g_axis, g_moment, g_theta, g_distance, workspace, workspace_bytes,
                                            (hipStream_t)stream);
    if (rc != REART_OK || B == 0 || N == 0 || !g_x) return rc;
    rigid_t_launch(trans, 16, part, G, N, P, B, g_x, (hipStream_t)stream);
    REART_CHECK_LAUNCH();
    return REART_OK;
}

// ------------------------------------------------------------------------- BaseModel: gradient of the canonical cloud
// [R(p6d) | pt] of every (frame, part) as rows 0..2 of a 4x4 -> table [n][12]
__global__ __launch_bounds__(256) void rt_rows_kernel(const float *__restrict__ p6d, const float *__restrict__ pt, int n,
                                                      float *__restrict__ table) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float d[6], R[9];
#pragma unroll
    for (int c = 0; c < 6; ++c) d[c] = p6d[6 * (size_t)i + c];
    r6d_to_matrix(d, R);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float *o = table + 12 * (size_t)i + 4 * c;
        o[0] = R[3 * c]; o[1] = R[3 * c + 1]; o[2] = R[3 * c + 2]; o[3] = pt[3 * (size_t)i + c];
    }
}

// One thread per point:
//   dw[p]  = sum_b G[b,n] . (R_bp x_n + t_bp)          the straight-through weights' gradient, b ascending
//   rigid  = sum_b R[b,hard_n]^T G[b,n]
//   ds[p]  = y_p (dw_p - sum_q y_q dw_q) / tau          softmax backward (the forward's yT)
//   dh[j]  = [h_j > 0] sum_p W2[p,j] ds_p               the forward's hT decides the ReLU
//   g_cano = rigid + sum_j dh_j W1[j,:]
// W2 is held transposed and zero-padded to 32 parts ([H][32]: the sum over p is eight 16-byte LDS reads, every lane the
// same address), W1 as [H][3]; ds_p = 0 for p >= P.
__global__ __launch_bounds__(TG_BS) void base_cano_kernel(const float *__restrict__ cano, const float *__restrict__ W1,
                                                          const float *__restrict__ W2, const float *__restrict__ table,
                                                          const float *__restrict__ yT, const float *__restrict__ hT,
                                                          const int32_t *__restrict__ hard_idx, float tau,
                                                          const float *__restrict__ G, int N, int P, int B, int H, int tb,
                                                          float *__restrict__ g_cano) {
    extern __shared__ float s_bc[];   // W2T [H][32] | W1 [H][3] | pose rows [tb][P][12]
    float *s_w2t = s_bc, *s_w1 = s_w2t + (size_t)H * TG_MAX_PB, *s_rt = s_w1 + (size_t)H * 3;
    const int tid = threadIdx.x, n = blockIdx.x * TG_BS + tid;
    const bool live = n < N;
    for (int e = tid; e < H * TG_MAX_PB; e += TG_BS) {
        const int j = e / TG_MAX_PB, p = e % TG_MAX_PB;
        s_w2t[e] = p < P ? W2[(size_t)p * H + j] : 0.f;
    }
    for (int e = tid; e < H * 3; e += TG_BS) s_w1[e] = W1[e];
    const size_t nn = live ? n : 0;
    const float x0 = cano[3 * nn], x1 = cano[3 * nn + 1], x2 = cano[3 * nn + 2];
    int hard = hard_idx[nn];
    hard = hard < 0 ? 0 : (hard >= P ? P - 1 : hard);
    float dw[TG_MAX_PB];
#pragma unroll
    for (int p = 0; p < TG_MAX_PB; ++p) dw[p] = 0.f;
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
    for (int t0 = 0; t0 < B; t0 += tb) {
        const int nt = B - t0 < tb ? B - t0 : tb;
        __syncthreads();              // the previous run of frames has been read (first trip: nothing to wait for)
        stage_pose_rows(s_rt, table, 12, (size_t)t0 * P, nt * P);
        __syncthreads();              // (first trip: also the weights)
        for (int u = 0; u < nt; ++u) {
            const float *g = G + 3 * ((size_t)(t0 + u) * N + nn);
            const float g0 = g[0], g1 = g[1], g2 = g[2];
            const float *Tb = s_rt + 12 * u * P;
#pragma unroll
            for (int p = 0; p < TG_MAX_PB; ++p)
                if (p < P) {
                    const float *T = Tb + 12 * p;
                    const float v0 = fmaf(x2, T[2], fmaf(x1, T[1], x0 * T[0])) + T[3];
                    const float v1 = fmaf(x2, T[6], fmaf(x1, T[5], x0 * T[4])) + T[7];
                    const float v2 = fmaf(x2, T[10], fmaf(x1, T[9], x0 * T[8])) + T[11];
                    dw[p] = fmaf(g2, v2, fmaf(g1, v1, fmaf(g0, v0, dw[p])));
                }
            const float *T = Tb + 12 * hard;
            r0 = fmaf(T[8], g2, fmaf(T[4], g1, fmaf(T[0], g0, r0)));
            r1 = fmaf(T[9], g2, fmaf(T[5], g1, fmaf(T[1], g0, r1)));
            r2 = fmaf(T[10], g2, fmaf(T[6], g1, fmaf(T[2], g0, r2)));
        }
    }
    if (B == 0) __syncthreads();      // the weights, where no frame's barrier covered them
    // softmax backward; dw becomes ds
    float y[TG_MAX_PB], dot = 0.f;
#pragma unroll
    for (int p = 0; p < TG_MAX_PB; ++p) {
        y[p] = p < P ? yT[(size_t)p * N + nn] : 0.f;
        dot = fmaf(y[p], dw[p], dot);
    }
#pragma unroll
    for (int p = 0; p < TG_MAX_PB; ++p) dw[p] = (y[p] * (dw[p] - dot)) / tau;
    // hidden layer and first layer
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int j = 0; j < H; ++j) {
        const float h = hT[(size_t)j * N + nn];
        const float4 *w = (const float4 *)(s_w2t + (size_t)j * TG_MAX_PB);
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < TG_MAX_PB / 4; ++q) {
            const float4 wv = w[q];
            acc = fmaf(wv.x, dw[4 * q], acc);
            acc = fmaf(wv.y, dw[4 * q + 1], acc);
            acc = fmaf(wv.z, dw[4 * q + 2], acc);
            acc = fmaf(wv.w, dw[4 * q + 3], acc);
        }
        const float dh = h > 0.f ? acc : 0.f;
        s0 = fmaf(s_w1[3 * j], dh, s0);
        s1 = fmaf(s_w1[3 * j + 1], dh, s1);
        s2 = fmaf(s_w1[3 * j + 2], dh, s2);
    }
    if (live) {
        g_cano[3 * (size_t)n] = r0 + s0;
        g_cano[3 * (size_t)n + 1] = r1 + s1;
        g_cano[3 * (size_t)n + 2] = r2 + s2;
    }
}

extern "C" size_t reart_base_backward_cano_workspace_bytes(int P, int B) {
    if (P < 1 || P > TG_MAX_PB || B <= 0 || B > REART_MAX_POSE_LEN) return 0;
    return reart_align_up(sizeof(float) * 12 * (size_t)B * P, 256);
}

extern "C" int reart_base_backward_cano(const float *cano, int N, int P, int B, const float *W1, const float *b1, const float *W2,
                                        int H, const float *prop6d, const float *propt, const float *yT, const float *hT,
                                        const int32_t *hard_idx, float tau, const float *G, float *g_cano, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    if (N < 0 || P < 1 || P > TG_MAX_PB || B < 0 || B > REART_MAX_POSE_LEN || H < 1) return REART_ERR_INVALID_ARG;
    if (H > TG_MAX_H) return REART_ERR_UNSUPPORTED;
    if (N == 0) return REART_OK;
    (void)b1;                                         // the forward's hT carries the ReLU decision
    if (!cano || !W1 || !W2 || !yT || !hT || !hard_idx || !g_cano || !(tau > 0.f)) return REART_ERR_INVALID_ARG;
    if (B > 0 && (!prop6d || !propt || !G || !workspace || workspace_bytes < reart_base_backward_cano_workspace_bytes(P, B)))
        return REART_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    float *table = (float *)workspace;
    int tb = TG_CANO_POSE_FLOATS / (P * 12);          // >= 8
    if (tb > B) tb = B;
    if (B > 0)
        hipLaunchKernelGGL(rt_rows_kernel, dim3(reart_div_up(B * P, 256)), dim3(256), 0, st, prop6d, propt, B * P, table);
    const size_t lds = sizeof(float) * ((size_t)H * (TG_MAX_PB + 3) + 12 * (size_t)tb * P);   // <= 35 KiB + 12 KiB
    hipLaunchKernelGGL(base_cano_kernel, dim3(reart_div_up(N, TG_BS)), dim3(TG_BS), lds, st, cano, W1, W2, table, yT, hT, hard_idx,
                       tau, G, N, P, B, H, tb, g_cano);
    REART_CHECK_LAUNCH();
    return REART_OK;
}
