// reart_amd/csrc/kinpost.hip -- what the kinematic projection's iteration does between the assignment re-solve and the FK backward
// (reference run_robot.py:165-209 for `--model kinematic --use_assign_loss [--use_flow_loss]`): the matched pairs' loss and its
// gradient (:177-184), the flow targets of every frame pair (blend_anchor_motion x (T-1), :194-201), the flow loss (:203-209,
// networks/loss.py:10-21) and dL/d pc_trans of both -- as ONE entry point of nine launches.  reart_amd/kinematic_engine.py used to
// issue this part as ~45 launches (36 of them the per-frame searches and blends, the rest ATen tensor expressions: cat / sub /
// gather / index_put / mul / add): with the re-solve's median at 1.1 ms they were as long as the solve (round 6).
//
// The values are the ones the tensor expressions produced, operation for operation: dL/d pc_trans is bit-identical to the former
// path; the two loss sums are accumulated in double precision (the former path: torch's fp32 tree sums).
#include "common.h"
#include "internal.h"
#include "consumer_dev.h"
#include <math.h>

struct KinPostArgs {
    const float *pc_trans;   // [B][N][3] the articulated frames (canonical frame not among them)
    const float *cano;       // [N][3]
    int B, N, c;             // c = cano_idx: comp = pc_trans[:c] | cano | pc_trans[c:]   ([T = B + 1][N][3])
    float *comp, *pred;      // [T][N][3] | [B][N][3] = comp[f + 1] - comp[f]
    // assignment branch
    const float *pc_src;     // [B][n][3] the sampled source points as the solve saw them
    const float *tgt;        // [B][n][3]
    const int *cols;         // [B][n] the optimum
    const int *slot;         // [N] sample slot of canonical point p, or -1
    int n;
    float two_lambda, lambda_assign;
    // flow branch (gp null: none)
    const float *gp;         // [B][N][3] d flow loss / d pred
    const float *loss_flow;  // device scalar (unscaled flow loss)
    float lambda_flow;
    float *G;                // [B][N][3] out: dL / d pc_trans
    float *matched;          // [B][n][3] out (nullable): the matched target of every sampled point
    double *partial;         // [blocks] the assignment loss's partial sums
    float *losses;           // [3] out: lambda_assign x assignment loss | lambda_flow x flow loss | total
    // Chamfer input (reart_kin_post_recon only): losses is [4] then -- the two terms above | Chamfer loss | total
    const float *g_recon;    // [B][N][3] d Chamfer loss / d pc_trans, rows in the order the caller stored the cloud for its search
    const int *inv_x;        // [N] stored row of canonical point p (null: identity)
    const float *loss_recon; // device scalar
};

__global__ __launch_bounds__(256) void kin_comp_kernel(KinPostArgs a) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)a.N * 3, total = (size_t)(a.B + 1) * per;
    if (e >= total) return;
    const int ci = (int)(e / per);
    const size_t r = e - (size_t)ci * per;
    auto at = [&](int f) { return f < a.c ? a.pc_trans[(size_t)f * per + r] : (f == a.c ? a.cano[r] : a.pc_trans[(size_t)(f - 1) * per + r]); };
    const float v = at(ci);
    a.comp[e] = v;
    if (ci < a.B) a.pred[e] = at(ci + 1) - v;
}

#define KP_BS 256
// RECON: G starts from the Chamfer gradient of the point's stored row, the pairs' term and the flow term are added to it in this
// order, each sum rounded once (the fused relaxation step's rule for the same sum); without it the body is reart_kin_post's
template <bool RECON> __device__ __forceinline__ void kin_grad_body(const KinPostArgs &a, double *s_red) {
    const int fi = blockIdx.y, p = blockIdx.x * KP_BS + threadIdx.x;
    double acc = 0.0;
    if (p < a.N) {
        const size_t per = (size_t)a.N * 3, o = (size_t)fi * per + 3 * (size_t)p;
        float g0 = 0.f, g1 = 0.f, g2 = 0.f;
        if (RECON) {
            const int r = a.inv_x ? a.inv_x[p] : p;
            if (r >= 0 && r < a.N) {      // a row outside the cloud contributes nothing and is never read
                const float *q = a.g_recon + (size_t)fi * per + 3 * (size_t)r;
                g0 = q[0]; g1 = q[1]; g2 = q[2];
            }
        }
        const int sl = a.slot ? a.slot[p] : -1;
        if (sl >= 0) {
            const size_t so = ((size_t)fi * a.n + sl) * 3;
            const int cj = a.cols[(size_t)fi * a.n + sl];
            const float *t = a.tgt + ((size_t)fi * a.n + cj) * 3;
            const float d0 = a.pc_src[so] - t[0], d1 = a.pc_src[so + 1] - t[1], d2 = a.pc_src[so + 2] - t[2];
            if (RECON) { g0 = g0 + a.two_lambda * d0; g1 = g1 + a.two_lambda * d1; g2 = g2 + a.two_lambda * d2; }
            else { g0 = a.two_lambda * d0; g1 = a.two_lambda * d1; g2 = a.two_lambda * d2; }
            acc = (double)(d0 * d0) + (double)(d1 * d1) + (double)(d2 * d2);
            if (a.matched) { a.matched[so] = t[0]; a.matched[so + 1] = t[1]; a.matched[so + 2] = t[2]; }
        }
        if (a.gp) {
            // pred = comp[1:] - comp[:-1]: +gp to frame ci of the later pair, -gp of the earlier one; the canonical frame takes none
            const int ci = fi < a.c ? fi : fi + 1;
            const size_t r = 3 * (size_t)p;
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                float t = ci >= 1 ? a.gp[(size_t)(ci - 1) * per + r + x] * a.lambda_flow : 0.f;
                if (ci <= a.B - 1) t = t - a.gp[(size_t)ci * per + r + x] * a.lambda_flow;
                if (x == 0) g0 = g0 + t; else if (x == 1) g1 = g1 + t; else g2 = g2 + t;
            }
        }
        a.G[o] = g0; a.G[o + 1] = g1; a.G[o + 2] = g2;
    }
    acc = reart_block_sum_d<KP_BS>(acc, s_red);
    if (threadIdx.x == 0) a.partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}
__global__ __launch_bounds__(KP_BS) void kin_grad_kernel(KinPostArgs a) {
    __shared__ double s_red[KP_BS / 64];
    kin_grad_body<false>(a, s_red);
}
__global__ __launch_bounds__(KP_BS) void kin_grad_recon_kernel(KinPostArgs a) {
    __shared__ double s_red[KP_BS / 64];
    kin_grad_body<true>(a, s_red);
}

// The partials come from the launch before this one: plain loads (reart_partials_sum_d's agent-scope loads are for partials
// written inside the same launch and would change the scope of these)
template <bool RECON> __device__ __forceinline__ void kin_loss_body(const KinPostArgs &a, int blocks) {
    double t = 0.0;
    for (int e = threadIdx.x; e < blocks; e += 64) t += a.partial[e];
    t = reart_wave_sum_d(t);
    if (threadIdx.x == 0) {
        const float ass = a.lambda_assign * (float)t;
        const float fl = a.gp ? *a.loss_flow * a.lambda_flow : 0.f;
        if (RECON) {      // the order in which the operator loop adds them: assignment, Chamfer, flow
            const float rec = *a.loss_recon;
            a.losses[0] = ass; a.losses[1] = fl; a.losses[2] = rec; a.losses[3] = (ass + rec) + fl;
        } else {
            a.losses[0] = ass; a.losses[1] = fl; a.losses[2] = ass + fl;
        }
    }
}
__global__ __launch_bounds__(64) void kin_loss_kernel(KinPostArgs a, int blocks) { kin_loss_body<false>(a, blocks); }
__global__ __launch_bounds__(64) void kin_loss_recon_kernel(KinPostArgs a, int blocks) { kin_loss_body<true>(a, blocks); }

// the flow loss's and the batched blend's own workspaces come last, each at the size its operator reports (flow only)
struct KinPostWs { float *comp, *pred, *gt, *gp, *loss_flow; uint8_t *mask; double *partial; char *fl, *blend; size_t blend_bytes; };
static size_t kp_layout(int B, int N, int nr_max, int k, bool flow, void *workspace, KinPostWs *w) {
    reart_arena ws(workspace);
    const size_t pts = (size_t)N * 3;
    w->comp = ws.take<float>(pts * (B + 1)); w->pred = ws.take<float>(pts * B);
    w->gt = ws.take<float>(pts * B); w->mask = ws.take<uint8_t>((size_t)B * N);
    w->gp = ws.take<float>(pts * B); w->loss_flow = ws.take<float>(1);
    w->partial = ws.take<double>((size_t)B * reart_div_up(N, KP_BS));
    w->fl = ws.take<char>(flow ? reart_flow_loss_workspace_bytes() : 0);
    w->blend_bytes = flow ? reart_blend_anchor_motion_batch_workspace_bytes(B, N, nr_max, k) : 0;
    w->blend = ws.take<char>(w->blend_bytes, 1);
    return ws.off;
}

extern "C" size_t reart_kin_post_workspace_bytes(int B, int N, int nr_max, int k) {
    if (B <= 0 || N <= 0) return 0;
    KinPostWs w;
    return kp_layout(B, N, nr_max > 0 ? nr_max : 1, k > 0 ? k : 1, nr_max > 0, nullptr, &w);
}

// both entries: `recon` selects the kernels that start G from the Chamfer gradient and write four losses
static int kp_run(const float *pc_trans, const float *cano, int B, int N, int cano_idx, const float *pc_src, const float *tgt,
                  const int32_t *cols, const int32_t *slot_of_point, int n, float lambda_assign, const float *ref,
                  const float *ref_flow, const int64_t *ref_len, int nr_max, int k, int euclidean, float lambda_flow, int robust,
                  float smooth_weight, float *G, float *matched, float *losses, void *workspace, size_t workspace_bytes,
                  void *stream, bool recon, const float *g_recon, const int32_t *inv_x, const float *loss_recon) {
    if (B < 1 || N < 1 || n < 0 || cano_idx < 0 || cano_idx > B) return REART_ERR_INVALID_ARG;
    if (!pc_trans || !cano || !G || !losses || !workspace) return REART_ERR_INVALID_ARG;
    if (n > 0 && (!pc_src || !tgt || !cols || !slot_of_point)) return REART_ERR_INVALID_ARG;
    const bool flow = ref != nullptr;
    if (flow && (!ref_flow || nr_max < k || k < 1)) return REART_ERR_INVALID_ARG;
    KinPostWs w;
    if (workspace_bytes < kp_layout(B, N, flow ? nr_max : 1, flow ? k : 1, flow, workspace, &w)) return REART_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    KinPostArgs a{};
    a.pc_trans = pc_trans; a.cano = cano; a.B = B; a.N = N; a.c = cano_idx;
    a.comp = w.comp; a.pred = w.pred;
    a.pc_src = pc_src; a.tgt = tgt; a.cols = cols; a.slot = n > 0 ? slot_of_point : nullptr; a.n = n;
    a.two_lambda = (float)(2.0 * (double)lambda_assign); a.lambda_assign = lambda_assign;
    a.gp = flow ? w.gp : nullptr; a.loss_flow = w.loss_flow; a.lambda_flow = lambda_flow;
    a.G = G; a.matched = matched; a.partial = w.partial; a.losses = losses;
    a.g_recon = g_recon; a.inv_x = inv_x; a.loss_recon = loss_recon;
    if (flow) {
        const size_t total = (size_t)(B + 1) * N * 3;
        hipLaunchKernelGGL(kin_comp_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
        REART_CHECK_LAUNCH();
        int rc = reart_blend_anchor_motion_batch(a.comp, ref, ref_flow, ref_len, B, N, nr_max, k, euclidean, w.gt, w.mask, w.blend,
                                                 w.blend_bytes, stream);
        if (rc != REART_OK) return rc;
        rc = reart_flow_loss(w.gt, a.pred, w.mask, B, N, robust, smooth_weight, w.loss_flow, w.gp, w.fl,
                             reart_flow_loss_workspace_bytes(), stream);
        if (rc != REART_OK) return rc;
    }
    const int gx = reart_div_up(N, KP_BS);
    if (recon) hipLaunchKernelGGL(kin_grad_recon_kernel, dim3(gx, B), dim3(KP_BS), 0, st, a);
    else hipLaunchKernelGGL(kin_grad_kernel, dim3(gx, B), dim3(KP_BS), 0, st, a);
    REART_CHECK_LAUNCH();
    if (recon) hipLaunchKernelGGL(kin_loss_recon_kernel, dim3(1), dim3(64), 0, st, a, gx * B);
    else hipLaunchKernelGGL(kin_loss_kernel, dim3(1), dim3(64), 0, st, a, gx * B);
    REART_CHECK_LAUNCH();
    return REART_OK;
}

extern "C" int reart_kin_post(const float *pc_trans, const float *cano, int B, int N, int cano_idx, const float *pc_src, const float *tgt,
                              const int32_t *cols, const int32_t *slot_of_point, int n, float lambda_assign, const float *ref,
                              const float *ref_flow, const int64_t *ref_len, int nr_max, int k, int euclidean, float lambda_flow, int robust,
                              float smooth_weight, float *G, float *matched, float *losses, void *workspace, size_t workspace_bytes,
                              void *stream) {
    return kp_run(pc_trans, cano, B, N, cano_idx, pc_src, tgt, cols, slot_of_point, n, lambda_assign, ref, ref_flow, ref_len, nr_max, k,
                  euclidean, lambda_flow, robust, smooth_weight, G, matched, losses, workspace, workspace_bytes, stream, false, nullptr,
                  nullptr, nullptr);
}

// reart_kin_post with the Chamfer term's gradient and value as inputs (the engine's recon_with_assign mode): the same launches,
// G = Chamfer gradient (through inv_x) + pairs' term + flow term, losses [4].  n = 0: the Chamfer-only form (with or without flow)
extern "C" int reart_kin_post_recon(const float *pc_trans, const float *cano, int B, int N, int cano_idx, const float *pc_src,
                                    const float *tgt, const int32_t *cols, const int32_t *slot_of_point, int n, float lambda_assign,
                                    const float *ref, const float *ref_flow, const int64_t *ref_len, int nr_max, int k, int euclidean,
                                    float lambda_flow, int robust, float smooth_weight, const float *g_recon, const int32_t *inv_x,
                                    const float *loss_recon, float *G, float *matched, float *losses, void *workspace,
                                    size_t workspace_bytes, void *stream) {
    if (!g_recon || !loss_recon) return REART_ERR_INVALID_ARG;
    return kp_run(pc_trans, cano, B, N, cano_idx, pc_src, tgt, cols, slot_of_point, n, lambda_assign, ref, ref_flow, ref_len, nr_max, k,
                  euclidean, lambda_flow, robust, smooth_weight, G, matched, losses, workspace, workspace_bytes, stream, true, g_recon,
                  inv_x, loss_recon);
}
