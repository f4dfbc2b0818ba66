/*
 * reart_hip.h -- C ABI of libreart_hip.so: the MI355X (gfx950) implementation of
 * reart's per-iteration point-cloud hot path.
 *
 * Conventions:
 *   - plain pointers + sizes, no torch / pybind types; every pointer is a DEVICE
 *     pointer unless the parameter name starts with `h_`;
 *   - the library never allocates, frees or retains device memory: outputs and
 *     scratch are caller-owned (sizes from the *_workspace_bytes queries);
 *   - every entry point is asynchronous on the hipStream_t passed as `stream`
 *     (void* so that this header needs no HIP headers), re-entrant, does no host
 *     read of device data and is therefore hipGraph-capture safe;
 *   - return value: REART_OK (0) or a negative reart_status; never exit(), never
 *     throws.  (The reference's wrappers return 1 and exit(-1) on launch failure,
 *     networks/pointnet_lib/src/ball_query.cpp:25, ball_query_gpu.cu:62-66.)
 *   - fp32 data, int64 indices at the chamferdist / knn_cuda boundaries, int32 at
 *     the pointnet2_cuda boundary, exactly as the reference interfaces; the K-NN
 *     forward also takes fp64 clouds (reart_knn_points_idx_f64), as upstream's does.
 *
 * Each entry point names the reference interface (file:line under the upstream
 * stevenlsw/reart tree) it replaces.
 */
#ifndef REART_HIP_H
#define REART_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    REART_OK = 0,
    REART_ERR_INVALID_ARG = -1,   /* null pointer, negative size, bad enum      */
    REART_ERR_UNSUPPORTED = -2,   /* e.g. D > REART_MAX_D, K > REART_MAX_K_LIST  */
    REART_ERR_LAUNCH = -3,        /* hipGetLastError() after a launch            */
    REART_ERR_NO_DEVICE = -4      /* no HIP device visible                       */
} reart_status;

#define REART_MAX_K 16            /* neighbours kept in registers per query      */
#define REART_MAX_K_LIST 1024     /* K-NN searches with K > REART_MAX_K keep a    */
                                  /* sorted key list per query in LDS (one wave   */
                                  /* per query); above this they are unsupported  */
#define REART_MAX_POSE_LEN 1024   /* frames B = T - 1 of the relaxation model and   */
                                  /* the fused step: 1 <= B <= REART_MAX_POSE_LEN   */
#define REART_MAX_D 256           /* point dimension of the K-NN searches and     */
                                  /* their backward: 1 <= D <= REART_MAX_D        */

/* Library / device probes (host side, no device work). */
int reart_version(void);                       /* 100*major + minor              */
int reart_device_count(void);                  /* 0 when no GPU is visible       */
const char *reart_status_string(int status);

/* ------------------------------------------------------------------------ */
/* K-nearest neighbours / Chamfer                                            */
/* ------------------------------------------------------------------------ */

/* Replaces chamferdist._C.knn_points_idx(p1,p2,lengths1,lengths2,K,version)
 * (utils/chamfer.py:174; contract in the docstring :145-171).
 *   p1 [N,P1,D], p2 [N,P2,D] f32 contiguous, 1 <= D <= REART_MAX_D (D = 0: invalid
 *   argument, D > REART_MAX_D: unsupported); lengths1/2 [N] i64 or NULL (= full);
 *   dists [N,P1,K] f32 squared L2, idx [N,P1,K] i64 into p2, ascending by
 *   (distance, index); rows >= lengths1[n] and slots >= lengths2[n] are zero.
 * Distance contract: ((d0*d0)+(d1*d1))+(d2*d2)+... with dc = p1[c]-p2[c], summed in
 * ascending c, fp32, no FMA; ties -> lowest j.
 * 1 <= K <= REART_MAX_K_LIST.  D = 3: K <= REART_MAX_K runs the register-list kernels,
 * larger K the LDS-list kernel; D != 3: the any-D LDS-list kernel of csrc/knn_anyd.hip (same
 * result contract).
 * workspace (SoA target image + per-slice partial results; D != 3 also a query image):
 *   reart_knn_points_workspace_bytes_d(N,P1,P2,D,K) bytes (0 when D or K is out of range);
 *   reart_knn_points_workspace_bytes(N,P1,P2,K) is the D = 3 size. */
size_t reart_knn_points_workspace_bytes(int N, int P1, int P2, int K);
size_t reart_knn_points_workspace_bytes_d(int N, int P1, int P2, int D, int K);
int reart_knn_points_idx(const float *p1, const float *p2,
                         const int64_t *lengths1, const int64_t *lengths2,
                         int N, int P1, int P2, int D, int K,
                         float *dists, int64_t *idx,
                         void *workspace, size_t workspace_bytes, void *stream);

/* The float64 form of chamferdist._C.knn_points_idx (the upstream forward dispatches
 * on float and double and returns dists in the input's dtype).  Same arguments, status
 * codes and contract as reart_knn_points_idx with double in place of float:
 *   p1 [N,P1,D], p2 [N,P2,D] f64 contiguous, 1 <= D <= REART_MAX_D, 1 <= K <= REART_MAX_K_LIST
 *   (0: invalid argument, above: unsupported); dists [N,P1,K] f64 squared L2, idx [N,P1,K] i64,
 *   ascending by (distance, index); rows >= lengths1[n] and slots >= lengths2[n] are zero.
 * Distance contract: ((d0*d0)+(d1*d1))+(d2*d2)+... with dc = p1[c]-p2[c], summed in ascending
 * c, every operation a correctly rounded fp64 one: no FMA, no matrix cores.  NaN / Inf
 * coordinates are outside the contract.  One kernel serves every D and K (csrc/knn_anyd.hip,
 * the any-D search in double).
 * There is no float64 backward (the upstream backward is float-only).
 * workspace: reart_knn_points_workspace_bytes_f64(N,P1,P2,D,K) bytes (0 when D or K is out of range). */
size_t reart_knn_points_workspace_bytes_f64(int N, int P1, int P2, int D, int K);
int reart_knn_points_idx_f64(const double *p1, const double *p2,
                             const int64_t *lengths1, const int64_t *lengths2,
                             int N, int P1, int P2, int D, int K,
                             double *dists, int64_t *idx,
                             void *workspace, size_t workspace_bytes, void *stream);

/* Replaces chamferdist._C.knn_points_backward(p1,p2,lengths1,lengths2,idx,grad_dists)
 * (utils/chamfer.py:206-208).  p1 [N,P1,D], p2 [N,P2,D], 1 <= D <= REART_MAX_D;
 * grad_p1 [N,P1,D], grad_p2 [N,P2,D] are fully written (zero where nothing
 * contributes).  Deterministic: the scatter into grad_p2 is a per-target gather
 * over a counting sort of idx, summed in ascending (i,k) order with
 * v = (2g)*diff, g1 += v, g2 -= v -- no float atomics.  The workspace does not
 * depend on D.
 *   workspace: reart_knn_points_backward_workspace_bytes(N,P1,P2,K) bytes. */
size_t reart_knn_points_backward_workspace_bytes(int N, int P1, int P2, int K);
int reart_knn_points_backward(const float *p1, const float *p2,
                              const int64_t *lengths1, const int64_t *lengths2,
                              const int64_t *idx, const float *grad_dists,
                              int N, int P1, int P2, int D, int K,
                              float *grad_p1, float *grad_p2,
                              void *workspace, size_t workspace_bytes, void *stream);

/* Both directions of ChamferDistance.forward(bidirectional=True)
 * (utils/chamfer.py:78-123) in one launch: x,y [N,P,3];
 *   d_xy/i_xy: NN of each x point in y; d_yx/i_yx: NN of each y point in x. */
size_t reart_chamfer_bidir_workspace_bytes(int N, int P);
int reart_chamfer_bidir(const float *x, const float *y, int N, int P,
                        float *d_xy, int64_t *i_xy, float *d_yx, int64_t *i_yx,
                        void *workspace, size_t workspace_bytes, void *stream);

/* Replaces knn_cuda.KNN(k, transpose_mode=True).forward(ref, query)
 * (run_robot.py:65-66,122; shape contract utils/model_utils.py:42):
 *   ref [B,nr,D], query [B,nq,D] -> dist [B,nq,k] ascending, idx [B,nq,k] i64,
 *   1 <= D <= REART_MAX_D (distance contract of reart_knn_points_idx).
 * euclidean != 0: dist = sqrt(squared distance) (upstream KNN_CUDA 0.2).
 * 1 <= k <= min(nr, REART_MAX_K_LIST).
 * workspace: reart_knn_points_workspace_bytes_d(B, nq, nr, D, k). */
int reart_knn_cuda(const float *ref, const float *query, int B, int nr, int nq,
                   int D, int k, int euclidean, float *dist, int64_t *idx,
                   void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------ */
/* Flow loss                                                                 */
/* ------------------------------------------------------------------------ */

/* Replaces blend_anchor_motion(query_loc, reference_loc, reference_flow, knn, return_mask=True)
 * (utils/flow_utils.py:147-170) including its knn_cuda.KNN(k) call (:158):
 *   query [nq,3], ref [nr,3], ref_flow [nr,3] -> flow [nq,3], mask [nq] (uint8 0/1). */
size_t reart_blend_anchor_motion_workspace_bytes(int nq, int nr, int k);
int reart_blend_anchor_motion(const float *query, const float *ref, const float *ref_flow,
                              int nq, int nr, int k, int euclidean,
                              float *flow, uint8_t *mask,
                              void *workspace, size_t workspace_bytes, void *stream);

/* The T-1 calls of blend_anchor_motion an iteration makes (run_robot.py:194-201: one per frame pair; utils/flow_utils.py:147-170)
 * as one: query [B,nq,3], ref / ref_flow [B,nr_max,3] (every frame's reference set padded to the longest), ref_len [B] int64 the
 * true lengths (NULL: all nr_max; each >= k) -> flow [B,nq,3], mask [B,nq].  Bit for bit what B calls of
 * reart_blend_anchor_motion return (one search over the batch with per-batch target lengths, one blend launch). */
size_t reart_blend_anchor_motion_batch_workspace_bytes(int B, int nq, int nr_max, int k);
int reart_blend_anchor_motion_batch(const float *query, const float *ref, const float *ref_flow, const int64_t *ref_len,
                                    int B, int nq, int nr_max, int k, int euclidean, float *flow, uint8_t *mask,
                                    void *workspace, size_t workspace_bytes, void *stream);

/* The kinematic projection's iteration between the assignment re-solve and the FK backward, as one call (csrc/kinpost.hip;
 * run_robot.py:165-209 for `--model kinematic --use_assign_loss [--use_flow_loss]`):
 *   assignment branch (:177-184)  loss = lambda_assign x sum |pc_src - tgt[cols]|^2 over the n sampled points of every frame, its
 *                                 gradient scattered to the sampled points' places in dL/d pc_trans (slot_of_point [N]: sample slot
 *                                 of canonical point p or -1; pc_src [B,n,3] = the sampled points of pc_trans as the solve saw them;
 *                                 tgt [B,n,3]; cols [B,n] the optimum) -- n = 0: no such branch;
 *   flow branch (:194-209)        comp = pc_trans[:cano_idx] | cano | pc_trans[cano_idx:]; blend_anchor_motion of every frame pair
 *                                 (reart_blend_anchor_motion_batch: ref / ref_flow [B,nr_max,3], ref_len [B] or NULL), flow_loss of
 *                                 comp[1:] - comp[:-1] against it (robust, smooth_weight), times lambda_flow; ref = NULL: none.
 * Outputs: G [B,N,3] = dL/d pc_trans of both branches (bit for bit what the reference's tensor expressions give through autograd's
 * operator order), matched [B,n,3] (nullable) the matched targets, losses [3] (device) = the assignment term, the flow term, their
 * sum.  workspace: reart_kin_post_workspace_bytes(B, N, nr_max or 0, k).  Nine launches on `stream`, no host synchronisation. */
size_t reart_kin_post_workspace_bytes(int B, int N, int nr_max, int k);
int reart_kin_post(const float *pc_trans, const float *cano, int B, int N, int cano_idx, const float *pc_src, const float *tgt,
                   const int32_t *cols, const int32_t *slot_of_point, int n, float lambda_assign, const float *ref,
                   const float *ref_flow, const int64_t *ref_len, int nr_max, int k, int euclidean, float lambda_flow, int robust,
                   float smooth_weight, float *G, float *matched, float *losses, void *workspace, size_t workspace_bytes,
                   void *stream);

/* reart_kin_post with the Chamfer term of the same iteration as an input (run_real.py:175-203 / run_sapien.py:174-203 of the
 * reference add recon_loss in every iteration and ass_loss on top of it from --assign_iter on; KinematicEngine's
 * recon_with_assign mode).  The arguments of reart_kin_post, plus
 *   g_recon [B,N,3]  d Chamfer loss / d predicted cloud (reart_chamfer_loss's grad_x), its rows in the order in which the caller
 *                    stored that cloud for the search;
 *   inv_x [N] i32    the stored row of canonical point p; NULL: identity.  An entry outside [0, N) is range-checked: that point
 *                    takes no Chamfer gradient and nothing is read for it;
 *   loss_recon       device scalar, the Chamfer loss;
 *   losses [4]       lambda_assign x assignment loss (0 when n = 0) | lambda_flow x flow loss | *loss_recon |
 *                    fl(fl(losses[0] + losses[2]) + losses[1]) -- the order in which the operator loop adds them.
 * G[b][p][c] is built in this order, every sum rounded once to float32 (the fused relaxation step's rule for the same sum):
 * g = g_recon[b][inv_x[p]][c]; at a sampled point g = g + two_lambda x d_c; with the flow branch g = g + t_c -- two_lambda, d_c
 * and t_c exactly the values reart_kin_post forms.  n = 0 is the Chamfer-only form, with or without flow (the iterations before
 * --assign_iter).  NULL g_recon or loss_recon: REART_ERR_INVALID_ARG; every other refusal, the workspace
 * (reart_kin_post_workspace_bytes) and the number of launches are reart_kin_post's; no host synchronisation, no atomics. */
int reart_kin_post_recon(const float *pc_trans, const float *cano, int B, int N, int cano_idx, const float *pc_src, const float *tgt,
                         const int32_t *cols, const int32_t *slot_of_point, int n, float lambda_assign, const float *ref,
                         const float *ref_flow, const int64_t *ref_len, int nr_max, int k, int euclidean, float lambda_flow, int robust,
                         float smooth_weight, const float *g_recon, const int32_t *inv_x, const float *loss_recon, float *G,
                         float *matched, float *losses, void *workspace, size_t workspace_bytes, void *stream);

/* Replaces flow_loss(gt_flow_list, pred_flow_list, flow_mask_list, robust, smooth_weight)
 * (networks/loss.py:10-21): gt, pred [B,N,3]; mask [B,N] uint8 or NULL (= all ones);
 * loss: device float scalar; grad_pred [B,N,3] or NULL = d loss / d pred. */
size_t reart_flow_loss_workspace_bytes(void);
int reart_flow_loss(const float *gt, const float *pred, const uint8_t *mask, int B, int N,
                    int robust, float smooth_weight, float *loss, float *grad_pred,
                    void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------ */
/* Relaxation model (BaseModel) and rigid transforms                         */
/* ------------------------------------------------------------------------ */

/* Replaces BaseModel.forward(cano_pc, tau=...) (networks/model.py:39-70): seg head
 * 3->H->P (networks/blocks.py:99-118; W1 [H,3], b1 [H], W2 [P,H], last layer bias-free),
 * hard Gumbel-softmax with the -log(Exp(1)) noise `gumbel` [N,P] supplied by the caller
 * (F.gumbel_softmax draws it from torch's generator), rotation_6d_to_matrix
 * (screw_se3/geo_utils.py:632-651) and the per-part rigid apply.
 *   out [B,N,3]; seg_part [N] i64 = arg-max of the noise-free logits (:70);
 *   trans_list [B,P,4,4]; saved for backward: yT [P,N], hT [H,N], hard_idx [N] i32.
 *   seg_part / trans_list / yT / hT / hard_idx may be NULL.  P <= 32.  A pose table [B,P] that fits in LDS is
 *   served by the kernels of model.hip, a longer one (up to B = REART_MAX_POSE_LEN) by model_long.hip: the same
 *   arithmetic per element, the same results bit for bit (see reart_base_path). */
int reart_base_forward(const float *cano, int N, int P, int B,
                       const float *W1, const float *b1, const float *W2, int H,
                       const float *prop6d, const float *propt,
                       const float *gumbel, float tau,
                       float *out, int64_t *seg_part, float *trans_list,
                       float *yT, float *hT, int32_t *hard_idx, void *stream);

/* The noise F.gumbel_softmax(logits, tau, hard=True) adds (networks/model.py:44: -log(Exp(1)) samples from torch's
 * generator) as the fused step draws it IN the forward kernel when reart_relax_buffers.gumbel is NULL: a Philox4x32-10
 * stream keyed by `seed`, counter (point, part / 4, iteration).  out [N,P] = exactly the samples iteration `iter` of an
 * engine with that seed uses, so the production path can be checked (distribution, independence) and replayed
 * (inject `out` as `gumbel`: same bits).  */
int reart_gumbel_noise(uint64_t seed, int64_t iter, int N, int P, float *out, void *stream);

/* Backward of the above (the reference relies on autograd): G = dL/d out [B,N,3] ->
 * gradients of W1, b1, W2, proposal_6d [B,P,6], proposal_t [B,P,3].  Deterministic
 * (fixed-order chunked reductions, no atomics).
 *   hT may be NULL where the pose table fits in LDS (reart_base_path(..., 1) == 0): the kernel then re-evaluates the hidden
 *   layer from cano, W1 and b1 with the forward's own expression -- the same gradients bit for bit, and the forward need not
 *   save hT (the fused step does not).  With hT the call reads it as before and ignores W1 / b1.  The long path needs hT:
 *   REART_ERR_UNSUPPORTED without it. */
size_t reart_base_backward_workspace_bytes(int N, int P, int B, int H);
/* Which kernels serve the model at a shape: 0 = pose table [B*P][12] (backward: also the gradient tile [B][64*3]) in LDS,
 * 1 = the long path (forward: pose rows from a table in global memory; backward: frames in LDS tiles), chosen by fit alone
 * and only where 0 does not fit; REART_ERR_UNSUPPORTED where neither serves (P > 32, B > REART_MAX_POSE_LEN beyond what
 * fits in LDS, H too large for LDS).  backward: 0 = reart_base_forward, 1 = reart_base_backward.  The launchers decide
 * with this very function.  Needs no device. */
int reart_base_path(int P, int B, int H, int backward);
int reart_base_backward(const float *cano, int N, int P, int B,
                        const float *W1, const float *b1, const float *W2, int H,
                        const float *prop6d, const float *propt,
                        const float *yT, const float *hT, const int32_t *hard_idx, float tau,
                        const float *G,
                        float *gW1, float *gb1, float *gW2, float *g6d, float *gt,
                        void *workspace, size_t workspace_bytes, void *stream);

/* Replaces compute_pc_transform(cano_pc, pose_list, cano_part) (utils/model_utils.py:54-67)
 * and the hard-label apply of KinematicModel.forward (networks/model.py:161-165):
 *   cano [N,3], pose [B,P,4,4], part [N] i64 -> out [B,N,3]. */
int reart_compute_pc_transform(const float *cano, const float *pose, const int64_t *part,
                               int N, int P, int B, float *out, void *stream);

/* Replaces rotation_6d_to_matrix (screw_se3/geo_utils.py:632-651): d6 [n,6] -> R [n,3,3]. */
int reart_rotation_6d_to_matrix(const float *d6, int n, float *R, void *stream);

/* ---- First-order gradients through the transforms (transform_grad.hip).  The reference gets them from autograd: its
 * trans_list, fk(...), compute_pc_transform and cano_pc are ordinary tensors.  float32; deterministic (fixed-order sums, no
 * atomics: two runs agree bit for bit); no host synchronisation, capturable; bad arguments are refused before any launch. */

/* Backward of reart_rotation_6d_to_matrix: d6 [n,6], gR = dL/dR [n,3,3] -> g6 [n,6].  The Gram-Schmidt backward of
 * screw_se3/geo_utils.py:632-651 with F.normalize's eps: a vector of norm <= 1e-12 is divided by 1e-12 and its gradient too. */
int reart_rotation_6d_to_matrix_backward(const float *d6, const float *gR, int n, float *g6, void *stream);

/* Backward of reart_compute_pc_transform: cano [N,3], pose [B,P,4,4], part [N] i64, G = dL/d out [B,N,3] ->
 *   g_cano [N,3] = sum_b R[b,part_n]^T G[b,n], b ascending (a label outside [0,P): zero);
 *   g_pose [B,P,4,4]: rows 0..2 = [ sum_{n in p} G[b,n] x_n^T | sum_{n in p} G[b,n] ], the points added as reart_fk_backward
 *   adds them (ascending inside a slice of the cloud, the slices in ascending order); row 3 = 0; a part without points: zeros.
 * Either output may be NULL (not computed); the workspace is needed for g_pose only.  P <= 1024: REART_ERR_INVALID_ARG above
 * (the workspace query then returns 0). */
size_t reart_compute_pc_transform_backward_workspace_bytes(int N, int P, int B);
int reart_compute_pc_transform_backward(const float *cano, const float *pose, const int64_t *part, const float *G,
                                        int N, int P, int B, float *g_cano, float *g_pose,
                                        void *workspace, size_t workspace_bytes, void *stream);

/* BaseModel.forward's trans_list is [rotation_6d_to_matrix(proposal_6d) | proposal_t] (networks/model.py:60-68): an upstream
 * g_trans [n,4,4] on it (n = B*P rows) -> gt (+)= g_trans[:, :3, 3], g6d (+)= the 6D backward of g_trans[:, :3, :3] at p6d [n,6].
 * Row 3 is ignored.  accumulate != 0 adds onto g6d / gt (what reart_base_backward left there), 0 overwrites them.  A kernel of
 * its own over the rows: every pose_len of the model is served alike. */
int reart_pose_trans_backward(const float *p6d, const float *g_trans, int n, float *g6d, float *gt, int accumulate, void *stream);

/* Gradient of the canonical cloud through reart_base_forward: the arguments of reart_base_backward (yT, hT, hard_idx as the
 * forward saved them, all required; b1 is not read: hT carries the ReLU decision) -> g_cano [N,3] = the sum of
 *   the rigid term            sum_b R[b,hard_n]^T G[b,n], and
 *   the straight-through term dL/dw_p = sum_b G[b,n] . (R_bp x_n + t_bp) -> softmax backward with 1/tau -> W2^T -> the
 *                             forward's ReLU activity (hT > 0) -> W1^T.
 * The hard part and the ReLU activity are the forward's decisions.  The pose table [B*P][12] is built into the workspace and
 * read from there, whichever kernels served the forward (reart_base_path).  P <= 32, B <= REART_MAX_POSE_LEN
 * (REART_ERR_INVALID_ARG above; the workspace query then returns 0); H <= 256 (REART_ERR_UNSUPPORTED above). */
size_t reart_base_backward_cano_workspace_bytes(int P, int B);
int reart_base_backward_cano(const float *cano, int N, int P, int B,
                             const float *W1, const float *b1, const float *W2, int H,
                             const float *prop6d, const float *propt,
                             const float *yT, const float *hT, const int32_t *hard_idx, float tau,
                             const float *G, float *g_cano,
                             void *workspace, size_t workspace_bytes, void *stream);

/* One torch.optim.Adam step on one tensor (run_robot.py:145-151,219-221; amsgrad off,
 * weight_decay 0).  `step` is the 1-based step count. */
int reart_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                    int n, int step, float lr, float beta1, float beta2, float eps,
                    void *stream);

/* The same step on up to 8 tensors in ONE launch (run_robot.py:145-151: one optimizer over theta / axis / moment, each a
 * few hundred floats): param / grad / exp_avg / exp_avg_sq are HOST arrays of `count` device pointers, n and lr host arrays
 * of their sizes and learning rates, read at the call.  Same arithmetic per element as reart_adam_step. */
int reart_adam_step_multi(int count, float *const *param, const float *const *grad, float *const *exp_avg,
                          float *const *exp_avg_sq, const int *n, const float *lr, int step, float beta1, float beta2,
                          float eps, void *stream);

/* torch.optim.Adam's step for a user's own loop (reart_amd.optim.Adam): up to REART_ADAM_MAX_TENSORS tensors of any sizes,
 * of one or several parameter groups, in ONE launch.  `tensors` is a HOST array of `count` records, read at the call and
 * passed to the kernel by value (no table is copied to device memory, nothing is allocated, no synchronisation):
 *   param, grad, exp_avg, exp_avg_sq: device float32 arrays of n elements, 4-byte alignment suffices (a view at any element
 *     offset); grad is read only; max_exp_avg_sq: the amsgrad maximum, or NULL for no amsgrad;
 *   step_size = lr / (1 - beta1^step) and bias_correction2_sqrt = sqrt(1 - beta2^step) of THIS tensor's 1-based step count,
 *     formed in double by the caller as torch's non-capturable path forms them (torch keeps `step` per parameter and lr /
 *     weight_decay per group, hence per record); weight_decay: torch's L2 form g = fma(weight_decay, p, g) (0: none);
 *     maximize != 0: the gradient is negated.  Neither changes `grad` in memory.
 * Per element, float32, every rounding as written, fused where torch's multi-tensor kernels fuse (csrc/adam.hip):
 *   m = fma(1 - beta1, g - m, m);  v = fma(1 - beta2, g * g, v * beta2);  vmax = max(vmax, v);
 *   p = fma(-step_size, m / (sqrt(v or vmax) / bias_correction2_sqrt + eps), p)
 * with 1 - beta1 and 1 - beta2 formed in double and rounded once.  Tensors whose betas or eps differ go into separate
 * calls, more than REART_ADAM_MAX_TENSORS tensors into several.  A record with n = 0 touches nothing (its pointers may be
 * NULL); a call whose records are all empty launches nothing.  Refused before any launch and without touching a device,
 * REART_ERR_INVALID_ARG: count < 0 or above the limit, a NULL table with count > 0, n < 0, a NULL param / grad / exp_avg /
 * exp_avg_sq with n > 0, a bias_correction2_sqrt that is not finite and positive. */
#define REART_ADAM_MAX_TENSORS 32
typedef struct reart_adam_tensor {
    float *param;
    const float *grad;
    float *exp_avg, *exp_avg_sq;
    float *max_exp_avg_sq;
    int n;
    float step_size, bias_correction2_sqrt, weight_decay;
    int maximize;
} reart_adam_tensor;
int reart_adam_groups(const reart_adam_tensor *tensors, int count, double beta1, double beta2, double eps, void *stream);

/* ------------------------------------------------------------------------ */
/* Fused relaxation iteration                                                */
/* ------------------------------------------------------------------------ */

/* One iteration of the reference's optimisation loop (run_robot.py:154-221, branch
 * "Chamfer reconstruction loss [+ flow loss]", i.e. i < assign_iter): BaseModel forward
 * with in-kernel Gumbel noise, recon_loss, blend_anchor_motion x (T-1) + flow_loss,
 * backward, Adam with the reference's two parameter groups, cosine temperature schedule.
 * Everything that changes between iterations (counter, RNG offset, tau, loss log) lives in
 * device memory, so one call enqueues a fixed launch sequence: capture it once in a
 * hipGraph / torch.cuda.CUDAGraph and replay. */
typedef struct reart_relax_config {
    int N, P, B, H;          /* points, parts (<=32), frames-1 (<= REART_MAX_POSE_LEN), seg-head width (128) */
    int cano_idx;            /* position of the canonical frame in the T = B+1 sequence   */
    int use_flow;            /* --use_flow_loss                                           */
    int robust;              /* --use_robust_loss (Huber, delta 1)                        */
    int euclidean;           /* knn_cuda distance convention: 1 = sqrt (upstream)         */
    int flow_k;              /* neighbours blended; 3 (run_robot.py:66)                   */
    int M_max;               /* largest flow reference set                                */
    int M_total;             /* sum of the reference set sizes                            */
    int n_iter;              /* --n_iter: period of the cosine schedule                   */
    int ring;                /* rows in the loss log                                      */
    float lambda_flow;       /* --lambda_flow                                             */
    float smooth_weight;     /* flow_loss smooth_weight, 1e-2                             */
    float trans_lr, seg_lr;  /* --trans_lr, --seg_lr                                      */
    float beta1, beta2, eps; /* Adam defaults 0.9, 0.999, 1e-8                            */
    float start_tau, end_tau;/* --start_tau, --end_tau                                    */
    float fixed_tau;         /* > 0: frozen temperature (resume, run_robot.py:96-97)      */
    /* The newest field stands in the four bytes of padding in front of the 8-byte `seed`, where a caller that zeroes the */
    /* struct has always left 0: every older field keeps its offset and the struct its size.                             */
    int recon_with_assign;   /* 1: with use_assign, the Chamfer loss stays and the assignment loss is added to it, as the   */
                             /*    reference's run_real.py:175-203 / run_sapien.py:174-203 do: the searches and the Chamfer */
                             /*    consumer run as with use_assign = 0, and that consumer adds the term of `assign_map` in   */
                             /*    the same launch: G = fl(G_chamfer + fl(lambda_assign * fl(2 (x - y_map)))) per component, */
                             /*    G_chamfer itself where the map holds -1 (or anything outside [0, N)).  Without use_assign */
                             /*    it means nothing.  Sizes the workspace: fixed for an instance's life.  0: the default      */
    uint64_t seed;           /* Philox key of the Gumbel noise                            */
    int use_grid;            /* 1: exact grid search for the static targets (pc_list, flow */
                             /*    references); 0: brute force everywhere (same results)   */
    int use_boxes;           /* 1: bounding-box block-skip test in the brute-force searches */
                             /*    (exact; pays off when the clouds are stored in Morton order) */
    int use_assign;          /* 1: the assignment loss replaces the Chamfer loss (run_robot.py:164-187, */
                             /*    i >= assign_iter): lambda_assign * sum |x_src - y_assigned|^2 over   */
                             /*    the pairs of `assign_map`.  With recon_with_assign (below) the term  */
                             /*    is ADDED to the Chamfer loss instead                                 */
    float lambda_assign;     /* --lambda_assign                                           */
    float weight_decay;      /* --weight_decay: torch.optim.Adam's L2 form g += wd * p (run_robot.py:146-148) */
    /* Tuning and measurement switches.  0 = the library default everywhere.  The library reads NO environment
     * variable in any call path: the caller decides once per instance (reart_amd/relax.py maps REART_* variables
     * to these fields when an engine is built), so the ranks of a job cannot diverge mid-run. */
    int search_mode;         /* 0: exact box-pruned warm-started search (default); 1: cold brute force (same results); */
                             /* 2 | 3 | 4: the pruned search in the forms only very large shapes take by themselves,   */
                             /* for tests (same results): 2 frame offsets as 64-bit products (arrays of 2^31 bytes and  */
                             /* more), 3 launch positions through the order array and the query map instead of item    */
                             /* words (more than 2^21 - 1 pairs), 4 both                                                */
    int tune_slices;         /* waves (box slices) per search workgroup, 1..4 (default 3)  */
    int tune_slices_flow;    /* the same for the K = 3 flow search (default: tune_slices)  */
    int tune_sparse;         /* boxes needed by <= n queries of a wave go through the (query, box) queue instead of a  */
                             /* 64-lane scan: 1..64 (default 40), < 0: dense scans only                                */
    int tune_fwd_pts;        /* points per forward workgroup: 64 | 32 (default 32)         */
    int tune_bwd_pts;        /* points per backward workgroup: 64 | 32 | 16 (default 32)   */
    int tune_reorder;        /* < 0: keep the static launch order of the search items      */
    int tune_cloud;          /* 1 | 2 | 4 | 8: cloud-resident form of the search (16-wave workgroups that copy their target   */
                             /* cloud into LDS, that many box slices per query group; clouds up to ~7000 points).  Exact and  */
                             /* tested, but measured slower than the default (targets from L2): the launch is bound by       */
                             /* instruction issue, not by the latency the LDS copy removes                                  */
    int tune_xcd;            /* > 0: every XCD runs one contiguous eighth of the (frame, query group) pairs (a run of */
                             /* frames per L2) instead of every 8th pair; measured slower: frames differ 10x in work  */
    int profile;             /* 1: the search launch of every iteration records per-workgroup wall-clock stamps and  */
                             /*    its executed distance evaluations, reduced on the device (reart_relax_profile)    */
    int tune_share;          /* < 0: a query's search bound comes from its own seeds only; default: also from the    */
                             /*    seeds of the 15 neighbouring queries of its row (same results, fewer boxes), the  */
                             /*    candidates split over the waves of the search workgroup; 1: every wave all of them */
    int tune_long;           /* 1: the model's long path (reart_base_path = 1) also where the pose table fits in LDS: */
                             /*    same forward bit for bit, same backward sums; for tests and A/B timing            */
} reart_relax_config;

typedef struct reart_relax_buffers {
    const float *cano;       /* [N,3]                                                     */
    const float *pc_list;    /* [B,N,3] observed frames without the canonical one         */
    const float *ref_loc;    /* [M_total,3] flow reference points, sets concatenated      */
    const float *ref_flow;   /* [M_total,3] their flow vectors                            */
    const int *ref_off;      /* [B+1] int32 prefix offsets of the sets                    */
    const float *gumbel;     /* NULL (in-kernel Philox) or injected noise [N,P] (tests)   */
    float *W1, *b1, *W2;     /* seg head [H,3], [H], [P,H]; updated in place              */
    float *p6d, *pt;         /* proposal_6d [B,P,6], proposal_t [B,P,3]                   */
    float *adam_m, *adam_v;  /* [3H+H+PH+9BP] each, order W1|b1|W2|p6d|pt, start at zero   */
    int64_t *iter;           /* device scalar: completed iterations (caller initialises)  */
    float *tau;              /* device scalar: temperature of the next iteration          */
    float *losses;           /* [ring][4]: recon, lambda*flow, total, tau; row iter%ring.  recon is the Chamfer sum, or  */
                             /* the assignment term (use_assign), or Chamfer + assignment term (recon_with_assign)      */
    float *pc_trans;         /* [B,N,3] forward output of the last iteration              */
    int64_t *seg_part;       /* [N] or NULL                                               */
    float *trans_list;       /* [B,P,4,4] or NULL                                         */
    /* optional fork/join: with all three set, the flow branch (K=3 search + blend) runs on      */
    /* aux_stream concurrently with the Chamfer search; the hipEvent_t's are caller-owned.       */
    void *aux_stream, *ev_fork, *ev_join;
    /* use_assign: [B,N] int32, assign_map[b][i] = index into pc_list[b] of the point assigned to     */
    /* pc_trans[b][i], or -1 when point i is not among the sampled sources (the caller refreshes it   */
    /* every assign_gap iterations from FPS + linear assignment, run_robot.py:165-178)                */
    const int *assign_map;
    /* optional [ring]: entry iter%ring = the assignment term (lambda_assign * sum of the squared pair distances) that   */
    /* recon_with_assign added into losses[..][0]; 0 in every other mode.  NULL: not written                            */
    float *losses_assign;
} reart_relax_buffers;

/* Bytes of one instance's workspace; 0 for a configuration the step does not take.  What grows with the sequence: the
 * SoA images, search records and gradients are O(B * N); the backward's per-chunk partial rows are
 * ceil(N / 16) * (P*H + 4*H + 12*B*P) floats (room for the 16-point form: at B = 1024, N = 4096, P = 20, H = 128 that is
 * 256 rows of 1 MB, of which the default 32-point form writes 128 = 127 MB per iteration); the [R|t] table is 48 * B * P bytes. */
size_t reart_relax_workspace_bytes(const reart_relax_config *cfg);
/* once per problem: static SoA images of pc_list / reference sets, tau(iter) */
int reart_relax_prepare(const reart_relax_config *cfg, const reart_relax_buffers *bufs,
                        void *workspace, size_t workspace_bytes, void *stream);
/* forward only, for the CURRENT iteration (same temperature and Gumbel noise the next reart_relax_step
 * will use): fills pc_trans / seg_part / trans_list and changes nothing else.  The assignment loss needs
 * the transformed clouds of iteration i to compute the assignment used in iteration i. */
int reart_relax_forward(const reart_relax_config *cfg, const reart_relax_buffers *bufs,
                        void *workspace, size_t workspace_bytes, void *stream);
/* enqueue one iteration (5 launches in the default configuration, no host sync, no environment lookups) */
int reart_relax_step(const reart_relax_config *cfg, const reart_relax_buffers *bufs,
                     void *workspace, size_t workspace_bytes, void *stream);
/* K independent instances of ONE shape (same N, B, P, H, M_max and switches in every cfgs[k]; clouds, parameters,
 * canonical index, seed and learning rates are each instance's own) advance one iteration in the five launches of a
 * single instance: every kernel runs once with K argument blocks, instance k on plane k of its grid.  cfgs / bufs are
 * arrays of K, workspaces[k] is instance k's workspace (each prepared with reart_relax_prepare).  Each instance
 * computes exactly what reart_relax_step computes for it.  This is how a sweep over canonical frames
 * (/root/reference/README.md:60, run_robot.py: one process per cano_idx) fills the chip: one instance occupies a fraction
 * of the 256 compute units and is a chain of dependent launches.  Box-pruned search paths: Chamfer + flow loss (five
 * launches), Chamfer only, and the assignment loss with or without flow (run_robot.py:164-192: the pairs in each
 * instance's assign_map), or both losses together (recon_with_assign); every instance in the same mode -- Chamfer, assignment
 * loss, or both -- 1 <= K <= 6.  Any other search path (use_grid,
 * search_mode 1, use_boxes 0, tune_cloud): REART_ERR_UNSUPPORTED, for K = 1 as well; instances that differ in shape or
 * mode, or K out of range: REART_ERR_INVALID_ARG. */
int reart_relax_step_batch(const reart_relax_config *cfgs, const reart_relax_buffers *bufs, void *const *workspaces,
                           size_t workspace_bytes, int K, void *stream);
/* measurement aid: the same sequence with hipEvents between phases on `stream`; synchronises
 * and ADDS per-phase milliseconds to the HOST array h_ms[REART_RELAX_PHASES]:
 * 0 forward, 1 flow K=3 search, 2 flow blend, 3 Chamfer K=1 search, 4 Chamfer merge + gradient (or the
 * assignment loss), 5 model backward + Adam + bookkeeping, 6-7 unused.  With the pruned searches (the
 * default) every search of the iteration is ONE launch, and it is timed as phase 1: phase 3 is then
 * empty.  With the flow loss on as well (the default configuration) both consumers share ONE launch:
 * 2 is empty too, 1 = the search launch, 4 = the consumer launch.  Always serial (no fork/join); event
 * pairs around single launches over-read short kernels by a few microseconds. */
#define REART_RELAX_PHASES 8
int reart_relax_step_timed(const reart_relax_config *cfg, const reart_relax_buffers *bufs,
                           void *workspace, size_t workspace_bytes, void *stream, float *h_ms);
/* measurement aid (cfg->profile = 1, default search path with the flow loss): the search launch of every
 * reart_relax_step -- eager or replayed from a graph -- leaves per-workgroup wall-clock stamps that the consumer
 * launch reduces on the device.  h_out[0] = launches since the last reset, [1] = their summed duration in seconds
 * (first workgroup start to last workgroup end, constant-rate clock), [2] = query-target distance evaluations they
 * executed, [3] = the clock rate in Hz, [4] = the summed lifetimes of the launches' workgroups in seconds.
 * h_out holds 5 doubles.  Synchronises `stream`; reset != 0 clears the accumulators. */
int reart_relax_profile(const reart_relax_config *cfg, void *workspace, size_t workspace_bytes, void *stream,
                        double *h_out, int reset);

/* ------------------------------------------------------------------------ */
/* PointNet++ sampling / grouping (the live kernels of pointnet2_cuda)       */
/* ------------------------------------------------------------------------ */

/* Replaces furthest_point_sampling_wrapper(b,n,m, points, temp, idx)
 * (networks/pointnet_lib/src/sampling.cpp:38-49 -> sampling_gpu.cu:93-209) and the CPU
 * fallback farthest_point_sample (networks/pointnet2_utils.py:74-99).
 *   xyz [B,N,3]; start [B] i32 first index per cloud or NULL (= 0, the CUDA kernel's rule;
 *   the CPU fallback draws it from torch's RNG: inject it);  cuda_mode = 0: arg-max = first
 *   maximum (torch.max), 1: the CUDA kernel's block-tree tie rule.  No `temp` buffer is
 *   needed: the running minimum distances live in registers.
 *   idx32 [B,npoint] i32 and/or idx64 [B,npoint] i64 (either may be NULL).
 *   N <= REART_FPS_MAX_N_LDS (the cloud is staged in LDS); larger clouds: reart_fps_temp. */
#define REART_FPS_MAX_N_LDS 12288         /* reart_fps: 12 B of LDS per point              */
#define REART_FPS_MAX_N (1 << 21)         /* reart_fps_temp: 21-bit index in the tie key   */
int reart_fps(const float *xyz, int B, int N, int npoint, const int32_t *start, int cuda_mode,
              int32_t *idx32, int64_t *idx64, void *stream);

/* The same sampling, same arguments and both tie rules, for 1 <= N <= REART_FPS_MAX_N, with the
 * reference wrapper's caller-allocated distance buffer (sampling.cpp:38-49 temp_tensor).
 *   temp: f32 [B,N] (B * N * sizeof(float) bytes), scratch only: the kernel initialises the
 *   entries it uses and the caller's contents are never read.  For N <= REART_FPS_MAX_N_LDS the
 *   call is reart_fps and `temp` is not touched; above it one 1024-thread workgroup per cloud
 *   keeps 16 384 running minima in registers and the rest in `temp`.
 *   N > REART_FPS_MAX_N: REART_ERR_UNSUPPORTED. */
int reart_fps_temp(const float *xyz, int B, int N, int npoint, const int32_t *start, int cuda_mode,
                   float *temp, int32_t *idx32, int64_t *idx64, void *stream);

/* Replaces ball_query_wrapper(b,n,m,radius,nsample,new_xyz,xyz,idx)
 * (networks/pointnet_lib/src/ball_query.cpp:15-26 -> ball_query_gpu.cu:9-45) and the CPU
 * fallback query_ball_point (networks/pointnet2_utils.py:102-140).
 *   cuda_mode = 0: d2 <= float32(radius^2), first nsample in index order, padded with the
 *   nearest point;  1: d2 < float(radius)*float(radius), padded with the first hit (0 if none).
 *   Distance: direct difference ((dx*dx)+(dy*dy))+(dz*dz).
 *   idx32 [B,S,nsample] i32 and/or idx64 [B,S,nsample] i64. */
int reart_ball_query(const float *xyz, const float *new_xyz, int B, int N, int S,
                     double radius, int nsample, int cuda_mode,
                     int32_t *idx32, int64_t *idx64, void *stream);

/* The channel-major operators of the reference's pybind module `pointnet2_cuda` that nothing in the reference calls
 * (networks/pointnet_lib/src/pointnet2_api.cpp:14-25; only pointnet2_modules.py reaches them, and nothing imports it) --
 * here so that the module is whole (reart_amd/pointnet2_cuda.py).  int32 indices, caller-allocated outputs.
 *   reart_pn2_gather_points:       out[b][c][m] = points[b][c][idx[b][m]]; points [B,C,N], idx [B,M], out [B,C,M]
 *       (gather_points_wrapper, sampling_gpu.cu:8-24; group_points_wrapper, group_points_gpu.cu:39-54, is the same map with
 *       idx [B, npoints * nsample] and out [B,C,npoints,nsample]);
 *   reart_pn2_gather_points_grad:  grad_points[b][c][idx[b][m]] += grad_out[b][c][m] (float atomics, as sampling_gpu.cu:46-63 /
 *       group_points_gpu.cu:8-21; the caller zeroes grad_points, pointnet_lib/pointnet2_utils.py:70,231);
 *   reart_pn2_three_interpolate:   out[b][c][n] = (w0 p[i0] + w1 p[i1]) + w2 p[i2], p = points[b][c][:]; points [B,C,M],
 *       idx / weight [B,N,3], out [B,C,N] (interpolate_gpu.cu:149-169);
 *   reart_pn2_three_interpolate_grad: grad_points[b][c][i_j] += grad_out[b][c][n] * w_j (interpolate_gpu.cu:192-214). */
int reart_pn2_gather_points(const float *points, const int32_t *idx, int B, int C, int N, int M, float *out, void *stream);
int reart_pn2_gather_points_grad(const float *grad_out, const int32_t *idx, int B, int C, int N, int M, float *grad_points,
                                 void *stream);
int reart_pn2_three_interpolate(const float *points, const int32_t *idx, const float *weight, int B, int C, int M, int N,
                                float *out, void *stream);
int reart_pn2_three_interpolate_grad(const float *grad_out, const int32_t *idx, const float *weight, int B, int C, int N, int M,
                                     float *grad_points, void *stream);

/* ------------------------------------------------------------------------ */
/* Projection model: screw-joint forward kinematics                          */
/* ------------------------------------------------------------------------ */

/* Replaces fk(paths_to_base, reverse_topo, edge_index, axis_list, moment_list, theta_list,
 * distance_list) (utils/kinematic_utils.py:151-198) including
 * screw_param_to_exponential_coordinates / transform_from_exponential_coordinates
 * (screw_se3/screw_utils.py:6-30) and se3_exp_map (screw_se3/geo_utils.py:147-222).
 * The joint tree is passed as arrays instead of the reference's dicts:
 *   parent[c] (-1 = root), edge_of_part[c] (index of edge "c_parent" in edge_index),
 *   order = reverse_topo (parts from root to leaf), all i32 [P];
 *   axis, moment [E,3]; theta [B,E]; distance [B,E] or NULL (= 1e-6, :176);
 *   trans [B,P,4,4] out.  P <= 64, the limit of reart_fk_backward (REART_ERR_INVALID_ARG above it).
 *   A single part (P = 1, E = 0) has no joint: its empty axis / moment / theta (and the joint gradients of the backward
 *   entries) may be NULL. */
int reart_fk_forward(const int32_t *parent, const int32_t *edge_of_part, const int32_t *order,
                     int P, const float *axis, const float *moment, const float *theta,
                     const float *distance, int B, int E, float *trans, void *stream);

/* Backward of `fk` + the hard-label rigid apply of KinematicModel.forward
 * (networks/model.py:161-165): x [N,3], part [N] i64, G = dL/d pc_trans [B,N,3], trans = the
 * forward's output -> g_axis [E,3], g_moment [E,3], g_theta [B,E], g_distance [B,E] or NULL.
 * Deterministic (ordered reductions).  P <= 64. */
size_t reart_fk_backward_workspace_bytes(int P, int B, int E);
int reart_fk_backward(const float *x, const int64_t *part, const float *G, int N,
                      const int32_t *parent, const int32_t *edge_of_part, const int32_t *order,
                      int P, const float *axis, const float *moment, const float *theta,
                      const float *distance, int B, int E, const float *trans,
                      float *g_axis, float *g_moment, float *g_theta, float *g_distance,
                      void *workspace, size_t workspace_bytes, void *stream);

/* reart_fk_backward with two more arguments, both nullable (workspace: reart_fk_backward_workspace_bytes):
 *   g_trans [B,P,4,4]: an upstream on the forward's `trans`.  Its rows 0..2 are added onto the pose gradients of the points
 *     before the leaves -> root walk; row 3 (constants) is not read.
 *   g_x [N,3] out: the gradient of the cloud under the hard labels, sum_b R[b,part_n]^T G[b,n] with R from `trans`.
 * N = 0 with x, part, G NULL is legal (`fk` alone: only g_trans drives the joints).  With both NULL the four joint gradients
 * are reart_fk_backward's bit for bit (the same launches).  P <= 64.  float32, deterministic, capturable. */
int reart_fk_backward_trans(const float *x, const int64_t *part, const float *G, int N,
                            const int32_t *parent, const int32_t *edge_of_part, const int32_t *order,
                            int P, const float *axis, const float *moment, const float *theta,
                            const float *distance, int B, int E, const float *trans, const float *g_trans,
                            float *g_axis, float *g_moment, float *g_theta, float *g_distance, float *g_x,
                            void *workspace, size_t workspace_bytes, void *stream);

/* Retargeting: replaces the optimisation loop of ik (utils/kinematic_utils.py:200-266) for a kinematic model without
 * distance_list, joint types or root motion: per novel pose m, n_iter steps of
 *   pc = rigid_apply(fk(theta[m]), src, part);  loss = sum |pc - tgt[m]|^2;  Adam(amsgrad, no weight decay) on theta[m]
 * with the gradient of fk and the apply as reart_fk_backward computes it.  All M poses in ONE launch, one workgroup
 * per pose, the whole loop inside the kernel: no workspace, no host synchronisation, capturable; pose m's result does
 * not depend on M, and two runs are bit-identical.
 *   parent, edge_of_part, order, axis, moment: the tree as for reart_fk_forward, E = P - 1, distance = 1e-6 (:176);
 *   src [n,3] sparse canonical points, part [n] i64 their parts (a label outside [0,P): the point is skipped);
 *   tgt [M,n,3] where those points are in each novel pose;
 *   theta_init [M,E] or NULL = 1e-6 everywhere (:230); the optimiser state starts at zero;
 *   theta [M,E] out; loss [M, n_iter+1] out or NULL: loss[m,i] at the parameters before step i, loss[m,n_iter] at the
 *   returned theta (n_iter = 0: theta = theta_init and its loss).
 * P > 64 or E != P - 1: REART_ERR_INVALID_ARG; n > REART_IK_MAX_POINTS: REART_ERR_UNSUPPORTED; M = 0: REART_OK. */
#define REART_IK_MAX_POINTS 1024
int reart_ik_fit(const int32_t *parent, const int32_t *edge_of_part, const int32_t *order, int P,
                 const float *axis, const float *moment, int E, const float *src, const int64_t *part, int n,
                 const float *tgt, int M, const float *theta_init, int n_iter, float lr, float beta1, float beta2,
                 float eps, float *theta, float *loss, void *stream);

/* ------------------------------------------------------------------------ */
/* PointNet++ correspondence extractor: dense layers and interpolation       */
/* ------------------------------------------------------------------------ */

/* One fused layer  Y = relu(X Wt + bias) [max-pooled over pool_k consecutive rows]  on the fp32
 * matrix cores (v_mfma_f32_32x32x2_f32, exact fp32).  Replaces Conv2d/Conv1d(1x1) + BatchNorm
 * (eval, folded into Wt/bias by the caller) + ReLU and the max over nsample of
 * PointNetSetAbstractionMsg / PointNetSetAbstraction / PointNetFeaturePropagation
 * (networks/pointnet2_utils.py:209-235, 257-295, 309-348).
 *   Plain input: X [rows, ldx].  Gathered input (gather_idx != NULL; replaces index_points +
 *   centre subtraction + cat of :270-281 / sample_and_group_all :186-188 without materialising
 *   the grouped tensor): row r takes point gather_idx[r] (i64, [B,S,K] flattened) of cloud
 *   r / (S*K); columns = [F (D) | Q - C[r / K]] (xyz_first = 0) or [Q | F] (xyz_first = 1,
 *   C may be NULL); F [B*Npts, D], Q [B*Npts, 3], C [B*S, 3]; Cin must equal D + 3.
 *   Wt [Cin, Cout] (transposed conv weight), bias [Cout] or NULL; pool_k = 0 (no pooling) or any group size >= 1 that
 *   divides rows (REART_ERR_INVALID_ARG otherwise): nsample 16, 24, 48 ..., group_all over any point count.  The pooled
 *   output is the maximum over each group of the rows the un-pooled call writes, bit for bit; 32, 64 and 128 pool inside
 *   the waves' own rows, every other size through LDS (groups above 128 rows: one workgroup per group);
 *   Y [rows (/pool_k), ldy], written at columns ycol0 .. ycol0 + Cout. */
int reart_mlp_layer(const float *X, int ldx, const int64_t *gather_idx, int K, int S, int Npts,
                    const float *F, int D, const float *Q, const float *C, int xyz_first,
                    const float *Wt, const float *bias, int rows, int Cin, int Cout, int relu,
                    int pool_k, float *Y, int ldy, int ycol0, void *stream);
/* Host only, no device needed: the kernel instantiation reart_mlp_layer launches for these sizes, packed as
 * NB | BK << 8 | ANY << 16 -- NB accumulators of 32 columns per wave (1, 2, 3 or 7), a K step of BK (8 or 16), ANY = 1 for
 * group sizes pooled through LDS; 0 where Cin < 1, Cout < 1 or pool_k < 0.  The launcher decides by this function. */
int reart_mlp_layer_kernel(int Cin, int Cout, int pool_k);

/* Three such layers in ONE launch for a scale of the first set-abstraction level (PointNetSetAbstractionMsg,
 * networks/pointnet2_utils.py:257-295): gathered input [F (3) | Q - C] (6 columns) -> C1 -> C2 -> C3 (each with bias and
 * ReLU) -> max over the K rows of a group; the activations between the layers never leave the compute unit (LDS).
 * Same arguments as the gathered form of reart_mlp_layer (D = 3, xyz_first = 0, pool_k = K); rows = B*S*K.
 * Bit-identical to three reart_mlp_layer calls.  Built for the extractor's three scales, (C1, C2, C3, K) =
 * (32, 32, 64, 32), (64, 64, 128, 64), (64, 96, 128, 128) (networks/feature_extractor.py:19-21); anything else returns
 * REART_ERR_UNSUPPORTED (call the layers one by one). */
int reart_mlp_chain3(const int64_t *gather_idx, int K, int S, int Npts, const float *F, const float *Q, const float *C,
                     const float *W1t, const float *b1, int C1, const float *W2t, const float *b2, int C2,
                     const float *W3t, const float *b3, int C3, int rows, float *Y, int ldy, int ycol0, void *stream);

/* The same fusion for a scale of the SECOND set-abstraction level: gathered input [F (D) | Q - C] (D + 3 columns, D % 4 == 0,
 * F 16-byte aligned) -> C1 -> C2 -> C3 -> max over the K rows of a group.  The weights stream through LDS in 16-row slabs,
 * a workgroup carries 128 rows through all three layers (rows % 128 == 0).  Bit-identical to three reart_mlp_layer calls.
 * workspace (16-byte aligned, reart_mlp_chain3_wide_workspace_bytes(D, C1, C2, C3)): every call first writes an image of
 * the three weight matrices there in the order the matrix cores' B fragments are read (one small launch).
 * Built for (C1, C2, C3, K) = (128, 128, 256, 64), (128, 196, 256, 128) (networks/feature_extractor.py:22-23); anything
 * else returns REART_ERR_UNSUPPORTED. */
size_t reart_mlp_chain3_wide_workspace_bytes(int D, int C1, int C2, int C3);
int reart_mlp_chain3_wide(const int64_t *gather_idx, int K, int S, int Npts, const float *F, int D, const float *Q,
                          const float *C, const float *W1t, const float *b1, int C1, const float *W2t, const float *b2,
                          int C2, const float *W3t, const float *b3, int C3, int rows, float *Y, int ldy, int ycol0,
                          void *workspace, size_t workspace_bytes, void *stream);

/* The fused gathered chain for the shapes the two kernels above are not built for: gathered input [F (D) | Q - C]
 * (xyz_first = 0) or [Q - C | F] (xyz_first = 1; C may be NULL: absolute xyz; D = 0: F may be NULL) -> C1 -> C2 -> C3 (bias and
 * ReLU each) -> max over the K rows of a group.  Activations stay in LDS, the weights stream through it as in
 * reart_mlp_chain3_wide (workspace: 16-byte aligned, reart_mlp_chain_workspace_bytes(D, C1, C2, C3), rewritten by every call).
 * Bit-identical to three reart_mlp_layer calls.
 * reart_mlp_chain_serves (host only, no device needed): 1 for D in 0 .. 512, K in {16, 32, 64, 128}, C1 % 32 == 0, C3 % 32 == 0,
 * C2 % 4 == 0, each <= 256, rows % 128 == 0 -- EXCEPT the shapes reart_mlp_chain3 (D = 3) and reart_mlp_chain3_wide (D % 4 == 0)
 * are built for with xyz_first = 0, which stay theirs; 0 otherwise.  reart_mlp_chain returns REART_ERR_UNSUPPORTED where the
 * predicate says 0 (call the layers one by one). */
int reart_mlp_chain_serves(int D, int K, int C1, int C2, int C3, int rows, int xyz_first);
size_t reart_mlp_chain_workspace_bytes(int D, int C1, int C2, int C3);
int reart_mlp_chain(const int64_t *gather_idx, int K, int S, int Npts, const float *F, int D, const float *Q, const float *C,
                    int xyz_first, const float *W1t, const float *b1, int C1, const float *W2t, const float *b2, int C2,
                    const float *W3t, const float *b3, int C3, int rows, float *Y, int ldy, int ycol0, void *workspace,
                    size_t workspace_bytes, void *stream);

/* square_distance of networks/pointnet2_utils.py:30-51 for 3-d points: src [B,N,3], dst [B,M,3] -> out [B,N,M], the matmul
 * expansion with torch's CPU rounding, d = ((-2*fma(qz,tz,fma(qy,ty,qx*tx))) + |q|^2) + |t|^2 (as in reart_three_nn). */
int reart_square_distance(const float *src, const float *dst, int B, int N, int M, float *out, void *stream);

/* 3-NN inverse-distance interpolation of PointNetFeaturePropagation
 * (networks/pointnet2_utils.py:326-336): xyz1 [B,N,3], xyz2 [B,S2,3], points2 [B,S2,D] ->
 * out [B*N, ldo] columns col0 .. col0 + D (so the cat with the skip features, :338-342, is free).
 * Distances: the reference's matmul expansion (square_distance, :33-55) with torch's CPU rounding,
 * d = ((-2*fma(qz,tz,fma(qy,ty,qx*tx))) + |q|^2) + |t|^2 -- bit-equal to the reference on its CPU path
 * (tests/golden/three_interp.npz); the three smallest by (d, index).
 * reart_three_nn alone: dist3 f32 [B,N,3], idx3 i64 [B,N,3] (= square_distance(...).sort()[:3]). */
int reart_three_nn(const float *xyz1, const float *xyz2, int B, int N, int S2, float *dist3,
                   int64_t *idx3, void *stream);
size_t reart_three_interpolate_workspace_bytes(int B, int N, int S2);
int reart_three_interpolate(const float *xyz1, const float *xyz2, const float *points2, int B,
                            int N, int S2, int D, float *out, int ldo, int col0,
                            void *workspace, size_t workspace_bytes, void *stream);

/* First-order backward of reart_mlp_layer (csrc/pointnet_grad.hip).  The layer is A = relu?(X Wt + b), Y = the max over groups
 * of pool_k rows of A, or A itself.  The operand description (X / ldx, or gather_idx / K / S / Npts / F / D / Q / C / xyz_first),
 * Wt, rows, Cin, Cout, relu and pool_k are the forward's; A [rows, Cout] is what reart_mlp_layer writes with pool_k = 0 (for an
 * un-pooled layer: its output); dY [rows (/pool_k), lddy] is read at columns dycol0 .. dycol0 + Cout.
 *   dZ[r,c] = dY[group(r),c] where row r is selected and (with relu) A[r,c] > 0, else exactly 0.  Without pooling every row is
 *   selected; with pooling the LOWEST row of the group whose A equals the group's maximum (with relu a group whose maximum is 0
 *   selects nothing).
 * Outputs, each NULL = not wanted and not computed:
 *   dWt [Cin, Cout] = X^T dZ and dbias [Cout] = column sums of dZ, on v_mfma_f32_32x32x2_f32: the rows are cut into chunks of
 *     REART_MLP_GRAD_ROW_CHUNK, each chunk's tile goes to the workspace, the tiles are added in ascending chunk order (no
 *     floating-point atomics: two runs agree in every bit).  A gathered X is formed element by element as the forward forms it
 *     (the same float32 Q - C) and never materialised; a gather index outside [0, Npts) contributes a zero row;
 *   dX [rows, lddx] (plain input only) = dZ Wt^T, computed by reart_mlp_layer on dZ with the transposed weight;
 *   dF [B*Npts, D] (gathered input only; B = rows / (S*K)): the feature columns of dX summed over the rows that name the point,
 *     in ascending row order (inverse lists by a stable counting sort); a point no row names gets exactly 0, an index outside
 *     [0, Npts) is skipped, the xyz columns are dropped (coordinates get no gradient).
 * Limits and error codes are reart_mlp_layer's; dX with a gathered input or dF with a plain one: REART_ERR_INVALID_ARG.
 * Non-finite input gives meaningless values, never an out-of-range access.
 * workspace: reart_mlp_layer_backward_scratch_bytes(rows, Cin, Cout, B, Npts, D) with B = Npts = D = 0 for a plain input. */
#define REART_MLP_GRAD_ROW_CHUNK 256
size_t reart_mlp_layer_backward_scratch_bytes(int rows, int Cin, int Cout, int B, int Npts, int D);
int reart_mlp_layer_backward(const float *X, int ldx, const int64_t *gather_idx, int K, int S, int Npts,
                             const float *F, int D, const float *Q, const float *C, int xyz_first,
                             const float *Wt, int rows, int Cin, int Cout, int relu, int pool_k,
                             const float *A, const float *dY, int lddy, int dycol0,
                             float *dWt, float *dbias, float *dX, int lddx, float *dF,
                             void *workspace, size_t workspace_bytes, void *stream);

/* Backward of reart_three_interpolate with respect to points2: dpoints2[b,s,:] = sum of w[b,n,j] * dOut[b*N + n, col0 .. col0 + D)
 * over the pairs (n, j) with idx3[b,n,j] = s, in ascending (n, j) (the same inverse lists as above); idx3 and w are the forward's
 * (reart_three_nn, w_j = (1 / (d_j + 1e-8)) / ((w_0 + w_1) + w_2)).  A coarse point no fine point selects gets exactly 0.
 * dOut [B*N, ldo]; dpoints2 [B,S2,D]; weights: NULL, or [B,N,3] to receive w.  Limits as reart_three_interpolate. */
size_t reart_three_interpolate_backward_scratch_bytes(int B, int N, int S2);
int reart_three_interpolate_backward(const float *xyz1, const float *xyz2, const float *dOut, int ldo, int col0,
                                     int B, int N, int S2, int D, float *dpoints2, float *weights,
                                     void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------ */
/* Exact K-NN against static target sets (uniform grid)                      */
/* ------------------------------------------------------------------------ */

/* Same result, bit for bit, as reart_knn_points_idx / reart_knn_cuda (same distance expression,
 * ties -> lowest index) for K in {1, 3}, computed through a 16^3 uniform grid over each target
 * set: ~30-50x fewer distance evaluations when the targets do not change between calls (the
 * observed frames and the flow reference sets of the relaxation loop).  This entry builds the grid
 * and queries it in one call; the fused step (reart_relax_prepare/step) builds once.
 *   targets: [E,Nt_max,3] (offsets NULL) or ragged sets concatenated with offsets [E+1] i32;
 *   queries [E,nq,3]; dists [E,nq,K] squared, ascending; idx [E,nq,K] i32.  Every set needs >= K points. */
size_t reart_grid_knn_workspace_bytes(int E, int Nt_max);
int reart_grid_knn(const float *targets, const int32_t *offsets, int E, int Nt_max,
                   const float *queries, int nq, int K, float *dists, int32_t *idx,
                   void *workspace, size_t workspace_bytes, void *stream);

/* Warm-started exact K-NN for repeated searches on slowly moving clouds (the relaxation loop repeats
 * the searches of utils/chamfer.py:78-94 and utils/flow_utils.py:158 every iteration).  Same result,
 * bit for bit, as reart_knn_points_idx for K in {1, 3} (full lengths), whatever `seed` holds: the
 * seeds (neighbour indices of an earlier call, -1 / out-of-range / repeated entries are tolerated)
 * only bound the search so that bounding boxes of 16 consecutive targets can be skipped, which pays
 * when both clouds are stored in a spatially coherent order (k-d tree leaf or Morton order).
 *   p1 [N,P1,3] queries, p2 [N,P2,3] targets; seed [N,P1,K] i32 in/out (receives idx);
 *   dists [N,P1,K] squared, ascending; idx [N,P1,K] i64.  The fused step uses the same kernels. */
size_t reart_knn_points_warm_workspace_bytes(int N, int P1, int P2, int K);
int reart_knn_points_idx_warm(const float *p1, const float *p2, int N, int P1, int P2, int K,
                              int32_t *seed, float *dists, int64_t *idx, void *workspace,
                              size_t workspace_bytes, void *stream);

/* The bidirectional K = 1 Chamfer sum of networks/loss.py:24-29 with its gradient as ONE call, warm-started from its own
 * previous call (csrc/chamfer_loss.hip):
 *   loss = sum_n ( sum_i |x_i - y_nn(i)|^2 + sum_j |y_j - x_nn'(j)|^2 ),   x [N,P1,3], y [N,P2,3] float32, P1 != P2 allowed.
 * Both searches run in ONE launch of the exact box-pruned search of reart_knn_points_idx_warm (same distances and indices,
 * bit for bit, ties -> lowest index in the numbering THIS entry sees, whatever the seeds hold; a caller that stores its clouds
 * in another order, as utils.chamfer.ChamferLoss does by default, resolves ties between distinct targets in that order);
 * one consumer launch writes everything else.
 *   seed_xy [N,P1], seed_yx [N,P2] i32 in/out: neighbour indices of the previous call (-1, out-of-range or repeated entries
 *       are tolerated: seeds only bound the search); they receive this call's indices;
 *   y_unchanged != 0: y is bit for bit the y of the previous call with THIS workspace and these shapes: its SoA image and
 *       boxes in the workspace are reused.  The first call with a workspace passes 0;
 *   d_xy, i_xy [N,P1], d_yx, i_yx [N,P2] (each nullable): squared distances and int64 indices of both directions;
 *   loss [1] (device): the per-point distances added in a fixed order in double, rounded once;
 *   grad_x [N,P1,3] = 2 (x_i - y_nn(i)) + 2 sum_{j: nn'(j) = i} (x_i - y_j); grad_y [N,P2,3] (nullable) likewise for y.
 *       The sums over j are 64-bit fixed-point sums of the float32 differences: deterministic, each addend truncated by
 *       less than 2^-fx_bits[n];
 *   fx_bits [N] i32 (device, out): fractional bits used for batch element n, 0..39, chosen from the clouds' boxes so that
 *       max(P1,P2) addends of magnitude up to twice the largest |coordinate| stay below 2^62 (coordinates so large that
 *       even 0 bits do not fit -- max(P1,P2) * max|coordinate| >= 2^60 -- are outside the contract).
 * Non-finite coordinates give meaningless values, never an out-of-range access.  N <= 65535.  N, P1 or P2 = 0: REART_OK,
 * nothing is launched or written.  Five launches (three when y is unchanged) and one 4-byte memset on `stream` (the counter
 * of the loss reduction, cleared in front of every call: no call depends on how an earlier one ended, so a failed or
 * aborted launch leaves nothing behind that a later call would trip over); no host synchronisation. */
size_t reart_chamfer_loss_workspace_bytes(int N, int P1, int P2);
int reart_chamfer_loss(const float *x, const float *y, int N, int P1, int P2, int32_t *seed_xy, int32_t *seed_yx,
                       int y_unchanged, float *d_xy, int64_t *i_xy, float *d_yx, int64_t *i_yx, float *loss,
                       float *grad_x, float *grad_y, int32_t *fx_bits, void *workspace, size_t workspace_bytes,
                       void *stream);

/* The same warm-started search with the per-point distances as the result and a backward for per-point upstream gradients
 * (utils.chamfer.ChamferPoints): what a caller needs who weights, masks, truncates or averages the distances of
 * utils/chamfer.py:78-123 before reducing them.  x [N,P1,3], y [N,P2,3] float32, P1 != P2 allowed; the limits, the workspace
 * (reart_chamfer_loss_workspace_bytes, same layout: an image of y built by either entry serves the other), the seeds, the tie
 * rule and the range checks are those of reart_chamfer_loss.
 *   reart_chamfer_points: directions is a bit mask, 1 = x -> y, 2 = y -> x, 3 = both (anything else: REART_ERR_INVALID_ARG).
 *       A direction that is not asked for is not searched, its outputs and seeds are left untouched and may be NULL; only the
 *       target cloud of a searched direction is prepared (y for 1, unless y_unchanged; x for 2), so a call with directions = 2
 *       neither needs nor builds y's image.  Distances and indices are bit for bit those of reart_knn_points_idx with K = 1
 *       and full lengths, whatever the seeds hold.  No loss, no gradient.  Two to five launches, no memset, no host
 *       synchronisation.
 *   reart_chamfer_points_backward: from the clouds, the indices and distances of a forward and the upstream gradients
 *           grad_x[n,i] = 2 g_xy[n,i] (x_i - y_{i_xy[i]}) + 2 sum_{j: i_yx[j] = i} g_yx[n,j] (x_i - y_j)
 *           grad_y[n,j] = 2 g_yx[n,j] (y_j - x_{i_yx[j]}) + 2 sum_{i: i_xy[i] = j} g_xy[n,i] (y_j - x_i)
 *       in ONE launch without a workspace or any state of an earlier call.  g_xy, g_yx and grad_y may each be NULL: a NULL
 *       upstream drops that direction's terms (its i_ / d_ pointers may then be NULL too), a NULL grad_y is not computed.
 *       Rounding: the first term is fl(fl(2 g) fl(x_i - y_nn)); every addend of a sum is fl(g_j fl(x_i - y_j)), added into a
 *       64-bit fixed-point sum (deterministic, truncated by less than 2^-bits each); the sum is doubled, rounded to float32
 *       once and added.  With g = 1 everywhere this is reart_chamfer_loss's arithmetic.
 *       fx_bits [N,2] i32 (device, out, written in every call): fractional bits of the sums into x ([n,0]) and into y
 *       ([n,1]; 0 when grad_y is NULL).  Rule: with m = max_j |g_j| sqrt(d_j) over the upstream and distances of the OTHER
 *       cloud of batch element n (which bounds every component of an addend), m (1 + 2^-20) < 2^e and max(P1,P2) <= 2^c:
 *       bits = clamp(61 - c - e, 0, 39), so every sum stays below 2^62.  d must be the distances that belong to the indices
 *       (as the forward returns them); upstreams so large that 0 bits do not fit are outside the contract.
 * Non-finite inputs give meaningless values, never an out-of-range access: every index is range-checked.  N, P1 or P2 = 0:
 * REART_OK, nothing is launched or written. */
int reart_chamfer_points(const float *x, const float *y, int N, int P1, int P2, int directions, int32_t *seed_xy,
                         int32_t *seed_yx, int y_unchanged, float *d_xy, int64_t *i_xy, float *d_yx, int64_t *i_yx,
                         void *workspace, size_t workspace_bytes, void *stream);
int reart_chamfer_points_backward(const float *x, const float *y, int N, int P1, int P2, const int64_t *i_xy,
                                  const int64_t *i_yx, const float *d_xy, const float *d_yx, const float *g_xy,
                                  const float *g_yx, float *grad_x, float *grad_y, int32_t *fx_bits, void *stream);

/* The three entries above for batches whose clouds differ in length, padded to [N,P1,3] and [N,P2,3]: the arguments of the dense
 * sibling, then len_x, len_y [N] i32 (device; either may be NULL = every element has P1, respectively P2, points; both NULL is
 * the dense entry, which is implemented as exactly that call).  Per batch element n with lx = len_x[n], ly = len_y[n] this is
 * reart_knn_points_idx(x, y, lengths1, lengths2, K = 1) in both directions:
 *   rows i < lx of d_xy / i_xy: distance and lowest index of the nearest of y's first ly points, bit for bit; rows i >= lx,
 *       and every row when ly = 0: distance 0, index 0, next seed -1.  Likewise for d_yx / i_yx;
 *   loss: the live rows' distances of both directions, added in double in the fixed order, rounded once;
 *   gradients: the dense formula over live points only; rows of padding points are exactly 0, grad is written completely;
 *       an upstream (g_xy, g_yx) at a padding row is never read;
 *   fx_bits: from max(lx, ly) and the live points alone, so element n equals a dense call on the two trimmed clouds in every
 *       output bit (distances, indices, gradients, fx_bits).
 * The contents of padding rows of x and y are never part of a result (zeros, NaN, +-INF, anything).  A length outside [0, P]
 * reads as clamped.  A seed that names a padding target is unusable like any other garbage seed.  Limits as the dense entries.
 * Workspace of reart_chamfer_loss_ragged and reart_chamfer_points_ragged with a length given: reart_chamfer_ragged_bytes(N, P1,
 * P2) -- the dense layout at the dense offsets (y's image serves both), then a staged query image of each cloud, in which the
 * padding rows repeat the element's last live point, and the clamped lengths (the search kernels take no query count: padding
 * lanes cost one coherent query and their records are ignored).  During the call the padding rows of a searched direction's
 * seed array hold a copy of the last live row's seed.  y_unchanged != 0 also asserts that len_y is unchanged.  One more
 * launch than the dense sibling (the staging); the backward has none and no workspace. */
size_t reart_chamfer_ragged_bytes(int N, int P1, int P2);
int reart_chamfer_loss_ragged(const float *x, const float *y, int N, int P1, int P2, int32_t *seed_xy, int32_t *seed_yx,
                              int y_unchanged, float *d_xy, int64_t *i_xy, float *d_yx, int64_t *i_yx, float *loss,
                              float *grad_x, float *grad_y, int32_t *fx_bits, void *workspace, size_t workspace_bytes,
                              void *stream, const int32_t *len_x, const int32_t *len_y);
int reart_chamfer_points_ragged(const float *x, const float *y, int N, int P1, int P2, int directions, int32_t *seed_xy,
                                int32_t *seed_yx, int y_unchanged, float *d_xy, int64_t *i_xy, float *d_yx, int64_t *i_yx,
                                void *workspace, size_t workspace_bytes, void *stream, const int32_t *len_x,
                                const int32_t *len_y);
int reart_chamfer_points_backward_ragged(const float *x, const float *y, int N, int P1, int P2, const int64_t *i_xy,
                                         const int64_t *i_yx, const float *d_xy, const float *d_yx, const float *g_xy,
                                         const float *g_yx, float *grad_x, float *grad_y, int32_t *fx_bits, void *stream,
                                         const int32_t *len_x, const int32_t *len_y);

/* One iteration's flow term (run_robot.py:194-209: blend_anchor_motion of every frame pair, flow_loss, and the gradient that
 * autograd carries through the cat and the subtraction) as ONE call over reference sets prepared once, warm-started from its own
 * previous call (csrc/flow_term.hip).  K = 3 only.
 *   reart_flow_term_prepare, once per run: ref, ref_flow [B,nr_max,3] padded, ref_len [B] i64 or NULL (all nr_max), every
 *       length >= 3.  Builds the sets' searchable image (SoA rows, boxes of 16 consecutive targets), their lengths and a copy of
 *       their flows inside `workspace`; ref and ref_flow are not read again.
 *   reart_flow_term: comp = pc_trans[:cano_idx] | cano | pc_trans[cano_idx:] (pc_trans [B,N,3], cano [N,3], by indexing); pair f
 *       searches comp[f] in reference set f, pred[f] = comp[f + 1] - comp[f].
 *     order [N] i32 or NULL: the point visited at position i (a permutation; the search is fastest when consecutive positions
 *         are neighbours in space).  Only the visiting order changes: every output below is in the caller's numbering;
 *     seed [B,N,3] i32 in/out, by visit position: neighbour indices of the previous call (any contents: -1, out-of-range and
 *         repeated entries are tolerated, seeds only bound the search); receives this call's;
 *     gt_flow [B,N,3], mask [B,N] u8, dists [B,N,3], idx [B,N,3] i64 (each nullable): the blended flow and validity mask of
 *         reart_blend_anchor_motion_batch, and the neighbours of reart_knn_cuda (K = 3), bit for bit, whatever the seeds hold
 *         (dists squared, or their sqrt when `euclidean`; ties -> lowest index in the numbering prepare saw);
 *     loss [1] (device, nullable) = weight x float32(sum): the per-point terms of reart_flow_loss added in a fixed order in
 *         double and rounded once;
 *     G [B,N,3] = d loss / d pc_trans: with gp[f] = (d flow_loss / d pred[f]) x weight, complete frame j gets
 *         gp[j - 1] - gp[j] (a term that does not exist is dropped; the canonical frame gets none).  accumulate != 0 adds that
 *         finished difference onto G instead of storing it.
 * workspace_bytes must be exactly what reart_flow_term_workspace_bytes(B, N, nr_max) returned, for prepare and for every call:
 * it is how the call knows nr_max.  B <= REART_MAX_POSE_LEN, N and nr_max <= 2^20, B x N and B x nr_max <= 2^26; beyond that the
 * size is 0 and the entries return REART_ERR_UNSUPPORTED.  Non-finite coordinates give meaningless values, never an out-of-range
 * access.  A call is three launches on `stream` and no memset (the first launch also clears the counters of the last: no call
 * depends on how an earlier one ended); no host synchronisation, no buffers other than the arguments: capturable in a graph. */
size_t reart_flow_term_workspace_bytes(int B, int N, int nr_max);
int reart_flow_term_prepare(const float *ref, const float *ref_flow, const int64_t *ref_len, int B, int nr_max, void *workspace,
                            size_t workspace_bytes, void *stream);
int reart_flow_term(const float *pc_trans, const float *cano, const int32_t *order, int B, int N, int cano_idx, int euclidean,
                    int robust, float smooth_weight, float weight, int32_t *seed, float *gt_flow, uint8_t *mask, float *dists,
                    int64_t *idx, float *loss, float *G, int accumulate, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------ */
/* Batched linear assignment (assignment loss)                               */
/* ------------------------------------------------------------------------ */

/* Replaces `[linear_sum_assignment(c) for c in cost]` / `parallel_lap(cost)` of the assignment loss
 * (run_robot.py:172-176, utils/model_utils.py:85-89) for square cost matrices.
 *   cost [B,n,n] fp32, n <= 4096; col4row [B,n] i32 = column assigned to row i (minimum total cost).
 * epsilon-scaling auction + an exact dual certificate in fp64: certified[b] = 1 means the assignment of matrix
 * b is optimal (equal to scipy's whenever the optimum is unique); certified[b] = 0 means the certificate
 * did not close and the caller must solve that matrix with the host solver (the Python wrapper does).
 * price_in (nullable, [B,n] f64): column potentials returned by an earlier call on a similar batch (the loop
 * re-solves slowly moving matrices every assign_gap iterations): warm start; price_out (nullable, [B,n] f64)
 * receives the potentials of this batch (may alias price_in). */
size_t reart_lap_workspace_bytes(int B, int n);
int reart_lap_auction(const float *cost, int B, int n, int32_t *col4row, int32_t *certified,
                      const double *price_in, double *price_out, void *workspace, size_t workspace_bytes,
                      void *stream);

/* The same solve for Euclidean costs between two point sets: cost must be reart_cdist(src, tgt) (src, tgt [B,n,3]) -- what
 * /root/reference/utils/model_utils.py:92-104 (compute_ass_err) and run_robot.py:170-176 build with torch.cdist.  The long
 * single-bidder chains at the end of every phase then recompute their rows from the points instead of reading them
 * (a dependent row read per link otherwise).  Result and potentials identical to reart_lap_auction on the same matrix. */
int reart_lap_auction_points(const float *cost, const float *src, const float *tgt, int B, int n, int32_t *col4row,
                             int32_t *certified, const double *price_in, double *price_out, void *workspace,
                             size_t workspace_bytes, void *stream);

/* A cold solve as a RACE over epsilon schedules: `racers` (1..13) workgroups per matrix run the auction with different
 * (first epsilon, shrink factor) pairs on compute units that would otherwise idle (T-1 = 19 matrices on 256 units); the first
 * racer whose certificate closes publishes its result, the others stop at their next look at the flag.  The fastest schedule
 * depends on the matrix: over five schedules the slowest matrix of a batch is done 20 % earlier than under the best single
 * one.  The ASSIGNMENT is the optimum whichever racer wins; price_out holds the winner's potentials (valid duals, but not
 * reproducible from run to run).  src / tgt as in reart_lap_auction_points, or both NULL; workspace:
 * reart_lap_race_workspace_bytes.  Used where only the assignment matters: /root/reference/utils/model_utils.py:92-104
 * (compute_ass_err) and the assignment refresh of run_robot.py:165-178. */
size_t reart_lap_race_workspace_bytes(int B, int n, int racers);
int reart_lap_auction_race(const float *cost, const float *src, const float *tgt, int B, int n, int racers,
                           int32_t *col4row, int32_t *certified, double *price_out, void *workspace,
                           size_t workspace_bytes, void *stream);

/* The race with WARM racers in the field: price_in / col4row_in are the potentials and the assignment an earlier solve of a
 * similar batch returned; up to three of the `racers` (2..16, at most 13 of them cold) start from them, the others cold.  A loop that re-solves every
 * few iterations (run_robot.py:165-178) need not know whether its matrices moved little -- a warm racer is then done in a
 * fraction of a cold solve -- or jumped (a cold one wins).  price_out != price_in, col4row != col4row_in. */
int reart_lap_auction_race_warm(const float *cost, const float *src, const float *tgt, int B, int n, int racers,
                                const int32_t *col4row_in, const double *price_in, int32_t *col4row, int32_t *certified,
                                double *price_out, void *workspace, size_t workspace_bytes, void *stream);

/* The cold solve for matrices of up to 8192 columns: the same epsilon-scaling auction, augmenting searches and fp64
 * certificate as reart_lap_auction, in an instance of its kernel that keeps prices, owners and the assignment in LDS (16 B per
 * column) and the bids of a round in the workspace.  One workgroup per matrix, not raced: the result is a function of the
 * matrix.  Accepts every 1 <= n <= REART_LAP_LARGE_MAX_N (the Python wrapper sends it n > 4096 only; below, the entries
 * above are faster).  src / tgt: both NULL, or both given with cost == reart_cdist(src, tgt) -- accepted so that a caller
 * passes the same arguments at every size; this form reads its rows from the matrix throughout.  price_out [B,n] f64
 * (required) receives the potentials.  The certificate takes at most 256 rounds (each a pass of one compute unit over the
 * matrix); a matrix that needs more comes back with certified[b] = 0, for the host solver like any other uncertified one.
 * workspace: reart_lap_large_workspace_bytes (0 unless B >= 0 and 1 <= n <= REART_LAP_LARGE_MAX_N); diagnostics [B][4]
 * (phases, rounds, bids, certificate rounds) at the same offset as in reart_lap_workspace_bytes' layout. */
#define REART_LAP_LARGE_MAX_N 8192
size_t reart_lap_large_workspace_bytes(int B, int n);
int reart_lap_auction_large(const float *cost, const float *src, const float *tgt, int B, int n,
                            int32_t *col4row, int32_t *certified, double *price_out,
                            void *workspace, size_t workspace_bytes, void *stream);

/* Byte offset of the diagnostics block [B][4] i32 in the workspace of every reart_lap_* solver (they all begin with the same two
 * blocks), for a host that reads the statistics words or hands them to reart_publish_words.  Host only, launches nothing.
 * 0 unless B >= 0 and 1 <= n <= REART_LAP_LARGE_MAX_N. */
size_t reart_lap_stats_offset(int B, int n);

/* The same solve warm-started from an earlier solve of a similar batch (the loop re-solves every assign_gap
 * iterations): on entry col4row holds that solve's assignment and price_in (required) its potentials; pairs that are
 * still epsilon-tight under the new costs are kept.  Certified like a cold solve.  Use when the costs move smoothly
 * (KinematicModel); with BaseModel's resampled part labels a cold solve is faster. */
int reart_lap_auction_warm(const float *cost, int B, int n, int32_t *col4row, int32_t *certified,
                           const double *price_in, double *price_out, void *workspace, size_t workspace_bytes,
                           void *stream);

/* Re-solve of a slowly moving batch (the kinematic projection, README.md:125: --assign_gap=1 re-solves its T-1 matrices
 * after every Adam step, run_robot.py:165-178): shortest augmenting paths (Jonker-Volgenant) started from the previous
 * solve's assignment (col4row on entry) and potentials (price_in, required) -- pairs that still attain their row's
 * minimum are kept, every other row costs one Dijkstra search over the reduced costs.  Same outputs, same exact
 * certificate as reart_lap_auction; the first solve of a sequence comes from reart_lap_auction.  For n >= 512 the call is
 * four launches on `stream`: the rows' (min, arg-min) under the incoming potentials on the whole chip, the sequential
 * part with one workgroup per matrix, the first certificate round on the whole chip, and the remaining certificate
 * rounds for a matrix that needs them (normally none); the intermediate arrays live in `workspace`. */
int reart_lap_resolve(const float *cost, int B, int n, int32_t *col4row, int32_t *certified,
                      const double *price_in, double *price_out, void *workspace, size_t workspace_bytes,
                      void *stream);

/* reart_lap_resolve for matrices of up to 8192 columns (every 1 <= n <= REART_LAP_LARGE_MAX_N is accepted; the Python wrapper
 * sends it n > 4096 only): the same steps -- kept pairs, greedy take-up, augmenting row reduction, one Dijkstra search per
 * row still free, fp64 certificate -- in an instance of the same kernel that keeps its four index arrays in LDS (16 B per
 * column) and the row potentials in the workspace.  Always four launches, one workgroup per matrix in the sequential part, not
 * raced: the result is a function of the matrix and the incoming state, bit for bit.  Same arguments as reart_lap_resolve:
 * col4row holds the previous assignment on entry (out-of-range entries are free rows, a repeated column keeps its lowest
 * row), price_in (required) the previous potentials; price_out is required and may alias price_in.
 * Two caps bound a call whose state is useless (the matrices jumped): the certificate takes at most 256 rounds, as in
 * reart_lap_auction_large, and a matrix takes at most `max_steps` row-reduction + path-search steps (each a dependent row
 * read; <= 0: the library's default, a multiple of n).  A matrix that reaches either cap comes back with certified[b] = 0,
 * the step cap also sets bit 30 of its first diagnostics word; the call still returns REART_OK and the caller solves that
 * matrix cold (reart_lap_auction_large).
 * workspace: reart_lap_resolve_large_workspace_bytes (0 unless B >= 0 and 1 <= n <= REART_LAP_LARGE_MAX_N); diagnostics
 * [B][4] at the same offset as in reart_lap_workspace_bytes' layout, in reart_lap_resolve's meaning: released rows (+ bit
 * 30), rows left for the searches, search steps, certificate rounds + row-reduction steps << 8. */
size_t reart_lap_resolve_large_workspace_bytes(int B, int n);
int reart_lap_resolve_large(const float *cost, int B, int n, int max_steps, int32_t *col4row, int32_t *certified,
                            const double *price_in, double *price_out, void *workspace, size_t workspace_bytes,
                            void *stream);

/* Measurement aid for the latency roofline of reart_lap_resolve_points (no reference counterpart): B workgroups run
 * `steps` path-search steps of the re-solve stripped to what cannot be removed -- the workgroup-wide (distance, column)
 * arg-min over n <= 2048 labels held in registers and its one barrier, with the solver's own primitives -- and
 * *h_us_per_step (HOST pointer) receives the slowest workgroup's microseconds per step on the GPU's constant-rate
 * clock.  A re-solve of S sequential steps cannot take less than S x this.  Synchronises `stream`.  workspace: 16 B bytes. */
int reart_lap_step_floor(int B, int n, int steps, void *workspace, size_t workspace_bytes, double *h_us_per_step, void *stream);

/* Measurement aid for the headline iteration (run_robot.py:154-221 as five dependent launches; no reference counterpart):
 * enqueues `iters` times a chain of `nk` <= 8 launches of a kernel that does NO arithmetic.  shape [nk][5] (HOST ints): grid
 * size, block size, dynamic LDS bytes, dependent global loads per thread (a pointer chase through `workspace`, 64 KB of it,
 * L2-resident), workgroup barriers.  Launched with the shapes and dependent-access counts of the step's kernels, the chain's
 * time per iteration is what those launches cost when their arithmetic is free: dispatch, drain and the latency of the
 * dependent chain -- a floor of the five-launch iteration (bench.py reports it as roofline.step_floor_us).  Asynchronous and
 * graph-capturable: the caller times it.  workspace: >= 64 KB + 64 B, initialised by the first call's own set-up launch. */
int reart_relax_step_floor(const int *shape, int nk, int iters, void *workspace, size_t workspace_bytes, void *stream);

/* The same re-solve for Euclidean costs between two point sets, without a cost matrix: src, tgt [B,n,3], n <= 2048;
 * c_ij is the value reart_cdist(src, tgt) would hold (same fp32 expression), recomputed from LDS copies of both sets
 * wherever the solver needs a cost -- a path-search step then reads no memory beyond LDS.  Result identical to
 * reart_lap_resolve on reart_cdist's matrix. */
int reart_lap_resolve_points(const float *src, const float *tgt, int B, int n, int32_t *col4row,
                             int32_t *certified, const double *price_in, double *price_out, void *workspace,
                             size_t workspace_bytes, void *stream);

/* reart_lap_resolve_points with `racers` (2..13) workgroups per problem on otherwise idle compute units (a re-solve keeps
 * one workgroup per problem busy: 19 of 256 compute units at README.md:125's 20 frames).  Every racer runs the same exact
 * algorithm from the same start and differs only in the order in which it takes the free rows (ascending, descending,
 * fixed pseudo-random permutations); the first to finish publishes, the others leave at their next step.  The assignment is the optimum either way; the potentials written to price_out -- and, between optima
 * of exactly equal cost, the assignment -- are the winner's, so not reproducible run to run.  stats[b][0] carries the
 * winning racer in bits 16+.  workspace: reart_lap_race_workspace_bytes(B, n, racers).  n < 512 runs the plain re-solve. */
int reart_lap_resolve_points_race(const float *src, const float *tgt, int B, int n, int racers, int32_t *col4row,
                                  int32_t *certified, const double *price_in, double *price_out, void *workspace,
                                  size_t workspace_bytes, void *stream);

/* reart_lap_resolve_points[_race] with one search per WAVE (csrc/lap_mw.hip): the free rows a refresh leaves (run_robot.py:164-187
 * re-solves every assign_gap iterations) are mostly independent of each other, so every wave of a problem's workgroup follows
 * its own free row -- row-reduction chain, then a shortest augmenting path -- on columns it holds in registers, and commits
 * under a workgroup lock after checking that the columns it is about to write are still as it saw them.  512 <= n <= 2048
 * (REART_ERR_UNSUPPORTED otherwise: call reart_lap_resolve_points_race).  racers >= 1 workgroups per problem (free rows taken
 * in different orders); workspace: reart_lap_race_workspace_bytes(B, n, racers).  Outputs, certificate and the caveat on the
 * potentials as reart_lap_resolve_points_race; stats[b] = released rows (+ winner << 16), rows left for the path searches |
 * commit conflicts << 16, path-search steps, 1 + 256 * row-reduction steps. */
int reart_lap_resolve_points_mw(const float *src, const float *tgt, int B, int n, int racers, int32_t *col4row,
                                int32_t *certified, const double *price_in, double *price_out, void *workspace,
                                size_t workspace_bytes, void *stream);

/* reart_lap_resolve_points_mw with every problem's row reduction spread over `arr_wgs` workgroups (1..256; csrc/lap_mw.hip:
 * lap_mc_arr_kernel -- the chains only meet in the column they commit on, so their state lives in memory and a commit is a
 * lock-free compare-and-swap on the column's owner), the path searches then one workgroup per problem and racer.  Three
 * launches between the two whole-chip passes.  512 <= n <= 2048; workspace: reart_lap_mc_workspace_bytes(B, n, racers).
 * Outputs, certificate, statistics and the caveat on the potentials as reart_lap_resolve_points_mw; certified [B] and the
 * statistics need no clearing by the caller (the set-up launch defines them: no fill launches in front of a refresh). */
size_t reart_lap_mc_workspace_bytes(int B, int n, int racers);
int reart_lap_resolve_points_mc(const float *src, const float *tgt, int B, int n, int racers, int arr_wgs, int32_t *col4row,
                                int32_t *certified, const double *price_in, double *price_out, void *workspace,
                                size_t workspace_bytes, void *stream);

/* Is the optimum a solve returned the ONLY optimal assignment?  (csrc/ties.hip; reference: the refresh is scipy's
 * linear_sum_assignment, a pure function of the cost matrix, run_robot.py:172-176, so a run repeats under --manual_seed,
 * run_robot.py:37-49; the raced solvers above return SOME optimum.)  Inputs: the points of reart_lap_resolve_points, the
 * optimum col4row [B,n] and its column potentials price [B,n] as those calls leave them; n <= 4096.  Outputs (caller-owned):
 *   cols [B,n,K]   per row the columns j != s(i) whose pair is tight under the potentials,
 *                  c_ij + p_j - (c_i,s(i) + p_s(i)) <= 1e-13 x cost scale (the certificate's tolerance), costs by reart_cdist's
 *                  expression -- the first K of them (1 <= K <= 32); cnt [B,n] how many the row has (may exceed K);
 *   tie [B]        0: no alternating cycle among the tight pairs -- the optimum is unique; 1: there is one -- other optima of
 *                  the same cost exist (the host chooses: reart_amd/utils/lap.py canonical_among_ties); 2: a row has more
 *                  than K tight pairs (the host lists them itself); 3: col4row is not an assignment.
 * Two launches on `stream`, no workspace, no host synchronisation. */
int reart_lap_ties(const float *src, const float *tgt, int B, int n, const int32_t *col4row, const double *price,
                   int32_t *tie, int32_t *cols, int32_t *cnt, int K, void *stream);

/* reart_lap_resolve_points_mc followed by the tie check of reart_lap_ties, with the tight pairs listed by the solve's own
 * certificate pass (its scan meets exactly the pairs within the tolerance of the row's minimum: no second pass over the costs).
 * Same inputs / outputs as the two calls; n >= 512.  A problem whose certificate needed more rounds than the pass (its
 * potentials moved afterwards) comes back with tie = 2: the host lists its pairs itself.  Reference: run_robot.py:172-176 (the
 * refresh as a function of the cost matrix), run_robot.py:37-49 (runs repeat under --manual_seed). */
int reart_lap_resolve_points_mc_ties(const float *src, const float *tgt, int B, int n, int racers, int arr_wgs, int32_t *col4row,
                                     int32_t *certified, const double *price_in, double *price_out, int32_t *tie, int32_t *cols,
                                     int32_t *cnt, int K, void *workspace, size_t workspace_bytes, void *stream);

/* Device-side glue of an assignment refresh (run_robot.py:165-178), so that a loop which re-solves on the GPU touches the host
 * only for the B certificate flags (csrc/assign.hip):
 *   reart_gather_points: out[b][r] = pc[b][index[r]] -- `index_points(pc_trans_list, fps_idx)` (run_robot.py:169) for ONE sample
 *     shared by all frames; pc [B,N,3], index [n] (0 <= index[r] < N), out [B,n,3].
 *   reart_assign_pairs: the solved columns as the fused step's pair map (run_robot.py:177-178: `pc_tgt` gathered by the
 *     solver's columns, paired with the sampled source points in order): assign_map[b][p] = -1 where slot_of_point[p] < 0, else
 *     tgt_index[b][col4row[b][slot_of_point[p]]].  col4row [B,n], slot_of_point [N] (sample slot of canonical point p or -1),
 *     tgt_index [B,n] (index of the r-th sampled target point in frame b's cloud), assign_map [B,N] (reart_relax_buffers). */
int reart_gather_points(const float *pc, const int32_t *index, int B, int N, int n, float *out, void *stream);
/*   reart_publish_words: host_out = a[0..na) | b[0..nb) | c[0..nc) (int32 words in device memory; b, c may be empty), written by one
 *     launch into PINNED host memory (`host_out`: the pointer hipHostMalloc / torch's pin_memory returned) -- the certificate
 *     flags, tie flags and statistics the host reads after a refresh, without a copy launch each. */
int reart_publish_words(const int32_t *a, int na, const int32_t *b, int nb, const int32_t *c, int nc, int32_t *host_out, void *stream);
int reart_assign_pairs(const int32_t *col4row, const int32_t *slot_of_point, const int32_t *tgt_index, int B, int N, int n,
                       int32_t *assign_map, void *stream);

/* Cost matrices for the above: replaces `torch.cdist(pc_src, pc_tgt)` (run_robot.py:171, utils/model_utils.py:93).
 *   a [B,n,3], b [B,m,3] -> out [B,n,m] = Euclidean distance, sqrt(((dx*dx)+(dy*dy))+(dz*dz)) in fp32. */
int reart_cdist(const float *a, const float *b, int B, int n, int m, float *out, void *stream);

/* ------------------------------------------------------------------------ */
/* Correspondence matching on the extractor's descriptors                    */
/* ------------------------------------------------------------------------ */

/* Replaces match_smnn(desc1, desc2, th=0.9) (utils/flow_utils.py:48-100; called once per frame pair
 * by compute_corr_list_filter :116-143): nearest / second-nearest descriptor ratio test in both
 * directions and the mutual filter, without the [N1,N2] distance matrix.
 *   desc1 [E,N1,64], desc2 [E,N2,64] (point-major rows);  keep [E,N1] u8 = 1 where point i of desc1
 *   has a mutual match; tgt [E,N1] i64 = its nearest descriptor in desc2 (valid where keep).
 *   The matches of pair e, sorted by source index, are {(i, tgt[e,i]) : keep[e,i]}.
 *   th < 0 skips the ratio test: plain mutual nearest neighbours = the reference's matching="mnn" branch
 *   (k = 1 KNN in both directions + find_mutual_correspondences, utils/flow_utils.py:102-113, 126-137). */
size_t reart_match_smnn_workspace_bytes(int E, int N1, int N2);
int reart_match_smnn(const float *desc1, const float *desc2, int E, int N1, int N2, int D, float th,
                     uint8_t *keep, int64_t *tgt, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------ */
/* End-of-run structure extraction (run_robot.py:224-330)                     */
/* ------------------------------------------------------------------------ */

/* Screw decomposition and joint-type costs of relative part motions, one launch.  Replaces
 * compute_relative_trans + compute_geo_cost (utils/graph_utils.py:170-186, :131-167), compute_screw_trans /
 * compute_screw_cost (:235-292), compute_mean_screw_param (:207-232), frobenius_cost (:189-196), the identity
 * cost of merge_graph (:338-342) and the per-edge screw parameters of build_graph
 * (utils/kinematic_utils.py:84-99), with transform_to_dq / dq_to_screw (screw_se3/dq_utils.py:129-182).
 *   trans [T,P,4,4]; pairs [E,2] i32 (src, tgt): the relative motion of edge e in frame t is
 *   inv(trans[t,src]) * trans[t,tgt].  pairs == NULL: trans IS the relative motion, [T,E,4,4] (P ignored).
 *   plain_mean != 0: mean axis / moment over all frames (build_graph's single-edge call); 0: over the frames
 *   that are not a unit transform (compute_mean_screw_param), all frames when every frame is one or E <= 1.
 * Outputs (nullable unless noted): screw [T,E,8] = axis(3), moment(3), theta, distance;  rel [T,E,4,4];
 * mean [E,6] = mean axis, mean moment;  recon [T,E,4,4] = reconstruction with the cheaper joint type;
 * cost [E,4] (required) = revolute cost, prismatic cost, their minimum, mean over frames of |rel - I|^2;
 * mean_cost = mean_e(minimum) / T (compute_screw_cost's scalar).  workspace is needed when mean == NULL. */
size_t reart_screw_fit_workspace_bytes(int T, int E);
int reart_screw_fit(const float *trans, int T, int P, const int32_t *pairs, int E, int plain_mean,
                    float *screw, float *rel, float *mean, float *recon, float *cost, float *mean_cost,
                    void *workspace, size_t workspace_bytes, void *stream);

/* The screw-consistency term of networks/loss.py structure_loss (:32-57) with its gradient, as an operator of an
 * iteration: parallel over (edge, frame), at most two launches, no host synchronisation, no atomics.
 *   trans [T,P,4,4] and pairs [E,2] i32 (src, tgt) exactly as reart_screw_fit reads them; pairs == NULL: trans IS the
 *   relative motion [T,E,4,4] (P ignored).  Per edge e = (a, b) and frame t, with M = inv(trans[t,a]) * trans[t,b] and
 *   (l, m, theta, d) its screw parameters:
 *     unit(t,e)    = (|theta| <= 1e-5 or |theta - pi| <= 1e-5) and d <= 1e-5            (d signed)
 *     mean l, m    over the non-unit frames of e; over all frames when there is none or E <= 1
 *     prismatic(e) = mean_t |d| > mean_t |theta|            (structure_loss's rule, not reart_screw_fit's cost rule)
 *     G(t,e)       = screw -> SE(3) of (mean l, mean m, prismatic ? 1e-6f : theta, prismatic ? d : 1e-6f)
 *     edge_cost[e] = sum_t |M inv(G) - I|^2_F,   loss = weight * sum_e edge_cost[e]   (added in double, rounded once)
 *   G is a constant (the reference builds it under no_grad): grad = dloss/dtrans runs through M only,
 *   dloss/dM = 2 weight (M inv(G) - I) inv(G)^T on rows 0..2, carried to trans[t,a] and trans[t,b] through the rigid
 *   inverse [R^T | -R^T t].  grad has the shape of trans and is written completely: zeros where nothing arrives and in
 *   row 3, which holds constants (the reference's 4x4 products leave a non-zero gradient there that reaches no parameter).
 *   A part's gradient is the sum over its incident edges in ascending edge number: the same bits on every run.
 * Outputs: loss (required), edge_cost [E], prismatic [E] u8, grad (all three nullable).
 * T <= REART_MAX_POSE_LEN, P <= 64, E <= 4096: beyond them the workspace query returns 0 and the call
 * REART_ERR_UNSUPPORTED.  NULL trans / loss, T or P <= 0, E < 0, a NULL or short workspace: REART_ERR_INVALID_ARG.
 * E == 0: loss 0, grad zeros.  A pair index outside [0,P) is the caller's error (such an edge is skipped). */
size_t reart_structure_term_workspace_bytes(int T, int P, int E);
int reart_structure_term(const float *trans, int T, int P, const int32_t *pairs, int E, float weight, float *loss,
                         float *edge_cost, uint8_t *prismatic, float *grad, void *workspace, size_t workspace_bytes,
                         void *stream);

/* Reverse mode of rel[t,e] = inv(trans[t,src]) * trans[t,tgt] (reart_screw_fit's `rel`, compute_relative_trans of
 * utils/graph_utils.py:162-175) with the rigid inverse: grad_rel [T,E,4,4] (row 3 ignored) -> grad_trans [T,P,4,4],
 * written completely, row 3 zero, a part's sum over its incident edges in ascending edge number.  Limits and statuses
 * as reart_structure_term; pairs is required. */
size_t reart_rel_trans_backward_workspace_bytes(int T, int P, int E);
int reart_rel_trans_backward(const float *trans, int T, int P, const int32_t *pairs, int E, const float *grad_rel,
                             float *grad_trans, void *workspace, size_t workspace_bytes, void *stream);

/* The connection term of networks/loss.py compute_connection_loss (:60-78) as two operators of an iteration: the selection of
 * the pairs in the canonical cloud, and their cost in the predicted frames with its gradient.  No host synchronisation, no
 * floating-point atomics, the same bits on every run.
 *
 * reart_connection_select: cano [N,3], seg [N] i64, pairs [E,2] i32 (src part a, tgt part b) -> src_idx, tgt_idx [E,k] i32
 * (indices into cano), sel_dist [E,k] (nullable), valid [E] u8.  A label outside [0,P) belongs to no part.  Per edge:
 *     d_i          = min over j with seg[j] == b of ((dx*dx)+(dy*dy))+(dz*dz), for every i with seg[i] == a   (fp32, no FMA:
 *                    the rounding of the K-NN searches at D = 3); the neighbour of i is the LOWEST j attaining the minimum
 *     row r        = the r-th smallest key (bits of d_i, i), r = 0 .. k-1: src_idx = i, tgt_idx = its neighbour, sel_dist = d_i
 *     valid[e]     = a, b in [0,P), |a| >= k and |b| >= 1 (outside that the reference raises); an invalid edge gets
 *                    valid = 0, indices 0, distance 0, and contributes nothing to reart_connection_term
 *   A self edge (a, a) follows from the rule: every d_i = +0, the k lowest indices of the part, each paired with the lowest
 *   index at its coordinates (itself, unless an earlier point of the part coincides with it).
 *   Every index written is a member of its part, or the edge is invalid, whatever the coordinates hold: non-finite
 *   coordinates give a meaningless selection, never an out-of-range access.
 *   Three launches: the parts' member lists (a stable counting sort by label), the search (the sources of an edge divided
 *   among up to 16 workgroups of 256, the target members tiled through LDS, a top-k per wave), the merge of the workgroups'
 *   partial lists.
 *
 * reart_connection_term: pc_trans [T,N,3] and the tables above ->
 *     edge_cost[e] = (1/k) sum_t sum_r |p[t,src(e,r)] - p[t,tgt(e,r)]|^2     (the squared distances in fp32 with the rounding
 *                    above, added in double in a fixed order, divided by k, rounded once)
 *     loss         = weight * sum_e edge_cost[e]                             (in double, rounded once)
 *     grad[t,n]    = sum of +-(2 weight / k)(p[t,src] - p[t,tgt]) over the records that name n, + as a source, - as a target.
 *   A record is 2 (e k + r) + role (role 0: the source of row r of edge e, 1: its target); a point's records are added in
 *   ascending record number, in fp32: the order depends on the index tables only.  grad is written completely, zeros where no
 *   record arrives.  Rows of an edge with valid = 0, and rows with an index outside [0,N), take no part.
 *   Three launches with grad (the edge costs; the records grouped by point; the gradient and the loss), two without.
 * Outputs: loss (required), edge_cost [E], grad (both nullable).
 *
 * Limits: T <= REART_MAX_POSE_LEN, P <= 64, E <= 4096, 1 <= k <= REART_CONN_MAX_K, N <= REART_CONN_MAX_N (a key carries two
 * point indices in 32 bits): beyond them the workspace queries return 0 and the calls REART_ERR_UNSUPPORTED.  A NULL required
 * pointer (the tables and pairs are required when E > 0), a non-positive T, N, P or k, E < 0, a NULL or short workspace:
 * REART_ERR_INVALID_ARG.  E == 0: nothing selected; loss 0, grad zeros. */
#define REART_CONN_MAX_N 65536
#define REART_CONN_MAX_K 64
size_t reart_connection_select_workspace_bytes(int N, int P, int E, int k);
int reart_connection_select(const float *cano, const int64_t *seg, int N, int P, const int32_t *pairs, int E, int k,
                            int32_t *src_idx, int32_t *tgt_idx, float *sel_dist, uint8_t *valid, void *workspace,
                            size_t workspace_bytes, void *stream);
size_t reart_connection_term_workspace_bytes(int T, int N, int E, int k);
int reart_connection_term(const float *pc_trans, const int32_t *src_idx, const int32_t *tgt_idx, const uint8_t *valid, int T,
                          int N, int E, int k, float weight, float *loss, float *edge_cost, float *grad, void *workspace,
                          size_t workspace_bytes, void *stream);

/* Replaces fps_sample_cano (utils/graph_utils.py:37-52): farthest point sampling inside every part, one
 * workgroup per part.  cano [N,3], seg [N] i64, labels [Ps] i64 -> idx [Ps,num_fps] i64 (indices into cano,
 * start = the part's first point like the reference's CUDA FPS; -1 when the part has fewer than num_fps
 * points), count [Ps] i32 = part sizes.  cuda_mode as in reart_fps.
 * The whole cloud's member list and running distances live in LDS: N <= REART_PART_FPS_MAX_N, REART_ERR_UNSUPPORTED
 * above (N <= 6144 fits the default 48 KB; above that the entry point opts in to the large LDS window). */
#define REART_PART_FPS_MAX_N 19200        /* reart_part_fps: 8 B of LDS per point of the cloud */
int reart_part_fps(const float *cano, const int64_t *seg, int N, const int64_t *labels, int Ps, int num_fps,
                   int cuda_mode, int64_t *idx, int32_t *count, void *stream);

/* Replaces compute_spatial_cost (utils/graph_utils.py:70-84) and compute_joint_cost (:87-100) over all
 * ordered part pairs.  cano_fps [Ps,F,3]; frame_fps [T,Ps,F,3] (nullable: the same points in the predicted
 * frames) -> cano_dist [Ps,Ps] = squared distance of the closest pair (i -> j), pair [Ps,Ps,2] i64 = that
 * pair's (source, target) FPS slots (first minimum), joint [Ps,Ps] = its squared distance summed over frames. */
int reart_part_pair_cost(const float *cano_fps, const float *frame_fps, int T, int Ps, int F, float *cano_dist,
                         int64_t *pair, float *joint, void *stream);

/* Replaces compute_group_temporal_err (utils/model_utils.py:107-118).  pcs [T,N,3], seg [N] i64,
 * labels [Ps] i64 -> per_part [Ps], worst = max over parts. */
int reart_group_temporal_err(const float *pcs, int T, int N, const int64_t *seg, const int64_t *labels, int Ps,
                             float *per_part, float *worst, void *stream);

/* The contrastive descriptor loss (PointInfoNCE) on two descriptor sets, streaming: the N1 x N2 logits are formed tile by tile
 * on the fp32 matrix cores and never stored (csrc/infonce.hip).
 *   f1 [B,N1,C], f2 [B,N2,C] f32 contiguous; pos [B,N1] i64: the column of f2 that is the positive of row i, an entry outside
 *   [0, N2) (the conventional -1) = row not used; col_mask [B,N2] u8 or NULL: 0 = the column takes part in no row's sum, and a
 *   row whose positive is masked out is not used; tau > 0.  s_ij = <f1_i, f2_j> / tau.
 * reart_infonce_forward -> for the used rows lse = log sum_j exp(s_ij) over the live columns, row_loss = lse - s_i,pos(i),
 *   top = the lowest live column attaining the row maximum (unused rows: 0, 0, -1); count [1] i64 = used rows of the batch;
 *   loss [1] = the sum of row_loss in double, a fixed order, divided by count and rounded once (count = 0: exactly 0).
 *   All of loss, row_loss, lse [B,N1] f32, top [B,N1] i64 and count are required.  Three launches.
 * reart_infonce_backward: from the forward's operands, its lse and count, and an upstream scalar g [1] on the device (NULL = 1):
 *   with p'_ij = exp(s_ij - lse_i) - [j = pos(i)] on live columns of used rows, 0 elsewhere,
 *   dF1_i = g / (count tau) sum_j p'_ij f2_j [B,N1,C], dF2_j = g / (count tau) sum_i p'_ij f1_i [B,N2,C]; either may be NULL (not
 *   computed).  Every row of a computed output is written, unused rows and masked columns with zeros.  One or two launches each.
 * Nothing is kept between calls but what the caller holds.  No floating-point atomics, a fixed summation order for every
 * output entry (the same bits on every run), no host synchronisation, the given stream only.  Non-finite descriptors give
 * meaningless values, never an out-of-range access; pos is range-checked on the device.
 * Limits: 1 <= C <= REART_MAX_D, N1 and N2 <= REART_NCE_MAX_N, B <= REART_NCE_MAX_B; beyond them the workspace query returns 0
 * and the calls REART_ERR_UNSUPPORTED.  tau <= 0, C < 1, a negative size, a NULL required pointer, a NULL or short workspace:
 * REART_ERR_INVALID_ARG.  B = 0 or N1 = 0: REART_OK, loss 0, count 0.  One workspace size serves both calls. */
#define REART_NCE_MAX_N 65536
#define REART_NCE_MAX_B 1024
size_t reart_infonce_scratch_bytes(int B, int N1, int N2, int C);
int reart_infonce_forward(const float *f1, const float *f2, const int64_t *pos, const uint8_t *col_mask, int B, int N1, int N2,
                          int C, float tau, float *loss, float *row_loss, float *lse, int64_t *top, int64_t *count,
                          void *workspace, size_t workspace_bytes, void *stream);
int reart_infonce_backward(const float *f1, const float *f2, const int64_t *pos, const uint8_t *col_mask, const float *lse,
                           const int64_t *count, const float *g, int B, int N1, int N2, int C, float tau, float *dF1, float *dF2,
                           void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* REART_HIP_H */
