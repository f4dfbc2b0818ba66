// reart_amd/csrc/ik.hip -- retargeting for gfx950: fit the joint angles of a screw-joint tree to M novel poses in ONE launch.
//
// Replaces, fused, the optimisation loop of the reference's ik for a kinematic model (utils/kinematic_utils.py:200-266):
// per novel pose 200 x ( KinematicModel.forward on the sparse points, sum of squared distances to their targets, autograd
// backward, Adam(amsgrad) step on theta ).  As separate launches that is some two dozen kernels per step (label transfer,
// fk_fwd_kernel, pc_transform_kernel, pose_grad_kernel, pose_grad_sum_kernel, fk_bwd_kernel, lm_reduce_kernel, the
// optimiser) for a problem of a few dozen numbers; here one wave per pose keeps the tree, the points, theta and the optimiser
// state in LDS / registers and runs every step without touching global memory (the optional loss history apart).  The poses
// are independent: no workgroup talks to another, no atomics, and pose m's result is the same whatever M is.
//
// Mapping (one wave = one workgroup = one pose):
//   lane c <-> part c (P <= 64).  A part other than the root owns the edge to its parent: its axis, moment, theta, the
//              Adam state of that theta and T_rel live in lane c's registers; screw_fwd / screw_bwd / Adam run on all
//              lanes at once.
//   the tree is walked by DEPTH LEVEL (derived once from `parent`): forward FK[c] = FK[parent] T_rel(c) for all parts of
//              a level at once, root to leaves; backward leaves to root, where a part first adds the contributions of its
//              children in ascending child label (a fixed order) to the pose gradient of its own points.
//   lane <-> point (stride 64) for the residuals and the loss; the loss is the wave butterfly sum of the lanes' partial sums.
//   lane <-> (part, entry of the 3x4 pose gradient) for the sums over a part's points, which are added in ascending point
//              index as pose_grad_kernel adds them: the points are grouped by part once, by a stable counting sort.
// Points whose label is outside [0, P) take no part (as in assign_pairs_kernel).
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see DESIGN.md, "Fused retargeting".
#include "common.h"
#include "internal.h"
#include <math.h>

#define FK_MAXP 64
#include "screw_dev.h"

#define IK_MAXN REART_IK_MAX_POINTS
#define IK_NOLABEL 0xFFFFu

// one wave per workgroup: the barrier orders the wave's own LDS traffic
#define IK_SYNC() __syncthreads()

__global__ __launch_bounds__(64) void ik_fit_kernel(const int *__restrict__ parent, const int *__restrict__ edge_of_part, int P,
                                                    const float *__restrict__ axis, const float *__restrict__ moment, int E,
                                                    const float *__restrict__ src, const int64_t *__restrict__ part, int n,
                                                    const float *__restrict__ tgt, const float *__restrict__ theta_init,
                                                    int n_iter, float lr, float beta1, float beta2, float eps,
                                                    float *__restrict__ theta, float *__restrict__ loss) {
    __shared__ float s_x[3 * IK_MAXN];            // source points, grouped by part
    __shared__ float s_t[3 * IK_MAXN];            // their targets in this pose
    __shared__ float s_g[3 * IK_MAXN];            // dL / d pc = 2 (pc - target)
    __shared__ unsigned short s_lab[IK_MAXN];     // label of point i; after the sort: of grouped point j
    __shared__ unsigned short s_perm[IK_MAXN];    // grouped point j -> point i
    __shared__ int s_off[FK_MAXP + 1];            // grouped points of part p: [s_off[p], s_off[p + 1])
    __shared__ int s_par[FK_MAXP];
    __shared__ int s_cnt[FK_MAXP];
    __shared__ int s_child[FK_MAXP];              // children of part p: s_child[coff .. coff + ccnt), ascending
    __shared__ float s_F[12 * FK_MAXP];           // FK of every part, 3x4 row-major
    __shared__ float s_gown[12 * FK_MAXP];        // pose gradient of a part's own points
    __shared__ float s_con[12 * FK_MAXP];         // what a part adds to its parent's pose gradient
    __shared__ float s_th[FK_MAXP];               // theta by edge, on the way in and out

    const int lane = threadIdx.x;
    const size_t pose = blockIdx.x;
    const float *tg = tgt + 3 * pose * (size_t)n;

    // ---- the tree: parent, own edge, depth, children
    int par = -1, e = -1;
    if (lane < P) {
        par = parent[lane];
        e = edge_of_part[lane];
        if (par < 0 || par >= P || par == lane || e < 0 || e >= E) { par = -1; e = -1; }      // the root, or not a joint
    }
    s_par[lane] = par;
    for (int k = lane; k < E; k += 64) s_th[k] = theta_init ? theta_init[pose * (size_t)E + k] : 1e-6f;
    for (int i = lane; i < n; i += 64) {
        const int64_t p = part[i];
        s_lab[i] = (p >= 0 && p < P) ? (unsigned short)p : (unsigned short)IK_NOLABEL;
    }
    IK_SYNC();
    int depth = 0;
    if (lane < P)
        for (int q = lane; s_par[q] >= 0 && depth < P; q = s_par[q]) ++depth;
    if (depth >= P) { depth = 0; par = -1; e = -1; }                                         // on or under a cycle: not a joint
    int maxd = depth;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int v = __shfl_xor(maxd, o, 64); maxd = v > maxd ? v : maxd; }
    IK_SYNC();
    s_par[lane] = par;
    IK_SYNC();
    // children of every part (ascending) and the points of every part (ascending: a stable counting sort)
    int ccnt = 0, npts = 0;
    if (lane < P) {
        for (int c = 0; c < P; ++c) ccnt += (s_par[c] == lane);
        for (int i = 0; i < n; ++i) npts += (s_lab[i] == lane);
    }
    s_cnt[lane] = ccnt;
    s_off[lane + 1] = npts;                                      // counts for now
    IK_SYNC();
    int coff = 0, poff = 0;
    for (int q = 0; q < lane; ++q) { coff += s_cnt[q]; poff += s_off[q + 1]; }
    int nv = 0;
    for (int q = 0; q < P; ++q) nv += s_off[q + 1];              // the points that carry a label
    IK_SYNC();
    if (lane < P) {
        int k = coff;
        for (int c = 0; c < P; ++c)
            if (s_par[c] == lane) s_child[k++] = c;
        k = poff;
        for (int i = 0; i < n; ++i)
            if (s_lab[i] == lane) s_perm[k++] = (unsigned short)i;
    }
    s_off[lane] = poff;                                          // lanes >= P: nv
    if (lane == 63) s_off[FK_MAXP] = nv;
    IK_SYNC();
    for (int j = lane; j < nv; j += 64) {
        const int i = s_perm[j];
#pragma unroll
        for (int k = 0; k < 3; ++k) { s_x[3 * j + k] = src[3 * (size_t)i + k]; s_t[3 * j + k] = tg[3 * (size_t)i + k]; }
    }
    if (lane < P)
        for (int j = poff; j < poff + npts; ++j) s_lab[j] = (unsigned short)lane;
#pragma unroll
    for (int k = 0; k < 12; ++k) s_F[12 * lane + k] = (k % 5 == 0) ? 1.f : 0.f;
    float l[3] = {0.f, 0.f, 0.f}, mo[3] = {0.f, 0.f, 0.f}, th = 0.f;
    if (e >= 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { l[k] = axis[3 * e + k]; mo[k] = moment[3 * e + k]; }
    }
    IK_SYNC();
    if (e >= 0) th = s_th[e];

    // ---- the steps
    float am = 0.f, av = 0.f, avmax = 0.f;
    double b1t = 1.0, b2t = 1.0;
    float *lrow = loss ? loss + pose * ((size_t)n_iter + 1) : nullptr;
    for (int it = 0;; ++it) {
        float Tr[12];
        if (e >= 0) screw_fwd(l, mo, th, 1e-6f, Tr);
        for (int d = 1; d <= maxd; ++d) {
            if (depth == d && e >= 0) {
                const float *Fp = s_F + 12 * par;
                float F[12];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float acc = Fp[4 * i] * Tr[j];
                        acc = fmaf(Fp[4 * i + 1], Tr[4 + j], acc);
                        acc = fmaf(Fp[4 * i + 2], Tr[8 + j], acc);
                        if (j == 3) acc = fmaf(Fp[4 * i + 3], 1.0f, acc);
                        F[4 * i + j] = acc;
                    }
#pragma unroll
                for (int k = 0; k < 12; ++k) s_F[12 * lane + k] = F[k];
            }
            IK_SYNC();
        }
        // residuals and the loss
        float ls = 0.f;
        for (int j = lane; j < nv; j += 64) {
            const float *T = s_F + 12 * s_lab[j];
            const float x0 = s_x[3 * j], x1 = s_x[3 * j + 1], x2 = s_x[3 * j + 2];
            float r[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float acc = x0 * T[4 * c];
                acc = fmaf(x1, T[4 * c + 1], acc);
                acc = fmaf(x2, T[4 * c + 2], acc);
                r[c] = (acc + T[4 * c + 3]) - s_t[3 * j + c];
                s_g[3 * j + c] = 2.0f * r[c];
            }
            ls += (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
        }
        ls = reart_wave_sum(ls);
        if (lrow && lane == 0) lrow[it] = ls;
        if (it == n_iter) break;
        IK_SYNC();
        // pose gradient of every part's own points: [ g x^T | g ], a part's points in ascending index
        for (int task = lane; task < 12 * P; task += 64) {
            const int p = task / 12, c = task % 12, gi = c >> 2, xi = c & 3;
            float acc = 0.f;
            for (int j = s_off[p]; j < s_off[p + 1]; ++j) {
                const float g = s_g[3 * j + gi];
                acc += xi < 3 ? g * s_x[3 * j + xi] : g;
            }
            s_gown[task] = acc;
        }
        IK_SYNC();
        // leaves -> root
        float gTr[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) gTr[k] = 0.f;
        for (int d = maxd; d >= 1; --d) {
            if (depth == d && e >= 0) {
                float gF[12];
#pragma unroll
                for (int k = 0; k < 12; ++k) gF[k] = s_gown[12 * lane + k];
                for (int q = coff; q < coff + ccnt; ++q) {
                    const float *cc = s_con + 12 * s_child[q];
#pragma unroll
                    for (int k = 0; k < 12; ++k) gF[k] += cc[k];
                }
                const float *Fp = s_F + 12 * par;
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        gTr[4 * i + j] = fmaf(Fp[8 + i], gF[8 + j], fmaf(Fp[4 + i], gF[4 + j], Fp[i] * gF[j]));
#pragma unroll
                for (int i = 0; i < 3; ++i) {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        s_con[12 * lane + 4 * i + k] = fmaf(gF[4 * i + 3], Tr[4 * k + 3],
                                                            fmaf(gF[4 * i + 2], Tr[4 * k + 2],
                                                                 fmaf(gF[4 * i + 1], Tr[4 * k + 1], gF[4 * i] * Tr[4 * k])));
                    s_con[12 * lane + 4 * i + 3] = gF[4 * i + 3];
                }
            }
            IK_SYNC();
        }
        // d loss / d theta and Adam(amsgrad) as torch.optim.Adam steps a float32 tensor
        b1t *= (double)beta1;
        b2t *= (double)beta2;
        if (e >= 0) {
            float gl[3] = {0.f, 0.f, 0.f}, gm[3] = {0.f, 0.f, 0.f}, g, gd;
            screw_bwd(l, mo, th, 1e-6f, gTr, gl, gm, &g, &gd);
            const float step_size = (float)((double)lr / (1.0 - b1t));
            const float bc2s = (float)sqrt(1.0 - b2t);
            am = am + (g - am) * (1.0f - beta1);
            av = av * beta2 + ((1.0f - beta2) * g) * g;
            avmax = fmaxf(avmax, av);
            const float denom = sqrtf(avmax) / bc2s + eps;
            th = th - step_size * (am / denom);
        }
    }
    if (e >= 0) s_th[e] = th;
    IK_SYNC();
    for (int k = lane; k < E; k += 64) theta[pose * (size_t)E + k] = s_th[k];
}

extern "C" int reart_ik_fit(const int32_t *parent, const int32_t *edge_of_part, const int32_t *order, int P,
                            const float *axis, const float *moment, int E, const float *src, const int64_t *part, int n,
                            const float *tgt, int M, const float *theta_init, int n_iter, float lr, float beta1, float beta2,
                            float eps, float *theta, float *loss, void *stream) {
    if (P < 1 || P > FK_MAXP || E != P - 1 || n < 1 || M < 0 || n_iter < 0) return REART_ERR_INVALID_ARG;
    if (!parent || !edge_of_part || !order || !src || !part || !tgt) return REART_ERR_INVALID_ARG;
    if (E > 0 && (!axis || !moment || !theta)) return REART_ERR_INVALID_ARG;
    if (n > REART_IK_MAX_POINTS) return REART_ERR_UNSUPPORTED;
    if (M == 0) return REART_OK;
    hipLaunchKernelGGL(ik_fit_kernel, dim3(M), dim3(64), 0, (hipStream_t)stream, parent, edge_of_part, P, axis, moment, E, src,
                       part, n, tgt, theta_init, n_iter, lr, beta1, beta2, eps, theta, loss);
    REART_CHECK_LAUNCH();
    return REART_OK;
}
