// reart_amd/csrc/flow_dev.h -- the per-point expressions of the flow term, shared by the kernels of flow.hip (blend_kernel,
// blend_batch_kernel, flow_loss_kernel) and of flow_term.hip: one definition, so that every path rounds alike.  The fused
// step's flow_blend_body (step.hip) takes huber1 / huber1_grad from here and keeps the rest inline (see there).
#pragma once
#include "common.h"
#include <math.h>

// blend of one query (utils/flow_utils.py:160-167): inverse-distance weights of its k neighbours' flows and the validity mask
//   d[d < 1e-10] = 1e-10; w = 1/d; w /= sum w; flow = sum_k w_k f[idx_k];  mask = min d <= max_k |f[idx_k]|^2  or  min d <= 0.05
// dist / idx: the query's k distances and neighbour indices (memory or registers), rf: the reference flows of its set
template <class Idx>
__device__ __forceinline__ bool reart_blend_point(const float *dist, const Idx *idx, const int k, const float *__restrict__ rf,
                                                  float &a0, float &a1, float &a2) {
    float wsum = 0.f, dmin = INFINITY, fmx = -INFINITY;
    for (int j = 0; j < k; ++j) {
        float d = dist[j];
        if (d < 1e-10f) d = 1e-10f;
        wsum += 1.0f / d;
        dmin = fminf(dmin, d);
        const float *f = rf + 3 * idx[j];
        fmx = fmaxf(fmx, (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]);
    }
    a0 = 0.f; a1 = 0.f; a2 = 0.f;
    for (int j = 0; j < k; ++j) {
        float d = dist[j];
        if (d < 1e-10f) d = 1e-10f;
        const float wn = (1.0f / d) / wsum;
        const float *f = rf + 3 * idx[j];
        a0 += f[0] * wn; a1 += f[1] * wn; a2 += f[2] * wn;
    }
    return (dmin <= fmx) || (dmin <= 0.05f);
}

__device__ __forceinline__ float huber1(float x) {
    const float a = fabsf(x);
    return a <= 1.0f ? 0.5f * x * x : (a - 0.5f);
}
__device__ __forceinline__ float huber1_grad(float x) {
    return fabsf(x) <= 1.0f ? x : (x > 0.f ? 1.0f : -1.0f);
}

// flow loss of one point (networks/loss.py:10-21): m f + smooth (not m) |pred|^2, f = |pred - gt|^2 or Huber(delta = 1), as a
// double, and d loss / d pred into grad[0..2] (nullable)
__device__ __forceinline__ double reart_flow_point(const float *gt, const float *pred, const bool m, const int robust,
                                                   const float smooth, float *grad) {
    float f = 0.f, sm = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float p = pred[c], d = p - gt[c];
        f += robust ? huber1(d) : d * d;
        sm += p * p;
        if (grad) {
            const float gf = robust ? huber1_grad(d) : 2.0f * d;
            grad[c] = m ? gf : smooth * (2.0f * p);
        }
    }
    return m ? (double)f : (double)(smooth * sm);
}
