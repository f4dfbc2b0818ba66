// reart_amd/csrc/screw_dev.h -- device helpers shared by kinematic.hip, ik.hip and structure.hip:
// one screw joint (l, m, theta, d) -> rigid transform (screw_fwd) and its reverse mode (screw_bwd), i.e. the reference's
//   screw_param_to_exponential_coordinates  screw_se3/screw_utils.py:6-23
//   transform_from_exponential_coordinates  screw_se3/screw_utils.py:27-30
//   se3_exp_map (+ _so3_exp_map, _se3_V_matrix) screw_se3/geo_utils.py:90-222
// composed (clamp on the SQUARED rotation norm at 1e-4, strict fp32 no-rotation test).
#pragma once
#include <math.h>

#define PI_F 3.14159265358979323846f

__device__ __forceinline__ void mat3_mul(const float *A, const float *B, float *C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            C[3 * i + j] = fmaf(A[3 * i + 2], B[6 + j], fmaf(A[3 * i + 1], B[3 + j], A[3 * i] * B[j]));
}

// one joint: (l, m, theta, d) -> T = [R | tr] (3x4 row-major, T[4*i+j])
__device__ __forceinline__ void screw_fwd(const float *l, const float *m, float theta, float d, float *T) {
    const bool no_rot = (fabsf(theta) < 1e-6f) || (fabsf(theta - PI_F) < 1e-6f);
    const float q[3] = {l[1] * m[2] - l[2] * m[1], l[2] * m[0] - l[0] * m[2], l[0] * m[1] - l[1] * m[0]};
    const float h = d / theta;
    const float ql[3] = {q[1] * l[2] - q[2] * l[1], q[2] * l[0] - q[0] * l[2], q[0] * l[1] - q[1] * l[0]};
    float om[3], u[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float w = no_rot ? 0.f : l[c];
        const float v = no_rot ? l[c] : ql[c] + h * l[c];
        om[c] = w * theta;
        u[c] = v * theta;
    }
    const float n2 = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2];
    const float ph = sqrtf(n2 < 1e-4f ? 1e-4f : n2);
    const float inv = 1.0f / ph;
    const float s = sinf(ph), c = cosf(ph);
    const float fac1 = inv * s, fac2 = inv * inv * (1.0f - c);
    const float K[9] = {0.f, -om[2], om[1], om[2], 0.f, -om[0], -om[1], om[0], 0.f};
    float K2[9];
    mat3_mul(K, K, K2);
    const float bV = (1.0f - c) / (ph * ph), cV = (ph - s) / (ph * ph * ph);
    float V[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const float id = (i % 4 == 0) ? 1.0f : 0.0f;
        T[4 * (i / 3) + i % 3] = (fac1 * K[i] + fac2 * K2[i]) + id;
        V[i] = (id + K[i] * bV) + K2[i] * cV;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
        T[4 * i + 3] = fmaf(V[3 * i + 2], u[2], fmaf(V[3 * i + 1], u[1], V[3 * i] * u[0]));
}

// reverse mode of screw_fwd: gT (3x4) -> gl, gm (accumulated), gtheta, gd (returned by pointer)
__device__ __forceinline__ void screw_bwd(const float *l, const float *m, float theta, float d,
                                          const float *gT, float *gl, float *gm, float *gtheta, float *gd) {
    const bool no_rot = (fabsf(theta) < 1e-6f) || (fabsf(theta - PI_F) < 1e-6f);
    const float q[3] = {l[1] * m[2] - l[2] * m[1], l[2] * m[0] - l[0] * m[2], l[0] * m[1] - l[1] * m[0]};
    const float h = d / theta;
    const float ql[3] = {q[1] * l[2] - q[2] * l[1], q[2] * l[0] - q[0] * l[2], q[0] * l[1] - q[1] * l[0]};
    float w[3], v[3], om[3], u[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        w[c] = no_rot ? 0.f : l[c];
        v[c] = no_rot ? l[c] : ql[c] + h * l[c];
        om[c] = w[c] * theta;
        u[c] = v[c] * theta;
    }
    const float n2 = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2];
    const bool clamped = n2 < 1e-4f;
    const float ph = sqrtf(clamped ? 1e-4f : n2);
    const float s = sinf(ph), c = cosf(ph);
    const float ph2 = ph * ph, ph3 = ph2 * ph, ph4 = ph2 * ph2;
    const float a = s / ph, b = (1.0f - c) / ph2, cV = (ph - s) / ph3;
    const float K[9] = {0.f, -om[2], om[1], om[2], 0.f, -om[0], -om[1], om[0], 0.f};
    float K2[9];
    mat3_mul(K, K, K2);
    float V[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) V[i] = (((i % 4 == 0) ? 1.0f : 0.0f) + K[i] * b) + K2[i] * cV;
    // tr = V u
    float gV[9], gu[3] = {0.f, 0.f, 0.f}, gR[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            gR[3 * i + j] = gT[4 * i + j];
            gV[3 * i + j] = gT[4 * i + 3] * u[j];
            gu[j] += V[3 * i + j] * gT[4 * i + 3];
        }
    float ga = 0.f, gb = 0.f, gc = 0.f, gK[9], gK2[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        ga += gR[i] * K[i];
        gb += gR[i] * K2[i] + gV[i] * K[i];
        gc += gV[i] * K2[i];
        gK[i] = a * gR[i] + b * gV[i];
        gK2[i] = b * gR[i] + cV * gV[i];
    }
    // K2 = K K : gK += gK2 K^T + K^T gK2
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) acc += gK2[3 * i + k] * K[3 * j + k] + K[3 * k + i] * gK2[3 * k + j];
            gK[3 * i + j] += acc;
        }
    float gom[3] = {gK[7] - gK[5], gK[2] - gK[6], gK[3] - gK[1]};
    if (!clamped) {
        const float da = (ph * c - s) / ph2;
        const float db = (ph * s - 2.0f * (1.0f - c)) / ph3;
        const float dc = ((1.0f - c) * ph - 3.0f * (ph - s)) / ph4;
        const float gph = ga * da + gb * db + gc * dc;
#pragma unroll
        for (int k = 0; k < 3; ++k) gom[k] += gph * om[k] / ph;
    }
    float gth = 0.f, gw[3], gv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        gth += gom[k] * w[k] + gu[k] * v[k];
        gw[k] = theta * gom[k];
        gv[k] = theta * gu[k];
    }
    float gdd = 0.f;
    if (!no_rot) {
        // v = q x l + h l ; q = l x m ; w = l ; h = d / theta
        const float gq[3] = {l[1] * gv[2] - l[2] * gv[1], l[2] * gv[0] - l[0] * gv[2], l[0] * gv[1] - l[1] * gv[0]};
        const float gvq[3] = {gv[1] * q[2] - gv[2] * q[1], gv[2] * q[0] - gv[0] * q[2], gv[0] * q[1] - gv[1] * q[0]};
        const float gh = gv[0] * l[0] + gv[1] * l[1] + gv[2] * l[2];
        const float mgq[3] = {m[1] * gq[2] - m[2] * gq[1], m[2] * gq[0] - m[0] * gq[2], m[0] * gq[1] - m[1] * gq[0]};
        const float gql[3] = {gq[1] * l[2] - gq[2] * l[1], gq[2] * l[0] - gq[0] * l[2], gq[0] * l[1] - gq[1] * l[0]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            gl[k] += gvq[k] + h * gv[k] + mgq[k] + gw[k];
            gm[k] += gql[k];
        }
        gdd = gh / theta;
        gth -= gh * d / (theta * theta);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) gl[k] += gv[k];
    }
    *gtheta = gth;
    *gd = gdd;
}
