// reart_amd/csrc/screw_dev.h -- device helpers shared by kinematic.hip, ik.hip and structure.hip:
// one screw joint (l, m, theta, d) -> rigid transform (screw_fwd) and its reverse mode (screw_bwd), i.e. the reference's
//   screw_param_to_exponential_coordinates  screw_se3/screw_utils.py:6-23
//   transform_from_exponential_coordinates  screw_se3/screw_utils.py:27-30
//   se3_exp_map (+ _so3_exp_map, _se3_V_matrix) screw_se3/geo_utils.py:90-222
// composed (clamp on the SQUARED rotation norm at 1e-4, strict fp32 no-rotation test), and the way back shared by
// structure.hip and structure_term.hip: rel_transform (inv(A) B), transform_to_screw (transform_to_dq + dq_to_screw,
// screw_se3/dq_utils.py:129-182) and frob_cost (utils/graph_utils.py frobenius_cost).
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

// ------------------------------------------------------------------------------------------------------------
// relative transform inv(A) * B of two [R|t] (4x4 row-major in memory) -> 3x4
__device__ __forceinline__ void rel_transform(const float *A, const float *B, float *M) {
    float tinv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)  // -R_a^T t_a
        tinv[i] = (-A[i] * A[3] + -A[4 + i] * A[7]) + -A[8 + i] * A[11];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) M[4 * i + j] = (A[i] * B[j] + A[4 + i] * B[4 + j]) + A[8 + i] * B[8 + j];
        M[4 * i + 3] = ((A[i] * B[3] + A[4 + i] * B[7]) + A[8 + i] * B[11]) + tinv[i];
    }
}

__device__ __forceinline__ void q_mul(const float *q1, const float *q2, float *o) {  // dq_utils.py:63-83
    o[0] = ((q2[0] * q1[0] - q2[1] * q1[1]) - q2[2] * q1[2]) - q2[3] * q1[3];
    o[1] = ((q2[0] * q1[1] + q2[1] * q1[0]) - q2[2] * q1[3]) + q2[3] * q1[2];
    o[2] = ((q2[0] * q1[2] + q2[1] * q1[3]) + q2[2] * q1[0]) - q2[3] * q1[1];
    o[3] = ((q2[0] * q1[3] - q2[1] * q1[2]) + q2[2] * q1[1]) + q2[3] * q1[0];
}

// rigid transform M (3x4) -> screw parameters: axis l, moment m, angle theta, displacement d
__device__ __forceinline__ void transform_to_screw(const float *M, float *l, float *m, float &theta, float &d) {
    const float eps = 1e-6f;
    const float m00 = M[0], m01 = M[1], m02 = M[2], m10 = M[4], m11 = M[5], m12 = M[6], m20 = M[8], m21 = M[9], m22 = M[10];
    const float a[4] = {((1.0f + m00) + m11) + m22, ((1.0f + m00) - m11) - m22, ((1.0f - m00) + m11) - m22,
                        ((1.0f - m00) - m11) + m22};
    float qa[4];
    int best = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        qa[i] = a[i] > 0.f ? sqrtf(a[i]) : 0.f;
        if (qa[i] > qa[best]) best = i;  // first maximum
    }
    float c[4];
    if (best == 0) { c[0] = qa[0] * qa[0]; c[1] = m21 - m12; c[2] = m02 - m20; c[3] = m10 - m01; }
    else if (best == 1) { c[0] = m21 - m12; c[1] = qa[1] * qa[1]; c[2] = m10 + m01; c[3] = m02 + m20; }
    else if (best == 2) { c[0] = m02 - m20; c[1] = m10 + m01; c[2] = qa[2] * qa[2]; c[3] = m12 + m21; }
    else { c[0] = m10 - m01; c[1] = m20 + m02; c[2] = m21 + m12; c[3] = qa[3] * qa[3]; }
    const float den = 2.0f * fmaxf(qa[best], 0.1f);
    float qr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qr[i] = c[i] / den;
    const float tq[4] = {0.f, M[3], M[7], M[11]};
    float qd[4];
    q_mul(tq, qr, qd);
#pragma unroll
    for (int i = 0; i < 4; ++i) qd[i] *= 0.5f;
    const float nq = sqrtf(((qr[0] * qr[0] + qr[1] * qr[1]) + qr[2] * qr[2]) + qr[3] * qr[3]);
    const float qn[4] = {qr[0] / nq, qr[1] / nq, qr[2] / nq, qr[3] / nq};
    const float nim = sqrtf((qn[1] * qn[1] + qn[2] * qn[2]) + qn[3] * qn[3]);
    float th = 2.0f * atan2f(nim, qn[0]);
    const bool no_rot = (fabsf(th) < eps) || (fabsf(th - PI_F) < eps);
    const float conj[4] = {qr[0], -qr[1], -qr[2], -qr[3]};
    const float qd2[4] = {2.0f * qd[0], 2.0f * qd[1], 2.0f * qd[2], 2.0f * qd[3]};
    float tt[4];
    q_mul(qd2, conj, tt);
    const float t[3] = {tt[1], tt[2], tt[3]};
    float dd;
    if (!no_rot) {
        const float s = sinf(th / 2.0f);
        l[0] = qr[1] / s; l[1] = qr[2] / s; l[2] = qr[3] / s;
        dd = 0.f;
    } else {
        dd = sqrtf((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
        const float dn = dd + 1e-10f;
        l[0] = t[0] / dn; l[1] = t[1] / dn; l[2] = t[2] / dn;
    }
    const float cs = (l[0] + l[1]) + l[2];
    if (!(cs >= 0.f)) { th = -th; l[0] = -l[0]; l[1] = -l[1]; l[2] = -l[2]; if (no_rot) dd = -dd; }
    if (!no_rot) dd = (t[0] * l[0] + t[1] * l[1]) + t[2] * l[2];
    // torch.isclose(d, 0): |d| <= 1e-8
    if (no_rot && fabsf(dd) <= 1e-8f) l[0] = 1.0f;
    if (no_rot) th = eps;
    const float tl[3] = {t[1] * l[2] - t[2] * l[1], t[2] * l[0] - t[0] * l[2], t[0] * l[1] - t[1] * l[0]};
    const float tn = tanf(th / 2.0f);
    const float u[3] = {tl[0] / tn, tl[1] / tn, tl[2] / tn};
    m[0] = 0.5f * (tl[0] + (l[1] * u[2] - l[2] * u[1]));
    m[1] = 0.5f * (tl[1] + (l[2] * u[0] - l[0] * u[2]));
    m[2] = 0.5f * (tl[2] + (l[0] * u[1] - l[1] * u[0]));
    theta = th;
    d = dd;
}

// sum of squares of (P * inv(G) - I) for two 3x4 rigid transforms (frobenius_cost; the 4th row contributes 0)
__device__ __forceinline__ float frob_cost(const float *Pm, const float *Gm) {
    // inv(G) = [G_R^T | -G_R^T g_t]
    float gi[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) gi[4 * i + j] = Gm[4 * j + i];
        gi[4 * i + 3] = (-Gm[i] * Gm[3] + -Gm[4 + i] * Gm[7]) + -Gm[8 + i] * Gm[11];
    }
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float e = ((Pm[4 * i] * gi[j] + Pm[4 * i + 1] * gi[4 + j]) + Pm[4 * i + 2] * gi[8 + j]) - (i == j ? 1.f : 0.f);
            acc += e * e;
        }
        const float e = ((Pm[4 * i] * gi[3] + Pm[4 * i + 1] * gi[7]) + Pm[4 * i + 2] * gi[11]) + Pm[4 * i + 3];
        acc += e * e;
    }
    return acc;
}
