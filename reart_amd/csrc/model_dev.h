// reart_amd/csrc/model_dev.h -- device helpers and layout constants shared by the relaxation-model kernels
// (model.hip: pose table in LDS; model_long.hip: pose table too long for LDS).  Not part of the C ABI.
#pragma once
#include "common.h"
#include "internal.h"
#include <math.h>

#define RED_CHUNK 64    // points per partial-reduction chunk

__device__ __forceinline__ float dot3f(const float *a, const float *b) {
    return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0]));
}
__device__ __forceinline__ void cross3f(const float *a, const float *b, float *c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ float norm3f(const float *a) {
    return sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
}

// screw_se3/geo_utils.py:632-651 (rows b1,b2,b3); same operation order as oracle/model.c
__device__ __forceinline__ void r6d_to_matrix(const float *d6, float *R) {
    const float *a1 = d6, *a2 = d6 + 3;
    const float n1 = fmaxf(norm3f(a1), 1e-12f);
    float b1[3] = {a1[0] / n1, a1[1] / n1, a1[2] / n1};
    const float d = (b1[0] * a2[0] + b1[1] * a2[1]) + b1[2] * a2[2];
    float u[3] = {a2[0] - d * b1[0], a2[1] - d * b1[1], a2[2] - d * b1[2]};
    const float n2 = fmaxf(norm3f(u), 1e-12f);
    float b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
    float b3[3];
    cross3f(b1, b2, b3);
#pragma unroll
    for (int c = 0; c < 3; ++c) { R[c] = b1[c]; R[3 + c] = b2[c]; R[6 + c] = b3[c]; }
}

__device__ __forceinline__ void r6d_backward(const float *d6, const float *gR, float *g6) {
    const float *a1 = d6, *a2 = d6 + 3;
    const float n1r = norm3f(a1), n1 = fmaxf(n1r, 1e-12f);
    float b1[3] = {a1[0] / n1, a1[1] / n1, a1[2] / n1};
    const float d = (b1[0] * a2[0] + b1[1] * a2[1]) + b1[2] * a2[2];
    float u[3] = {a2[0] - d * b1[0], a2[1] - d * b1[1], a2[2] - d * b1[2]};
    const float n2r = norm3f(u), n2 = fmaxf(n2r, 1e-12f);
    float b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
    float gb1[3] = {gR[0], gR[1], gR[2]}, gb2[3] = {gR[3], gR[4], gR[5]};
    const float gb3[3] = {gR[6], gR[7], gR[8]};
    float t[3];
    cross3f(b2, gb3, t);
    gb1[0] += t[0]; gb1[1] += t[1]; gb1[2] += t[2];
    cross3f(gb3, b1, t);
    gb2[0] += t[0]; gb2[1] += t[1]; gb2[2] += t[2];
    float gu[3];
    if (n2r > 1e-12f) {
        const float s = dot3f(b2, gb2);
#pragma unroll
        for (int c = 0; c < 3; ++c) gu[c] = (gb2[c] - b2[c] * s) / n2;
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) gu[c] = gb2[c] / n2;
    }
    float ga2[3] = {gu[0], gu[1], gu[2]};
    const float gd = -dot3f(gu, b1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gb1[c] += -d * gu[c] + gd * a2[c];
        ga2[c] += gd * b1[c];
    }
    if (n1r > 1e-12f) {
        const float s = dot3f(b1, gb1);
#pragma unroll
        for (int c = 0; c < 3; ++c) g6[c] = (gb1[c] - b1[c] * s) / n1;
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) g6[c] = gb1[c] / n1;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) g6[3 + c] = ga2[c];
}

// v = R x + t with R row-major 3x3 (fmaf chain in ascending column order)
__device__ __forceinline__ void apply_rt(const float *Rt /*[12]: R(9) t(3)*/, float x0, float x1,
                                         float x2, float *v) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float acc = x0 * Rt[3 * c];
        acc = fmaf(x1, Rt[3 * c + 1], acc);
        acc = fmaf(x2, Rt[3 * c + 2], acc);
        v[c] = acc + Rt[9 + c];
    }
}

// Hidden unit of the seg head (networks/blocks.py:99-118): relu(W1[j] . x + b1[j]) with wb = (W1[j][0..2], b1[j]) -- the
// ascending-c fmaf chain of oracle/model.c, then the bias, then the relu.  The ONE definition: the forward evaluates it, and
// the backward re-evaluates it from the same operands where no hT was saved, so both hold the same bits.
__device__ __forceinline__ float hidden_unit(const float4 wb, float x0, float x1, float x2) {
    float acc = wb.x * x0;
    acc = fmaf(wb.y, x1, acc);
    acc = fmaf(wb.z, x2, acc);
    acc = acc + wb.w;
    return acc > 0.f ? acc : 0.f;
}

// Philox4x32-10 counter-based generator (Salmon et al. 2011) for the in-kernel Gumbel noise
__device__ __forceinline__ void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                           uint32_t k0, uint32_t k1, uint32_t *out) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// -log(Exp(1)) sample: u in (0,1) -> e = -log u -> g = -log e   (F.gumbel_softmax recipe).
// 23 random bits + 0.5: every value (k + 0.5) * 2^-23 is exactly representable, so u never
// rounds to 1.0 (which would give e = 0, g = +inf and a NaN softmax once in 2^24 draws).
__device__ __forceinline__ float gumbel_from_bits(uint32_t bits) {
    const float u = ((float)(bits >> 9) + 0.5f) * (1.0f / 8388608.0f);
    return -logf(-logf(u));
}

// forward: points per workgroup (64, or 32 with half waves on different part pairs), parts per wave slice
#define FW_PTS 64
#define FW_PG 2

// layout of one partial row / of the reduced gradient vector
__host__ __device__ static inline int off_gW2() { return 0; }
__host__ __device__ static inline int off_gW1(int P, int H) { return P * H; }
__host__ __device__ static inline int off_gb1(int P, int H) { return P * H + 3 * H; }
__host__ __device__ static inline int off_gRt(int P, int H) { return P * H + 4 * H; }
__host__ __device__ static inline int n_out(int P, int H, int B) { return P * H + 4 * H + 12 * B * P; }

// backward: row stride of the 64-point LDS tiles, waves per workgroup and their split by role (model.hip, backward)
#define BW_LD (RED_CHUNK + 1)
#define BW_WAVES 16                       // block size of every instance: the launch bound, the kernel's strides, the launcher
#define BW_HID (BW_WAVES / 4)             // waves of the hidden-gradient role: dp, then gW1 / gb1 (4 row tiles at H = 128)
#define BW_MFMA (BW_WAVES - BW_HID)       // waves of the gR|gt / gW2 role (12 tiles at B = 19, H = 128)

// the 152 KiB of dynamic LDS a model kernel may ask for (160 KiB per CU on gfx950)
#define REART_MODEL_LDS_CAP ((size_t)152 * 1024)
