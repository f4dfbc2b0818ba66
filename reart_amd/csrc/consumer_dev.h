// reart_amd/csrc/consumer_dev.h -- the device pieces that the fused step's consumers (step.hip) and the stand-alone operators
// (chamfer_loss.hip, flow_term.hip, flow.hip, kinpost.hip) promise to compute alike, bit for bit: one definition of each, so
// that a change to one path is a change to all.  The flow term's per-point expressions are in flow_dev.h.
#pragma once
#include "common.h"
#include "internal.h"
#include <math.h>

// float -> 64-bit fixed point with `sbits` fractional bits (0 <= sbits <= 39) by integer shifts of the mantissa (gfx950 has
// no f64 -> i64 convert; llrint() is a long emulation): truncates toward zero below 2^-sbits (deterministic, error < one
// quantum per addend), saturates instead of shifting a bit out
__device__ __forceinline__ long long reart_fixed_from_float(float v, int sbits) {
    const unsigned bits = __float_as_uint(v);
    const int ex = (int)((bits >> 23) & 0xffu);
    const long long mant = (long long)((bits & 0x7fffffu) | (ex ? 0x800000u : 0u));
    const int sh = (ex ? ex : 1) - 150 + sbits;
    const long long mag = sh >= 0 ? (sh < 40 ? (mant << sh) : 0x7fffffffffffffffll) : (sh > -64 ? (mant >> (-sh)) : 0ll);
    return (bits >> 31) ? -mag : mag;
}

// Fractional bits of the fixed-point sums of the Chamfer operators: at most Pmax <= 2^c addends, each of magnitude below
// 2^(e+1) where the bound m < 2^e, so |sum| * 2^bits < 2^(c + e + 1 + bits) <= 2^62: bits = clamp(61 - c - e, 0, 39).
// (m denormal: e = -126; m = INF: e = 129.)
__device__ __forceinline__ int reart_fx_bits(int Pmax, float m) {
    const int c = 32 - __clz(Pmax > 1 ? Pmax - 1 : 1);
    const int e = (int)((__float_as_uint(m) >> 23) & 0xffu) - 126;
    const int b = 61 - c - e;
    return b > 39 ? 39 : (b < 0 ? 0 : b);
}

// Sum of `total` partials left by other workgroups of the launch, by ONE wave in a fixed order: lane l adds the partials
// l, l + 64, ... in double, then the butterfly.  Agent-scope loads: the partials meet in L2 whichever XCD wrote them.
__device__ __forceinline__ double reart_partials_sum_d(const double *part, int total) {
    double t = 0.0;
    for (int e = threadIdx.x & 63; e < total; e += 64) t += __hip_atomic_load(&part[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return reart_wave_sum_d(t);
}

// frame f of complete_pred = cat(pc_trans[:cano_idx], cano, pc_trans[cano_idx:])   (run_robot.py:206); X: pc_trans [B,N,3]
__device__ __forceinline__ const float *reart_complete_frame(const float *X, const float *cano, int N, int cano_idx, int f) {
    return f < cano_idx ? X + (size_t)f * N * 3 : (f == cano_idx ? cano : X + (size_t)(f - 1) * N * 3);
}

// Exact rescan of three 8-target blocks of an SoA image (tx, ty, tz) for the three nearest targets of the query q by the full
// (distance, index) key.  bb[cb]: first target of block cb (8-aligned, two 16-byte loads per axis), or negative: no block;
// nv[cb]: its live targets (0 .. 8).  kd / ki: ascending; fewer than three live targets leave (+INF, 0x7fffffff).
__device__ __forceinline__ void reart_rescan3(const float (&q)[3], const float *tx, const float *ty, const float *tz,
                                              const int (&bb)[3], const int (&nv)[3], float (&kd)[3], int (&ki)[3]) {
    float4 X[3][2], Y[3][2], Z[3][2];
#pragma unroll
    for (int cb = 0; cb < 3; ++cb) {
        const int blk = bb[cb] < 0 ? 0 : bb[cb];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            X[cb][h] = *(const float4 *)(tx + blk + 4 * h);
            Y[cb][h] = *(const float4 *)(ty + blk + 4 * h);
            Z[cb][h] = *(const float4 *)(tz + blk + 4 * h);
        }
    }
    // all 18 loads are in flight before the first compare: left to itself the scheduler sinks the loads of a
    // block into the insert code of the block before it (fewer live registers), one exposed round trip per group
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 3; ++k) { kd[k] = INFINITY; ki[k] = 0x7fffffff; }
#pragma unroll
    for (int cb = 0; cb < 3; ++cb) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float4 vx = X[cb][u >> 2], vy = Y[cb][u >> 2], vz = Z[cb][u >> 2];
            const int c = u & 3;
            const float px = c == 0 ? vx.x : (c == 1 ? vx.y : (c == 2 ? vx.z : vx.w));
            const float py = c == 0 ? vy.x : (c == 1 ? vy.y : (c == 2 ? vy.z : vy.w));
            const float pz = c == 0 ? vz.x : (c == 1 ? vz.y : (c == 2 ? vz.z : vz.w));
            float d = reart_sqdist3(q[0], q[1], q[2], px, py, pz);
            if (u >= nv[cb]) d = INFINITY;
            reart_top3_insert(kd, ki, d, d < INFINITY ? bb[cb] + u : 0x7fffffff);
        }
    }
}
