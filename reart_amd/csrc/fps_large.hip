// reart_amd/csrc/fps_large.hip -- farthest point sampling for clouds above the LDS-resident kernel's 12 288 points
// (pointnet.hip), up to REART_FPS_MAX_N = 2^21 points (gfx950).  DESIGN.md "FPS, large clouds".
//
// One workgroup of 1024 threads per cloud, one barrier per round, as in fps_kernel.  Thread t owns the points
// k = t + u * 1024: the first FPSL_REG of them (16 384 points per cloud) keep coordinates and running minimum in
// registers, the rest re-read their coordinates from global memory every round (L2 / MALL resident) and keep their
// running minimum in the caller's `temp` [B,N], which this kernel initialises.  Only the owning thread touches a
// point's `temp` entry, so the buffer needs no synchronisation.
//
// Tie rules, carried in a 31-bit key (21-bit index):
//   CUDA rule (sampling_gpu.cu's tree arg-max over 1024 threads): lowest k % 1024, then lowest k -> (k & 1023) << 21 | k
//   CPU rule (torch.max(...)[1]): first maximum -> k
// Inside one thread k % 1024 is constant and k ascends with u, so a thread's strict-'>' scan in u order already yields
// its smallest key under both rules; the wave and the workgroup then reduce (value, key) pairs as fps_kernel does.
#include "common.h"
#include "internal.h"
#include <math.h>

#define FPSL_BS 1024                  // threads per cloud = opt_n_threads(N) for every N > 1024
#define FPSL_NW (FPSL_BS / 64)
#define FPSL_REG 16                   // points per thread held in registers
#define FPSL_KEY_BITS 21

template <int STEPS>
__device__ __forceinline__ int fpsl_max(int v) {
    v = max(v, reart_bfly<0>(v));
    v = max(v, reart_bfly<1>(v));
    v = max(v, reart_bfly<2>(v));
    v = max(v, reart_bfly<3>(v));
    if (STEPS > 4) v = max(v, reart_bfly<4>(v));
    if (STEPS > 5) v = max(v, reart_bfly<5>(v));
    return v;
}
template <int STEPS>
__device__ __forceinline__ int fpsl_min(int v) {
    v = min(v, reart_bfly<0>(v));
    v = min(v, reart_bfly<1>(v));
    v = min(v, reart_bfly<2>(v));
    v = min(v, reart_bfly<3>(v));
    if (STEPS > 4) v = min(v, reart_bfly<4>(v));
    if (STEPS > 5) v = min(v, reart_bfly<5>(v));
    return v;
}

template <bool CUDA_MODE>
__global__ __launch_bounds__(FPSL_BS) void fps_large_kernel(const float *__restrict__ xyz, int N, int M,
                                                            const int *__restrict__ start, float *__restrict__ temp,
                                                            int *__restrict__ idx32, int64_t *__restrict__ idx64) {
    __shared__ int s_v[2][FPSL_NW], s_k[2][FPSL_NW];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float *p = xyz + (size_t)b * N * 3;
    float *tm = temp + (size_t)b * N;
    f2 px[FPSL_REG / 2], py[FPSL_REG / 2], pz[FPSL_REG / 2], dm[FPSL_REG / 2];
#pragma unroll
    for (int u = 0; u < FPSL_REG; ++u) {
        const int k = tid + u * FPSL_BS;
        const bool ok = k < N;
        px[u >> 1][u & 1] = ok ? p[3 * k] : 0.f; py[u >> 1][u & 1] = ok ? p[3 * k + 1] : 0.f; pz[u >> 1][u & 1] = ok ? p[3 * k + 2] : 0.f;
        dm[u >> 1][u & 1] = ok ? 1e10f : -INFINITY;  // padding can never win the arg-max
    }
    const int k_stream = FPSL_REG * FPSL_BS + tid;   // this thread's first point kept in `temp`
    for (int k = k_stream; k < N; k += FPSL_BS) tm[k] = 1e10f;
    int far = start ? start[b] : 0;
    far = far < 0 ? 0 : (far < N ? far : N - 1);   // an out-of-range start must not read outside the cloud
    for (int it = 0; it < M; ++it) {
        if (tid == 0) {
            if (idx32) idx32[(size_t)b * M + it] = far;
            if (idx64) idx64[(size_t)b * M + it] = far;
        }
        if (it == M - 1) break;
        const float fx = p[3 * far], fy = p[3 * far + 1], fz = p[3 * far + 2];
        const f2 fx2 = {fx, fx}, fy2 = {fy, fy}, fz2 = {fz, fz};
        int bv = (int)0xff800000, bk = 0;                                  // -inf, index
#pragma unroll
        for (int u = 0; u < FPSL_REG / 2; ++u) {
            const f2 dx = px[u] - fx2, dy = py[u] - fy2, dz = pz[u] - fz2;
            const f2 d = (dx * dx + dy * dy) + dz * dz;                    // reart_sqdist3, two points at a time
            dm[u].x = d.x < dm[u].x ? d.x : dm[u].x;
            dm[u].y = d.y < dm[u].y ? d.y : dm[u].y;
            const int v0 = __float_as_int(dm[u].x), v1 = __float_as_int(dm[u].y);
            bk = v0 > bv ? tid + 2 * u * FPSL_BS : bk;
            bv = max(bv, v0);
            bk = v1 > bv ? tid + (2 * u + 1) * FPSL_BS : bk;
            bv = max(bv, v1);
        }
#pragma unroll 4
        for (int k = k_stream; k < N; k += FPSL_BS) {
            const float d = reart_sqdist3(p[3 * k], p[3 * k + 1], p[3 * k + 2], fx, fy, fz);
            float m = tm[k];
            m = d < m ? d : m;
            tm[k] = m;
            const int v = __float_as_int(m);
            bk = v > bv ? k : bk;
            bv = max(bv, v);
        }
        const int key = CUDA_MODE ? ((tid << FPSL_KEY_BITS) | bk) : bk;
        const int wmax = fpsl_max<6>(bv);
        const int wkey = fpsl_min<6>(bv == wmax ? key : 0x7fffffff);
        const int buf = it & 1;
        if (lane == 0) { s_v[buf][wv] = wmax; s_k[buf][wv] = wkey; }
        __syncthreads();
        const int v = s_v[buf][lane & (FPSL_NW - 1)];
        const int k = s_k[buf][lane & (FPSL_NW - 1)];
        const int gmax = fpsl_max<4>(v);
        far = __builtin_amdgcn_readfirstlane(fpsl_min<4>(v == gmax ? k : 0x7fffffff)) & ((1 << FPSL_KEY_BITS) - 1);
    }
}

extern "C" int reart_fps_temp(const float *xyz, int B, int N, int npoint, const int32_t *start, int cuda_mode,
                              float *temp, int32_t *idx32, int64_t *idx64, void *stream) {
    if (B < 0 || N < 1 || npoint < 0) return REART_ERR_INVALID_ARG;
    if (N > REART_FPS_MAX_N) return REART_ERR_UNSUPPORTED;
    if (N <= REART_FPS_MAX_N_LDS) return reart_fps(xyz, B, N, npoint, start, cuda_mode, idx32, idx64, stream);
    if (B == 0 || npoint == 0) return REART_OK;
    if (!xyz || !temp || (!idx32 && !idx64)) return REART_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (cuda_mode)
        hipLaunchKernelGGL(fps_large_kernel<true>, dim3(B), dim3(FPSL_BS), 0, st, xyz, N, npoint, start, temp, idx32, idx64);
    else
        hipLaunchKernelGGL(fps_large_kernel<false>, dim3(B), dim3(FPSL_BS), 0, st, xyz, N, npoint, start, temp, idx32, idx64);
    REART_CHECK_LAUNCH();
    return REART_OK;
}
