// reart_amd/csrc/pointnet_grad.hip -- first-order gradients of the PointNet++ front end: the backward of one fused layer
// (reart_mlp_layer, gemm.hip) with respect to its weight, bias and incoming features, and the backward of the 3-NN
// interpolation (reart_three_interpolate) with respect to the coarse level's features.  Coordinates get no gradient.
//
// Layer  A = relu?(X Wt + b),  Y = max over groups of pool_k rows of A (or A).  Given A (the un-pooled call's output) and dY:
//   pg_dz_kernel      dZ [rows, Cout]: dY routed to the selected rows -- without pooling every row, with pooling the LOWEST row
//                     of a group whose A equals the group's maximum (the pooled output is that maximum bit for bit, so equality
//                     is well defined) -- and, with ReLU, only where A > 0; exactly 0 everywhere else.  A copy or a zero: exact.
//   pg_dw_kernel      dWt = X^T dZ and dbias = 1^T dZ on v_mfma_f32_32x32x2_f32: the matrix-core M dimension is the input channel
//                     (channel Cin is a column of ones: its row of the product is dbias), N the output column, the reduction runs
//                     over the rows.  Both operands are read in their fragment layout straight from memory (32 consecutive
//                     channels / columns of one row per half wave), a gathered X element by element as the forward forms it
//                     (the same float32 Q - C); X is never materialised.  The rows are cut into chunks of
//                     REART_MLP_GRAD_ROW_CHUNK; one wave owns (chunk, 32 channels, 64 columns) and writes its tile to the
//                     workspace.
//   pg_reduce_kernel  adds the chunks' tiles in ascending chunk order: nothing depends on scheduling, no floating-point atomics.
//   dX = dZ Wt^T      is reart_mlp_layer on dZ with the transposed weight (pg_transpose_kernel), no bias, no ReLU.  For a gathered
//                     input only the FEATURE columns are computed (the weight rows of the xyz columns are left out of the
//                     transposed image), into the workspace; then
//   reart_invlist_kernel<256, 4, PgRecords> (invlist_dev.h, shared with connection_term.hip) builds, per cloud, the list of
//                     rows that name each point (the rows of a point in ascending order; indices outside [0, Npts) are left
//                     out), and
//   pg_scatter_kernel sums a point's rows in that order into dF.  A point no row names gets exactly 0.
// The interpolation backward uses the same lists over the (fine point, neighbour) pairs.
#include "common.h"
#include "internal.h"
#include "invlist_dev.h"
#include <math.h>

typedef float pg_f16v __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------------------------------
// inverse lists (invlist_dev.h): rec [B][Rb] (i64 point indices; one outside [0, Npts) takes no place), start [B][Npts + 1],
// list [B * Rb].  One workgroup per 256 points of a cloud; its four waves walk the cloud's records in four contiguous runs.
// ---------------------------------------------------------------------------------------------------------------------
#define PGI_TILE 256
#define PGI_WAVES 4

struct PgRecords {
    const int64_t *rec;
    int Rb, Npts;
    __device__ int count() const { return Rb; }
    __device__ int points() const { return Npts; }
    __device__ bool point(int b, int q, int &pt) const {
        const int64_t p = rec[(size_t)b * Rb + q];
        pt = (int)p;
        return p >= 0 && p < Npts;
    }
};

static void pgi_launch(const int64_t *rec, int B, int Rb, int Npts, int *start, int *list, hipStream_t st) {
    hipLaunchKernelGGL((reart_invlist_kernel<PGI_TILE, PGI_WAVES, PgRecords>), dim3(reart_div_up(Npts, PGI_TILE), B), dim3(PGI_WAVES * 64), 0, st,
                       PgRecords{rec, Rb, Npts}, start, list);
}

// ---------------------------------------------------------------------------------------------------------------------
// the layer backward
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pg_dz_kernel(const float *__restrict__ A, const float *__restrict__ dY, int lddy, int dycol0,
                                                    int rows, int Cout, int relu, int pool_k, float *__restrict__ dZ) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pool_k <= 1) {
        if (gid >= (size_t)rows * Cout) return;
        const size_t r = gid / Cout;
        const int c = (int)(gid - r * Cout);
        const float g = dY[r * lddy + dycol0 + c];
        dZ[gid] = (!relu || A[gid] > 0.f) ? g : 0.f;
        return;
    }
    const size_t groups = (size_t)(rows / pool_k);
    if (gid >= groups * Cout) return;
    const size_t grp = gid / Cout;
    const int c = (int)(gid - grp * Cout);
    const float *__restrict__ a = A + grp * pool_k * Cout + c;
    float m = a[0];
    int sel = 0;
    for (int j = 1; j < pool_k; ++j) {                     // strict: an equal later row never displaces
        const float v = a[(size_t)j * Cout];
        if (v > m) { m = v; sel = j; }
    }
    if (relu && !(m > 0.f)) sel = -1;                      // the group's maximum is the clamp: nothing is selected
    const float g = dY[grp * lddy + dycol0 + c];
    float *__restrict__ z = dZ + grp * pool_k * Cout + c;
    for (int j = 0; j < pool_k; ++j) z[(size_t)j * Cout] = j == sel ? g : 0.f;
}

struct PgDwArgs {
    const float *X; int ldx;
    const int64_t *idx; int K, S, Npts;
    const float *F; int D;
    const float *Q, *C;
    int xyz_first;
    int rows, Cin, Cout;
    const float *dZ;                  // [rows, Cout]
    float *part;                      // [chunks][Cin + 1][Cout]
    int kt0;                          // first 32-channel tile of this launch
};

// element (r, k) of the layer's operand with a column of ones behind it (k = Cin); exact zeros beyond
__device__ __forceinline__ float pg_load_x(const PgDwArgs &a, int r, int r_end, int k) {
    if (r >= r_end || k > a.Cin) return 0.f;
    if (k == a.Cin) return 1.f;
    if (!a.idx) return a.X[(size_t)r * a.ldx + k];
    const int64_t p = a.idx[r];
    if (p < 0 || p >= a.Npts) return 0.f;
    const size_t prow = (size_t)(r / (a.S * a.K)) * a.Npts + (size_t)p;
    const int kx = a.xyz_first ? k : k - a.D;
    if (kx >= 0 && kx < 3) {
        const float c = a.C ? a.C[(size_t)(r / a.K) * 3 + kx] : 0.f;
        return a.Q[prow * 3 + kx] - c;
    }
    return a.F[prow * a.D + (a.xyz_first ? k - 3 : k)];
}

#define PG_NBC 2                      // 32-column accumulators per wave
__global__ __launch_bounds__(64) void pg_dw_kernel(PgDwArgs a) {
    const int lane = threadIdx.x, half = lane >> 5, l32 = lane & 31;
    const int chunk = blockIdx.x, kt = a.kt0 + blockIdx.y, ct0 = blockIdx.z * PG_NBC;
    const int r_begin = chunk * REART_MLP_GRAD_ROW_CHUNK;
    const int r_end = min(a.rows, r_begin + REART_MLP_GRAD_ROW_CHUNK);
    const int k = kt * 32 + l32;
    pg_f16v acc[PG_NBC];
#pragma unroll
    for (int n = 0; n < PG_NBC; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[n][e] = 0.f;
    // A fragment: lane -> (channel k = lane % 32, row r0 + lane / 32); B fragment: lane -> (row r0 + lane / 32, column lane % 32)
    for (int r0 = r_begin; r0 < r_end; r0 += 2) {
        const int r = r0 + half;
        const float av = pg_load_x(a, r, r_end, k);
#pragma unroll
        for (int n = 0; n < PG_NBC; ++n) {
            const int c = (ct0 + n) * 32 + l32;
            const float bv = (r < r_end && c < a.Cout) ? a.dZ[(size_t)r * a.Cout + c] : 0.f;
            acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[n], 0, 0, 0);
        }
    }
    // C/D layout: row (channel) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), column = lane & 31
#pragma unroll
    for (int n = 0; n < PG_NBC; ++n) {
        const int c = (ct0 + n) * 32 + l32;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int kk = kt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * half;
            if (kk <= a.Cin && c < a.Cout) a.part[((size_t)chunk * (a.Cin + 1) + kk) * a.Cout + c] = acc[n][reg];
        }
    }
}

__global__ __launch_bounds__(256) void pg_reduce_kernel(const float *__restrict__ part, int chunks, int Cin, int Cout,
                                                        float *__restrict__ dWt, float *__restrict__ dbias) {
    const size_t tile = (size_t)(Cin + 1) * Cout;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= tile) return;
    const bool is_bias = e >= (size_t)Cin * Cout;
    if (is_bias ? !dbias : !dWt) return;                   // not wanted: its tiles were not computed either
    float s = part[e];
    for (int ch = 1; ch < chunks; ++ch) s += part[(size_t)ch * tile + e];      // ascending chunk order
    if (is_bias) dbias[e - (size_t)Cin * Cout] = s;
    else dWt[e] = s;
}

// WtT [Cout][n] = rows k0 .. k0 + n of Wt [Cin][Cout], transposed
__global__ __launch_bounds__(256) void pg_transpose_kernel(const float *__restrict__ Wt, int Cout, int k0, int n, float *__restrict__ WtT) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)Cout * n) return;
    const int c = (int)(e / n), k = (int)(e - (size_t)c * n);
    WtT[e] = Wt[(size_t)(k0 + k) * Cout + c];
}

// dF[gp][d] = sum of dXf[row][d] over the rows of point gp's list, in list order
__global__ __launch_bounds__(256) void pg_scatter_kernel(const float *__restrict__ dXf, int D, const int *__restrict__ start,
                                                         const int *__restrict__ list, int B, int Npts, float *__restrict__ dF) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)B * Npts * D) return;
    const size_t gp = e / D;
    const int d = (int)(e - gp * D);
    const int b = (int)(gp / Npts), p = (int)(gp - (size_t)b * Npts);
    const int lo = start[(size_t)b * (Npts + 1) + p], hi = start[(size_t)b * (Npts + 1) + p + 1];
    float s = 0.f;
    for (int i = lo; i < hi; ++i) s += dXf[(size_t)list[i] * D + d];
    dF[e] = s;
}

struct PgLayerWs { float *dZ, *part, *WtT, *dXf; int *start, *list; };
static size_t pg_layer_ws_layout(int rows, int Cin, int Cout, int B, int Npts, int D, void *workspace, PgLayerWs *w) {
    reart_arena ws(workspace);
    const size_t chunks = (size_t)reart_div_up(rows, REART_MLP_GRAD_ROW_CHUNK);
    w->dZ = ws.take<float>((size_t)rows * Cout);
    w->part = ws.take<float>(chunks * (Cin + 1) * Cout);
    w->WtT = ws.take<float>((size_t)Cout * Cin);
    w->dXf = ws.take<float>(B > 0 ? (size_t)rows * D : 0);
    w->start = ws.take<int>(B > 0 ? (size_t)B * (Npts + 1) : 0);
    w->list = ws.take<int>(B > 0 ? (size_t)rows : 0);
    return ws.off;
}

extern "C" size_t reart_mlp_layer_backward_scratch_bytes(int rows, int Cin, int Cout, int B, int Npts, int D) {
    PgLayerWs w;
    if (rows <= 0 || Cin < 1 || Cout < 1 || B < 0 || Npts < 0 || D < 0) return 0;
    return pg_layer_ws_layout(rows, Cin, Cout, B, Npts, D, nullptr, &w);
}

extern "C" int reart_mlp_layer_backward(const float *X, int ldx, const int64_t *gather_idx, int K, int S, int Npts,
                                        const float *F, int D, const float *Q, const float *C, int xyz_first,
                                        const float *Wt, int rows, int Cin, int Cout, int relu, int pool_k,
                                        const float *A, const float *dY, int lddy, int dycol0,
                                        float *dWt, float *dbias, float *dX, int lddx, float *dF,
                                        void *workspace, size_t workspace_bytes, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (rows < 0 || Cin < 1 || Cout < 1) return REART_ERR_INVALID_ARG;
    int B = 0;
    if (gather_idx) {
        if (!Q || K < 1 || S < 1 || Npts < 1 || D < 0 || (D > 0 && !F) || Cin != D + 3 || dX) return REART_ERR_INVALID_ARG;
        if (rows % ((long)S * K) != 0) return REART_ERR_INVALID_ARG;
        B = (int)(rows / ((long)S * K));
    } else if (!X || ldx < Cin || dF || (dX && lddx < Cin)) {
        return REART_ERR_INVALID_ARG;
    }
    if (pool_k < 0 || (pool_k && rows % pool_k != 0)) return REART_ERR_INVALID_ARG;
    if (pool_k == 1) pool_k = 0;
    if (gather_idx && D == 0) dF = nullptr;
    if (rows == 0) {                                        // empty sums
        if (dWt && hipMemsetAsync(dWt, 0, sizeof(float) * Cin * Cout, st) != hipSuccess) return REART_ERR_LAUNCH;
        if (dbias && hipMemsetAsync(dbias, 0, sizeof(float) * Cout, st) != hipSuccess) return REART_ERR_LAUNCH;
        return REART_OK;
    }
    if (!dWt && !dbias && !dX && !dF) return REART_OK;
    if (!Wt || !A || !dY || dycol0 < 0 || lddy < dycol0 + Cout || !workspace) return REART_ERR_INVALID_ARG;
    PgLayerWs w;
    if (workspace_bytes < pg_layer_ws_layout(rows, Cin, Cout, B, Npts, D, workspace, &w)) return REART_ERR_INVALID_ARG;

    const size_t nz = pool_k ? (size_t)(rows / pool_k) * Cout : (size_t)rows * Cout;
    hipLaunchKernelGGL(pg_dz_kernel, dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, st, A, dY, lddy, dycol0, rows, Cout, relu,
                       pool_k, w.dZ);
    REART_CHECK_LAUNCH();

    if (dWt || dbias) {
        PgDwArgs a = {};
        a.X = X; a.ldx = ldx; a.idx = gather_idx; a.K = K; a.S = S; a.Npts = Npts; a.F = F; a.D = D; a.Q = Q; a.C = C;
        a.xyz_first = xyz_first; a.rows = rows; a.Cin = Cin; a.Cout = Cout; a.dZ = w.dZ; a.part = w.part;
        const int chunks = reart_div_up(rows, REART_MLP_GRAD_ROW_CHUNK);
        // channel tiles: the weight's (0 .. Cin) and the one that holds the column of ones (Cin)
        a.kt0 = dWt ? 0 : Cin / 32;
        const int kt1 = dbias ? Cin / 32 + 1 : reart_div_up(Cin, 32);
        hipLaunchKernelGGL(pg_dw_kernel, dim3(chunks, kt1 - a.kt0, reart_div_up(Cout, 32 * PG_NBC)), dim3(64), 0, st, a);
        REART_CHECK_LAUNCH();
        const size_t tile = (size_t)(Cin + 1) * Cout;
        hipLaunchKernelGGL(pg_reduce_kernel, dim3((unsigned)((tile + 255) / 256)), dim3(256), 0, st, w.part, chunks, Cin, Cout, dWt, dbias);
        REART_CHECK_LAUNCH();
    }
    if (dX || dF) {
        const int k0 = gather_idx ? (xyz_first ? 3 : 0) : 0, n = gather_idx ? D : Cin;
        hipLaunchKernelGGL(pg_transpose_kernel, dim3((unsigned)(((size_t)Cout * n + 255) / 256)), dim3(256), 0, st, Wt, Cout, k0, n, w.WtT);
        REART_CHECK_LAUNCH();
        // dX = dZ Wt^T: a plain layer on dZ, no bias, no ReLU, no pooling
        const int rc = reart_mlp_layer(w.dZ, Cout, nullptr, 0, 0, 0, nullptr, 0, nullptr, nullptr, 0, w.WtT, nullptr, rows, Cout, n, 0, 0,
                                       gather_idx ? w.dXf : dX, gather_idx ? n : lddx, 0, stream);
        if (rc != REART_OK) return rc;
    }
    if (dF) {
        pgi_launch(gather_idx, B, S * K, Npts, w.start, w.list, st);
        REART_CHECK_LAUNCH();
        const size_t ne = (size_t)B * Npts * D;
        hipLaunchKernelGGL(pg_scatter_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, w.dXf, D, w.start, w.list, B, Npts, dF);
        REART_CHECK_LAUNCH();
    }
    return REART_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the interpolation backward
// ---------------------------------------------------------------------------------------------------------------------
// the forward's weights (interp3_kernel, gemm.hip): w_k = 1 / (d_k + 1e-8), normalised by (w_0 + w_1) + w_2, restated here
// because gemm.hip keeps its kernel to itself; tests/test_pointnet_grad_gpu.py holds the two to the same bits.
__global__ __launch_bounds__(256) void pg_interp_weight_kernel(const float *__restrict__ dist, size_t n, float *__restrict__ W) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    float w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = 1.0f / (dist[q * 3 + k] + 1e-8f);
    const float ws = (w[0] + w[1]) + w[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) W[q * 3 + k] = w[k] / ws;
}

// dP2[b][s][d] = sum over the pairs (n, j) of coarse point s, in list order, of w[b][n][j] * dOut[b N + n][col0 + d]
__global__ __launch_bounds__(256) void pg_interp_scatter_kernel(const float *__restrict__ dOut, int ldo, int col0, int D,
                                                                const float *__restrict__ W, const int *__restrict__ start,
                                                                const int *__restrict__ list, int B, int S2, float *__restrict__ dP2) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)B * S2 * D) return;
    const size_t gp = e / D;
    const int d = (int)(e - gp * D);
    const int b = (int)(gp / S2), s = (int)(gp - (size_t)b * S2);
    const int lo = start[(size_t)b * (S2 + 1) + s], hi = start[(size_t)b * (S2 + 1) + s + 1];
    float acc = 0.f;
    for (int i = lo; i < hi; ++i) {
        const int rec = list[i];                            // = (b N + n) * 3 + j
        acc += W[rec] * dOut[(size_t)(rec / 3) * ldo + col0 + d];
    }
    dP2[e] = acc;
}

struct PgInterpWs { float *dist; int64_t *idx; float *W; int *start, *list; };
static size_t pg_interp_ws_layout(int B, int N, int S2, void *workspace, PgInterpWs *w) {
    reart_arena ws(workspace);
    w->dist = ws.take<float>((size_t)B * N * 3);
    w->idx = ws.take<int64_t>((size_t)B * N * 3);
    w->W = ws.take<float>((size_t)B * N * 3);
    w->start = ws.take<int>((size_t)B * (S2 + 1));
    w->list = ws.take<int>((size_t)B * N * 3);
    return ws.off;
}

extern "C" size_t reart_three_interpolate_backward_scratch_bytes(int B, int N, int S2) {
    PgInterpWs w;
    return (B <= 0 || N <= 0 || S2 <= 0) ? 0 : pg_interp_ws_layout(B, N, S2, nullptr, &w);
}

extern "C" int reart_three_interpolate_backward(const float *xyz1, const float *xyz2, const float *dOut, int ldo, int col0,
                                                int B, int N, int S2, int D, float *dpoints2, float *weights,
                                                void *workspace, size_t workspace_bytes, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (B < 0 || N < 0 || S2 < 3 || D < 1 || col0 < 0 || ldo < col0 + D) return REART_ERR_INVALID_ARG;
    if (B == 0) return REART_OK;
    if (!dpoints2) return REART_ERR_INVALID_ARG;
    if (N == 0) {
        if (hipMemsetAsync(dpoints2, 0, sizeof(float) * B * S2 * D, st) != hipSuccess) return REART_ERR_LAUNCH;
        return REART_OK;
    }
    if ((long)B * N * 3 > 0x7fffffffL) return REART_ERR_UNSUPPORTED;
    if (!xyz1 || !xyz2 || !dOut || !workspace) return REART_ERR_INVALID_ARG;
    PgInterpWs w;
    if (workspace_bytes < pg_interp_ws_layout(B, N, S2, workspace, &w)) return REART_ERR_INVALID_ARG;
    const int rc = reart_three_nn(xyz1, xyz2, B, N, S2, w.dist, w.idx, stream);
    if (rc != REART_OK) return rc;
    float *W = weights ? weights : w.W;
    const size_t nq = (size_t)B * N;
    hipLaunchKernelGGL(pg_interp_weight_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, w.dist, nq, W);
    REART_CHECK_LAUNCH();
    pgi_launch(w.idx, B, 3 * N, S2, w.start, w.list, st);
    REART_CHECK_LAUNCH();
    const size_t ne = (size_t)B * S2 * D;
    hipLaunchKernelGGL(pg_interp_scatter_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, dOut, ldo, col0, D, W, w.start,
                       w.list, B, S2, dpoints2);
    REART_CHECK_LAUNCH();
    return REART_OK;
}
