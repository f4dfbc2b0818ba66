// reart_amd/csrc/infonce.hip -- the contrastive descriptor loss (PointInfoNCE) on the extractor's descriptors for gfx950:
// with s_ij = <f1_i, f2_j> / tau, row_loss_i = log sum_j exp(s_ij) - s_i,pos(i) over the live columns, its mean over the used
// rows, and the gradients for both descriptor sets.  The N1 x N2 matrix never exists: the logits are formed tile by tile on the
// fp32 matrix cores (v_mfma_f32_32x32x2_f32, plain fp32 as in gemm.hip) and consumed where they appear.
//
// One tile kernel, nce_tile_kernel<NB, MODE>, serves the three passes.  A workgroup keeps one STATIONARY tile of descriptors in
// LDS (32 per wave: 128 for C <= 128, 64 above) and streams the other set through LDS 32 descriptors at a time, in 16-byte
// loads where C is a multiple of 4.  The logit MFMA takes the streamed descriptors as its rows (A operand) and the stationary
// ones as its columns (B operand), so lane (x = lane % 32, h = lane / 32) ends up with the 16 logits of ITS stationary
// descriptor x against the streamed descriptors y = J(reg) + 4 h, J(reg) = reg % 4 + 8 (reg / 4): everything that belongs to
// one stationary descriptor is private to two lanes and the inner loop needs no exchange between lanes.
//   MODE 0  forward, rows stationary: per lane a running maximum, the sum of exp(s - maximum) rescaled when the maximum rises,
//           the lowest column attaining the maximum, and the positive's logit when it comes by.  The two lanes of a row meet
//           once, at the end.  The columns may be split over up to 16 workgroups (small B); nce_rows_kernel merges the
//           splits in ascending order, writes lse, row_loss and top, and a block's sum of row_loss in double
//           (reart_block_sum_d, common.h); nce_loss_kernel adds the blocks' sums in a fixed order: three launches.
//   MODE 1  dF1, rows stationary; MODE 2 dF2, columns stationary.  p'_ij = exp(s_ij - lse_i) - [j = pos(i)] is formed in the
//           accumulator registers, which ARE the A operand of the second product (row x, k = the streamed descriptor of this
//           lane's half), against the streamed tile that is already in LDS as B operand: out[x][c] += sum_y p'[x][y] F[y][c],
//           C / 32 accumulators per wave.  No scatter: the positive is inside p'.  The streamed set may be split over up to
//           8 workgroups, whose partial tiles nce_merge_kernel adds in ascending order: one or two launches per gradient.
// exp(a - b) is taken as expf(hi) (1 + lo) with hi + lo = a - b exactly (nce_exp_diff): no rounding of the argument, so a
// probability is off by the logits' error and 3 * 2^-24 relative, whatever the logits' magnitude.
// LDS rows are 32 NB + 1 floats (NB = accumulators per wave: 1, 2, 4, 8): an odd stride, the 32 descriptors of a fragment
// read on 32 distinct banks; columns from C up hold zeros, so any C <= 256 runs through whole K steps of 2.
// No floating-point atomics, no host synchronisation, no allocation, every output entry has one writer, every sum a fixed order.
#include "common.h"
#include <math.h>

#define NCE_MAX_C REART_MAX_D
#define NCE_MAX_N REART_NCE_MAX_N
#define NCE_MAX_B REART_NCE_MAX_B
#define NCE_TILE 32           // streamed descriptors per step
#define NCE_MAX_SPLIT_F 16    // workgroups sharing the columns of a row tile in the forward
#define NCE_MAX_SPLIT_B 8     // workgroups sharing the streamed set in a backward pass
#define NCE_FILL 512          // workgroups wanted before the streamed set is left unsplit
#define NCE_J(r) (((r) & 3) + 8 * ((r) >> 2))

typedef float nce_f16v __attribute__((ext_vector_type(16)));

static bool nce_shape_ok(int B, int N1, int N2, int C) {
    return B >= 0 && B <= NCE_MAX_B && N1 >= 0 && N1 <= NCE_MAX_N && N2 >= 0 && N2 <= NCE_MAX_N && C >= 1 && C <= NCE_MAX_C;
}
static int nce_nb(int C) { return C <= 32 ? 1 : (C <= 64 ? 2 : (C <= 128 ? 4 : 8)); }
static int nce_waves(int C) { return C <= 128 ? 4 : 2; }          // the stationary tile of C > 128 would not fit beside the streamed one
// streamed tiles per split, and the splits that leaves, for a stationary set of nx descriptors in B clouds
static void nce_split(int B, int nx, int ny, int C, int cap, int *tps, int *S) {
    const int tiles_x = reart_div_up(nx, 32 * nce_waves(C)) * B, ts = reart_div_up(ny, NCE_TILE);
    int s = tiles_x > 0 ? reart_div_up(NCE_FILL, tiles_x) : 1;
    s = s < cap ? s : cap;
    s = s < ts ? s : ts;
    s = s > 1 ? s : 1;
    *tps = ts > 0 ? reart_div_up(ts, s) : 1;
    *S = ts > 0 ? reart_div_up(ts, *tps) : 0;
}

// forward: the splits' (maximum, sum, argmax) [S][R], the positives' logits [R], the blocks' sums and counts; backward: the
// splits' partial gradients (only where a pass is split).  One size serves both calls.
struct NceWs { float *part_m, *part_s, *spos; int *part_arg; double *bsum; long long *bcnt; float *g1, *g2; };
static size_t nce_ws_layout(int B, int N1, int N2, int C, void *workspace, NceWs *w) {
    reart_arena ws(workspace);
    const size_t R = (size_t)B * N1;
    int tps, S;
    nce_split(B, N1, N2, C, NCE_MAX_SPLIT_F, &tps, &S);
    const size_t SR = (size_t)(S > 0 ? S : 1) * (R > 0 ? R : 1);
    w->part_m = ws.take<float>(SR);
    w->part_s = ws.take<float>(SR);
    w->part_arg = ws.take<int>(SR);
    w->spos = ws.take<float>(R > 0 ? R : 1);
    const size_t nblk = (R + 255) / 256;
    w->bsum = ws.take<double>(nblk > 0 ? nblk : 1);
    w->bcnt = ws.take<long long>(nblk > 0 ? nblk : 1);
    nce_split(B, N1, N2, C, NCE_MAX_SPLIT_B, &tps, &S);
    w->g1 = ws.take<float>(S > 1 ? (size_t)S * R * C : 1);
    nce_split(B, N2, N1, C, NCE_MAX_SPLIT_B, &tps, &S);
    w->g2 = ws.take<float>(S > 1 ? (size_t)S * B * N2 * C : 1);
    return ws.off;
}

// exp(a - b): the difference is exact in double, hi is its float and lo the rest (|lo| <= 2^-24 |hi|), e^(hi + lo) =
// e^hi (1 + lo) up to lo^2.  expf is within 1 ulp (2^-23 relative), the fmaf rounds once: 3 * 2^-24 relative in all.
__device__ __forceinline__ float nce_exp_diff(float a, float b) {
    const double d = (double)a - (double)b;
    const float hi = (float)d;
    const float lo = (float)(d - (double)hi);
    const float e = expf(hi);
    return fmaf(e, lo, e);
}

// (maximum, sum of exp(. - maximum), lowest index attaining the maximum) of two disjoint column sets, the first one's columns
// taking precedence on a tie only through their lower indices
__device__ __forceinline__ void nce_merge(float &m, float &s, int &arg, float m2, float s2, int arg2) {
    if (arg2 < 0) return;                       // the second set had no live column
    if (arg < 0) { m = m2; s = s2; arg = arg2; return; }
    if (m2 > m) {
        s = s * nce_exp_diff(m, m2) + s2;
        m = m2;
        arg = arg2;
    } else {
        if (m2 == m && arg2 < arg) arg = arg2;
        s = s + s2 * nce_exp_diff(m2, m);
    }
}

struct NceArgs {
    const float *xs, *ys;         // stationary [B,NX,C] and streamed [B,NY,C] descriptors
    int NX, NY, C, vec;           // vec: 16-byte loads are possible (C % 4 == 0, aligned bases)
    const int64_t *pos;           // [B,N1]
    const uint8_t *mask;          // [B,N2] or NULL
    const float *lse;             // [B,N1] (backward)
    int N1, N2;
    float inv_tau, tau;
    int tps;                      // streamed tiles per split
    float *part_m, *part_s, *spos; int *part_arg;      // forward
    float *out;                   // backward: the gradient (one split) or the splits' partial tiles [S][B,NX,C]
    int final;                    // backward: one split, `out` is the gradient and takes the scale
    const long long *count;
    const float *g;
};

// the positive of row i of cloud b, -1 where the row is not used: pos outside [0, N2) or a masked column
__device__ __forceinline__ int nce_positive(const NceArgs &a, int b, int i, bool with_mask) {
    if (i >= a.N1) return -1;
    const int64_t p = a.pos[(size_t)b * a.N1 + i];
    if (p < 0 || p >= (int64_t)a.N2) return -1;
    if (with_mask && a.mask && a.mask[(size_t)b * a.N2 + (size_t)p] == 0) return -1;
    return (int)p;
}
__device__ __forceinline__ bool nce_col_live(const NceArgs &a, int b, int j) {
    return j < a.N2 && (!a.mask || a.mask[(size_t)b * a.N2 + j] != 0);
}
// g / (count tau), 0 where no row is used (every p' is 0 then)
__device__ __forceinline__ float nce_scale(const float *g, const long long *count, float tau) {
    const long long c = *count;
    if (c <= 0) return 0.f;
    return (float)((double)(g ? *g : 1.f) / ((double)c * (double)tau));
}

// `rows` descriptors from row0 on into LDS rows of CP floats, zeros beyond the cloud's end and from column C up
template <int NB>
__device__ __forceinline__ void nce_stage(float *__restrict__ dst, const float *__restrict__ src, int row0, int rows, int N, int C,
                                          int vec, int tid, int nthreads) {
    constexpr int CP = 32 * NB + 1, Q = 8 * NB;
    for (int e = tid; e < rows * Q; e += nthreads) {
        const int r = e / Q, c = 4 * (e % Q), row = row0 + r;
        float4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < N && c < C) {
            const float *p = src + (size_t)row * C + c;
            if (vec) {
                v = *(const float4 *)p;
            } else {
                v.x = p[0];
                if (c + 1 < C) v.y = p[1];
                if (c + 2 < C) v.z = p[2];
                if (c + 3 < C) v.w = p[3];
            }
        }
        float *d = dst + r * CP + c;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
}

template <int NB, int MODE>
__global__ __launch_bounds__(256) void nce_tile_kernel(NceArgs a) {
    constexpr int CP = 32 * NB + 1;
    extern __shared__ __attribute__((aligned(16))) float nce_sm[];
    __shared__ float s_f[NCE_TILE];
    __shared__ int s_i[NCE_TILE];
    const int tid = threadIdx.x, nthreads = blockDim.x, lane = tid & 63, wv = tid >> 6, h = lane >> 5, lr = lane & 31;
    const int rows_wg = nthreads >> 1;                   // 32 per wave
    float *St = nce_sm, *Bt = nce_sm + rows_wg * CP;
    const int b = blockIdx.y, x0 = blockIdx.x * rows_wg, x = x0 + wv * 32 + lr;
    const float *xs = a.xs + (size_t)b * a.NX * a.C, *ys = a.ys + (size_t)b * a.NY * a.C;
    const int ck = (a.C + 1) & ~1;
    const int ts = (a.NY + NCE_TILE - 1) / NCE_TILE;
    const int t_lo = blockIdx.z * a.tps, t_hi = min(ts, t_lo + a.tps);
    nce_stage<NB>(St, xs, x0, rows_wg, a.NX, a.C, a.vec, tid, nthreads);
    // what this lane knows of its stationary descriptor
    int posx = -1;
    float lsex = 0.f;
    bool livex = false;
    if (MODE == 0) posx = nce_positive(a, b, x, false);
    if (MODE == 1) {
        posx = nce_positive(a, b, x, true);
        lsex = posx >= 0 ? a.lse[(size_t)b * a.N1 + x] : 0.f;
    }
    if (MODE == 2) livex = nce_col_live(a, b, x);
    float m = -INFINITY, ssum = 0.f, spos = 0.f;
    int arg = -1;
    bool seen = false;
    nce_f16v o[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[n][r] = 0.f;
    const float *sp = St + (wv * 32 + lr) * CP + h, *bp = Bt + lr * CP + h;
    for (int t = t_lo; t < t_hi; ++t) {
        const int y0 = t * NCE_TILE;
        __syncthreads();                                 // the previous tile has been read
        nce_stage<NB>(Bt, ys, y0, NCE_TILE, a.NY, a.C, a.vec, tid, nthreads);
        if (tid < NCE_TILE) {
            const int y = y0 + tid;
            if (MODE == 2) {
                const int p = nce_positive(a, b, y, true);
                s_i[tid] = p;
                s_f[tid] = p >= 0 ? a.lse[(size_t)b * a.N1 + y] : 0.f;
            } else {
                s_i[tid] = nce_col_live(a, b, y) ? 1 : 0;
            }
        }
        __syncthreads();
        nce_f16v acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int kk = 0; kk < ck; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bp[kk], sp[kk], acc, 0, 0, 0);
        if (MODE == 0) {
            float mn = m;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int yl = NCE_J(r) + 4 * h;
                const float v = acc[r] * a.inv_tau;
                acc[r] = v;
                if (y0 + yl == posx) { spos = v; seen = true; }
                if (s_i[yl] && (v > mn || arg < 0)) { mn = v; arg = y0 + yl; }
            }
            if (arg >= 0) {
                if (mn > m) {                            // the maximum rises: what has been summed is rescaled to it
                    ssum = m == -INFINITY ? 0.f : ssum * nce_exp_diff(m, mn);
                    m = mn;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (s_i[NCE_J(r) + 4 * h]) ssum += nce_exp_diff(acc[r], m);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int yl = NCE_J(r) + 4 * h;
                const float v = acc[r] * a.inv_tau;
                float p = 0.f;
                if (MODE == 1) {
                    if (posx >= 0 && s_i[yl]) p = nce_exp_diff(v, lsex) - (y0 + yl == posx ? 1.f : 0.f);
                } else {
                    const int py = s_i[yl];
                    if (livex && py >= 0) p = nce_exp_diff(v, s_f[yl]) - (x == py ? 1.f : 0.f);
                }
                acc[r] = p;
            }
            // out[x][c] += sum_y p'[x][y] F[y][c]: p' is the A operand as it stands (row x = lane % 32, k = this half's y)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float *fp = Bt + (NCE_J(r) + 4 * h) * CP + lr;
                float bv[NB];
#pragma unroll
                for (int n = 0; n < NB; ++n) bv[n] = fp[32 * n];
#pragma unroll
                for (int n = 0; n < NB; ++n) o[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[r], bv[n], o[n], 0, 0, 0);
            }
        }
    }
    if (MODE == 0) {
        // the row's two lanes meet: the lower half's columns first
        const float m2 = __shfl_xor(m, 32, 64), s2 = __shfl_xor(ssum, 32, 64);
        const int arg2 = __shfl_xor(arg, 32, 64);
        if (h == 0) {
            nce_merge(m, ssum, arg, m2, s2, arg2);
            if (x < a.N1) {
                const size_t at = ((size_t)blockIdx.z * gridDim.y + b) * a.N1 + x;
                a.part_m[at] = m;
                a.part_s[at] = ssum;
                a.part_arg[at] = arg;
            }
        }
        if (seen && x < a.N1) a.spos[(size_t)b * a.N1 + x] = spos;     // one lane of one split meets the positive
    } else {
        const float sc = a.final ? nce_scale(a.g, a.count, a.tau) : 1.f;
        float *out = a.out + ((size_t)blockIdx.z * gridDim.y + b) * a.NX * a.C;
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const int c = 32 * n + lr;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int xr = x0 + wv * 32 + NCE_J(r) + 4 * h;
                if (xr < a.NX && c < a.C) out[(size_t)xr * a.C + c] = a.final ? o[n][r] * sc : o[n][r];
            }
        }
    }
}

// a thread per row: the splits merged in ascending order, lse = maximum + log(sum) (in double, rounded once), row_loss, top
__global__ __launch_bounds__(256) void nce_rows_kernel(NceArgs a, int S, size_t R, float *__restrict__ row_loss, float *__restrict__ lse,
                                                       int64_t *__restrict__ top, double *__restrict__ bsum, long long *__restrict__ bcnt) {
    __shared__ double s_w[4], s_c[4];          // an array per sum: reart_block_sum_d has no barrier in front
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    float rl = 0.f;
    int used = 0;
    if (e < R) {
        const int b = (int)(e / a.N1), i = (int)(e % a.N1);
        const int p = nce_positive(a, b, i, true);
        float l = 0.f;
        int tp = -1;
        if (p >= 0) {
            float m = -INFINITY, s = 0.f;
            int arg = -1;
            for (int z = 0; z < S; ++z) nce_merge(m, s, arg, a.part_m[z * R + e], a.part_s[z * R + e], a.part_arg[z * R + e]);
            const double ld = (double)m + log((double)s);
            l = (float)ld;
            rl = (float)(ld - (double)a.spos[e]);
            tp = arg;
            used = 1;
        }
        row_loss[e] = rl;
        lse[e] = l;
        top[e] = tp;
    }
    const double tot = reart_block_sum_d<256>((double)rl, s_w);
    const double cnt = reart_block_sum_d<256>((double)used, s_c);
    if (threadIdx.x == 0) { bsum[blockIdx.x] = tot; bcnt[blockIdx.x] = (long long)cnt; }
}

// loss = (sum of the blocks' sums, 256 strided threads then the fixed tree) / count, rounded once; 0 where no row is used
__global__ __launch_bounds__(256) void nce_loss_kernel(const double *__restrict__ bsum, const long long *__restrict__ bcnt, size_t nblk,
                                                       float *__restrict__ loss, long long *__restrict__ count) {
    __shared__ double s_w[4], s_c[4];
    double v = 0.0, c = 0.0;
    for (size_t q = threadIdx.x; q < nblk; q += 256) { v += bsum[q]; c += (double)bcnt[q]; }
    const double tot = reart_block_sum_d<256>(v, s_w);
    const double cnt = reart_block_sum_d<256>(c, s_c);                // at most 2^26 rows: exact
    if (threadIdx.x == 0) {
        *count = (long long)cnt;
        *loss = cnt > 0.0 ? (float)(tot / cnt) : 0.f;
    }
}

// out[e] = scale * (part[0][e] + part[1][e] + ...), ascending
__global__ __launch_bounds__(256) void nce_merge_kernel(const float *__restrict__ part, int S, size_t total, const float *g,
                                                        const long long *count, float tau, float *__restrict__ out) {
    const float sc = nce_scale(g, count, tau);
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        float v = part[e];
        for (int z = 1; z < S; ++z) v += part[z * total + e];
        out[e] = v * sc;
    }
}

// ------------------------------------------------------------------------------------------------------------ host
template <int NB, int MODE>
static int nce_launch_nb(const NceArgs &a, int B, int S, hipStream_t st) {
    const int waves = nce_waves(a.C);
    const size_t lds = sizeof(float) * (size_t)(32 * waves + NCE_TILE) * (32 * NB + 1);
    if (lds > REART_LDS_DEFAULT_CAP &&
        hipFuncSetAttribute((const void *)nce_tile_kernel<NB, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return REART_ERR_LAUNCH;
    hipLaunchKernelGGL((nce_tile_kernel<NB, MODE>), dim3(reart_div_up(a.NX, 32 * waves), B, S), dim3(64 * waves), lds, st, a);
    return REART_OK;
}
template <int MODE>
static int nce_launch(const NceArgs &a, int B, int S, hipStream_t st) {
    switch (nce_nb(a.C)) {
        case 1: return nce_launch_nb<1, MODE>(a, B, S, st);
        case 2: return nce_launch_nb<2, MODE>(a, B, S, st);
        case 4: return nce_launch_nb<4, MODE>(a, B, S, st);
        default: return nce_launch_nb<8, MODE>(a, B, S, st);
    }
}
static int nce_vec(int C, const float *p, const float *q) { return (C & 3) == 0 && (((size_t)p | (size_t)q) & 15) == 0; }

extern "C" size_t reart_infonce_scratch_bytes(int B, int N1, int N2, int C) {
    NceWs w;
    return nce_shape_ok(B, N1, N2, C) ? nce_ws_layout(B, N1, N2, C, nullptr, &w) : 0;
}

extern "C" int reart_infonce_forward(const float *f1, const float *f2, const int64_t *pos, const uint8_t *col_mask, int B, int N1, int N2,
                                     int C, float tau, float *loss, float *row_loss, float *lse, int64_t *top, int64_t *count,
                                     void *workspace, size_t workspace_bytes, void *stream) {
    if (B < 0 || N1 < 0 || N2 < 0 || C < 1 || !(tau > 0.f) || !loss || !count) return REART_ERR_INVALID_ARG;
    if (!nce_shape_ok(B, N1, N2, C)) return REART_ERR_UNSUPPORTED;
    const size_t R = (size_t)B * N1;
    if (R > 0 && (!f1 || !pos || !row_loss || !lse || !top || (N2 > 0 && !f2))) return REART_ERR_INVALID_ARG;
    NceWs w;
    if (!workspace || workspace_bytes < nce_ws_layout(B, N1, N2, C, workspace, &w)) return REART_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    const size_t nblk = (R + 255) / 256;
    if (R > 0) {
        NceArgs a = {};
        a.xs = f1; a.ys = f2; a.NX = N1; a.NY = N2; a.C = C; a.vec = nce_vec(C, f1, f2);
        a.pos = pos; a.mask = col_mask; a.N1 = N1; a.N2 = N2; a.inv_tau = 1.0f / tau; a.tau = tau;
        a.part_m = w.part_m; a.part_s = w.part_s; a.part_arg = w.part_arg; a.spos = w.spos;
        int S;
        nce_split(B, N1, N2, C, NCE_MAX_SPLIT_F, &a.tps, &S);
        if (S > 0) {
            const int rc = nce_launch<0>(a, B, S, st);
            if (rc != REART_OK) return rc;
        }
        hipLaunchKernelGGL(nce_rows_kernel, dim3((unsigned)nblk), dim3(256), 0, st, a, S, R, row_loss, lse, top, w.bsum, w.bcnt);
    }
    hipLaunchKernelGGL(nce_loss_kernel, dim3(1), dim3(256), 0, st, w.bsum, w.bcnt, nblk, loss, (long long *)count);
    REART_CHECK_LAUNCH();
    return REART_OK;
}

// one gradient: the set `xs` stationary, `ys` streamed
template <int MODE>
static int nce_grad(NceArgs a, int B, float *part, float *out, hipStream_t st) {
    if ((size_t)B * a.NX == 0) return REART_OK;
    int S;
    nce_split(B, a.NX, a.NY, a.C, NCE_MAX_SPLIT_B, &a.tps, &S);
    a.final = S <= 1;
    a.out = a.final ? out : part;
    const int rc = nce_launch<MODE>(a, B, S > 1 ? S : 1, st);          // no streamed tile: one split writes the zeros
    if (rc != REART_OK) return rc;
    if (!a.final) {
        const size_t total = (size_t)B * a.NX * a.C;
        const size_t blocks = (total + 255) / 256;
        hipLaunchKernelGGL(nce_merge_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, part, S, total, a.g, a.count,
                           a.tau, out);
    }
    return REART_OK;
}

extern "C" int reart_infonce_backward(const float *f1, const float *f2, const int64_t *pos, const uint8_t *col_mask, const float *lse,
                                      const int64_t *count, const float *g, int B, int N1, int N2, int C, float tau, float *dF1,
                                      float *dF2, void *workspace, size_t workspace_bytes, void *stream) {
    if (B < 0 || N1 < 0 || N2 < 0 || C < 1 || !(tau > 0.f) || !count) return REART_ERR_INVALID_ARG;
    if (!nce_shape_ok(B, N1, N2, C)) return REART_ERR_UNSUPPORTED;
    if ((size_t)B * N1 > 0 && (!f1 || !pos || !lse)) return REART_ERR_INVALID_ARG;
    if ((size_t)B * N2 > 0 && !f2) return REART_ERR_INVALID_ARG;
    NceWs w;
    if (!workspace || workspace_bytes < nce_ws_layout(B, N1, N2, C, workspace, &w)) return REART_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    NceArgs a = {};
    a.C = C; a.vec = nce_vec(C, f1, f2); a.pos = pos; a.mask = col_mask; a.lse = lse; a.N1 = N1; a.N2 = N2;
    a.inv_tau = 1.0f / tau; a.tau = tau; a.count = (const long long *)count; a.g = g;
    if (dF1) {
        a.xs = f1; a.ys = f2; a.NX = N1; a.NY = N2;
        const int rc = nce_grad<1>(a, B, w.g1, dF1, st);
        if (rc != REART_OK) return rc;
    }
    if (dF2) {
        a.xs = f2; a.ys = f1; a.NX = N2; a.NY = N1;
        const int rc = nce_grad<2>(a, B, w.g2, dF2, st);
        if (rc != REART_OK) return rc;
    }
    REART_CHECK_LAUNCH();
    return REART_OK;
}
