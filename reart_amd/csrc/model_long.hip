// reart_amd/csrc/model_long.hip -- the relaxation model for sequences whose pose table does not fit in LDS.
//
// model.hip keeps the whole table [B*P][12] of [R|t] rows in LDS (the backward also the whole upstream-gradient tile
// [B][64*3]); at P = 20, H = 128 that holds B <= 90 frames in the forward and B <= 58 in the backward.  The kernels here
// serve what lies beyond, up to B = REART_MAX_POSE_LEN, and nothing else: reart_base_path (model.hip) sends a shape here
// only when the in-LDS kernel does not fit (or reart_relax_config.tune_long asks for it).
//
//   forward:  a lane needs only the 12 floats of (t, k_n) of its own hard part k_n, so there is no table in LDS at all:
//             pose_table_kernel builds [R|t] once per iteration (the in-LDS forward rebuilds all of it in every
//             workgroup) and the lanes read their rows from global memory (983 KB at B = 1024, P = 20: L2-resident).
//             Everything in front of the rigid apply is base_fwd_kernel's code and operation order, so every output is
//             bit-identical to the in-LDS forward's.
//   backward: one workgroup per chunk of points like base_bwd_block_kernel, walking the frames in tiles of BT <= 32
//             frames: s_G [BT][64*3] and s_rt [BT*P][12].  Per tile, in one pass: the tile's frames are appended to the
//             dw = sum_t G[t].(R[t] x + t[t]) chains (accumulators stay in registers across tiles, ascending t: the
//             in-LDS order), and the tile's own gR|gt partials, which depend on nothing but G, x and the hard part, are
//             written.  After the last tile: softmax backward, gW2, dp, gW1 / gb1 as in the in-LDS kernel.  The partial
//             row layout n_out(P, H, B) is the same, so base_bwd_finalize_kernel is reused unchanged
//             (like the in-LDS block kernel, this one promotes the Adam step sizes that launch reads).
//             The next tile's global loads are issued before the current tile is consumed (one round trip deep, like the
//             prologue).  No atomics; every sum in a fixed order; reruns are bit-identical.
#include "common.h"
#include "internal.h"
#include "model_dev.h"
#include <math.h>

// ------------------------------------------------------------------------------- pose table
// [R|t] rows [n][12] and / or the homogeneous matrices [n][4][4] of n = B*P poses
__global__ __launch_bounds__(256) void pose_table_kernel(const float *__restrict__ p6d, const float *__restrict__ pt, int n,
                                                         float *__restrict__ table, float *__restrict__ trans_list) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float R[9], tv[3];
    r6d_to_matrix(p6d + 6 * (size_t)e, R);
#pragma unroll
    for (int c = 0; c < 3; ++c) tv[c] = pt[3 * (size_t)e + c];
    if (table) {
#pragma unroll
        for (int c = 0; c < 9; ++c) table[12 * (size_t)e + c] = R[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) table[12 * (size_t)e + 9 + c] = tv[c];
    }
    if (trans_list) {
        float *T = trans_list + 16 * (size_t)e;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) T[4 * r + c] = R[3 * r + c];
            T[4 * r + 3] = tv[r];
        }
        T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
    }
}

// ------------------------------------------------------------------------------- forward
// base_fwd_kernel (model.hip) without the table in LDS: same workgroup shape (W waves x the same 64 points, or half
// waves on different part pairs x 32 points), same code up to the rigid apply.  The apply of frame t is done by slice
// t mod NS as there; the row of (t, k_n) comes from a.rt_table, or, where the caller has no table (reart_base_forward),
// from the lane's own Gram-Schmidt of that pose: r6d_to_matrix is the same function either way.
#define FWL_TU 4     // frames per batch of the apply loop: their rows are in flight together

template <int PP, bool HALF, bool BATCH>
__global__ __launch_bounds__(64 * (HALF ? (((PP > 0 ? PP : 32) + 2 * FW_PG - 1) / (2 * FW_PG)) : (((PP > 0 ? PP : 32) + FW_PG - 1) / FW_PG)))
void base_fwd_long_kernel(Batched<BaseFwdArgs> ab) {
    const BaseFwdArgs &a = ab.a[BATCH ? blockIdx.y : 0];
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int PMAX = (PP > 0) ? PP : 32;
    constexpr int W = HALF ? (PMAX + 2 * FW_PG - 1) / (2 * FW_PG) : (PMAX + FW_PG - 1) / FW_PG;   // waves
    constexpr int NS = HALF ? 2 * W : W;                  // part-pair slices (one per wave, or per half wave)
    constexpr int PTS = HALF ? FW_PTS / 2 : FW_PTS;       // points per workgroup
    constexpr int BS = 64 * W;
    float *s_wb = smem;                                   // [H][4]  W1 row | b1
    float *s_w2T = s_wb + 4 * (size_t)a.H;                // [W][H][2]  W2 of wave g's two parts, j-major
    float *s_a = s_w2T + (size_t)a.H * PMAX;              // [PMAX][PTS]  logits, later y
    float *s_e = s_a + PMAX * PTS;                        // [PMAX][PTS]  z, later exp(z - max)
    float *s_hh = s_e + PMAX * PTS;                       // [PTS][H + 4]  hidden activations, point-major
    const int HS = a.H + 4;
    const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;
    const int pl = HALF ? (lane & 31) : lane;             // point of this lane inside the workgroup
    const int sid = HALF ? 2 * grp + (lane >> 5) : grp;   // part-pair slice of this lane
    const int P = (PP > 0) ? PP : a.P;
    // prologue: every group's first batch of loads is issued before anything is stored to LDS
    {
        float vw[PMAX];
        const int ew = tid < 4 * a.H ? tid : 0;
        const float wbv = (ew & 3) < 3 ? a.W1[3 * (ew >> 2) + (ew & 3)] : a.b1[ew >> 2];
        const int jw = tid < a.H ? tid : 0;
#pragma unroll
        for (int p = 0; p < PMAX; ++p) vw[p] = a.W2[(size_t)(p < P ? p : 0) * a.H + jw];
        if (tid < 4 * a.H) s_wb[tid] = wbv;
        if (tid < a.H) {
#pragma unroll
            for (int p = 0; p < PMAX; ++p) s_w2T[((p >> 1) * a.H + tid) * 2 + (p & 1)] = p < P ? vw[p] : 0.f;
        }
    }
    for (int e = tid + BS; e < 4 * a.H; e += BS) {
        const int j = e >> 2, c = e & 3;
        s_wb[e] = c < 3 ? a.W1[3 * j + c] : a.b1[j];
    }
    for (int j = tid + BS; j < a.H; j += BS)
        for (int p = 0; p < PMAX; ++p) s_w2T[((p >> 1) * a.H + j) * 2 + (p & 1)] = p < P ? a.W2[(size_t)p * a.H + j] : 0.f;

    const int n = blockIdx.x * PTS + pl;
    const bool live = n < a.N;
    const int nc = live ? n : a.N - 1;
    const float x0 = a.cano[3 * (size_t)nc], x1 = a.cano[3 * (size_t)nc + 1], x2 = a.cano[3 * (size_t)nc + 2];
    const int p0 = sid * FW_PG;
    const bool has1 = p0 + 1 < P;
    const float tau = a.tau_ptr ? a.tau_ptr[0] : a.tau;
    float g0, g1 = 0.f;
    if (a.gumbel) {
        g0 = a.gumbel[(size_t)nc * P + (p0 < P ? p0 : 0)];
        if (has1) g1 = a.gumbel[(size_t)nc * P + p0 + 1];
    } else {
        const uint64_t it = a.iter_ptr ? (uint64_t)a.iter_ptr[0] : 0ull;
        uint32_t r[4];
        philox4x32((uint32_t)n, (uint32_t)(p0 >> 2), (uint32_t)it, (uint32_t)(it >> 32), (uint32_t)a.seed,
                   (uint32_t)(a.seed >> 32), r);
        g0 = gumbel_from_bits(r[p0 & 3]);
        g1 = gumbel_from_bits(r[(p0 & 3) + 1]);   // p0 is even: p0 & 3 in {0, 2}
    }
    __syncthreads();
    // hidden layer once per point: slice sid evaluates its share of the H units
    {
        const int jq = (a.H + NS - 1) / NS, j0 = sid * jq, j1 = (j0 + jq < a.H) ? j0 + jq : a.H;
        for (int j = j0; j < j1; ++j) {
            const float4 wb = *(const float4 *)(s_wb + 4 * j);
            float acc = wb.x * x0;
            acc = fmaf(wb.y, x1, acc);
            acc = fmaf(wb.z, x2, acc);
            acc = acc + wb.w;
            const float h = acc > 0.f ? acc : 0.f;
            s_hh[pl * HS + j] = h;
            if (a.hT && live) a.hT[(size_t)j * a.N + n] = h;
        }
    }
    __syncthreads();
    // logits of this slice's two parts: the full ascending-j fmaf chain (the oracle's rounding order)
    float sp0 = 0.f, sp1 = 0.f;
    {
        const float *hrow = s_hh + pl * HS, *wrow = s_w2T + (size_t)(sid < PMAX / 2 ? sid : PMAX / 2 - 1) * a.H * 2;
        int j = 0;
        const int H4 = (a.H & 3) == 0 ? a.H : 0;   // rows are 16-byte aligned only when H is a multiple of 4
#pragma unroll 2
        for (; j + 4 <= H4; j += 4) {
            const float4 h4 = *(const float4 *)(hrow + j);
            const float4 wa = *(const float4 *)(wrow + 2 * j), wb2 = *(const float4 *)(wrow + 2 * j + 4);
            sp0 = fmaf(wa.x, h4.x, sp0); sp1 = fmaf(wa.y, h4.x, sp1);
            sp0 = fmaf(wa.z, h4.y, sp0); sp1 = fmaf(wa.w, h4.y, sp1);
            sp0 = fmaf(wb2.x, h4.z, sp0); sp1 = fmaf(wb2.y, h4.z, sp1);
            sp0 = fmaf(wb2.z, h4.w, sp0); sp1 = fmaf(wb2.w, h4.w, sp1);
        }
        for (; j < a.H; ++j) {
            const float h = hrow[j];
            sp0 = fmaf(wrow[2 * j], h, sp0);
            sp1 = fmaf(wrow[2 * j + 1], h, sp1);
        }
    }
    const float z0 = (sp0 + g0) / tau, z1 = has1 ? (sp1 + g1) / tau : -INFINITY;
    if (p0 < P) { s_a[p0 * PTS + pl] = sp0; s_e[p0 * PTS + pl] = z0; }
    if (has1) { s_a[(p0 + 1) * PTS + pl] = sp1; s_e[(p0 + 1) * PTS + pl] = z1; }
    __syncthreads();
    // noise-free arg-max (networks/model.py:70, first maximum) and the softmax max
    float m = -INFINITY;
    int am = 0;
    float sm = -INFINITY;
#pragma unroll
    for (int p = 0; p < PMAX; ++p)
        if (PP > 0 || p < P) {
            m = fmaxf(m, s_e[p * PTS + pl]);
            if (sid == 0) {
                const float sv = s_a[p * PTS + pl];
                if (sv > sm) { sm = sv; am = p; }
            }
        }
    __syncthreads();
    const float e0 = expf(z0 - m), e1 = has1 ? expf(z1 - m) : 0.f;
    if (p0 < P) s_e[p0 * PTS + pl] = e0;
    if (has1) s_e[(p0 + 1) * PTS + pl] = e1;
    __syncthreads();
    float sum = 0.f;
#pragma unroll
    for (int p = 0; p < PMAX; ++p)
        if (PP > 0 || p < P) sum += s_e[p * PTS + pl];   // ascending part order
    const float y0 = e0 / sum, y1 = e1 / sum;
    if (p0 < P) { s_a[p0 * PTS + pl] = y0; if (a.yT && live) a.yT[(size_t)p0 * a.N + n] = y0; }
    if (has1) { s_a[(p0 + 1) * PTS + pl] = y1; if (a.yT && live) a.yT[(size_t)(p0 + 1) * a.N + n] = y1; }
    __syncthreads();
    int k = 0;
    float yk = -1.f;
#pragma unroll
    for (int p = 0; p < PMAX; ++p)
        if (PP > 0 || p < P) {
            const float yv = s_a[p * PTS + pl];
            if (yv > yk) { yk = yv; k = p; }
        }
    const float w = (1.0f - yk) + yk;  // y_hard - y_soft.detach() + y_soft
    if (live && sid == 0) {
        if (a.seg_part) a.seg_part[n] = am;
        if (a.hard_idx) a.hard_idx[n] = k;
    }
    // rigid apply: FWL_TU frames of this slice per batch, their rows loaded first
    const float *tab = a.rt_table;
    for (int t0 = sid; t0 < a.B; t0 += FWL_TU * NS) {
        float rt[FWL_TU][12];
#pragma unroll
        for (int u = 0; u < FWL_TU; ++u) {
            const int t = t0 + u * NS < a.B ? t0 + u * NS : a.B - 1;
            const size_t e = (size_t)t * a.P + k;
            if (tab) {   // uniform.  Rows are 48 bytes and the table 256-byte aligned: three 16-byte loads
                const float4 *row = (const float4 *)(tab + 12 * e);
                const float4 r0 = row[0], r1 = row[1], r2 = row[2];
                rt[u][0] = r0.x; rt[u][1] = r0.y; rt[u][2] = r0.z; rt[u][3] = r0.w;
                rt[u][4] = r1.x; rt[u][5] = r1.y; rt[u][6] = r1.z; rt[u][7] = r1.w;
                rt[u][8] = r2.x; rt[u][9] = r2.y; rt[u][10] = r2.z; rt[u][11] = r2.w;
            } else {
                r6d_to_matrix(a.p6d + 6 * e, rt[u]);
#pragma unroll
                for (int c = 0; c < 3; ++c) rt[u][9 + c] = a.pt[3 * e + c];
            }
        }
#pragma unroll
        for (int u = 0; u < FWL_TU; ++u) {
            const int t = t0 + u * NS;
            if (t < a.B) {   // uniform per slice (a half wave when HALF: the DPP rows below lie inside one)
                float v[3];
                apply_rt(rt[u], x0, x1, x2, v);
                v[0] = w * v[0]; v[1] = w * v[1]; v[2] = w * v[2];
                if (live) {
                    float *o = a.out + 3 * ((size_t)t * a.N + n);
                    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
                }
                if (a.out_soa && n < a.Npad) {
                    float *o = a.out_soa + (size_t)t * 3 * a.Npad;
                    o[n] = live ? v[0] : INFINITY;
                    o[a.Npad + n] = live ? v[1] : INFINITY;
                    o[2 * (size_t)a.Npad + n] = live ? v[2] : INFINITY;
                }
                if (a.boxes && blockIdx.x * PTS < a.Npad) {
                    // AABBs of this workgroup's output points of frame t, one per NN_BOX consecutive points
                    float lo[3], hi[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        static_assert(NN_BOX == 16, "a box is one DPP row");
                        lo[c] = reart_row16_min(live ? v[c] : INFINITY);
                        hi[c] = reart_row16_max(live ? v[c] : -INFINITY);
                        if (hi[c] == -INFINITY) hi[c] = INFINITY;
                    }
                    const int pos = blockIdx.x * PTS + pl;
                    if ((pl & (NN_BOX - 1)) == 0 && pos < a.Npad) {
                        float *o = a.boxes + ((size_t)t * (a.Npad / NN_BOX) + pos / NN_BOX) * 8;
                        o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = hi[0]; o[4] = hi[1]; o[5] = hi[2];
                    }
                }
            }
        }
    }
}

template <int PP, bool HALF>
static int launch_fwd_long_t(const BaseFwdArgs *ak, int K, hipStream_t st) {
    const BaseFwdArgs &a = ak[0];
    constexpr int PMAX = (PP > 0) ? PP : 32;
    constexpr int W = HALF ? (PMAX + 2 * FW_PG - 1) / (2 * FW_PG) : (PMAX + FW_PG - 1) / FW_PG;
    constexpr int PTS = HALF ? FW_PTS / 2 : FW_PTS;
    const int cover = a.out_soa ? (a.Npad > a.N ? a.Npad : a.N) : a.N;
    const size_t lds = sizeof(float) * ((size_t)a.H * (4 + PMAX) + 2 * (size_t)PTS * PMAX + (size_t)(a.H + 4) * PTS);
    if (lds > REART_MODEL_LDS_CAP) return REART_ERR_UNSUPPORTED;
    if (lds > REART_LDS_DEFAULT_CAP &&
        (hipFuncSetAttribute((const void *)base_fwd_long_kernel<PP, HALF, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)REART_MODEL_LDS_CAP) != hipSuccess ||
         hipFuncSetAttribute((const void *)base_fwd_long_kernel<PP, HALF, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)REART_MODEL_LDS_CAP) != hipSuccess))
        return REART_ERR_LAUNCH;
    if (K == 1) hipLaunchKernelGGL((base_fwd_long_kernel<PP, HALF, false>), dim3(reart_div_up(cover, PTS)), dim3(64 * W), lds, st, reart_batched(ak, 1));
    else hipLaunchKernelGGL((base_fwd_long_kernel<PP, HALF, true>), dim3(reart_div_up(cover, PTS), K), dim3(64 * W), lds, st, reart_batched(ak, K));
    return REART_OK;
}
// a.pts = 64 | 32 as in the in-LDS forward (32, the default: half waves on different part pairs)
template <int PP>
static int launch_fwd_long(const BaseFwdArgs *a, int K, hipStream_t st) {
    return a[0].pts == 64 ? launch_fwd_long_t<PP, false>(a, K, st) : launch_fwd_long_t<PP, true>(a, K, st);
}

// the caller (reart_base_forward_launch) has checked K and that the instances share one shape
int reart_base_forward_long_launch(const BaseFwdArgs *ak, int K, hipStream_t st) {
    const BaseFwdArgs &a = ak[0];
    if (K < 1 || K > REART_BATCH_MAX || a.P < 1 || a.P > 32 || a.B < 1) return REART_ERR_INVALID_ARG;
    for (int k = 0; k < K; ++k)
        if (ak[k].rt_table || ak[k].trans_list)
            hipLaunchKernelGGL(pose_table_kernel, dim3(reart_div_up(a.B * a.P, 256)), dim3(256), 0, st, ak[k].p6d, ak[k].pt,
                               a.B * a.P, ak[k].rt_table, ak[k].trans_list);
    int rc;
    switch (a.P) {
        case 20: rc = launch_fwd_long<20>(ak, K, st); break;
        case 10: rc = launch_fwd_long<10>(ak, K, st); break;
        case 8: rc = launch_fwd_long<8>(ak, K, st); break;
        default: rc = launch_fwd_long<0>(ak, K, st); break;
    }
    if (rc != REART_OK) return rc;
    REART_CHECK_LAUNCH();
    return REART_OK;
}

// ------------------------------------------------------------------------------- backward
#define BWL_BT_MAX 32                                       // frames per tile at most: the prefetch registers below cover it
#define BWL_UG ((BWL_BT_MAX * RED_CHUNK * 3) / (64 * BW_WAVES))          // G entries of a tile per thread (6)
#define BWL_UR ((BWL_BT_MAX * 32 * 12) / (64 * BW_WAVES))                // [R|t] entries of a tile per thread at P = 32 (12)
static_assert(BWL_UG * 64 * BW_WAVES == BWL_BT_MAX * RED_CHUNK * 3 && BWL_UR * 64 * BW_WAVES == BWL_BT_MAX * 32 * 12, "one batch covers a tile");

// Frames per LDS tile for a shape, the LDS bytes of the launch and whether the hidden gradient gets a tile of its own
// (cpts = 0: asked without one, the smallest footprint -- what reart_base_path means by "fits").  0: not even one frame.
int reart_base_bwd_long_tile(int P, int B, int H, int cpts, int *dp_sep, size_t *lds) {
    if (P < 1 || P > 32 || B < 1 || H < 1) return 0;
    const int PMAX = (P == 20 || P == 10 || P == 8) ? P : 32;
    const size_t fixed = sizeof(float) * ((size_t)(H + PMAX) * BW_LD + RED_CHUNK * 5 + PMAX + 4 + (size_t)H * PMAX + (size_t)PMAX * BW_LD);
    const size_t per = sizeof(float) * ((size_t)RED_CHUNK * 3 + 12 * (size_t)P);          // one frame of s_G and s_rt
    const size_t dp = cpts > 0 ? sizeof(float) * (size_t)H * (cpts + 1) : 0;
    if (fixed + per > REART_MODEL_LDS_CAP) return 0;
    const int want = B < BWL_BT_MAX ? B : BWL_BT_MAX;
    // a tile of its own for dp (the tail's roles then overlap) unless that would leave fewer than 16 frames per tile
    const int sep = dp > 0 && fixed + dp + per * (size_t)(want < 16 ? want : 16) <= REART_MODEL_LDS_CAP;
    const size_t avail = REART_MODEL_LDS_CAP - fixed - (sep ? dp : 0);
    int bt = (int)(avail / per) < want ? (int)(avail / per) : want;
    bt = reart_div_up(B, reart_div_up(B, bt));              // equal tiles
    if (dp_sep) *dp_sep = sep;
    if (lds) *lds = fixed + (sep ? dp : 0) + per * (size_t)bt;
    return bt;
}

template <int PP, bool BATCH>
__global__ __launch_bounds__(64 * BW_WAVES) void base_bwd_long_kernel(Batched<BaseBwdArgs> ab, int BT) {
    const BaseBwdArgs &a = ab.a[BATCH ? blockIdx.y : 0];
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int PMAX = (PP > 0) ? PP : 32;
    constexpr int W = BW_WAVES;
    constexpr int BS = 64 * W;
    static_assert(2 * W >= PMAX, "phase b: one wave per part pair");
    static_assert(W >= (RED_CHUNK / 16) * ((PMAX + 15) / 16), "phase a: at most one dw tile per wave, its accumulator lives across the frame tiles");
    const int P = (PP > 0) ? PP : a.P;
    float *s_h = smem;                               // [H][BW_LD]  hT tile (a.dp_sep == 0: later the dp tile)
    float *s_ds = s_h + (size_t)a.H * BW_LD;         // [PMAX][BW_LD]  dw, later ds
    float *s_x = s_ds + (size_t)PMAX * BW_LD;        // [RED_CHUNK][3]
    float *s_w = s_x + RED_CHUNK * 3;                // [RED_CHUNK]
    int *s_kn = (int *)(s_w + RED_CHUNK);            // [RED_CHUNK] hard part of each point (-1: padding)
    float *s_w2T = (float *)(s_kn + RED_CHUNK + PMAX + 4);   // [H][PMAX]
    float *s_y = s_w2T + (size_t)a.H * PMAX;         // [PMAX][BW_LD]  yT tile
    const int dp_ld = a.dp_sep ? a.cpts + 1 : BW_LD;
    float *s_dp = a.dp_sep ? s_y + (size_t)PMAX * BW_LD : s_h;   // [H][dp_ld]  hidden gradient
    float *s_G = s_y + (size_t)PMAX * BW_LD + (a.dp_sep ? (size_t)a.H * dp_ld : 0);   // [BT][RED_CHUNK*3]  gradient tile of BT frames
    float *s_rt = s_G + (size_t)BT * RED_CHUNK * 3;  // [BT*P][12]  their [R|t] rows
    const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6, chunk = blockIdx.x;
    const int n0 = chunk * a.cpts;
    const int cn = (a.N - n0) < a.cpts ? (a.N - n0) : a.cpts;
    const int cn16 = (cn + 15) & ~15;
    float *prow = a.partial + (size_t)chunk * n_out(a.P, a.H, a.B);

    constexpr int UH = (128 * RED_CHUNK + BS - 1) / BS, UY = (PMAX * RED_CHUNK + BS - 1) / BS, UG = BWL_UG, UR = BWL_UR,
                  UW = (128 * PMAX + BS - 1) / BS;                      // H = 128: one batch each
    const int ilast = cn - 1, nH = a.H * RED_CHUNK, rlast = 3 * cn - 1, nW = a.H * P;
    const bool live = lane < cn;
    const int n = live ? n0 + lane : n0;
    auto load_h = [&](int e0, float (&v)[UH]) {
#pragma unroll
        for (int u = 0; u < UH; ++u) {
            const int e = e0 + u * BS;
            const int ec = e < nH ? e : lane;
            const int j = ec >> 6, i = ec & 63;            // RED_CHUNK == 64
            v[u] = a.hT[(size_t)j * a.N + n0 + (i < cn ? i : ilast)];
        }
    };
    auto store_h = [&](int e0, const float (&v)[UH]) {
#pragma unroll
        for (int u = 0; u < UH; ++u) {
            const int e = e0 + u * BS;
            if (e < nH) s_h[(e >> 6) * BW_LD + (e & 63)] = ((e & 63) < cn) ? v[u] : 0.f;
        }
    };
    // One tile = frames [t0, t0 + bt): its G rows (with the flow-loss terms of the two adjacent pairs, as load_g / store_g of
    // the in-LDS kernel add them: operation order (G + gh) - gl, end frames clamped) and its [R|t] rows.  One batch of
    // unconditional loads (clamped addresses, masked at the store) per tile.
    auto load_tile = [&](int t0, float (&g)[UG], float (&gh)[UG], float (&gl)[UG], float (&rv)[UR]) {
        const int bt = a.B - t0 < BT ? a.B - t0 : BT;
        const int nG = bt * RED_CHUNK * 3, nR = bt * a.P * 12;
#pragma unroll
        for (int u = 0; u < UG; ++u) {
            const int e = tid + u * BS;
            const int ec = e < nG ? e : lane;
            const int tl = ec / (RED_CHUNK * 3), r0_ = ec - tl * (RED_CHUNK * 3), t = t0 + tl;
            const int r = r0_ < 3 * cn ? r0_ : rlast;
            g[u] = a.G[3 * ((size_t)t * a.N + n0) + r];
            gh[u] = 0.f; gl[u] = 0.f;
            if (a.gpf) {   // uniform
                const int fc = t < a.cano_idx ? t : t + 1;   // complete-sequence index of frame t
                const int fh = fc - 1 >= 0 ? fc - 1 : 0, fl = fc <= a.B - 1 ? fc : a.B - 1;
                gh[u] = a.gpf[3 * ((size_t)fh * a.N + n0) + r];
                gl[u] = a.gpf[3 * ((size_t)fl * a.N + n0) + r];
            }
        }
        const float *rsrc = a.rt_table + (size_t)t0 * a.P * 12;
#pragma unroll
        for (int u = 0; u < UR; ++u) rv[u] = rsrc[tid + u * BS < nR ? tid + u * BS : 0];
    };
    auto store_tile = [&](int t0, const float (&g)[UG], const float (&gh)[UG], const float (&gl)[UG], const float (&rv)[UR]) {
        const int bt = a.B - t0 < BT ? a.B - t0 : BT;
        const int nG = bt * RED_CHUNK * 3, nR = bt * a.P * 12;
#pragma unroll
        for (int u = 0; u < UG; ++u) {
            const int e = tid + u * BS;
            if (e < nG) {
                const int tl = e / (RED_CHUNK * 3), r0_ = e - tl * (RED_CHUNK * 3), t = t0 + tl;
                float v = g[u];
                if (a.gpf) {
                    const int fc = t < a.cano_idx ? t : t + 1;
                    if (fc - 1 >= 0) v += gh[u];       // operation order: (G + gh) - gl
                    if (fc <= a.B - 1) v -= gl[u];
                }
                s_G[e] = r0_ < 3 * cn ? v : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < UR; ++u)
            if (tid + u * BS < nR) s_rt[tid + u * BS] = rv[u];
    };
    float vg[UG], vgh[UG], vgl[UG], vr[UR];
    {
        float vh[UH], vw[UW], vy[UY];
        load_tile(0, vg, vgh, vgl, vr);   // produced by the previous kernels on other XCDs: the longest latency first
        load_h(tid, vh);
#pragma unroll
        for (int u = 0; u < UW; ++u) vw[u] = a.W2[tid + u * BS < nW ? tid + u * BS : 0];   // entry e = (p, j) of W2 [P][H], a few per thread
#pragma unroll
        for (int u = 0; u < UY; ++u) {   // rows >= P and columns >= cn repeat real entries: finite, never part of a result
            const int e = tid + u * BS, p = e >> 6, i = e & 63;
            vy[u] = a.yT[(size_t)(p < P ? p : 0) * a.N + n0 + (i < cn ? i : ilast)];
        }
        const float x0 = a.cano[3 * (size_t)n], x1 = a.cano[3 * (size_t)n + 1], x2 = a.cano[3 * (size_t)n + 2];
        int kn = -1;
        if (grp == 0) kn = live ? a.hard_idx[n] : -1;
        // promotion of the Adam step sizes for the finalize launch behind this one, as in base_bwd_block_kernel
        const bool promote = a.step_next != nullptr && chunk == 0 && tid == 0;
        float4 stp = make_float4(0.f, 0.f, 0.f, 0.f);
        if (promote) stp = *(const float4 *)a.step_next;
        store_h(tid, vh);
#pragma unroll
        for (int u = 0; u < UW; ++u) {
            const int e = tid + u * BS, p = e / a.H;
            if (e < nW) s_w2T[(e - p * a.H) * PMAX + p] = vw[u];
        }
#pragma unroll
        for (int u = 0; u < UY; ++u) {
            const int e = tid + u * BS;
            if (e < PMAX * RED_CHUNK) s_y[(e >> 6) * BW_LD + (e & 63)] = vy[u];
        }
        for (int e0 = tid + UH * BS; e0 < nH; e0 += UH * BS) { load_h(e0, vh); store_h(e0, vh); }
        for (int e = tid + UW * BS; e < nW; e += BS) {
            const int p = e / a.H;
            s_w2T[(e - p * a.H) * PMAX + p] = a.W2[e];
        }
        if (grp == 0) {
            s_x[3 * lane] = live ? x0 : 0.f; s_x[3 * lane + 1] = live ? x1 : 0.f; s_x[3 * lane + 2] = live ? x2 : 0.f;
            s_kn[lane] = kn;
        }
        if (promote) *(float4 *)a.step_cur = stp;
    }
    const int p0 = grp * FW_PG;
    const bool has0 = p0 < P, has1 = p0 + 1 < P;
    // a. dw[n,p] = sum_t G[t,n] . (R[t,p] x_n + t[t,p]) on the matrix cores as in the in-LDS kernel (one 16 x 16 tile per wave,
    //    K = 12 B in ascending (t, r, c)); here the chain of a wave runs through all frame tiles, its accumulator in registers
    typedef float f4v __attribute__((ext_vector_type(4)));
    typedef float f16v __attribute__((ext_vector_type(16)));
    const int ntn = (P + 15) / 16, mtn = (cn + 15) >> 4, ndw = mtn * ntn;     // part tiles, point tiles, waves that own a dw tile
    const int dnt = grp / mtn, dmt = grp - dnt * mtn;
    const int nl = 16 * dmt + (lane & 15), kq = lane >> 4;                     // A row (point), k within the instruction
    const int pc = 16 * dnt + (lane & 15);                                     // B column (part)
    const bool pok = pc < P;
    f4v cdw = {0.f, 0.f, 0.f, 0.f};
    for (int t0 = 0; t0 < a.B; t0 += BT) {
        const int bt = a.B - t0 < BT ? a.B - t0 : BT;
        if (t0 > 0) __syncthreads();       // every wave has consumed the previous tile
        store_tile(t0, vg, vgh, vgl, vr);
        __syncthreads();
        if (t0 == 0) {                     // once: w_n = y_hard - y_soft.detach() + y_soft from the y tile (all of the prologue is stored)
            if (grp == 0) {
                const int kn = s_kn[lane];
                const float yk = s_y[(kn < 0 ? 0 : kn) * BW_LD + lane];
                s_w[lane] = (1.0f - yk) + yk;
            }
            __syncthreads();
        }
        if (t0 + BT < a.B) load_tile(t0 + BT, vg, vgh, vgl, vr);   // in flight while this tile is consumed
        if (grp < ndw) {
            const float xt = kq < 3 ? s_x[3 * nl + kq] : 1.0f;
            const float *gp = s_G + 3 * nl;                                // + tl * 192 + r
            const float *bp = s_rt + 12 * (pok ? pc : 0);                  // + tl * 12 P + (kq < 3 ? 3 r + kq : 9 + r)
            const int bo = kq < 3 ? kq : 9, bs = kq < 3 ? 3 : 1;
            constexpr int TU = 4;
            for (int tb = 0; tb < bt; tb += TU) {
                float av[TU][3], bv[TU][3];
#pragma unroll
                for (int u = 0; u < TU; ++u) {
                    const int tl = tb + u < bt ? tb + u : bt - 1;
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        av[u][r] = gp[tl * (RED_CHUNK * 3) + r];
                        bv[u][r] = bp[tl * 12 * a.P + bo + bs * r];
                    }
                }
#pragma unroll
                for (int u = 0; u < TU; ++u) {
                    const bool tok = tb + u < bt;
#pragma unroll
                    for (int r = 0; r < 3; ++r)
                        cdw = __builtin_amdgcn_mfma_f32_16x16x4f32(tok ? av[u][r] * xt : 0.f, (pok && tok) ? bv[u][r] : 0.f, cdw, 0, 0, 0);
                }
            }
        }
        // c2. gR | gt of this tile's frames (one-hot left factor: each output is the ascending-n running sum of its part's
        //     points, as in the in-LDS kernel).  32 columns (t, e) per wave and turn, dealt from the first wave without a dw tile.
        {
            const int n2 = (bt * 12 + 31) >> 5;
            const int pr = lane & 31, kh = lane >> 5;
            for (int g = (grp - ndw + W) % W; g < n2; g += W) {
                f16v c = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                const int col = g * 32 + (lane & 31);
                const bool cok = col < bt * 12;
                const int tl = cok ? col / 12 : 0, e = cok ? col - tl * 12 : 0;
                const int gr = e < 9 ? e / 3 : e - 9, xc = e < 9 ? e - 3 * (e / 3) : 0;
                const float *gcol = s_G + tl * (RED_CHUNK * 3) + gr;
                for (int kb = 0; kb < cn16; kb += 16) {
#pragma unroll
                    for (int kk = kb; kk < kb + 16; kk += 2) {
                        const int nn = kk + kh;
                        const float av = (s_kn[nn] == pr) ? 1.f : 0.f;
                        float bv = s_w[nn] * gcol[3 * nn];
                        if (e < 9) bv = bv * s_x[3 * nn + xc];
                        c = __builtin_amdgcn_mfma_f32_32x32x2f32(av, cok ? bv : 0.f, c, 0, 0, 0);
                    }
                }
                // C/D layout: row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), col = lane & 31
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int prow_p = (reg & 3) + 8 * (reg >> 2) + 4 * kh;
                    if (prow_p < P && cok) prow[off_gRt(a.P, a.H) + ((t0 + tl) * a.P + prow_p) * 12 + e] = c[reg];
                }
            }
        }
    }
    // C/D layout of the dw tile: row = 4 (lane >> 4) + reg, col = lane & 15
    if (grp < ndw) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
            if (pok) s_ds[pc * BW_LD + 16 * dmt + 4 * kq + reg] = cdw[reg];
    }
    __syncthreads();
    // b. softmax backward: dot over all parts in ascending order, ds for this wave's parts
    float ds0 = 0.f, ds1 = 0.f;
    if (has0) {
        const float dw0 = s_ds[p0 * BW_LD + lane];
        const float dw1 = has1 ? s_ds[(p0 + 1) * BW_LD + lane] : 0.f;
        const float tau = a.tau_ptr ? a.tau_ptr[0] : a.tau;
        float dot = 0.f;
#pragma unroll
        for (int p = 0; p < PMAX; ++p)
            if (PP > 0 || p < P) dot = fmaf(s_y[p * BW_LD + lane], s_ds[p * BW_LD + lane], dot);
        ds0 = (s_y[p0 * BW_LD + lane] * (dw0 - dot)) / tau;
        if (has1) ds1 = (s_y[(p0 + 1) * BW_LD + lane] * (dw1 - dot)) / tau;
    }
    __syncthreads();  // every wave has read dw before it is overwritten by ds
    if (has0) s_ds[p0 * BW_LD + lane] = live ? ds0 : 0.f;
    if (has1) s_ds[(p0 + 1) * BW_LD + lane] = live ? ds1 : 0.f;
    __syncthreads();
    // From here on ds, h, x and W2T are read-only and the roles run side by side: waves [0, BW_MFMA) the gW2 tiles, waves
    // [BW_MFMA, BW_WAVES) the hidden gradient dp and then gW1 / gb1 of their own rows of dp.
    const int n1 = (a.H + 31) >> 5;
    if (grp < BW_MFMA) {
        for (int g = grp; g < n1; g += BW_MFMA) {
            // c1. gW2[p,j] = sum_i ds[p,i] h[j,i]: v_mfma_f32_32x32x2_f32 is bit for bit the ascending-i fmaf chain
            f16v c = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const int pr = lane & 31, kh = lane >> 5;
            const int jc = g * 32 + (lane & 31);
            const float *ap = s_ds + (pr < P ? pr : 0) * BW_LD + kh;
            const float *bp = s_h + (jc < a.H ? jc : 0) * BW_LD + kh;
            const bool aok = pr < P, bok = jc < a.H;
            for (int kb = 0; kb < cn16; kb += 16) {
#pragma unroll
                for (int kk = kb; kk < kb + 16; kk += 2) {
                    const float av = aok ? ap[kk] : 0.f;
                    const float bv = bok ? bp[kk] : 0.f;
                    c = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, c, 0, 0, 0);
                }
            }
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int prow_p = (reg & 3) + 8 * (reg >> 2) + 4 * kh;
                if (prow_p < P && bok) prow[off_gW2() + prow_p * a.H + jc] = c[reg];
            }
        }
    }
    if (!a.dp_sep) __syncthreads();  // uniform.  dp overwrites the h tile: the gW2 tiles have consumed it
    if (grp >= BW_MFMA) {
        for (int jt = grp - BW_MFMA; jt < n1; jt += BW_HID) {
            const int j0 = 32 * jt, j1 = (j0 + 32 < a.H) ? j0 + 32 : a.H;
            // b'. dp[n,j] = relu'(h) * sum_p W2[p,j] ds[p]: the ascending-p fmaf chain from zero (rows = points, columns = j, k = p)
            const int jc = j0 + (lane & 31), kh = lane >> 5;
            const bool jok = jc < a.H;
            const float *bp = s_w2T + (jok ? jc : 0) * PMAX + kh;
            for (int nb = 0; nb < cn16; nb += 32) {
                f16v c = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                const float *ap = s_ds + kh * BW_LD + nb + (lane & 31);
#pragma unroll
                for (int p = 0; p < PMAX; p += 2) {   // PMAX is even
                    const bool ok = PP > 0 || p + kh < P;
                    const float av = ok ? ap[p * BW_LD] : 0.f;
                    const float bv = (ok && jok) ? bp[p] : 0.f;
                    c = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, c, 0, 0, 0);
                }
                // C/D layout: row (point) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), col (j) = lane & 31
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int nn = nb + (reg & 3) + 8 * (reg >> 2) + 4 * kh;
                    if (jok && nn < a.cpts) {
                        const float h = s_h[jc * BW_LD + nn];
                        s_dp[jc * dp_ld + nn] = (nn < cn && h > 0.f) ? c[reg] : 0.f;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // c3 reads the rows this very wave wrote, other lanes' entries
            __builtin_amdgcn_wave_barrier();
            // c3. gW1 / gb1 partial from (dp, x): output o = (j, c), two outputs per lane in flight; c == 3 (gb1) with x = 1
            {
                const int ob = 4 * j0 + lane;
                const bool ok0 = ob < 4 * j1, ok1 = ob + 64 < 4 * j1;
                const int ja = ok0 ? ob >> 2 : j0, jb = ok1 ? (ob + 64) >> 2 : ja, c = ob & 3, xo = c < 3 ? c : 0;
                float acc0 = 0.f, acc1 = 0.f;
                for (int ib = 0; ib < cn16; ib += 16) {
#pragma unroll
                    for (int i = ib; i < ib + 16; ++i) {
                        const float xs = s_x[3 * i + xo], xv = c < 3 ? xs : 1.0f;
                        acc0 = fmaf(s_dp[ja * dp_ld + i], xv, acc0);
                        acc1 = fmaf(s_dp[jb * dp_ld + i], xv, acc1);
                    }
                }
                if (c < 3) {
                    if (ok0) prow[off_gW1(a.P, a.H) + 3 * ja + c] = acc0;
                    if (ok1) prow[off_gW1(a.P, a.H) + 3 * jb + c] = acc1;
                } else {
                    if (ok0) prow[off_gb1(a.P, a.H) + ja] = acc0;
                    if (ok1) prow[off_gb1(a.P, a.H) + jb] = acc1;
                }
            }
        }
    }
}

template <int PP>
static int launch_bwd_long(const BaseBwdArgs *ak, int K, size_t lds, int BT, hipStream_t st) {
    if (lds > REART_LDS_DEFAULT_CAP &&
        (hipFuncSetAttribute((const void *)base_bwd_long_kernel<PP, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)REART_MODEL_LDS_CAP) != hipSuccess ||
         hipFuncSetAttribute((const void *)base_bwd_long_kernel<PP, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)REART_MODEL_LDS_CAP) != hipSuccess))
        return REART_ERR_LAUNCH;
    if (K == 1) hipLaunchKernelGGL((base_bwd_long_kernel<PP, false>), dim3(ak[0].nchunk), dim3(64 * BW_WAVES), lds, st, reart_batched(ak, 1), BT);
    else hipLaunchKernelGGL((base_bwd_long_kernel<PP, true>), dim3(ak[0].nchunk, K), dim3(64 * BW_WAVES), lds, st, reart_batched(ak, K), BT);
    return REART_OK;
}

// the block kernel of the backward for K instances that reart_base_backward_launch has prepared (cpts, nchunk, partial rows,
// [R|t] table) and checked; the caller launches base_bwd_finalize_kernel behind it
int reart_base_backward_long_launch(const BaseBwdArgs *args, int K, hipStream_t st) {
    if (K < 1 || K > REART_BATCH_MAX) return REART_ERR_INVALID_ARG;
    BaseBwdArgs ak[REART_BATCH_MAX];
    const BaseBwdArgs &a0 = args[0];
    int dp_sep = 0;
    size_t lds = 0;
    const int BT = reart_base_bwd_long_tile(a0.P, a0.B, a0.H, a0.cpts, &dp_sep, &lds);
    if (BT < 1 || BT > BWL_BT_MAX) return REART_ERR_UNSUPPORTED;
    for (int k = 0; k < K; ++k) {
        if (!args[k].rt_table || !args[k].partial) return REART_ERR_INVALID_ARG;
        ak[k] = args[k];
        ak[k].dp_sep = dp_sep;
    }
    switch (a0.P) {
        case 20: return launch_bwd_long<20>(ak, K, lds, BT, st);
        case 10: return launch_bwd_long<10>(ak, K, lds, BT, st);
        case 8: return launch_bwd_long<8>(ak, K, lds, BT, st);
        default: return launch_bwd_long<0>(ak, K, lds, BT, st);
    }
}
