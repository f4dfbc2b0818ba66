// reart_amd/csrc/model.hip -- relaxation-model kernels for gfx950.
//
// Replaces, fused, the per-iteration PyTorch graph of the reference's
//   BaseModel.forward            networks/model.py:39-70   (seg head networks/blocks.py:99-118,
//                                F.gumbel_softmax(hard=True), rotation_6d_to_matrix
//                                screw_se3/geo_utils.py:632-651, bmm + weighted sum :63-69)
// and its autograd backward, plus compute_pc_transform (utils/model_utils.py:54-67) and the
// Adam update (run_robot.py:145-151,219-221).
//
// The reference materialises [(T-1)*P, N, 3] three times per forward (18.7 MB each at
// T=20); here the forward is one pass: per point, logits -> Gumbel-softmax -> selected part
// -> B rigid transforms, ~1.3 MB of HBM traffic.  All of this is launch/latency bound
// (a few MFLOP); the layout goal is few launches and deterministic reductions.
//
// Internal layouts (caller-owned "saved" buffers): yT [P][N] soft assignment, hard_idx [N] sampled part, and optionally
// hT [H][N] hidden activations: where it is NULL the forward stores none and the backward re-evaluates them (hidden_unit,
// model_dev.h; bwd_fill_h below) -- the fused step runs that way, 4 H N bytes less written and read per iteration.
#include "common.h"
#include "internal.h"
#include "model_dev.h"
#include <math.h>


// ------------------------------------------------------------------------------- helpers
#ifdef REART_PHASE_CLOCK   // diagnostic build only: shader-clock stamps of workgroup 0 per phase
__device__ unsigned long long g_phase_ts[2][16];
extern "C" int reart_debug_phase_clock(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_ts), sizeof(g_phase_ts)) == hipSuccess ? REART_OK : REART_ERR_LAUNCH;
}
// (slots 12 / 13 of a row: the constant-rate 100 MHz wall clock next to the first / latest stamp -- the rate of s_memtime)
#define PHASE_TS(which, k) do { if (blockIdx.x == 1 && threadIdx.x == 0) { g_phase_ts[which][k] = __builtin_amdgcn_s_memtime(); \
    g_phase_ts[which][(k) == 0 ? 12 : 13] = wall_clock64(); } } while (0)
#else
#define PHASE_TS(which, k) do { } while (0)
#endif
#ifdef REART_PHASE_CLOCK
#define PHASE_SYNC_TS(which, k) do { __syncthreads(); PHASE_TS(which, k); } while (0)   // serialises: attribution only
#else
#define PHASE_SYNC_TS(which, k) do { } while (0)
#endif

// ------------------------------------------------------------------------------- forward
// Workgroup = W waves x the same 64 points, W = ceil(P/2): wave g owns parts {2g, 2g+1}.
//   * logits: each wave runs the full ascending-j fmaf chain of ITS parts (the oracle's
//     rounding order), weights broadcast from LDS;
//   * Gumbel noise, (s+g)/tau, exp and the division are evaluated only for the wave's own
//     parts; max / sum / arg-max meet in LDS (the sum is re-done by every lane in ascending
//     part order, again the oracle's order);
//   * the rigid apply of frame t is done by wave t mod W.
// The kernel is latency bound (a few thousand dependent instructions per wave at one wave per
// SIMD), so the design goal is the shortest per-wave instruction stream, not occupancy.

// HALF: a workgroup owns 32 points and the two halves of a wave work on different part pairs (lane = half * 32 +
// point), so that the same chains run in W/2 waves per workgroup on twice as many workgroups (the kernel is bound by the
// serial work of one workgroup; 256 CUs take the extra workgroups for free).  Same arithmetic per (point, part).
template <int PP, bool HALF, bool BATCH>
__global__ __launch_bounds__(64 * (HALF ? (((PP > 0 ? PP : 32) + 2 * FW_PG - 1) / (2 * FW_PG)) : (((PP > 0 ? PP : 32) + FW_PG - 1) / FW_PG)))
void base_fwd_kernel(Batched<BaseFwdArgs> ab) {
    const BaseFwdArgs &a = ab.a[BATCH ? blockIdx.y : 0];      // a single instance reads its block at a fixed offset
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int PMAX = (PP > 0) ? PP : 32;
    constexpr int W = HALF ? (PMAX + 2 * FW_PG - 1) / (2 * FW_PG) : (PMAX + FW_PG - 1) / FW_PG;   // waves
    constexpr int NS = HALF ? 2 * W : W;                  // part-pair slices (one per wave, or per half wave)
    constexpr int PTS = HALF ? FW_PTS / 2 : FW_PTS;       // points per workgroup
    constexpr int BS = 64 * W;
    float *s_rt = smem;                                   // [B*P][12]
    float *s_wb = s_rt + 12 * (size_t)a.B * a.P;          // [H][4]  W1 row | b1
    float *s_w2T = s_wb + 4 * (size_t)a.H;                // [W][H][2]  W2 of wave g's two parts, j-major: 16-byte reads give two j
    float *s_a = s_w2T + (size_t)a.H * PMAX;              // [PMAX][64]  logits, later y
    float *s_e = s_a + PMAX * PTS;                        // [PMAX][PTS]  z, later exp(z - max)
    float *s_hh = s_e + PMAX * PTS;                       // [64][H + 4]  hidden activations, point-major: a lane reads four j at once
    const int HS = a.H + 4;                               // row stride (16-byte aligned rows, lanes spread over the banks)
    const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;
    const int pl = HALF ? (lane & 31) : lane;             // point of this lane inside the workgroup
    const int sid = HALF ? 2 * grp + (lane >> 5) : grp;   // part-pair slice of this lane
    PHASE_TS(0, 0);
    const int P = (PP > 0) ? PP : a.P;
    // Prologue loads: the first batch of every group (pose parameters, W1|b1, one W2 column per thread) is
    // issued before anything is stored to LDS.  That is one memory round trip where the block covers B*P and 4*H
    // (640 threads); at 320 threads the pose tail (wave 0), the W1|b1 tail (waves 0-2) and then the point, the
    // temperature and the noise / iteration counter each wait behind the batch before: three to five round trips
    // by the emitted code.  One batch for all of them (clamped per-thread slots) was built and timed: prologue
    // 2.60 -> 2.69 us, workgroup 8.73 -> 8.55 us, not told from the run-to-run spread; dropped
    // Also built and timed against this form, none told from the run-to-run spread, all dropped: W2 in
    // 16-byte pieces over all threads (a part pair's four j: two loads, two 16-byte LDS stores) with the pose and W1|b1
    // tails moved from wave 0 to waves 1-3, and the logits loop below unrolled 4 and 8 deep (6 -> 12 / 24 LDS reads in flight).
    const int nRT = a.B * a.P;
    auto put_rt = [&](int e, const float (&d6)[6], const float (&tv)[3]) {
        float R[9];
        r6d_to_matrix(d6, R);
#pragma unroll
        for (int c = 0; c < 9; ++c) s_rt[12 * e + c] = R[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) s_rt[12 * e + 9 + c] = tv[c];
        if (blockIdx.x == 0) {
            if (a.trans_list) {
                float *T = a.trans_list + 16 * (size_t)e;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) T[4 * r + c] = R[3 * r + c];
                    T[4 * r + 3] = tv[r];
                }
                T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
            }
            if (a.rt_table) {
#pragma unroll
                for (int c = 0; c < 9; ++c) a.rt_table[12 * (size_t)e + c] = R[c];
#pragma unroll
                for (int c = 0; c < 3; ++c) a.rt_table[12 * (size_t)e + 9 + c] = tv[c];
            }
        }
    };
    {
        float d6[6], tv[3], vw[PMAX];
        const int e0 = tid < nRT ? tid : 0;
#pragma unroll
        for (int c = 0; c < 6; ++c) d6[c] = a.p6d[6 * (size_t)e0 + c];
#pragma unroll
        for (int c = 0; c < 3; ++c) tv[c] = a.pt[3 * (size_t)e0 + c];
        const int ew = tid < 4 * a.H ? tid : 0;
        const float wbv = (ew & 3) < 3 ? a.W1[3 * (ew >> 2) + (ew & 3)] : a.b1[ew >> 2];
        const int jw = tid < a.H ? tid : 0;
#pragma unroll
        for (int p = 0; p < PMAX; ++p) vw[p] = a.W2[(size_t)(p < P ? p : 0) * a.H + jw];
        if (tid < nRT) put_rt(tid, d6, tv);
        if (tid < 4 * a.H) s_wb[tid] = wbv;
        if (tid < a.H) {
#pragma unroll
            for (int p = 0; p < PMAX; ++p) s_w2T[((p >> 1) * a.H + tid) * 2 + (p & 1)] = p < P ? vw[p] : 0.f;
        }
    }
    for (int e = tid + BS; e < nRT; e += BS) {
        float d6[6], tv[3];
#pragma unroll
        for (int c = 0; c < 6; ++c) d6[c] = a.p6d[6 * (size_t)e + c];
#pragma unroll
        for (int c = 0; c < 3; ++c) tv[c] = a.pt[3 * (size_t)e + c];
        put_rt(e, d6, tv);
    }
    for (int e = tid + BS; e < 4 * a.H; e += BS) {
        const int j = e >> 2, c = e & 3;
        s_wb[e] = c < 3 ? a.W1[3 * j + c] : a.b1[j];
    }
    for (int j = tid + BS; j < a.H; j += BS)          // one hidden unit per thread: no integer division
        for (int p = 0; p < PMAX; ++p) s_w2T[((p >> 1) * a.H + j) * 2 + (p & 1)] = p < P ? a.W2[(size_t)p * a.H + j] : 0.f;

    const int n = blockIdx.x * PTS + pl;
    const bool live = n < a.N;
    const int nc = live ? n : a.N - 1;
    const float x0 = a.cano[3 * (size_t)nc], x1 = a.cano[3 * (size_t)nc + 1], x2 = a.cano[3 * (size_t)nc + 2];
    const int p0 = sid * FW_PG;
    const bool has1 = p0 + 1 < P;
    const float tau = a.tau_ptr ? a.tau_ptr[0] : a.tau;
    // Gumbel noise of this wave's parts (issued early: independent of the logits)
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
    PHASE_TS(0, 1);
    // hidden layer once per point: wave g evaluates its slice of the H units for the 64 points
    {
        const int jq = (a.H + NS - 1) / NS, j0 = sid * jq, j1 = (j0 + jq < a.H) ? j0 + jq : a.H;
        // a.hT == NULL (the fused step: the backward re-evaluates hidden_unit from the point and W1|b1): the loop holds no
        // global store and no 64-bit address arithmetic
        if (a.hT) {
            for (int j = j0; j < j1; ++j) {
                const float h = hidden_unit(*(const float4 *)(s_wb + 4 * j), x0, x1, x2);
                s_hh[pl * HS + j] = h;
                if (live) a.hT[(size_t)j * a.N + n] = h;
            }
        } else {
            for (int j = j0; j < j1; ++j) s_hh[pl * HS + j] = hidden_unit(*(const float4 *)(s_wb + 4 * j), x0, x1, x2);
        }
    }
    __syncthreads();
    // logits of this wave's two parts: the full ascending-j fmaf chain (the oracle's rounding order)
    float sp0 = 0.f, sp1 = 0.f;
    {
        const float *hrow = s_hh + pl * HS, *wrow = s_w2T + (size_t)(sid < PMAX / 2 ? sid : PMAX / 2 - 1) * a.H * 2;
        int j = 0;
        const int H4 = (a.H & 3) == 0 ? a.H : 0;   // rows are 16-byte aligned only when H is a multiple of 4
#pragma unroll 2
        for (; j + 4 <= H4; j += 4) {   // 16-byte LDS reads: four h of this point, two (w0, w1) pairs per read
            const float4 h4 = *(const float4 *)(hrow + j);
            const float4 wa = *(const float4 *)(wrow + 2 * j), wb2 = *(const float4 *)(wrow + 2 * j + 4);
            sp0 = fmaf(wa.x, h4.x, sp0); sp1 = fmaf(wa.y, h4.x, sp1);   // sp1: ignored when !has1 (weights are 0)
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
    PHASE_TS(0, 2);
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
    PHASE_TS(0, 3);
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
    PHASE_TS(0, 4);
    for (int t = sid; t < a.B; t += NS) {
        float v[3];
        apply_rt(s_rt + 12 * (t * a.P + k), x0, x1, x2, v);
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
            // (block-skip test of the K-NN kernels)
            float lo[3], hi[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                static_assert(NN_BOX == 16, "a box is one DPP row");
                lo[c] = reart_row16_min(live ? v[c] : INFINITY);        // four DPP steps each, no LDS crossbar; a row lies inside
                hi[c] = reart_row16_max(live ? v[c] : -INFINITY);       // one half wave, so its lanes are active together
                if (hi[c] == -INFINITY) hi[c] = INFINITY;
            }
            const int pos = blockIdx.x * PTS + pl;
            if ((pl & (NN_BOX - 1)) == 0 && pos < a.Npad) {
                float *o = a.boxes + ((size_t)t * (a.Npad / NN_BOX) + pos / NN_BOX) * 8;
                o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = hi[0]; o[4] = hi[1]; o[5] = hi[2];
            }
        }
    }
    PHASE_TS(0, 5);
}

template <int PP, bool HALF>
static void launch_base_fwd_t(const BaseFwdArgs *ak, int K, hipStream_t st) {
    const BaseFwdArgs &a = ak[0];
    constexpr int PMAX = (PP > 0) ? PP : 32;
    constexpr int W = HALF ? (PMAX + 2 * FW_PG - 1) / (2 * FW_PG) : (PMAX + FW_PG - 1) / FW_PG;
    constexpr int PTS = HALF ? FW_PTS / 2 : FW_PTS;
    const int cover = a.out_soa ? (a.Npad > a.N ? a.Npad : a.N) : a.N;
    const size_t lds = sizeof(float) * (12 * (size_t)a.B * a.P + (size_t)a.H * (4 + PMAX) + 2 * (size_t)PTS * PMAX +
                                        (size_t)(a.H + 4) * PTS);
    if (lds > REART_LDS_DEFAULT_CAP) {  // stateless: raise the dynamic-LDS cap whenever the launch needs it (160 KiB per CU on gfx950)
        (void)hipFuncSetAttribute((const void *)base_fwd_kernel<PP, HALF, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024);
        (void)hipFuncSetAttribute((const void *)base_fwd_kernel<PP, HALF, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024);
    }
    if (K == 1) hipLaunchKernelGGL((base_fwd_kernel<PP, HALF, false>), dim3(reart_div_up(cover, PTS)), dim3(64 * W), lds, st, reart_batched(ak, 1));
    else hipLaunchKernelGGL((base_fwd_kernel<PP, HALF, true>), dim3(reart_div_up(cover, PTS), K), dim3(64 * W), lds, st, reart_batched(ak, K));
}
// a.pts = 64 | 32: points per forward workgroup (32, the default: half waves on different part pairs)
template <int PP>
static void launch_base_fwd(const BaseFwdArgs *a, int K, hipStream_t st) {
    if (a[0].pts == 64) launch_base_fwd_t<PP, false>(a, K, st);
    else launch_base_fwd_t<PP, true>(a, K, st);
}

// LDS bytes the launchers reserve a pose table of B frames against: the forward's bound (its largest instantiation) and the
// backward's exact layout.  B = 0: what does not grow with the sequence -- all that the long kernels (model_long.hip) keep.
static size_t base_fwd_lds_bound(int P, int B, int H) {
    return ((size_t)B * P * 12 + 2 * FW_PTS * 32 + (size_t)H * (36 + FW_PTS) + 4 * FW_PTS) * sizeof(float);
}
static size_t base_bwd_lds(int P, int B, int H) {
    const int PMAX = (P == 20 || P == 10 || P == 8) ? P : 32;
    return sizeof(float) * ((size_t)(H + PMAX) * BW_LD + RED_CHUNK * 5 + PMAX + 4 +
                            (size_t)B * RED_CHUNK * 3 + (size_t)H * PMAX + 12 * (size_t)B * P +
                            (size_t)PMAX * BW_LD);
}

// Which kernels serve a shape: 0 = pose table in LDS (this file), 1 = the long path (model_long.hip), negative = neither.
// By fit alone, and the launchers below ask this very function: a shape the in-LDS kernels take never reaches the long ones.
extern "C" int reart_base_path(int P, int B, int H, int backward) {
    if (P < 1 || B < 1 || H < 1) return REART_ERR_INVALID_ARG;
    if (P > 32) return REART_ERR_UNSUPPORTED;
    if ((backward ? base_bwd_lds(P, B, H) : base_fwd_lds_bound(P, B, H)) <= REART_MODEL_LDS_CAP) return 0;
    if (B > REART_MAX_POSE_LEN) return REART_ERR_UNSUPPORTED;
    if (backward) return reart_base_bwd_long_tile(P, B, H, 0, nullptr, nullptr) >= 1 ? 1 : REART_ERR_UNSUPPORTED;
    return base_fwd_lds_bound(P, 0, H) <= REART_MODEL_LDS_CAP ? 1 : REART_ERR_UNSUPPORTED;
}

// the forward's one entry: K instances of one shape in one launch (K = 1: the C ABI below and the single fused step)
int reart_base_forward_launch(const BaseFwdArgs *ak, int K, hipStream_t st, int force_long) {
    if (K < 1 || K > REART_BATCH_MAX) return REART_ERR_INVALID_ARG;
    const BaseFwdArgs &a = ak[0];
    for (int k = 1; k < K; ++k)      // one launch geometry for all
        if (ak[k].N != a.N || ak[k].P != a.P || ak[k].B != a.B || ak[k].H != a.H || ak[k].Npad != a.Npad || ak[k].pts != a.pts ||
            !ak[k].out_soa != !a.out_soa)
            return REART_ERR_INVALID_ARG;
    if (a.P < 1 || a.P > 32) return REART_ERR_UNSUPPORTED;
    const int path = reart_base_path(a.P, a.B, a.H, 0);
    if (path < 0) return path;
    if (path == 1 || force_long) return reart_base_forward_long_launch(ak, K, st);
    switch (a.P) {
        case 20: launch_base_fwd<20>(ak, K, st); break;
        case 10: launch_base_fwd<10>(ak, K, st); break;
        case 8: launch_base_fwd<8>(ak, K, st); break;
        default: launch_base_fwd<0>(ak, K, st); break;
    }
    REART_CHECK_LAUNCH();
    return REART_OK;
}

extern "C" int reart_base_forward(const float *cano, int N, int P, int B, const float *W1,
                                  const float *b1, const float *W2, int H, const float *prop6d,
                                  const float *propt, const float *gumbel, float tau, float *out,
                                  int64_t *seg_part, float *trans_list, float *yT, float *hT,
                                  int32_t *hard_idx, void *stream) {
    if (N < 0 || P < 1 || B < 0 || H < 1) return REART_ERR_INVALID_ARG;
    if (N == 0 || B == 0) return REART_OK;
    if (!cano || !W1 || !b1 || !W2 || !prop6d || !propt || !gumbel || !out) return REART_ERR_INVALID_ARG;
    if (!(tau > 0.f)) return REART_ERR_INVALID_ARG;
    BaseFwdArgs a = {};
    a.cano = cano; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.p6d = prop6d; a.pt = propt;
    a.gumbel = gumbel; a.tau = tau; a.N = N; a.P = P; a.B = B; a.H = H; a.Npad = 0;
    a.out = out; a.seg_part = seg_part; a.trans_list = trans_list; a.yT = yT; a.hT = hT;
    a.hard_idx = hard_idx;
    return reart_base_forward_launch(&a, 1, (hipStream_t)stream, 0);
}

// The production noise stream, exported: out[n][p] = the Gumbel sample the forward kernel draws for (point n, part p) in
// iteration `iter` of an engine seeded with `seed` -- the same philox4x32 call (counter = n, p / 4, iter; key = seed; word
// p % 4) and the same gumbel_from_bits, so injecting `out` into the forward reproduces the in-kernel path bit for bit.
__global__ __launch_bounds__(256) void gumbel_noise_kernel(uint64_t seed, uint64_t it, int N, int P, float *__restrict__ out) {
    const int Q = (P + 3) >> 2;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)N * Q) return;
    const int n = (int)(e / Q), q = (int)(e % Q);
    uint32_t r[4];
    philox4x32((uint32_t)n, (uint32_t)q, (uint32_t)it, (uint32_t)(it >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (4 * q + w < P) out[(size_t)n * P + 4 * q + w] = gumbel_from_bits(r[w]);
}

extern "C" int reart_gumbel_noise(uint64_t seed, int64_t iter, int N, int P, float *out, void *stream) {
    if (N < 0 || P < 1 || iter < 0) return REART_ERR_INVALID_ARG;
    if (N == 0) return REART_OK;
    if (!out) return REART_ERR_INVALID_ARG;
    const size_t total = (size_t)N * ((P + 3) >> 2);
    gumbel_noise_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(seed, (uint64_t)iter, N, P, out);
    REART_CHECK_LAUNCH();
    return REART_OK;
}

// ------------------------------------------------------------------------------- backward

// [R|t] table [B*P][12] in global memory, so that the backward can read it with scalar loads
__global__ __launch_bounds__(256) void rt_table_kernel(const float *__restrict__ p6d,
                                                       const float *__restrict__ pt, int n,
                                                       float *__restrict__ table) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float R[9];
    r6d_to_matrix(p6d + 6 * (size_t)e, R);
#pragma unroll
    for (int c = 0; c < 9; ++c) table[12 * (size_t)e + c] = R[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) table[12 * (size_t)e + 9 + c] = pt[3 * (size_t)e + c];
}

// (1) One workgroup per chunk of up to 64 points, BW_WAVES waves x the same points:
//   a. dL/dw[n,p] = sum_t G[t,n].(R[t,p] x_n + t[t,p]) as one matrix product, one 16 x 16 tile per wave
//   b. softmax backward -> ds[n,:] (LDS): wave g < ceil(P/2) for parts {2g, 2g+1}, y from the LDS copy of the yT tile
//   c. partial sums over the chunk of every parameter gradient, each output accumulated
//      sequentially over the chunk's points (ascending n) -> deterministic:
//        gW2[p,j] = sum_n ds[n,p] h[n,j];  gW1[j,c] = sum_n dp[n,j] x[n,c];  gb1[j] = sum_n dp[n,j]
//        gR[t,p]  = sum_{n:k_n=p} w_n G[t,n] x_n^T;  gt[t,p] = sum_{n:k_n=p} w_n G[t,n]
//      Behind the barrier that completes ds the reductions need nothing from one another, so the waves split by ROLE
//      instead of walking them in turn: waves [0, BW_MFMA) take the gR|gt and gW2 tiles, waves [BW_MFMA, BW_WAVES) the
//      hidden gradient dp (b') and then gW1 / gb1 (c3) of THEIR OWN 32 rows j of dp -- so c3 needs no barrier at all,
//      only the wave's own LDS order.  dp has storage of its own (the h tile stays read-only for the gW2 tiles); where
//      the LDS budget does not allow that (a.dp_sep == 0) dp overwrites the h tile as before and one workgroup barrier
//      separates the two roles.
#ifdef REART_PHASE_CLOCK   // stamp of another wave's lane 0 (the roles of the tail)
#define PHASE_TS_WAVE(which, k, wave) do { if (blockIdx.x == 1 && (int)threadIdx.x == 64 * (wave)) g_phase_ts[which][k] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define PHASE_TS_WAVE(which, k, wave) do { } while (0)
#endif

// Tile staging of the block kernel: global memory -> the LDS tiles, in pieces of V consecutive words of a row: one 16-byte
// load (V = 4: 16-byte rows, see the call) or one dword load (V = 1: any N, H and any 4-byte-aligned pointer).
//   * Only the workgroup's own cw = a.cpts columns of the h / G / y tiles are loaded and stored (the tiles keep their
//     64-point layout).  Who reads a column >= cn of a tile, all of them covered by [0, cw) or by what phase a writes:
//       s_h   the gW2 tiles (c1) up to cn16; dp (b') at nn < a.cpts, where nn >= cn yields 0 whatever it reads
//             (a.hT == NULL: not staged here -- bwd_fill_h writes the same columns during phase a);
//       s_G   dw (a) and the gR|gt tiles (c2) up to cn16;
//       s_y   phase b, rows p < P, at its lane's column (a lane >= cn16 reads column 0 instead);
//       s_ds  phase b likewise: dw is written by phase a up to cn16; gW2 and dp up to cn16;   s_dp  gW1 / gb1 (c3) up to cn16.
//     A short last chunk loads nothing for the columns cn..cw and stores zeros there.
//   * Every load of the first batch of every group is issued before the first LDS store, G (written by the previous
//     kernel on other XCDs) first; no load is a clamped repeat: a piece outside its tile is not loaded at all.
//   * The groups are dealt to different threads (G from thread 0 up, W2 from thread 384 up, y from the last thread down),
//     W2 over P * H / V threads with the part running fastest: conflict-free LDS stores, no 20-deep chain on two waves.
//   * FAST: the template's shape (P = PP, H = 128, B = 19, 32 points, full chunk) with every count a constant, so a group
//     is one range test of the thread index.  Emitted code of that path, <20, false>: eight 16-byte loads plus wave 0's
//     point (one 12-byte, one dword load) before the first wait, five exec-mask blocks in the store section (one per group
//     that does not cover all threads), about 250 instructions (145 VALU) from the path's entry to the barrier -- against
//     about 50 dword loads, 45 blocks and 1 560 instructions (840 VALU) of the clamped 64-column form before.
template <int V> struct BwPiece { float v[V]; };
template <int V> __device__ __forceinline__ BwPiece<V> bw_load(const float *p) {
    BwPiece<V> r;
    if constexpr (V == 4) {
        const float4 q = *(const float4 *)p;
        r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int PP, int V, bool FAST, class LoadPoint>
__device__ __forceinline__ void bwd_stage_tiles(const BaseBwdArgs &a, int n0, int cn, float *s_h, float *s_G, float *s_w2T,
                                                float *s_rt, float *s_y, LoadPoint load_point) {
    typedef BwPiece<V> Pc;
    constexpr int PMAX = (PP > 0) ? PP : 32, BS = 64 * BW_WAVES;
    const int P = (PP > 0) ? PP : a.P;
    const int H = FAST ? 128 : a.H, B = FAST ? 19 : a.B, cw = FAST ? 32 : a.cpts;
    const int rsh = (cw == 64 ? 6 : (cw == 32 ? 5 : 4)) - (V == 4 ? 2 : 0);   // log2 of the pieces per tile row
    const int rp = 1 << rsh, gpc = 3 * rp;                                       // pieces per row of h / y, per frame of G
    const int nH = H << rsh, nY = P << rsh, nG = B * gpc, nR = B * P * 12 / V, nW = P * (H / V);
    // first batch of every group: H = 128, B = 19, P = 20 at 64 points fit (FAST: at 32 points, exactly)
    constexpr int UH = FAST ? 1 : 128 * RED_CHUNK / V / BS, UG = FAST ? 1 : (19 * RED_CHUNK * 3 / V + BS - 1) / BS,
                  UY = FAST ? 1 : (PMAX * RED_CHUNK / V + BS - 1) / BS, UR = (19 * 20 * 12 / V + BS - 1) / BS,
                  UW = FAST ? 1 : (PMAX * 128 / V + BS - 1) / BS;
    const int tid = threadIdx.x, tw = (tid + BS - 384) & (BS - 1), ty = BS - 1 - tid;
    const bool flow = a.gpf != nullptr;   // uniform
    // upstream gradient tile; the fused step adds the flow-loss terms of the two adjacent pairs
    // (complete frame fc = t or t + 1: + d/d pred_flow of pair fc - 1, - d/d pred_flow of pair fc)
    auto load_g = [&](int e, Pc &g, Pc &gh, Pc &gl) {
        const int t = (e >> rsh) / 3, r = (e - t * gpc) * V;
        if (e < nG && (FAST || r < 3 * cn)) {   // a piece that is not loaded stays unset: its store tests the same conditions
            g = bw_load<V>(a.G + 3 * ((size_t)t * a.N + n0) + r);
            if (flow) {
                const int fc = t < a.cano_idx ? t : t + 1;   // complete-sequence index of frame t
                const int fh = fc - 1 >= 0 ? fc - 1 : 0, fl = fc <= B - 1 ? fc : B - 1;
                gh = bw_load<V>(a.gpf + 3 * ((size_t)fh * a.N + n0) + r);
                gl = bw_load<V>(a.gpf + 3 * ((size_t)fl * a.N + n0) + r);
            }
        }
    };
    auto store_g = [&](int e, const Pc &g, const Pc &gh, const Pc &gl) {
        if (e < nG) {
            const int t = (e >> rsh) / 3, r = (e - t * gpc) * V;
            const int fc = t < a.cano_idx ? t : t + 1;
            const bool ah = flow && fc - 1 >= 0, al = flow && fc <= B - 1, in = FAST || r < 3 * cn;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                float v = in ? g.v[k] : 0.f;
                if (in && ah) v += gh.v[k];       // operation order: (G + gh) - gl
                if (in && al) v -= gl.v[k];
                s_G[t * (RED_CHUNK * 3) + r + k] = v;
            }
        }
    };
    // a [rows][N] matrix -> a [rows][BW_LD] tile (hT, yT)
    auto load_t = [&](const float *src, int e, int n) {
        Pc v;
        const int j = e >> rsh, i = (e & (rp - 1)) * V;
        if (e < n && (FAST || i < cn)) v = bw_load<V>(src + (size_t)j * a.N + n0 + i);
        return v;
    };
    auto store_t = [&](float *dst, int e, int n, const Pc &v) {
        if (e < n) {
            const int j = e >> rsh, i = (e & (rp - 1)) * V;
#pragma unroll
            for (int k = 0; k < V; ++k) dst[j * BW_LD + i + k] = (FAST || i < cn) ? v.v[k] : 0.f;
        }
    };
    auto load_r = [&](int e) {
        Pc v;
        if (e < nR) v = bw_load<V>(a.rt_table + V * (size_t)e);
        return v;
    };
    auto store_r = [&](int e, const Pc &v) {
        if (e < nR) {
#pragma unroll
            for (int k = 0; k < V; ++k) s_rt[V * e + k] = v.v[k];
        }
    };
    // W2 [P][H] -> s_w2T [H][PMAX]: piece e = (j / V, p), the part running fastest
    auto load_w = [&](int e) {
        Pc v;
        const int jq = (unsigned)e / (unsigned)P, p = e - jq * P;
        if (e < nW) v = bw_load<V>(a.W2 + (size_t)p * H + V * jq);
        return v;
    };
    auto store_w = [&](int e, const Pc &v) {
        if (e < nW) {
            const int jq = (unsigned)e / (unsigned)P, p = e - jq * P;
#pragma unroll
            for (int k = 0; k < V; ++k) s_w2T[(V * jq + k) * PMAX + p] = v.v[k];
        }
    };
    // a.hT == NULL (uniform): nobody saved the hidden activations.  The h tile is then none of this function's business:
    // the waves that have no dw tile in phase a fill it meanwhile (bwd_fill_h below).
    const bool reh = a.hT == nullptr;
    Pc vg[UG], vgh[UG], vgl[UG], vh[UH], vr[UR], vw[UW], vy[UY];
#pragma unroll
    for (int u = 0; u < UG; ++u) load_g(tid + u * BS, vg[u], vgh[u], vgl[u]);
#pragma unroll
    for (int u = 0; u < UH; ++u)
        if (!reh) vh[u] = load_t(a.hT, tid + u * BS, nH);
#pragma unroll
    for (int u = 0; u < UR; ++u) vr[u] = load_r(tid + u * BS);
#pragma unroll
    for (int u = 0; u < UW; ++u) vw[u] = load_w(tw + u * BS);
#pragma unroll
    for (int u = 0; u < UY; ++u) vy[u] = load_t(a.yT, ty + u * BS, nY);
    load_point();
    PHASE_TS(1, 9);
#ifdef REART_PHASE_CLOCK
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the stamp behind it is "loads returned" (diagnostic build only)
#endif
    PHASE_TS(1, 10);
#pragma unroll
    for (int u = 0; u < UG; ++u) store_g(tid + u * BS, vg[u], vgh[u], vgl[u]);
#pragma unroll
    for (int u = 0; u < UH; ++u)
        if (!reh) store_t(s_h, tid + u * BS, nH, vh[u]);
#pragma unroll
    for (int u = 0; u < UR; ++u) store_r(tid + u * BS, vr[u]);
#pragma unroll
    for (int u = 0; u < UW; ++u) store_w(tw + u * BS, vw[u]);
#pragma unroll
    for (int u = 0; u < UY; ++u) store_t(s_y, ty + u * BS, nY, vy[u]);
    if (!FAST) {   // what a larger shape has beyond the first batches
        for (int e = tid + UG * BS; e < nG; e += BS) { load_g(e, vg[0], vgh[0], vgl[0]); store_g(e, vg[0], vgh[0], vgl[0]); }
        if (!reh)
            for (int e = tid + UH * BS; e < nH; e += BS) store_t(s_h, e, nH, load_t(a.hT, e, nH));
        for (int e = tid + UR * BS; e < nR; e += BS) store_r(e, load_r(e));
        for (int e = tw + UW * BS; e < nW; e += BS) store_w(e, load_w(e));
        for (int e = ty + UY * BS; e < nY; e += BS) store_t(s_y, e, nY, load_t(a.yT, e, nY));
    }
}

// The h tile without a saved hT: hidden_unit (model_dev.h) of the chunk's points and W1 | b1 -- the forward's very expression
// on the forward's very operands, so the forward's bits.  Run by the `nt` threads (index it) of the waves that have no dw tile
// in phase a, BEHIND the first barrier (the points are in s_x) and in front of the barrier that ends phase a; h is first
// read behind the one after that (gW2 tiles, dp).  So the fill costs the critical path nothing: its one round trip to
// the L2-hot 2 KB of W1 | b1 and its 5 flops per value hide under the matrix product of the other waves, and the tile
// staging loses its largest load.  A piece = four columns of one row; columns cn..cpts are zero as in the staged form.
__device__ __forceinline__ void bwd_fill_h(const BaseBwdArgs &a, int cn, int it, int nt, const float *s_x, float *s_h) {
    const int sh = a.cpts == 64 ? 4 : (a.cpts == 32 ? 3 : 2);   // log2 of the pieces per row
    const int np = a.H << sh;
    constexpr int U = 2;                                        // pieces in flight per thread (H = 128, 32 points, 12 waves: one batch)
    for (int e0 = it; e0 < np; e0 += U * nt) {
        float4 wb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * nt, j = (e < np ? e : e0) >> sh;
            wb[u] = make_float4(a.W1[3 * j], a.W1[3 * j + 1], a.W1[3 * j + 2], a.b1[j]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * nt;
            if (e < np) {
                const int j = e >> sh, i = (e & ((1 << sh) - 1)) << 2;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float h = hidden_unit(wb[u], s_x[3 * (i + k)], s_x[3 * (i + k) + 1], s_x[3 * (i + k) + 2]);
                    s_h[j * BW_LD + i + k] = (i + k < cn) ? h : 0.f;
                }
            }
        }
    }
}

template <int PP, bool BATCH>
__global__ __launch_bounds__(64 * BW_WAVES) void base_bwd_block_kernel(Batched<BaseBwdArgs> ab) {
    const BaseBwdArgs &a = ab.a[BATCH ? blockIdx.y : 0];
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int PMAX = (PP > 0) ? PP : 32;
    constexpr int W = BW_WAVES;
    static_assert(2 * W >= PMAX, "phase b: one wave per part pair");
    const int P = (PP > 0) ? PP : a.P;
    float *s_h = smem;                               // [H][BW_LD]  hT tile (a.dp_sep == 0: later the dp tile)
    float *s_ds = s_h + (size_t)a.H * BW_LD;         // [PMAX][BW_LD]  dw, later ds
    float *s_x = s_ds + (size_t)PMAX * BW_LD;        // [RED_CHUNK][3]
    float *s_w = s_x + RED_CHUNK * 3;                // [RED_CHUNK]
    int *s_kn = (int *)(s_w + RED_CHUNK);            // [RED_CHUNK] hard part of each point (-1: padding)
    float *s_G = (float *)(s_kn + RED_CHUNK + PMAX + 4);  // [B][RED_CHUNK*3]  upstream gradient tile
    float *s_w2T = s_G + (size_t)a.B * RED_CHUNK * 3;// [H][PMAX]
    float *s_rt = s_w2T + (size_t)a.H * PMAX;        // [B*P][12]  [R|t] rows
    float *s_y = s_rt + (size_t)a.B * a.P * 12;      // [PMAX][BW_LD]  yT tile
    const int dp_ld = a.dp_sep ? a.cpts + 1 : BW_LD;
    float *s_dp = a.dp_sep ? s_y + (size_t)PMAX * BW_LD : s_h;   // [H][dp_ld]  hidden gradient
    const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6, chunk = blockIdx.x;
    // a workgroup owns a.cpts (64, 32 or 16) points; the tiles keep their 64-point layout (columns cn..a.cpts are zero, those
    // beyond are never written nor read), the matrix-core loops stop at cn16: with 32 points twice as many workgroups each run
    // half the reductions
    const int n0 = chunk * a.cpts;
    const int cn = (a.N - n0) < a.cpts ? (a.N - n0) : a.cpts;
    const int cn16 = (cn + 15) & ~15;   // tile columns beyond cn are zero: whole blocks of 16 points keep the loops unrolled
    float *prow = a.partial + (size_t)chunk * n_out(a.P, a.H, a.B);
    PHASE_TS(1, 0);

    // Tile loads: bwd_stage_tiles above (one batch of loads, then the stores).  The 16-byte form needs 16-byte rows: N and H
    // multiples of 4 and every base pointer 16-byte aligned (chosen here, uniformly); anything else takes the dword form.
    // The point coordinates and hard_idx (wave 0, one point per lane) ride in the same batch.
    const bool live = lane < cn;
    const int n = live ? n0 + lane : n0;
    const bool vec = ((a.N | a.H) & 3) == 0 &&
                     (((uintptr_t)a.hT | (uintptr_t)a.yT | (uintptr_t)a.G | (uintptr_t)a.gpf | (uintptr_t)a.rt_table | (uintptr_t)a.W2) & 15) == 0;
    float x0 = 0.f, x1 = 0.f, x2 = 0.f;
    int kn = -1;
    // Fused step: thread 0 of workgroup 0 promotes the Adam step sizes the bookkeeping workgroup of the previous finalize
    // launch left in step_next to step_cur, which the finalize launch behind this one reads (no workgroup of THIS launch
    // reads either).  The load rides in the batch; the store goes out with the point's, nobody waits for it.
    const bool promote = a.step_next != nullptr && chunk == 0 && tid == 0;
    float4 stp = make_float4(0.f, 0.f, 0.f, 0.f);
    auto load_point = [&]() {
        if (grp == 0) {
            x0 = a.cano[3 * (size_t)n]; x1 = a.cano[3 * (size_t)n + 1]; x2 = a.cano[3 * (size_t)n + 2];
            kn = live ? a.hard_idx[n] : -1;
            if (promote) stp = *(const float4 *)a.step_next;
        }
    };
    if (PP == 20 && vec && a.H == 128 && a.B == 19 && a.cpts == 32 && cn == 32)
        bwd_stage_tiles<PP, 4, true>(a, n0, cn, s_h, s_G, s_w2T, s_rt, s_y, load_point);
    else if (vec)
        bwd_stage_tiles<PP, 4, false>(a, n0, cn, s_h, s_G, s_w2T, s_rt, s_y, load_point);
    else
        bwd_stage_tiles<PP, 1, false>(a, n0, cn, s_h, s_G, s_w2T, s_rt, s_y, load_point);
    if (grp == 0) {
        s_x[3 * lane] = live ? x0 : 0.f; s_x[3 * lane + 1] = live ? x1 : 0.f; s_x[3 * lane + 2] = live ? x2 : 0.f;
        s_kn[lane] = kn;
        if (promote) *(float4 *)a.step_cur = stp;
    }
    PHASE_TS(1, 11);
    // a. dw[n,p] = sum_t G[t,n] . (R[t,p] x_n + t[t,p]) as ONE matrix product on the matrix cores:
    //      dw = A Bm,   A[n][(t,r,c)] = G[t,n,r] * (c < 3 ? x_n[c] : 1),   Bm[(t,r,c)][p] = [R|t][t,p][r][c]
    //    (K = 12 B, ascending (t, r, c): a fixed summation order, deterministic).  v_mfma_f32_16x16x4_f32:
    //    one 16 (points) x 16 (parts) tile per wave, the four k of an instruction are c = 0..3 of one (t, r).
    //    The per-lane VALU form of this sum (apply, then dot) was LDS-bound on the broadcast [R|t] rows.
    const int p0 = grp * FW_PG;
    const bool has0 = p0 < P, has1 = p0 + 1 < P;
    __syncthreads();
    PHASE_TS(1, 1);
    {
        typedef float f4v __attribute__((ext_vector_type(4)));
        const int ntn = (P + 15) / 16;                       // part tiles
        const int mtn = (cn + 15) >> 4;                      // point tiles
        if (a.hT == nullptr) {                               // uniform.  At most 8 of the 16 waves have a dw tile; the others fill h
            const int w0 = mtn * ntn < W ? mtn * ntn : 0;
            if (grp >= w0) bwd_fill_h(a, cn, tid - 64 * w0, 64 * (W - w0), s_x, s_h);
        }
        for (int tile = grp; tile < mtn * ntn; tile += W) {
            const int nt = tile / mtn, mt = tile - nt * mtn;
            const int nl = 16 * mt + (lane & 15), kq = lane >> 4;          // A row (point), k within the instruction
            const int pc = 16 * nt + (lane & 15);                          // B column (part)
            const bool pok = pc < P;
            const float xt = kq < 3 ? s_x[3 * nl + kq] : 1.0f;
            const float *gp = s_G + 3 * nl;                                // + t * 192 + r
            const float *bp = s_rt + 12 * (pok ? pc : 0);                  // + t * 12 P + (kq < 3 ? 3 r + kq : 9 + r)
            f4v c = {0.f, 0.f, 0.f, 0.f};
            const int bo = kq < 3 ? kq : 9;                     // offset of (r = 0, c = kq) inside a [R|t] row
            const int bs = kq < 3 ? 3 : 1;                      // stride over r
            constexpr int TU = 4;                               // frames per batch: 24 LDS reads in flight, then 12 MFMAs
            for (int t0 = 0; t0 < a.B; t0 += TU) {
                float av[TU][3], bv[TU][3];
#pragma unroll
                for (int u = 0; u < TU; ++u) {
                    const int t = t0 + u < a.B ? t0 + u : a.B - 1;
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        av[u][r] = gp[t * (RED_CHUNK * 3) + r];
                        bv[u][r] = bp[t * 12 * a.P + bo + bs * r];
                    }
                }
#pragma unroll
                for (int u = 0; u < TU; ++u) {
                    const bool tok = t0 + u < a.B;
#pragma unroll
                    for (int r = 0; r < 3; ++r)
                        c = __builtin_amdgcn_mfma_f32_16x16x4f32(tok ? av[u][r] * xt : 0.f, (pok && tok) ? bv[u][r] : 0.f, c, 0, 0, 0);
                }
            }
            // C/D layout: row = 4 (lane >> 4) + reg, col = lane & 15
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
                if (pok) s_ds[pc * BW_LD + 16 * mt + 4 * kq + reg] = c[reg];
        }
    }
    __syncthreads();
    PHASE_TS(1, 2);
    // b. softmax backward: dot over all parts in ascending order, ds for this wave's parts
    const int bl = lane < cn16 ? lane : 0;   // a lane beyond the tile's written columns reads column 0: its results are dropped (live)
    if (grp == 0) {
        const float yk = s_y[(kn < 0 ? 0 : kn) * BW_LD + bl];
        s_w[lane] = (1.0f - yk) + yk;
    }
    float ds0 = 0.f, ds1 = 0.f;
    if (has0) {
        const float dw0 = s_ds[p0 * BW_LD + bl];
        const float dw1 = has1 ? s_ds[(p0 + 1) * BW_LD + bl] : 0.f;
        const float tau = a.tau_ptr ? a.tau_ptr[0] : a.tau;
        float dot = 0.f;
#pragma unroll
        for (int p = 0; p < PMAX; ++p)
            if (PP > 0 || p < P) dot = fmaf(s_y[p * BW_LD + bl], s_ds[p * BW_LD + bl], dot);
        ds0 = (s_y[p0 * BW_LD + bl] * (dw0 - dot)) / tau;
        if (has1) ds1 = (s_y[(p0 + 1) * BW_LD + bl] * (dw1 - dot)) / tau;
    }
    __syncthreads();  // every wave has read dw before it is overwritten by ds
    if (has0) s_ds[p0 * BW_LD + lane] = live ? ds0 : 0.f;
    if (has1) s_ds[(p0 + 1) * BW_LD + lane] = live ? ds1 : 0.f;
    __syncthreads();
    PHASE_TS(1, 3);
    // From here on ds, h, G, x, w, kn and W2T are read-only: the roles run side by side.
    const int n2 = (a.B * 12 + 31) >> 5, n1 = (a.H + 31) >> 5;   // gR|gt tiles (dealt first: the longer ones), gW2 tiles
    if (grp < BW_MFMA) {
        typedef float f16v __attribute__((ext_vector_type(16)));
        for (int g = grp; g < n2 + n1; g += BW_MFMA) {
            f16v c = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const int pr = lane & 31, kh = lane >> 5;
            if (g >= n2) {
                // c1. gW2[p,j] = sum_i ds[p,i] h[j,i] on the matrix cores: v_mfma_f32_32x32x2_f32 is bit for bit the
                // ascending-i fmaf chain (cdna guide section 3).  One 32 (parts) x 32 (hidden) tile per wave.
                const int jc = (g - n2) * 32 + (lane & 31);
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
                // C/D layout: row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), col = lane & 31
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int prow_p = (reg & 3) + 8 * (reg >> 2) + 4 * kh;
                    if (prow_p < P && bok) prow[off_gW2() + prow_p * a.H + jc] = c[reg];
                }
                PHASE_TS_WAVE(1, 5, n2 % BW_MFMA);
            } else {
                // c2. gR | gt on the matrix cores:  out[p][(t, e)] = sum_n onehot[p][n] * v[n][(t, e)]  with
                //   v = (w_n G[t,n,r]) x_n[c]  (e = 3 r + c < 9)   or   w_n G[t,n,e-9]  (translation),
                // the operands built on the fly from the LDS tiles.  A one-hot left factor makes every product
                // exact (1 * v = v, 0 * v = 0), so each output is the ascending-n running sum of its part's
                // points: deterministic, no sorting, no atomics.
                const int col = g * 32 + (lane & 31);
                const bool cok = col < a.B * 12;
                const int t = cok ? col / 12 : 0, e = cok ? col - t * 12 : 0;
                const int gr = e < 9 ? e / 3 : e - 9, xc = e < 9 ? e - 3 * (e / 3) : 0;
                const float *gcol = s_G + t * (RED_CHUNK * 3) + gr;
                for (int kb = 0; kb < cn16; kb += 16) {
#pragma unroll
                    for (int kk = kb; kk < kb + 16; kk += 2) {
                        const int n = kk + kh;
                        const float av = (s_kn[n] == pr) ? 1.f : 0.f;
                        float bv = s_w[n] * gcol[3 * n];
                        if (e < 9) bv = bv * s_x[3 * n + xc];
                        c = __builtin_amdgcn_mfma_f32_32x32x2f32(av, cok ? bv : 0.f, c, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int prow_p = (reg & 3) + 8 * (reg >> 2) + 4 * kh;
                    if (prow_p < P && cok) prow[off_gRt(a.P, a.H) + (t * a.P + prow_p) * 12 + e] = c[reg];
                }
                PHASE_TS_WAVE(1, 4, 0);
            }
        }
    }
    if (!a.dp_sep) __syncthreads();  // uniform.  dp overwrites the h tile: the gW2 tiles have consumed it
    if (grp >= BW_MFMA) {
        typedef float f16v __attribute__((ext_vector_type(16)));
        // one 32-row tile of j per wave and turn: dp of these rows (b'), then their gW1 / gb1 (c3)
        for (int jt = grp - BW_MFMA; jt < n1; jt += BW_HID) {
            const int j0 = 32 * jt, j1 = (j0 + 32 < a.H) ? j0 + 32 : a.H;
            // b'. dp[n,j] = relu'(h) * sum_p W2[p,j] ds[p] on the matrix cores, the ascending-p fmaf chain from zero that
            // v_mfma_f32_32x32x2_f32 is bit for bit (rows = points, columns = j, k = p; a part beyond P adds fma(0, 0, acc)
            // = acc: the chain starts at +0 and so never holds -0).  The W2T row of a VALU lane would be a broadcast LDS
            // read per (j, p) and wave; here it is one operand read per instruction.
            const int jc = j0 + (lane & 31), kh = lane >> 5;
            const bool jok = jc < a.H;
            const float *bp = s_w2T + (jok ? jc : 0) * PMAX + kh;
            for (int nb = 0; nb < cn16; nb += 32) {
                f16v c = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                const float *ap = s_ds + kh * BW_LD + nb + (lane & 31);
#pragma unroll
                for (int p = 0; p < PMAX; p += 2) {   // PMAX is even
                    const bool pok = PP > 0 || p + kh < P;
                    const float av = pok ? ap[p * BW_LD] : 0.f;
                    const float bv = (pok && jok) ? bp[p] : 0.f;
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
            PHASE_TS_WAVE(1, 6, BW_MFMA);
            // c3. gW1 / gb1 partial from (dp, x): output o = (j, c), two outputs per lane in flight.  c == 3 (gb1) runs the
            // same chain with x = 1: fmaf(d, 1, acc) is d + acc rounded once, bit for bit the plain sum.
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
            PHASE_TS_WAVE(1, 7, BW_MFMA);
        }
    }
    PHASE_SYNC_TS(1, 8);   // diagnostic build only: the workgroup's end = the slower role's
}

// (2) sum the chunk partials in ascending chunk order; Gram-Schmidt backward for the
// 6-vectors; optionally the Adam update of the very parameter this thread reduced.

// One Adam step of one parameter from values ALREADY in registers: the caller loads p, m and v next to the partial rows
// (none of them depends on the gradient), so behind the sums there is arithmetic and three stores, no memory round trip.
struct AdamLoaded { float p, m, v; };
__device__ __forceinline__ AdamLoaded adam_load(const float *p, const float *m, const float *v) {
    AdamLoaded r;
    r.p = *p; r.m = *m; r.v = *v;
    return r;
}
__device__ __forceinline__ void adam_update(float *p, float g, float *m, float *v, const AdamLoaded &ld, float lr,
                                            float step_size_base, float bc2s, float beta1, float beta2,
                                            float eps, float weight_decay = 0.f) {
    (void)lr;
    if (weight_decay != 0.f) g = g + weight_decay * ld.p;   // torch.optim.Adam: grad.add(param, alpha=weight_decay)
    float mm = ld.m, vv = ld.v;
    mm = mm + (g - mm) * (1.0f - beta1);
    vv = vv * beta2 + ((1.0f - beta2) * g) * g;
    const float denom = sqrtf(vv) / bc2s + eps;
    *m = mm; *v = vv;
    *p = ld.p - step_size_base * (mm / denom);
}

__device__ __forceinline__ void base_bwd_finalize_body(const BaseBwdArgs &a, const FinalizeAdam &ad) {
    // Every output is summed over the partial rows by FOUR lanes, a quarter of the rows each (one batch of loads in
    // flight per lane at 128 rows instead of four dependent batches), combined in a fixed order by two xor-shuffles.
    // Everything else a lane needs from memory -- the step sizes of this step, the parameter it updates with its
    // two moments, the 6-vector of the Gram-Schmidt backward -- is independent of the gradient and is loaded IN FRONT of
    // the partial rows, so the whole body is one memory round trip deep.  The step sizes come ready-made (lr / bias
    // correction, divided once in double by whoever wrote ad.step): behind the sums a lane has single-precision
    // arithmetic only.
    const int og = blockIdx.x * 256 + threadIdx.x;
    const int nWr = a.P * a.H + 4 * a.H;                 // real weight entries
    const int nW = (4 * nWr + 63) & ~63;                 // four lanes per weight; pose groups start wave-aligned
    const int RQ = (a.nchunk + 3) >> 2;                  // rows per quarter
    const int o = og >> 2;                               // weight entry of this lane (first branch)
    const int no = n_out(a.P, a.H, a.B);
    // step sizes of THIS step: written by prepare or the previous bookkeeping workgroup, promoted by the block launch
    float ss_seg = 0.f, ss_tr = 0.f, bc2s = 1.f;
    if (ad.enabled) { ss_seg = ad.step[0]; ss_tr = ad.step[1]; bc2s = ad.step[2]; }
    if (og < nW) {
        if (o >= nWr) return;                            // whole quads leave together
        // partial-row order is W2 | W1 | b1; moment order is W1 | b1 | W2
        const int nW2 = a.P * a.H, nW1 = 3 * a.H;
        const int kind = o < nW2 ? 0 : (o < nW2 + nW1 ? 1 : 2);
        const int q = kind == 0 ? o : (kind == 1 ? o - nW2 : o - nW2 - nW1);          // entry inside its tensor
        const int mo = kind == 0 ? nW1 + a.H + q : (kind == 1 ? q : nW1 + q);         // entry inside the moments
        // (a branch per tensor, not a per-lane choice between the three pointers: that the compiler turns into a per-lane
        // LOAD of the chosen pointer from the argument block, a round trip in front of the load it is for)
        AdamLoaded ld = {0.f, 0.f, 0.f};
        if (ad.enabled) {                                // all four lanes of the quad: one address
            if (kind == 0) ld.p = ad.W2[q];
            else if (kind == 1) ld.p = ad.W1[q];
            else ld.p = ad.b1[q];
            ld.m = ad.m[mo]; ld.v = ad.v[mo];
        }
        float acc = 0.f;
        int c = (og & 3) * RQ;
        const int cend = c + RQ < a.nchunk ? c + RQ : a.nchunk;
        for (; c + 32 <= cend; c += 32) {  // 32 independent loads in flight, fixed add order
            float v[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) v[u] = a.partial[(size_t)(c + u) * no + o];
#pragma unroll
            for (int u = 0; u < 32; ++u) acc += v[u];
        }
        for (; c + 8 <= cend; c += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = a.partial[(size_t)(c + u) * no + o];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
        }
        for (; c < cend; ++c) acc += a.partial[(size_t)c * no + o];
        acc = acc + __shfl_xor(acc, 1, 64);              // (q0 + q1), (q2 + q3): commutative, every lane of the quad agrees
        acc = acc + __shfl_xor(acc, 2, 64);
        if (og & 3) return;
        if (kind == 0) {
            a.gW2[q] = acc;
            if (ad.enabled) adam_update(ad.W2 + q, acc, ad.m + mo, ad.v + mo, ld, ad.seg_lr, ss_seg, bc2s, ad.beta1, ad.beta2, ad.eps, ad.weight_decay);
        } else if (kind == 1) {
            a.gW1[q] = acc;
            if (ad.enabled) adam_update(ad.W1 + q, acc, ad.m + mo, ad.v + mo, ld, ad.seg_lr, ss_seg, bc2s, ad.beta1, ad.beta2, ad.eps, ad.weight_decay);
        } else {
            a.gb1[q] = acc;
            if (ad.enabled) adam_update(ad.b1 + q, acc, ad.m + mo, ad.v + mo, ld, ad.seg_lr, ss_seg, bc2s, ad.beta1, ad.beta2, ad.eps, ad.weight_decay);
        }
    } else if (og < nW + 64 * a.B * a.P) {
        // one wave per (frame, part): 4 row quarters x 16 lanes; lane c < 12 of a quarter sums one entry of dL/d[R|t]
        // over its rows (all its loads in flight at once), the quarters meet through two xor-shuffles, then every
        // 16-lane group holds the 12 sums and runs the Gram-Schmidt backward; the first group updates the parameters
        const int q = og - nW, e = q >> 6, tq = (q >> 4) & 3, c = q & 15;
        // lane c < 6 owns rotation entry c, lanes 6..8 the translation entries (the others repeat lane 8's addresses:
        // loaded, never stored)
        const int base6 = 3 * a.H + a.H + a.P * a.H, baset = base6 + 6 * a.B * a.P;
        const int k = c < 6 ? c : (c < 9 ? c - 6 : 2);
        const int mo = c < 6 ? base6 + 6 * e + k : baset + 3 * e + k;
        float *const pp = c < 6 ? ad.p6d + 6 * (size_t)e + k : ad.pt + 3 * (size_t)e + k;
        float d6[6];
#pragma unroll
        for (int u = 0; u < 6; ++u) d6[u] = a.p6d[6 * (size_t)e + u];
        AdamLoaded ld = {0.f, 0.f, 0.f};
        if (ad.enabled) ld = adam_load(pp, ad.m + mo, ad.v + mo);
        float acc = 0.f;
        if (c < 12) {
            const float *pr = a.partial + off_gRt(a.P, a.H) + 12 * (size_t)e + c;
            int ch = tq * RQ;
            const int chend = ch + RQ < a.nchunk ? ch + RQ : a.nchunk;
            for (; ch + 32 <= chend; ch += 32) {
                float v[32];
#pragma unroll
                for (int u = 0; u < 32; ++u) v[u] = pr[(size_t)(ch + u) * no];
#pragma unroll
                for (int u = 0; u < 32; ++u) acc += v[u];
            }
            for (; ch < chend; ++ch) acc += pr[(size_t)ch * no];
        }
        acc = acc + __shfl_xor(acc, 16, 64);
        acc = acc + __shfl_xor(acc, 32, 64);
        float gRt[12];
        const int lane0 = (threadIdx.x & 63) & ~15;
#pragma unroll
        for (int u = 0; u < 12; ++u) gRt[u] = __shfl(acc, lane0 + u, 64);
        // every lane of the group runs the (cheap) Gram-Schmidt backward; lane c < 6 then owns rotation
        // entry c and lanes 6..8 the translation entries: nine independent Adam updates instead of a
        // chain of nine on one lane
        if (c >= 9 || tq != 0) return;
        float g6[6];
        r6d_backward(d6, gRt, g6);
        float g;
        if (c < 6) {
            g = g6[0];
#pragma unroll
            for (int u = 1; u < 6; ++u) g = (c == u) ? g6[u] : g;
            a.g6d[6 * (size_t)e + c] = g;
        } else {
            g = k == 0 ? gRt[9] : (k == 1 ? gRt[10] : gRt[11]);
            a.gt[3 * (size_t)e + k] = g;
        }
        if (ad.enabled) adam_update(pp, g, ad.m + mo, ad.v + mo, ld, ad.trans_lr, ss_tr, bc2s, ad.beta1, ad.beta2, ad.eps, ad.weight_decay);
    }
}

// End-of-iteration bookkeeping of the fused step, run by ONE workgroup of the finalize launch (the extra, last one) beside
// the body workgroups: nothing it writes is read by any of them (StepBook, internal.h), so nobody waits for anybody.  The
// four waves share the work -- wave 0 sums the loss partials, lane 0 of waves 1 / 2 / 3 evaluates one double-precision
// chain each (pow and the two step sizes | pow and sqrt | the cosine of the next temperature; on ONE lane they took 2.2 us,
// profiles/r05_small_kernel_clocks.txt) -- and each stores what it computed.  The one barrier stands between the reads of
// `iter` and `tau` (every wave) and their stores.
__device__ __forceinline__ void base_bwd_finalize_book(const StepBook &bk) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#ifdef REART_PHASE_CLOCK
    if (blockIdx.y == 0 && threadIdx.x == 0) g_phase_ts[0][10] = __builtin_amdgcn_s_memtime();
#endif
    const long it = (long)bk.iter[0];
    const float tau_cur = bk.tau[0];
    double recon = 0.0, flow = 0.0, ass = 0.0, bc = 1.0;
    float tau_next = 0.f;
    if (w == 0) {
        // fixed assignment of terms to lanes + fixed-order tree: deterministic sums
        for (int b = l; b < bk.n_frame_part; b += 64) recon += bk.frame_loss[b];
        for (int i = l; i < bk.n_flow_part; i += 64) flow += bk.flow_part[i];
        recon = reart_wave_sum_d(recon);
        flow = reart_wave_sum_d(flow) * (double)bk.lambda_flow;
        if (bk.n_assign_part > 0) {   // recon_with_assign: the assignment term on top of the Chamfer term (wave-uniform branch)
            for (int b = l; b < bk.n_assign_part; b += 64) ass += bk.assign_part[b];
            ass = reart_wave_sum_d(ass);
            recon += ass;
        }
    } else if (l == 0) {
        // Adam step count of the next iteration: it + 2
        if (w == 1) bc = 1.0 - pow((double)bk.beta1, (double)(it + 2));
        else if (w == 2) bc = sqrt(1.0 - pow((double)bk.beta2, (double)(it + 2)));
        // iteration i (0-based) uses tau_cosine(i+1, ...) (run_robot.py:157)
        else tau_next = bk.fixed_tau > 0.f ? bk.fixed_tau : reart_tau_schedule(it + 2, bk.n_iter, bk.end_tau, bk.start_tau);
    }
    __syncthreads();
    if (l == 0) {
        float *row = (bk.losses && bk.ring > 0) ? bk.losses + 4 * (size_t)(it % bk.ring) : nullptr;
        if (w == 0) {
            if (row) { row[0] = (float)recon; row[1] = (float)flow; row[2] = (float)(recon + flow); }
            if (bk.losses_assign && bk.ring > 0) bk.losses_assign[it % bk.ring] = (float)ass;
        } else if (w == 1) {
            bk.step_next[0] = (float)((double)bk.seg_lr / bc);
            bk.step_next[1] = (float)((double)bk.trans_lr / bc);
            bk.iter[0] = it + 1;
        } else if (w == 2) {
            bk.step_next[2] = (float)bc;
        } else {
            if (row) row[3] = tau_cur;     // the temperature this iteration used
            bk.tau[0] = tau_next;
        }
    }
#ifdef REART_PHASE_CLOCK
    __syncthreads();   // diagnostic build only: the stamp is the slowest wave's end
    if (blockIdx.y == 0 && threadIdx.x == 0) g_phase_ts[0][14] = __builtin_amdgcn_s_memtime();
#endif
}

// 256 threads of column sums / pose gradients / Adam (base_bwd_finalize_body): no LDS, no barrier, no atomic.  With a step
// book the grid has one workgroup more, the last, which runs base_bwd_finalize_book instead.
template <bool BATCH>
__global__ __launch_bounds__(256) void base_bwd_finalize_kernel(Batched<BaseBwdArgs> ab, Batched<FinalizeAdam> adb, Batched<StepBook> bkb) {
    const StepBook &bk = bkb.a[BATCH ? blockIdx.y : 0];
    if (bk.enabled && blockIdx.x == gridDim.x - 1) { base_bwd_finalize_book(bk); return; }
    const BaseBwdArgs &a = ab.a[BATCH ? blockIdx.y : 0];
    const FinalizeAdam &ad = adb.a[BATCH ? blockIdx.y : 0];
#ifdef REART_PHASE_CLOCK
    if (blockIdx.x == 1 && blockIdx.y == 0 && threadIdx.x == 0) g_phase_ts[0][8] = __builtin_amdgcn_s_memtime();
#endif
    base_bwd_finalize_body(a, ad);
#ifdef REART_PHASE_CLOCK
    if (blockIdx.x == 1 && blockIdx.y == 0 && threadIdx.x == 0) g_phase_ts[0][9] = __builtin_amdgcn_s_memtime();
#endif
}

// offsets, not pointers: the K instances of a launch carve the same layout out of K workspaces
struct BaseBwdWs { size_t o_rt, o_part; };
static size_t base_bwd_ws_layout(int N, int P, int B, int H, BaseBwdWs *w) {
    const int nchunk = reart_div_up(N, 16);   // room for the 16-point form (four times the partial rows of the 64-point form)
    reart_arena ws;
    w->o_rt = ws.take_bytes(sizeof(float) * 12 * (size_t)B * P);
    w->o_part = ws.take_bytes(sizeof(float) * (size_t)nchunk * n_out(P, H, B));
    return ws.off;
}

extern "C" size_t reart_base_backward_workspace_bytes(int N, int P, int B, int H) {
    BaseBwdWs w;
    return (N <= 0 || P <= 0 || B <= 0 || H <= 0) ? 0 : base_bwd_ws_layout(N, P, B, H, &w);
}

template <int PP>
static int launch_bwd_block(const BaseBwdArgs *ak, int K, size_t lds, hipStream_t st) {
    if (lds > REART_LDS_DEFAULT_CAP &&
        (hipFuncSetAttribute((const void *)base_bwd_block_kernel<PP, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024) != hipSuccess ||
         hipFuncSetAttribute((const void *)base_bwd_block_kernel<PP, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024) != hipSuccess))
        return REART_ERR_LAUNCH;
    if (K == 1) hipLaunchKernelGGL((base_bwd_block_kernel<PP, false>), dim3(ak[0].nchunk), dim3(64 * BW_WAVES), lds, st, reart_batched(ak, 1));
    else hipLaunchKernelGGL((base_bwd_block_kernel<PP, true>), dim3(ak[0].nchunk, K), dim3(64 * BW_WAVES), lds, st, reart_batched(ak, K));
    return REART_OK;
}

// The backward's one entry: K instances of one shape (K = 1: the C ABI below and the single fused step); workspaces[k] is
// instance k's backward workspace.  a.rt_table == NULL: the table is built into the workspace first (one extra tiny launch
// per instance)
int reart_base_backward_launch(const BaseBwdArgs *args, const FinalizeAdam *adam, const StepBook *book, void *const *workspaces,
                               size_t workspace_bytes, int K, hipStream_t st, int force_long) {
    if (K < 1 || K > REART_BATCH_MAX) return REART_ERR_INVALID_ARG;
    BaseBwdArgs ak[REART_BATCH_MAX];
    for (int k = 0; k < K; ++k) ak[k] = args[k];
    const BaseBwdArgs &a0 = ak[0];
    if (a0.P > 32) return REART_ERR_UNSUPPORTED;
    BaseBwdWs w;
    const size_t need = base_bwd_ws_layout(a0.N, a0.P, a0.B, a0.H, &w);
    if (!workspaces || workspace_bytes < need) return REART_ERR_INVALID_ARG;
    for (int k = 0; k < K; ++k) {
        BaseBwdArgs &a = ak[k];
        a.cpts = (a.cpts == 64 || a.cpts == 32 || a.cpts == 16) ? a.cpts : 32;   // points per backward workgroup
        a.nchunk = reart_div_up(a.N, a.cpts);
        if (a.N != a0.N || a.P != a0.P || a.B != a0.B || a.H != a0.H || a.cpts != a0.cpts || !workspaces[k]) return REART_ERR_INVALID_ARG;
        if (!a.hT && (!a.W1 || !a.b1)) return REART_ERR_INVALID_ARG;   // no saved hidden layer: it is re-evaluated from W1 | b1
        char *ws = (char *)workspaces[k];
        a.partial = (float *)(ws + w.o_part);
        if (!a.rt_table) {
            float *table = (float *)(ws + w.o_rt);
            hipLaunchKernelGGL(rt_table_kernel, dim3(reart_div_up(a.B * a.P, 256)), dim3(256), 0, st, a.p6d, a.pt,
                               a.B * a.P, table);
            a.rt_table = table;
        }
    }
    const int path = reart_base_path(a0.P, a0.B, a0.H, 1);
    if (path < 0) return path;
    int rc;
    if (path == 1 || force_long) {
        for (int k = 0; k < K; ++k)
            if (!ak[k].hT) return REART_ERR_UNSUPPORTED;                             // the long kernels read the saved hT
        rc = reart_base_backward_long_launch(ak, K, st);                             // the partial rows in frame tiles
    } else {
        size_t lds = base_bwd_lds(a0.P, a0.B, a0.H);
        // the hidden gradient gets a tile of its own ([H][cpts + 1]) where it fits: then the tail's roles overlap
        const size_t lds_dp = sizeof(float) * (size_t)a0.H * (a0.cpts + 1);
        const int dp_sep = lds + lds_dp <= 152 * 1024;
        if (dp_sep) lds += lds_dp;
        for (int k = 0; k < K; ++k) ak[k].dp_sep = dp_sep;
        switch (a0.P) {
            case 20: rc = launch_bwd_block<20>(ak, K, lds, st); break;
            case 10: rc = launch_bwd_block<10>(ak, K, lds, st); break;
            case 8: rc = launch_bwd_block<8>(ak, K, lds, st); break;
            default: rc = launch_bwd_block<0>(ak, K, lds, st); break;
        }
    }
    if (rc != REART_OK) return rc;
    Batched<FinalizeAdam> adb = {};
    Batched<StepBook> bkb = {};
    static_assert(sizeof(Batched<BaseBwdArgs>) + sizeof(adb) + sizeof(bkb) <= 3584, "kernel-argument segment");
    for (int k = 0; k < K; ++k) {
        if (adam) adb.a[k] = adam[k];
        if (book) bkb.a[k] = book[k];
    }
    // weights: one thread per entry; poses: 16 lanes per (frame, part); nW is rounded up to a multiple of 64
    // inside the kernel's indexing so that a 16-lane group never straddles a wave
    const int nfin = (int)reart_align_up((size_t)4 * (a0.P * a0.H + 4 * a0.H), 64) + 64 * a0.B * a0.P;
    // + the bookkeeping workgroup, in every instance plane or in none
    int nbook = 0;
    for (int k = 0; k < K; ++k) nbook += bkb.a[k].enabled ? 1 : 0;
    if (nbook != 0 && nbook != K) return REART_ERR_INVALID_ARG;
    const int nwg = reart_div_up(nfin, 256) + (nbook ? 1 : 0);
    if (K == 1) hipLaunchKernelGGL(base_bwd_finalize_kernel<false>, dim3(nwg), dim3(256), 0, st, reart_batched(ak, 1), adb, bkb);
    else hipLaunchKernelGGL(base_bwd_finalize_kernel<true>, dim3(nwg, K), dim3(256), 0, st, reart_batched(ak, K), adb, bkb);
    REART_CHECK_LAUNCH();
    return REART_OK;
}

extern "C" int reart_base_backward(const float *cano, int N, int P, int B, const float *W1,
                                   const float *b1, const float *W2, int H, const float *prop6d,
                                   const float *propt, const float *yT, const float *hT,
                                   const int32_t *hard_idx, float tau, const float *G, float *gW1,
                                   float *gb1, float *gW2, float *g6d, float *gt, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    if (N <= 0 || P < 1 || B <= 0 || H < 1) return REART_ERR_INVALID_ARG;
    if (!cano || !W2 || !prop6d || !propt || !yT || !hard_idx || !G || !gW1 || !gb1 || !gW2 ||
        !g6d || !gt)
        return REART_ERR_INVALID_ARG;
    if (!hT && (!W1 || !b1)) return REART_ERR_INVALID_ARG;   // hT == NULL: the hidden layer is re-evaluated from W1 | b1
    BaseBwdArgs a = {};
    a.cano = cano; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.p6d = prop6d; a.pt = propt; a.yT = yT; a.hT = hT;
    a.hard_idx = hard_idx; a.tau = tau; a.G = G; a.N = N; a.P = P; a.B = B; a.H = H;
    a.gW1 = gW1; a.gb1 = gb1; a.gW2 = gW2; a.g6d = g6d; a.gt = gt;
    return reart_base_backward_launch(&a, nullptr, nullptr, &workspace, workspace_bytes, 1, (hipStream_t)stream, 0);
}

// --------------------------------------------------------------- hard-label rigid apply
// utils/model_utils.py:54-67 (compute_pc_transform) and the apply in KinematicModel.forward
// (networks/model.py:161-165): out[t,n] = R[t,part_n] x_n + t[t,part_n], pose [B,P,4,4].
__global__ __launch_bounds__(256) void pc_transform_kernel(const float *__restrict__ cano,
                                                           const float *__restrict__ pose,
                                                           const int64_t *__restrict__ part, int N,
                                                           int P, int B, float *__restrict__ out) {
    const int n = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (n >= N) return;
    const float *T = pose + 16 * ((size_t)t * P + part[n]);
    const float x0 = cano[3 * (size_t)n], x1 = cano[3 * (size_t)n + 1], x2 = cano[3 * (size_t)n + 2];
    float *o = out + 3 * ((size_t)t * N + n);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float acc = x0 * T[4 * c];
        acc = fmaf(x1, T[4 * c + 1], acc);
        acc = fmaf(x2, T[4 * c + 2], acc);
        o[c] = acc + T[4 * c + 3];
    }
}

extern "C" int reart_compute_pc_transform(const float *cano, const float *pose, const int64_t *part,
                                          int N, int P, int B, float *out, void *stream) {
    if (N < 0 || P < 1 || B < 0) return REART_ERR_INVALID_ARG;
    if (N == 0 || B == 0) return REART_OK;
    if (!cano || !pose || !part || !out) return REART_ERR_INVALID_ARG;
    hipLaunchKernelGGL(pc_transform_kernel, dim3(reart_div_up(N, 256), B), dim3(256), 0,
                       (hipStream_t)stream, cano, pose, part, N, P, B, out);
    REART_CHECK_LAUNCH();
    return REART_OK;
}

extern "C" int reart_rotation_6d_to_matrix(const float *d6, int n, float *R, void *stream);
__global__ __launch_bounds__(256) void r6d_kernel(const float *__restrict__ d6, int n, float *__restrict__ R) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float r[9];
    r6d_to_matrix(d6 + 6 * (size_t)i, r);
#pragma unroll
    for (int c = 0; c < 9; ++c) R[9 * (size_t)i + c] = r[c];
}
extern "C" int reart_rotation_6d_to_matrix(const float *d6, int n, float *R, void *stream) {
    if (n < 0) return REART_ERR_INVALID_ARG;
    if (n == 0) return REART_OK;
    if (!d6 || !R) return REART_ERR_INVALID_ARG;
    hipLaunchKernelGGL(r6d_kernel, dim3(reart_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, d6, n, R);
    REART_CHECK_LAUNCH();
    return REART_OK;
}

// ------------------------------------------------------------------------------- Adam
// torch.optim.Adam single-tensor step (amsgrad off, weight_decay 0), up to 8 tensors per
// launch.  `step_ptr` (device int64, nullable) holds the number of steps ALREADY taken, so
// a captured graph needs no per-iteration host argument.

__global__ __launch_bounds__(256) void adam_kernel(AdamArgs a) {
    const AdamSeg s = a.seg[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= s.n) return;
    const int step = a.step_ptr ? (int)a.step_ptr[0] + 1 : a.step;
    const double bc1 = 1.0 - pow((double)a.beta1, (double)step);
    const double bc2 = 1.0 - pow((double)a.beta2, (double)step);
    const float step_size = (float)((double)s.lr / bc1);
    const float bc2s = (float)sqrt(bc2);
    const float g = s.g[i];
    float m = s.m[i], v = s.v[i];
    m = m + (g - m) * (1.0f - a.beta1);
    v = v * a.beta2 + ((1.0f - a.beta2) * g) * g;
    const float denom = sqrtf(v) / bc2s + a.eps;
    s.m[i] = m; s.v[i] = v;
    s.p[i] = s.p[i] - step_size * (m / denom);
}

int reart_adam_ex(const AdamArgs &a, hipStream_t st) {
    int maxn = 0;
    for (int k = 0; k < a.nseg; ++k) maxn = a.seg[k].n > maxn ? a.seg[k].n : maxn;
    if (maxn == 0) return REART_OK;
    hipLaunchKernelGGL(adam_kernel, dim3(reart_div_up(maxn, 256), a.nseg), dim3(256), 0, st, a);
    REART_CHECK_LAUNCH();
    return REART_OK;
}

// reart_adam_step for up to 8 tensors in ONE launch (the pointer and size arrays are host arrays, read at the call): the three
// parameter tensors of the kinematic model were three launches, each a 5 us slot of the iteration whatever its size.
extern "C" int reart_adam_step_multi(int count, float *const *param, const float *const *grad, float *const *exp_avg,
                                     float *const *exp_avg_sq, const int *n, const float *lr, int step, float beta1, float beta2,
                                     float eps, void *stream) {
    if (count < 0 || count > 8 || step < 1) return REART_ERR_INVALID_ARG;
    if (count == 0) return REART_OK;
    if (!param || !grad || !exp_avg || !exp_avg_sq || !n || !lr) return REART_ERR_INVALID_ARG;
    AdamArgs a = {};
    for (int k = 0; k < count; ++k) {
        if (n[k] < 0) return REART_ERR_INVALID_ARG;
        if (n[k] > 0 && (!param[k] || !grad[k] || !exp_avg[k] || !exp_avg_sq[k])) return REART_ERR_INVALID_ARG;
        a.seg[k] = {param[k], grad[k], exp_avg[k], exp_avg_sq[k], n[k], lr[k]};
    }
    a.nseg = count; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.step = step;
    return reart_adam_ex(a, (hipStream_t)stream);
}

extern "C" int reart_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                               int n, int step, float lr, float beta1, float beta2, float eps,
                               void *stream) {
    if (n < 0 || step < 1) return REART_ERR_INVALID_ARG;
    if (n == 0) return REART_OK;
    if (!param || !grad || !exp_avg || !exp_avg_sq) return REART_ERR_INVALID_ARG;
    AdamArgs a = {};
    a.seg[0] = {param, grad, exp_avg, exp_avg_sq, n, lr};
    a.nseg = 1; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.step = step;
    return reart_adam_ex(a, (hipStream_t)stream);
}
