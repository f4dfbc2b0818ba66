// reart_amd/csrc/chamfer_loss.hip -- the bidirectional K = 1 Chamfer sum of networks/loss.py:24-29 with its gradient as
// ONE warm-started C-ABI call (reart_chamfer_loss):
//   soa_kernel + box_kernel   SoA images and 16-target boxes of x (every call) and of y (unless the caller says y is unchanged)
//   search                    both directions in ONE reart_search_launch (SearchArgs.k1[0..1], n1 = 2): exact, box-pruned,
//                             bounded by the seeds of the previous call (prune.hip, unchanged)
//   chamfer_loss_kernel       the consumer below: distances, indices, next seeds, the loss and the complete gradients
// The consumer uses the technique of the fused step's chamfer_grad_body (step.hip): a workgroup owns a range of
// targets, walks the records of the OTHER cloud and adds the differences of the points that chose one of its targets into
// 64-bit fixed-point sums in LDS by integer atomics -- exact to one quantum per addend and independent of the order of
// arrival, so the gradient is deterministic without a sort, there is no floating-point atomic and no global accumulator.
// The fixed-point conversion, the block sum and the last workgroup's sum are the step's own (consumer_dev.h).  The walk is
// not: the step's merges slice partials over a 1024-target range and captures its own d1; here P1 != P2, there is a
// gradient for y, a fixed-point scale per batch element taken from the boxes the prep has just computed, and the loss is
// reduced inside the same launch by the last workgroup to finish.
// Clouds of differing lengths in one padded batch (the _ragged entries; the dense ones are these with both lengths NULL): the
// targets' lengths go to the prep and the search (SoaJob.len, KnnJob.tlen), the queries are staged once per call
// (chamfer_stage_kernel), and the consumers treat rows beyond a length as padding (cl_len).
#include "common.h"
#include "internal.h"
#include "consumer_dev.h"
#include <math.h>
#include <type_traits>

#define CL_BS 256        // threads per consumer workgroup = targets it owns
#define CL_IL 4          // records of the other cloud in flight per thread

struct ChamferLossPlan {
    int S, Ppad1, Ppad2, nqg, nr1, nr2, nparts;
    size_t o_xsoa, o_ysoa, o_xbox, o_ybox, o_pd0, o_pi0, o_pd1, o_pi1, o_part, o_ticket, total;
    size_t o_xq, o_yq, o_len64, o_len32;     // ragged entries only, behind the dense layout
};
// ragged: the layout of the _ragged entries -- the dense one (same offsets: an image of y serves both) followed by the staged
// query images and the clamped lengths
static int chamfer_loss_plan(int N, int P1, int P2, ChamferLossPlan *p, bool ragged = false) {
    if (N < 0 || N > 65535 || P1 < 0 || P2 < 0) return REART_ERR_INVALID_ARG;   // N is a grid dimension
    // record and gradient offsets are 64-bit, the per-batch products below stay in int
    if ((long long)N * ((long long)(P1 > P2 ? P1 : P2) + 2 * CL_BS) >= (1ll << 30)) return REART_ERR_INVALID_ARG;
    const int Pmin = P1 < P2 ? P1 : P2;
    p->S = 4;                                                    // waves per search workgroup: as reart_knn_points_idx_warm,
    while (p->S > 1 && reart_div_up(Pmin, p->S) < 64) p->S -= 1; // from the smaller of the two target clouds (one S per launch)
    p->Ppad1 = (int)reart_align_up((size_t)(P1 > 0 ? P1 : 1), NN_BOX);
    p->Ppad2 = (int)reart_align_up((size_t)(P2 > 0 ? P2 : 1), NN_BOX);
    const int q1 = reart_div_up(P1, NN_BS), q2 = reart_div_up(P2, NN_BS);
    p->nqg = q1 > q2 ? q1 : q2;
    p->nr1 = reart_div_up(P1, CL_BS); p->nr2 = reart_div_up(P2, CL_BS);
    p->nparts = N * (p->nr1 + p->nr2);
    reart_arena ws;
    p->o_xsoa = ws.take_bytes(sizeof(float) * 3 * (size_t)N * p->Ppad1);
    p->o_ysoa = ws.take_bytes(sizeof(float) * 3 * (size_t)N * p->Ppad2);
    p->o_xbox = ws.take_bytes(sizeof(float) * 8 * (size_t)N * (p->Ppad1 / NN_BOX));
    p->o_ybox = ws.take_bytes(sizeof(float) * 8 * (size_t)N * (p->Ppad2 / NN_BOX));
    p->o_pd0 = ws.take_bytes(sizeof(float) * (size_t)N * P1);
    p->o_pi0 = ws.take_bytes(sizeof(int) * (size_t)N * P1);
    p->o_pd1 = ws.take_bytes(sizeof(float) * (size_t)N * P2);
    p->o_pi1 = ws.take_bytes(sizeof(int) * (size_t)N * P2);
    p->o_part = ws.take_bytes(sizeof(double) * (size_t)(p->nparts > 0 ? p->nparts : 1));
    p->o_ticket = ws.take_bytes(sizeof(unsigned int));
    p->o_xq = p->o_yq = p->o_len64 = p->o_len32 = 0;
    if (ragged) {
        p->o_xq = ws.take_bytes(sizeof(float) * 3 * (size_t)N * P1);
        p->o_yq = ws.take_bytes(sizeof(float) * 3 * (size_t)N * P2);
        p->o_len64 = ws.take_bytes(sizeof(int64_t) * 2 * (size_t)N);
        p->o_len32 = ws.take_bytes(sizeof(int) * 2 * (size_t)N);
    }
    p->total = ws.off;
    return REART_OK;
}

// ---- what the two gradient kernels below (chamfer_loss_kernel, chamfer_points_bwd_kernel) share.  A workgroup (r, n) of
// cloud d owns the points r0 = r * CL_BS .. of cloud d ("own", Pw points) of batch element n; the other cloud has Po points.

// Ragged batches: live points of cloud d of batch element n = len[d][n] clamped into [0, P] (uniform; NULL: all P).  Every
// kernel below takes it as "Lw" (own cloud) and "Lo" (other cloud): rows beyond it are padding, which is never read as a
// coordinate, an index or an upstream, and is written as distance 0, index 0, seed -1, gradient 0.
__device__ __forceinline__ int cl_len(const int *len, int n, int P) {
    const int l = len ? len[n] : P;
    return l < 0 ? 0 : (l > P ? P : l);
}

// largest of the threads' values over the workgroup (fmaxf drops NaN); contains one barrier
__device__ __forceinline__ float cl_block_max(float mx, float *s_mx) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
    if ((threadIdx.x & 63) == 0) s_mx[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = s_mx[0];
#pragma unroll
    for (int w = 1; w < CL_BS / REART_WAVE; ++w) mx = fmaxf(mx, s_mx[w]);
    return mx;
}

// The walk over ALL points j of the other cloud: one whose neighbour io[j] is an own point of this workgroup adds
// fl(own - other_j), times its upstream gradient gg[j] where gg is given (uniform; a zero adds nothing: a masked point), to
// that point's fixed-point sum in LDS.  Idx: int records of the search or int64 indices of a caller.  An index is used only
// if it is in range of the own cloud AND of this workgroup's targets, else there is no access at all.
template <class Idx>
__device__ __forceinline__ void cl_scatter_walk(const float *own, const float *oth, const Idx *io, const float *gg, int Pw, int Po,
                                                int r0, int sbits, unsigned long long *s_acc) {
    typedef typename std::make_unsigned<Idx>::type U;
    for (int jb = threadIdx.x; jb < Po; jb += CL_IL * CL_BS) {
        int jl[CL_IL];
#pragma unroll
        for (int u = 0; u < CL_IL; ++u) {
            const int j = jb + u * CL_BS;
            const Idx t = io[j < Po ? j : Po - 1];
            jl[u] = (j < Po && (U)t < (U)Pw && (U)(t - r0) < (U)CL_BS) ? (int)(t - r0) : -1;
        }
#pragma unroll
        for (int u = 0; u < CL_IL; ++u) {
            if (jl[u] < 0) continue;
            const int j = jb + u * CL_BS;
            const float gj = gg ? gg[j] : 1.0f;
            if (gg && gj == 0.0f) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float df = own[3 * (size_t)(r0 + jl[u]) + k] - oth[3 * (size_t)j + k];
                atomicAdd(&s_acc[3 * jl[u] + k], (unsigned long long)reart_fixed_from_float(gg ? gj * df : df, sbits));
            }
        }
    }
}

// gradient of the thread's own point: its own term + 2 * (fixed-point sum)
__device__ __forceinline__ void cl_grad_store(float *G, const float (&first)[3], const unsigned long long *s_acc, int sbits) {
    const double inv2 = 2.0 * exp2((double)-sbits);
#pragma unroll
    for (int k = 0; k < 3; ++k) G[k] = first[k] + (float)((double)(long long)s_acc[3 * threadIdx.x + k] * inv2);
}

struct ChamferLossArgs {
    const float *c[2];          // the clouds [N,P[d],3]: 0 = x, 1 = y
    const float *box[2];        // their boxes [N][Ppad[d]/NN_BOX][8]
    const float *pd[2];         // search records of cloud d's points against the other cloud [N,P[d]]
    const int *pi[2];
    int P[2], nbox[2], nr[2];   // points, boxes and consumer ranges per batch element
    const int *len[2];          // nullable [N]: live points of cloud d (cl_len)
    float *od[2];               // nullable outputs [N,P[d]]
    int64_t *oi[2];
    int *seed[2];               // [N,P[d]] next seeds
    float *grad[2];             // [N,P[d],3]; grad[1] nullable
    int *bits;                  // [N] fractional bits of the fixed-point sums of batch element n
    double *part;               // [N * (nr[0] + nr[1])] loss partials
    unsigned int *ticket;       // zeroed in front of every launch
    float *loss;
    int N;
};

// Workgroup (r, n) of direction d owns the points r*CL_BS .. of cloud d ("own") of batch element n; o = 1 - d is the other cloud.
//   1. scale: the largest |coordinate| of both clouds of the batch element, from their boxes
//   2. own record: distance, index and next seed of its points, the loss terms, the first gradient term
//   3. walk over ALL records of the other cloud: a point whose neighbour is one of its own adds (own - other) to that
//      point's fixed-point sum in LDS
//   4. gradient; loss partial; the last workgroup of the launch adds all partials in index order in double, rounds once
// Every index read from a record is range-checked before it addresses memory.
__global__ __launch_bounds__(CL_BS) void chamfer_loss_kernel(ChamferLossArgs a) {
    __shared__ unsigned long long s_acc[CL_BS * 3];
    __shared__ double s_red[CL_BS / REART_WAVE];
    __shared__ float s_mx[CL_BS / REART_WAVE];
    __shared__ int s_last;
    const int tid = threadIdx.x, n = blockIdx.y;
    const int d = (int)blockIdx.x < a.nr[0] ? 0 : 1, o = 1 - d;
    const int r = (int)blockIdx.x - (d ? a.nr[0] : 0);
    const int Pw = a.P[d], Po = a.P[o];
    const float *own = a.c[d] + (size_t)n * Pw * 3, *oth = a.c[o] + (size_t)n * Po * 3;
    const bool want = a.grad[d] != nullptr;      // uniform
    for (int e = tid; e < CL_BS * 3; e += CL_BS) s_acc[e] = 0ull;
    // ---- 1. largest finite |coordinate| of the batch element (fmaxf drops NaN; +INF padding sides are skipped)
    float mx = 0.f;
    for (int q = 0; q < 2; ++q) {
        const float *bx = a.box[q] + (size_t)n * a.nbox[q] * 8;
        for (int e = tid; e < a.nbox[q] * 8; e += CL_BS) {
            const float v = fabsf(bx[e]);
            if ((e & 7) < 6 && v < INFINITY) mx = fmaxf(mx, v);
        }
    }
    // ---- 2. own record (a padding row reads the last live row's, and uses none of it)
    const int Lw = cl_len(a.len[d], n, Pw), Lo = cl_len(a.len[o], n, Po);      // uniform
    const int i = r * CL_BS + tid;
    const bool live = i < Lw;
    const int ic = live ? i : (Lw > 0 ? Lw - 1 : 0);
    const size_t ow = (size_t)n * Pw + ic;
    float d0 = a.pd[d][ow];
    int j0 = a.pi[d][ow];
    const bool ok0 = live && (unsigned)j0 < (unsigned)Lo;
    d0 = ok0 ? d0 : 0.0f;
    const int j0c = ok0 ? j0 : 0;
    float xo[3], yn[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { xo[k] = own[3 * (size_t)ic + k]; yn[k] = oth[3 * (size_t)j0c + k]; }
    // sums of at most max(Lw, Lo) differences, each of magnitude at most 2 mx
    const int sbits = reart_fx_bits(Lw > Lo ? Lw : Lo, cl_block_max(mx, s_mx));
    if (blockIdx.x == 0 && tid == 0) a.bits[n] = sbits;
    const size_t os = (size_t)n * Pw + i;        // the row this thread writes (live or padding)
    if (i < Pw) {
        if (a.od[d]) a.od[d][os] = d0;
        if (a.oi[d]) a.oi[d][os] = (int64_t)j0c;
        a.seed[d][os] = ok0 ? j0 : -1;
    }
    // ---- 3. the other cloud's live records (none can name a target of a range beyond the live points)
    if (want && r * CL_BS < Lw) cl_scatter_walk(own, oth, a.pi[o] + (size_t)n * Po, nullptr, Lw, Lo, r * CL_BS, sbits, s_acc);
    __syncthreads();
    // ---- 4. gradient and loss
    double term = 0.0;
    if (live) {
        term = (double)d0;
        if (want) {
            float first[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) first[k] = ok0 ? 2.0f * (xo[k] - yn[k]) : 0.0f;
            cl_grad_store(a.grad[d] + 3 * os, first, s_acc, sbits);
        }
    } else if (i < Pw && want) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a.grad[d][3 * os + k] = 0.0f;
    }
    term = reart_block_sum_d<CL_BS>(term, s_red);
    const int nbx = a.nr[0] + a.nr[1], total = nbx * a.N;
    if (tid == 0) {
        // device-scope atomics: the partial and the ticket meet in L2 whichever XCD the workgroups ran on
        __hip_atomic_store(&a.part[(size_t)n * nbx + blockIdx.x], term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned int k = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (k == (unsigned int)(total - 1));
    }
    __syncthreads();
    if (!s_last) return;
    if (tid < 64) {
        const double t = reart_partials_sum_d(a.part, total);      // fixed order, one rounding to float
        if (tid == 0) a.loss[0] = (float)t;
    }
}

// ---- ragged batches: what the _ragged entries put in front of the dense prep.  The search kernels have no per-element query
// count, so they get a STAGED query image of each searched direction's query cloud in which the padding rows repeat the
// element's last live point (zeros where it has none) and, in the caller's seed array, that point's seed: padding lanes are
// one coherent, bounded query that widens no row's bounds, and nothing a caller left in its padding rows reaches the search.
// Their records are ignored by the consumers, which write the padding rows' seeds back to -1.  The clamped lengths go to
// the workspace in the two widths the prep (SoaJob.len, int64) and the search (KnnJob.tlen, int) read.
struct ChamferStageArgs {
    const float *c[2];          // the clouds [N,P[d],3]
    const int *len[2];          // nullable [N]
    float *q[2];                // staged image [N,P[d],3]; NULL: cloud d is no query cloud of this call
    int *seed[2];               // [N,P[d]] with q[d]
    int64_t *len64;             // [2][N]
    int *len32;                 // [2][N]
    int P[2], N;
};
__global__ __launch_bounds__(CL_BS) void chamfer_stage_kernel(ChamferStageArgs a) {
    const int n = blockIdx.y, d = blockIdx.z;
    const int i = blockIdx.x * CL_BS + threadIdx.x;
    const int P = a.P[d], l = cl_len(a.len[d], n, P);
    if (i == 0) { a.len64[(size_t)d * a.N + n] = (int64_t)l; a.len32[(size_t)d * a.N + n] = l; }
    if (i >= P || !a.q[d]) return;
    const size_t row = (size_t)n * P;
    float v[3] = {0.f, 0.f, 0.f};
    if (l > 0) {
        const float *s = a.c[d] + 3 * (row + (i < l ? i : l - 1));
        v[0] = s[0]; v[1] = s[1]; v[2] = s[2];
    }
    float *q = a.q[d] + 3 * (row + i);
    q[0] = v[0]; q[1] = v[1]; q[2] = v[2];
    // rows >= l are written here and read by nobody in this launch; row l - 1 is only read
    if (i >= l) a.seed[d][row + i] = l > 0 ? a.seed[d][row + l - 1] : -1;
}
// queries: bit d set = cloud d is the query cloud of a searched direction
static int chamfer_stage_launch(const float *x, const float *y, const int32_t *len_x, const int32_t *len_y, int N, int P1, int P2,
                                int queries, int32_t *seed_xy, int32_t *seed_yx, char *ws, const ChamferLossPlan &p, hipStream_t st) {
    ChamferStageArgs a = {};
    a.c[0] = x; a.c[1] = y; a.len[0] = len_x; a.len[1] = len_y; a.P[0] = P1; a.P[1] = P2; a.N = N;
    a.q[0] = (queries & 1) ? (float *)(ws + p.o_xq) : nullptr; a.q[1] = (queries & 2) ? (float *)(ws + p.o_yq) : nullptr;
    a.seed[0] = seed_xy; a.seed[1] = seed_yx;
    a.len64 = (int64_t *)(ws + p.o_len64); a.len32 = (int *)(ws + p.o_len32);
    hipLaunchKernelGGL(chamfer_stage_kernel, dim3(reart_div_up(P1 > P2 ? P1 : P2, CL_BS), N, 2), dim3(CL_BS), 0, st, a);
    REART_CHECK_LAUNCH();
    return REART_OK;
}

extern "C" size_t reart_chamfer_loss_workspace_bytes(int N, int P1, int P2) {
    ChamferLossPlan p;
    if (N < 1 || P1 < 1 || P2 < 1) return 0;
    return chamfer_loss_plan(N, P1, P2, &p) == REART_OK ? p.total : 0;
}
extern "C" size_t reart_chamfer_ragged_bytes(int N, int P1, int P2) {
    ChamferLossPlan p;
    if (N < 1 || P1 < 1 || P2 < 1) return 0;
    return chamfer_loss_plan(N, P1, P2, &p, true) == REART_OK ? p.total : 0;
}

// reart_chamfer_loss is this with both lengths NULL: no staging launch, the callers' clouds as queries, the dense layout
extern "C" int reart_chamfer_loss_ragged(const float *x, const float *y, int N, int P1, int P2, int32_t *seed_xy, int32_t *seed_yx,
                                         int y_unchanged, float *d_xy, int64_t *i_xy, float *d_yx, int64_t *i_yx, float *loss,
                                         float *grad_x, float *grad_y, int32_t *fx_bits, void *workspace, size_t workspace_bytes,
                                         void *stream, const int32_t *len_x, const int32_t *len_y) {
    const bool ragged = len_x || len_y;
    ChamferLossPlan p;
    int rc = chamfer_loss_plan(N, P1, P2, &p, ragged);
    if (rc != REART_OK) return rc;
    if (N == 0 || P1 == 0 || P2 == 0) return REART_OK;
    if (!x || !y || !seed_xy || !seed_yx || !loss || !grad_x || !fx_bits) return REART_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < p.total) return REART_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    float *xsoa = (float *)(ws + p.o_xsoa), *ysoa = (float *)(ws + p.o_ysoa);
    float *xbox = (float *)(ws + p.o_xbox), *ybox = (float *)(ws + p.o_ybox);
    const int64_t *len64 = ragged ? (const int64_t *)(ws + p.o_len64) : nullptr;
    const int *len32 = ragged ? (const int *)(ws + p.o_len32) : nullptr;
    if (ragged) {
        rc = chamfer_stage_launch(x, y, len_x, len_y, N, P1, P2, 3, seed_xy, seed_yx, ws, p, st);
        if (rc != REART_OK) return rc;
    }
    // ---- prep: x always; y's image and boxes only when y is new to this workspace.  The ticket of the consumer's last-
    // workgroup test is cleared in front of every call (4 bytes): a call never depends on how an earlier one ended
    if (hipMemsetAsync(ws + p.o_ticket, 0, sizeof(unsigned int), st) != hipSuccess) return REART_ERR_LAUNCH;
    SoaArgs sa = {};
    sa.job[0].src = x; sa.job[0].len = len64; sa.job[0].dst = xsoa; sa.job[0].P = P1; sa.job[0].Ppad = p.Ppad1;
    sa.job[1] = sa.job[0];
    if (!y_unchanged) {
        sa.job[1].src = y; sa.job[1].len = ragged ? len64 + N : nullptr; sa.job[1].dst = ysoa; sa.job[1].P = P2; sa.job[1].Ppad = p.Ppad2;
    }
    rc = reart_soa_launch(sa, p.Ppad1 > p.Ppad2 ? p.Ppad1 : p.Ppad2, N, y_unchanged ? 1 : 2, st);
    if (rc != REART_OK) return rc;
    rc = reart_boxes_launch(xsoa, N, p.Ppad1, xbox, st);
    if (rc != REART_OK) return rc;
    if (!y_unchanged) {
        rc = reart_boxes_launch(ysoa, N, p.Ppad2, ybox, st);
        if (rc != REART_OK) return rc;
    }
    // ---- both directions in one search launch.  The launch has one (batch, query group) count for both jobs: both take
    // the larger number of groups; a group beyond a job's own queries repeats that job's last query and writes nothing
    SearchArgs sr = {};
    for (int j = 0; j < 2; ++j) {
        KnnJob &jb = sr.k1[j];
        jb.q = j ? y : x; jb.tsoa = j ? xsoa : ysoa; jb.boxes = j ? xbox : ybox;
        if (ragged) { jb.q = (const float *)(ws + (j ? p.o_yq : p.o_xq)); jb.tlen = len32 + (j ? 0 : N); }
        jb.seed = j ? seed_yx : seed_xy;
        jb.P1 = j ? P2 : P1; jb.P2 = j ? P1 : P2; jb.Ppad = j ? p.Ppad1 : p.Ppad2; jb.L = 0; jb.nqg = p.nqg;
        jb.pd = (float *)(ws + (j ? p.o_pd1 : p.o_pd0)); jb.pi = (int *)(ws + (j ? p.o_pi1 : p.o_pi0));
    }
    sr.n1 = 2; sr.G = N * p.nqg; sr.S1 = sr.S3 = p.S; sr.sparse = 40; sr.share = 2;
    rc = reart_search_launch(sr, st);
    if (rc != REART_OK) return rc;
    // ---- consumer
    ChamferLossArgs a = {};
    a.c[0] = x; a.c[1] = y; a.box[0] = xbox; a.box[1] = ybox;
    a.pd[0] = sr.k1[0].pd; a.pd[1] = sr.k1[1].pd; a.pi[0] = sr.k1[0].pi; a.pi[1] = sr.k1[1].pi;
    a.P[0] = P1; a.P[1] = P2; a.nbox[0] = p.Ppad1 / NN_BOX; a.nbox[1] = p.Ppad2 / NN_BOX; a.nr[0] = p.nr1; a.nr[1] = p.nr2;
    a.len[0] = len_x; a.len[1] = len_y;
    a.od[0] = d_xy; a.od[1] = d_yx; a.oi[0] = i_xy; a.oi[1] = i_yx; a.seed[0] = seed_xy; a.seed[1] = seed_yx;
    a.grad[0] = grad_x; a.grad[1] = grad_y; a.bits = fx_bits;
    a.part = (double *)(ws + p.o_part); a.ticket = (unsigned int *)(ws + p.o_ticket); a.loss = loss; a.N = N;
    hipLaunchKernelGGL(chamfer_loss_kernel, dim3(p.nr1 + p.nr2, N), dim3(CL_BS), 0, st, a);
    REART_CHECK_LAUNCH();
    return REART_OK;
}
extern "C" int reart_chamfer_loss(const float *x, const float *y, int N, int P1, int P2, int32_t *seed_xy, int32_t *seed_yx,
                                  int y_unchanged, float *d_xy, int64_t *i_xy, float *d_yx, int64_t *i_yx, float *loss,
                                  float *grad_x, float *grad_y, int32_t *fx_bits, void *workspace, size_t workspace_bytes,
                                  void *stream) {
    return reart_chamfer_loss_ragged(x, y, N, P1, P2, seed_xy, seed_yx, y_unchanged, d_xy, i_xy, d_yx, i_yx, loss, grad_x, grad_y,
                                     fx_bits, workspace, workspace_bytes, stream, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------
// Per-point distances as outputs, per-point upstream gradients as inputs (reart_chamfer_points and
// reart_chamfer_points_backward): the same prep, search, workspace layout and fixed-point sums as above, split at the
// point where a caller weights, masks or averages the distances before it reduces them.
// ---------------------------------------------------------------------------------------------
struct ChamferPointsArgs {
    const float *pd[2];         // search records of direction d (0: x -> y, 1: y -> x) [N,P[d]]
    const int *pi[2];
    int P[2], nr[2];            // points of the query cloud; consumer ranges (0: the direction was not searched)
    const int *len[2];          // nullable [N]: live points of cloud d (cl_len)
    float *od[2];               // [N,P[d]]
    int64_t *oi[2];
    int *seed[2];
};

// the own-record part of chamfer_loss_kernel alone: distance, index and next seed of every query of the searched directions
__global__ __launch_bounds__(CL_BS) void chamfer_points_kernel(ChamferPointsArgs a) {
    const int n = blockIdx.y;
    const int d = (int)blockIdx.x < a.nr[0] ? 0 : 1, o = 1 - d;
    const int i = ((int)blockIdx.x - (d ? a.nr[0] : 0)) * CL_BS + threadIdx.x;
    if (i >= a.P[d]) return;
    const size_t ow = (size_t)n * a.P[d] + i;
    const float d0 = a.pd[d][ow];
    const int j0 = a.pi[d][ow];
    const bool ok0 = i < cl_len(a.len[d], n, a.P[d]) && (unsigned)j0 < (unsigned)cl_len(a.len[o], n, a.P[o]);
    a.od[d][ow] = ok0 ? d0 : 0.0f;
    a.oi[d][ow] = (int64_t)(ok0 ? j0 : 0);
    a.seed[d][ow] = ok0 ? j0 : -1;
}

// reart_chamfer_points is this with both lengths NULL
extern "C" int reart_chamfer_points_ragged(const float *x, const float *y, int N, int P1, int P2, int directions, int32_t *seed_xy,
                                           int32_t *seed_yx, int y_unchanged, float *d_xy, int64_t *i_xy, float *d_yx, int64_t *i_yx,
                                           void *workspace, size_t workspace_bytes, void *stream, const int32_t *len_x,
                                           const int32_t *len_y) {
    const bool ragged = len_x || len_y;
    ChamferLossPlan p;
    int rc = chamfer_loss_plan(N, P1, P2, &p, ragged);
    if (rc != REART_OK) return rc;
    if (directions < 1 || directions > 3) return REART_ERR_INVALID_ARG;
    if (N == 0 || P1 == 0 || P2 == 0) return REART_OK;
    const bool xy = (directions & 1) != 0, yx = (directions & 2) != 0;
    if (!x || !y) return REART_ERR_INVALID_ARG;
    if (xy && (!seed_xy || !d_xy || !i_xy)) return REART_ERR_INVALID_ARG;
    if (yx && (!seed_yx || !d_yx || !i_yx)) return REART_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < p.total) return REART_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    float *xsoa = (float *)(ws + p.o_xsoa), *ysoa = (float *)(ws + p.o_ysoa);
    float *xbox = (float *)(ws + p.o_xbox), *ybox = (float *)(ws + p.o_ybox);
    const int64_t *len64 = ragged ? (const int64_t *)(ws + p.o_len64) : nullptr;
    const int *len32 = ragged ? (const int *)(ws + p.o_len32) : nullptr;
    if (ragged) {
        rc = chamfer_stage_launch(x, y, len_x, len_y, N, P1, P2, directions, seed_xy, seed_yx, ws, p, st);
        if (rc != REART_OK) return rc;
    }
    // ---- prep: only the TARGET cloud of a searched direction needs an image: y for x -> y (unless unchanged), x for y -> x
    const bool prep_x = yx, prep_y = xy && !y_unchanged;
    SoaArgs sa = {};
    int njobs = 0, maxPpad = 0;
    if (prep_x) {
        SoaJob &jb = sa.job[njobs++];
        jb.src = x; jb.len = len64; jb.dst = xsoa; jb.P = P1; jb.Ppad = p.Ppad1; maxPpad = p.Ppad1;
    }
    if (prep_y) {
        SoaJob &jb = sa.job[njobs++];
        jb.src = y; jb.len = ragged ? len64 + N : nullptr; jb.dst = ysoa; jb.P = P2; jb.Ppad = p.Ppad2;
        maxPpad = p.Ppad2 > maxPpad ? p.Ppad2 : maxPpad;
    }
    if (njobs) {
        if (njobs == 1) sa.job[1] = sa.job[0];
        rc = reart_soa_launch(sa, maxPpad, N, njobs, st);
        if (rc != REART_OK) return rc;
    }
    if (prep_x) {
        rc = reart_boxes_launch(xsoa, N, p.Ppad1, xbox, st);
        if (rc != REART_OK) return rc;
    }
    if (prep_y) {
        rc = reart_boxes_launch(ysoa, N, p.Ppad2, ybox, st);
        if (rc != REART_OK) return rc;
    }
    // ---- one search launch over the asked directions.  Both: exactly the launch of reart_chamfer_loss.  One: that job alone
    // with the query groups of its own cloud
    const int nqg = directions == 3 ? p.nqg : reart_div_up(xy ? P1 : P2, NN_BS);
    SearchArgs sr = {};
    ChamferPointsArgs a = {};
    for (int j = 0; j < 2; ++j) {
        if (!(directions & (1 << j))) continue;
        KnnJob &jb = sr.k1[sr.n1++];
        jb.q = j ? y : x; jb.tsoa = j ? xsoa : ysoa; jb.boxes = j ? xbox : ybox;
        if (ragged) { jb.q = (const float *)(ws + (j ? p.o_yq : p.o_xq)); jb.tlen = len32 + (j ? 0 : N); }
        jb.seed = j ? seed_yx : seed_xy;
        jb.P1 = j ? P2 : P1; jb.P2 = j ? P1 : P2; jb.Ppad = j ? p.Ppad1 : p.Ppad2; jb.L = 0; jb.nqg = nqg;
        jb.pd = (float *)(ws + (j ? p.o_pd1 : p.o_pd0)); jb.pi = (int *)(ws + (j ? p.o_pi1 : p.o_pi0));
        a.pd[j] = jb.pd; a.pi[j] = jb.pi; a.nr[j] = j ? p.nr2 : p.nr1;
    }
    if (sr.n1 == 1) sr.k1[1] = sr.k1[0];
    sr.G = N * nqg; sr.S1 = sr.S3 = p.S; sr.sparse = 40; sr.share = 2;
    rc = reart_search_launch(sr, st);
    if (rc != REART_OK) return rc;
    // ---- consumer
    a.P[0] = P1; a.P[1] = P2; a.len[0] = len_x; a.len[1] = len_y;
    a.od[0] = d_xy; a.od[1] = d_yx; a.oi[0] = i_xy; a.oi[1] = i_yx; a.seed[0] = seed_xy; a.seed[1] = seed_yx;
    hipLaunchKernelGGL(chamfer_points_kernel, dim3(a.nr[0] + a.nr[1], N), dim3(CL_BS), 0, st, a);
    REART_CHECK_LAUNCH();
    return REART_OK;
}
extern "C" int reart_chamfer_points(const float *x, const float *y, int N, int P1, int P2, int directions, int32_t *seed_xy,
                                    int32_t *seed_yx, int y_unchanged, float *d_xy, int64_t *i_xy, float *d_yx, int64_t *i_yx,
                                    void *workspace, size_t workspace_bytes, void *stream) {
    return reart_chamfer_points_ragged(x, y, N, P1, P2, directions, seed_xy, seed_yx, y_unchanged, d_xy, i_xy, d_yx, i_yx, workspace,
                                       workspace_bytes, stream, nullptr, nullptr);
}

struct ChamferPointsBwdArgs {
    const float *c[2];          // the clouds [N,P[d],3]: 0 = x, 1 = y
    const int64_t *idx[2];      // neighbour of every point of cloud d in the other cloud [N,P[d]] (NULL with g[d])
    const float *dd[2];         // its squared distance
    const float *g[2];          // upstream gradient of that distance; NULL: the direction's terms are dropped
    float *grad[2];             // [N,P[d],3]; grad[1] nullable
    int *bits;                  // [N,2] fractional bits of the fixed-point sums into cloud d of batch element n
    int P[2], nr[2];
    const int *len[2];          // nullable [N]: live points of cloud d (cl_len)
};

// Workgroup (r, n) of cloud d owns the points r*CL_BS .. of cloud d ("own"); o = 1 - d is the other cloud.
//   1. scale: m = max_j |g[o][j]| sqrt(dd[o][j]) over the other cloud of the batch element bounds every component of an
//      addend into an own point (|own_k - other_k| <= |own - other| = sqrt(d_j) up to a few roundings)
//   2. own term: fl(2 g[d][i]) * fl(own_i - other_nn(i))
//   3. walk over ALL indices of the other cloud: a point j whose neighbour is one of its own adds fl(g[o][j] * fl(own - other_j))
//      to that point's fixed-point sum in LDS
//   4. gradient = own term + 2 * sum
// Every index is range-checked before it addresses memory.  Nothing but the arguments is read: no workspace, no state.
__global__ __launch_bounds__(CL_BS) void chamfer_points_bwd_kernel(ChamferPointsBwdArgs a) {
    __shared__ unsigned long long s_acc[CL_BS * 3];
    __shared__ float s_mx[CL_BS / REART_WAVE];
    const int tid = threadIdx.x, n = blockIdx.y;
    const int d = (int)blockIdx.x < a.nr[0] ? 0 : 1, o = 1 - d;
    const int r = (int)blockIdx.x - (d ? a.nr[0] : 0);
    const int Pw = a.P[d], Po = a.P[o];
    const float *own = a.c[d] + (size_t)n * Pw * 3, *oth = a.c[o] + (size_t)n * Po * 3;
    const float *gw = a.g[d], *go = a.g[o];      // uniform
    const int Lw = cl_len(a.len[d], n, Pw), Lo = cl_len(a.len[o], n, Po);      // uniform
    for (int e = tid; e < CL_BS * 3; e += CL_BS) s_acc[e] = 0ull;
    // ---- 1. scale over the other cloud's live points (fmaxf drops NaN, non-finite products are skipped)
    float mx = 0.f;
    if (go) {
        const float *gg = go + (size_t)n * Po, *dj = a.dd[o] + (size_t)n * Po;
        for (int j = tid; j < Lo; j += CL_BS) {
            const float v = fabsf(gg[j]) * sqrtf(dj[j]);
            if (v < INFINITY) mx = fmaxf(mx, v);
        }
    }
    // ---- 2. own term
    const int i = r * CL_BS + tid;
    const bool live = i < Lw;
    const size_t ow = (size_t)n * Pw + i;        // used where i < Pw only
    float first[3] = {0.f, 0.f, 0.f};
    if (gw && live) {                            // a padding row's index and upstream are never read
        const int64_t j0 = a.idx[d][ow];
        const bool ok0 = (unsigned long long)j0 < (unsigned long long)Lo;
        const size_t j0c = ok0 ? (size_t)j0 : 0;
        const float g2 = 2.0f * gw[ow];
#pragma unroll
        for (int k = 0; k < 3; ++k) first[k] = ok0 ? g2 * (own[3 * (size_t)i + k] - oth[3 * j0c + k]) : 0.0f;
    }
    // sums of at most max(Lw, Lo) addends, each of magnitude at most m (1 + 2^-20) < m * 1.000002f
    const int sbits = reart_fx_bits(Lw > Lo ? Lw : Lo, cl_block_max(mx, s_mx) * 1.000002f);
    if (r == 0 && tid == 0) {
        a.bits[2 * n + d] = sbits;
        if (d == 0 && !a.grad[1]) a.bits[2 * n + 1] = 0;      // no sums into y in this call
    }
    // ---- 3. the other cloud's indices
    if (go && r * CL_BS < Lw) cl_scatter_walk(own, oth, a.idx[o] + (size_t)n * Po, go + (size_t)n * Po, Lw, Lo, r * CL_BS, sbits, s_acc);
    __syncthreads();
    // ---- 4. gradient
    if (live) cl_grad_store(a.grad[d] + 3 * ow, first, s_acc, sbits);
    else if (i < Pw) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a.grad[d][3 * ow + k] = 0.0f;
    }
}

// reart_chamfer_points_backward is this with both lengths NULL
extern "C" int reart_chamfer_points_backward_ragged(const float *x, const float *y, int N, int P1, int P2, const int64_t *i_xy,
                                                    const int64_t *i_yx, const float *d_xy, const float *d_yx, const float *g_xy,
                                                    const float *g_yx, float *grad_x, float *grad_y, int32_t *fx_bits, void *stream,
                                                    const int32_t *len_x, const int32_t *len_y) {
    ChamferLossPlan p;
    const int rc = chamfer_loss_plan(N, P1, P2, &p);
    if (rc != REART_OK) return rc;
    if (N == 0 || P1 == 0 || P2 == 0) return REART_OK;
    if (!x || !y || !grad_x || !fx_bits) return REART_ERR_INVALID_ARG;
    if (g_xy && (!i_xy || !d_xy)) return REART_ERR_INVALID_ARG;
    if (g_yx && (!i_yx || !d_yx)) return REART_ERR_INVALID_ARG;
    ChamferPointsBwdArgs a = {};
    a.c[0] = x; a.c[1] = y; a.idx[0] = i_xy; a.idx[1] = i_yx; a.dd[0] = d_xy; a.dd[1] = d_yx; a.g[0] = g_xy; a.g[1] = g_yx;
    a.grad[0] = grad_x; a.grad[1] = grad_y; a.bits = fx_bits;
    a.P[0] = P1; a.P[1] = P2; a.nr[0] = p.nr1; a.nr[1] = grad_y ? p.nr2 : 0;
    a.len[0] = len_x; a.len[1] = len_y;
    hipLaunchKernelGGL(chamfer_points_bwd_kernel, dim3(a.nr[0] + a.nr[1], N), dim3(CL_BS), 0, (hipStream_t)stream, a);
    REART_CHECK_LAUNCH();
    return REART_OK;
}
extern "C" int reart_chamfer_points_backward(const float *x, const float *y, int N, int P1, int P2, const int64_t *i_xy,
                                             const int64_t *i_yx, const float *d_xy, const float *d_yx, const float *g_xy,
                                             const float *g_yx, float *grad_x, float *grad_y, int32_t *fx_bits, void *stream) {
    return reart_chamfer_points_backward_ragged(x, y, N, P1, P2, i_xy, i_yx, d_xy, d_yx, g_xy, g_yx, grad_x, grad_y, fx_bits, stream,
                                                nullptr, nullptr);
}
