// reart_amd/csrc/flow_term.hip -- one iteration's flow term (reference run_robot.py:194-209: blend_anchor_motion per frame pair,
// flow_loss, and autograd through the cat and the subtraction) as ONE warm-started C-ABI call over reference sets that were
// prepared once:
//   reart_flow_term_prepare   once per run: the B ragged reference sets as +INF padded SoA rows with boxes of 16 consecutive
//                             targets (prune.hip), their lengths and a copy of their flows, all inside the workspace
//   reart_flow_term           three launches, no memset:
//     flow_stage_kernel       the queries comp[f] = pc_trans[:c] | cano | pc_trans[c:] of every pair in the order they are
//                             visited (`order`), and the counters of the consumer cleared in front of every call
//     search                  ONE K = 3 reart_search_launch: exact, box-pruned, bounded by the seeds (prune.hip, unchanged)
//     flow_term_kernel        the consumer below: exact rescan of the three best blocks, distances, indices, next seeds, blend
//                             and mask (reart_blend_point), loss term and d loss / d pred (reart_flow_point); the last
//                             workgroup of a column of points turns the pairs' gradients into d loss / d pc_trans, the last
//                             workgroup of the launch adds the loss partials in a fixed order in double and rounds once
// The consumer reads pred = comp[f + 1] - comp[f] from pc_trans and cano by indexing; only the queries are staged, because the
// search kernel reads them where a wave's 64 lanes are 64 consecutive rows.
#include "common.h"
#include "internal.h"
#include "consumer_dev.h"
#include "flow_dev.h"
#include <math.h>

#define FT_BS 256                      // threads per staging / consumer workgroup = visit positions of a column
#define FT_MAX_POINTS (1 << 20)        // N and nr_max
#define FT_MAX_ROWS (1ll << 26)        // B * N and B * padded reference length: every 32-bit product below stays in range

// Workspace: [ reference part, sized by (B, Ppad) ][ call part, sized by (B, N) ].  reart_flow_term is not told nr_max: it finds
// the padded length whose reference part, with its own call part, gives exactly workspace_bytes -- ref_bytes grows by at least 256
// with every step of Ppad, so there is one at most.
struct FlowTermRef { size_t o_soa, o_box, o_flow, o_len, total; };
static void flow_term_ref_layout(int B, int Ppad, FlowTermRef *r) {
    size_t off = 0;
    r->o_soa = off; off += sizeof(float) * 3 * (size_t)B * Ppad;                  // 192 B bytes per step of 16
    r->o_box = off; off += sizeof(float) * 8 * (size_t)B * (Ppad / NN_BOX);       //  32 B
    r->o_flow = off; off += sizeof(float) * 3 * (size_t)B * Ppad;                 // 192 B (multiples of 32 so far: 16-byte loads)
    r->o_len = off; off += sizeof(int) * (size_t)B;
    r->total = reart_align_up(off, 256);
}
struct FlowTermCall { int nbx; size_t o_q, o_pd, o_pi, o_gp, o_part, o_col, o_ticket, total; };
static void flow_term_call_layout(int B, int N, FlowTermCall *c) {
    c->nbx = reart_div_up(N, FT_BS);
    const size_t rows = sizeof(float) * 3 * (size_t)B * N;
    reart_arena ws;
    c->o_q = ws.take_bytes(rows); c->o_pd = ws.take_bytes(rows); c->o_pi = ws.take_bytes(rows); c->o_gp = ws.take_bytes(rows);
    c->o_part = ws.take_bytes(sizeof(double) * (size_t)B * c->nbx);
    c->o_col = ws.take_bytes(sizeof(unsigned int) * (size_t)c->nbx);
    c->o_ticket = ws.take_bytes(sizeof(unsigned int));
    c->total = ws.off;
}
static bool flow_term_served(int B, int N, int nr_max) {
    return B >= 1 && B <= REART_MAX_POSE_LEN && N >= 1 && N <= FT_MAX_POINTS && nr_max >= 3 && nr_max <= FT_MAX_POINTS &&
           (long long)B * N <= FT_MAX_ROWS && (long long)B * (long long)reart_align_up((size_t)nr_max, NN_BOX) <= FT_MAX_ROWS;
}

extern "C" size_t reart_flow_term_workspace_bytes(int B, int N, int nr_max) {
    if (!flow_term_served(B, N, nr_max)) return 0;
    FlowTermRef r; FlowTermCall c;
    flow_term_ref_layout(B, (int)reart_align_up((size_t)nr_max, NN_BOX), &r);
    flow_term_call_layout(B, N, &c);
    return r.total + c.total;
}

// ------------------------------------------------------------------------------------------------------ prepare
__global__ __launch_bounds__(256) void flow_term_ref_kernel(const float *__restrict__ ref_flow, const int64_t *__restrict__ ref_len,
                                                            int B, int nr_max, int Ppad, float *__restrict__ flow, int *__restrict__ len) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    int64_t n = ref_len ? ref_len[b] : (int64_t)nr_max;
    n = n < 0 ? 0 : (n > nr_max ? (int64_t)nr_max : n);
    if (j == 0) len[b] = (int)n;
    if (j >= Ppad) return;
    // rows beyond the set's length are never named by the search (their coordinates are +INF); they read as zero flows
#pragma unroll
    for (int c = 0; c < 3; ++c) flow[((size_t)b * Ppad + j) * 3 + c] = j < (int)n ? ref_flow[((size_t)b * nr_max + j) * 3 + c] : 0.f;
}

extern "C" int reart_flow_term_prepare(const float *ref, const float *ref_flow, const int64_t *ref_len, int B, int nr_max,
                                       void *workspace, size_t workspace_bytes, void *stream) {
    if (B < 1 || nr_max < 3) return REART_ERR_INVALID_ARG;
    if (!flow_term_served(B, 1, nr_max)) return REART_ERR_UNSUPPORTED;
    if (!ref || !ref_flow || !workspace) return REART_ERR_INVALID_ARG;
    const int Ppad = (int)reart_align_up((size_t)nr_max, NN_BOX);
    FlowTermRef r;
    flow_term_ref_layout(B, Ppad, &r);
    if (workspace_bytes < r.total) return REART_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    SoaArgs sa = {};
    for (int j = 0; j < 2; ++j) {
        sa.job[j].src = ref; sa.job[j].len = ref_len; sa.job[j].dst = (float *)(ws + r.o_soa); sa.job[j].P = nr_max; sa.job[j].Ppad = Ppad;
    }
    int rc = reart_soa_launch(sa, Ppad, B, 1, st);
    if (rc != REART_OK) return rc;
    rc = reart_boxes_launch((const float *)(ws + r.o_soa), B, Ppad, (float *)(ws + r.o_box), st);
    if (rc != REART_OK) return rc;
    hipLaunchKernelGGL(flow_term_ref_kernel, dim3(reart_div_up(Ppad, 256), B), dim3(256), 0, st, ref_flow, ref_len, B, nr_max, Ppad,
                       (float *)(ws + r.o_flow), (int *)(ws + r.o_len));
    REART_CHECK_LAUNCH();
    return REART_OK;
}

// ------------------------------------------------------------------------------------------------------ the call
struct FlowTermArgs {
    const float *X, *cano;      // pc_trans [B,N,3], canonical cloud [N,3]
    const int *order;           // nullable [N]: the point visited at position i
    int B, N, c, Ppad;
    int euclidean, robust, accumulate;
    float smooth, weight;
    float *qs;                  // [B,N,3] staged queries, by visit position
    const float *pd; const int *pi;   // [B,N,3] search records: the three best 8-target blocks (minimum, first index)
    const float *rsoa, *rflow; const int *rlen;
    int *seed;                  // [B,N,3] by visit position
    float *gt; uint8_t *mask; float *dists; int64_t *idx;   // nullable outputs, caller numbering
    float *gp;                  // [B,N,3] d (weight x loss) / d pred, by visit position
    float *G;                   // [B,N,3] caller numbering
    double *part;               // [B * nbx]
    unsigned int *col, *ticket; // [nbx] pairs finished per column | workgroups finished
    float *loss;                // nullable
};

// the point visited at position i; an entry outside [0, N) (never from a permutation) reads as i itself
__device__ __forceinline__ int flow_term_point(const FlowTermArgs &a, int i) {
    const int p = a.order ? a.order[i] : i;
    return (unsigned)p < (unsigned)a.N ? p : i;
}

__global__ __launch_bounds__(FT_BS) void flow_stage_kernel(FlowTermArgs a) {
    const int i = blockIdx.x * FT_BS + threadIdx.x, f = blockIdx.y;
    if (i >= a.N) return;
    if (f == 0) {     // i < nbx <= N: every counter has a thread
        if (i < (int)gridDim.x) a.col[i] = 0u;
        if (i == 0) a.ticket[0] = 0u;
    }
    const float *s = reart_complete_frame(a.X, a.cano, a.N, a.c, f) + 3 * (size_t)flow_term_point(a, i);
    float *d = a.qs + 3 * ((size_t)f * a.N + i);
    d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
}

// Workgroup (bx, f): the visit positions bx * FT_BS .. of pair f.  Every index taken from a record or from `order` is
// range-checked before it addresses memory, and every loop runs over counts fixed by the shapes.
__global__ __launch_bounds__(FT_BS) void flow_term_kernel(FlowTermArgs a) {
    __shared__ double s_red[FT_BS / REART_WAVE];
    __shared__ int s_lastcol, s_last;
    const int tid = threadIdx.x, bx = blockIdx.x, f = blockIdx.y, nbx = gridDim.x;
    const int i = bx * FT_BS + tid;
    const bool live = i < a.N;
    const int ic = live ? i : a.N - 1;
    const int p = flow_term_point(a, ic);
    const size_t ov = ((size_t)f * a.N + ic) * 3;        // by visit position
    const size_t oc = ((size_t)f * a.N + p) * 3;         // caller numbering
    double term = 0.0;
    {
        // the point in both frames of the pair and the records: independent of each other, requested first
        const float *c0 = reart_complete_frame(a.X, a.cano, a.N, a.c, f) + 3 * (size_t)p;
        const float *c1 = reart_complete_frame(a.X, a.cano, a.N, a.c, f + 1) + 3 * (size_t)p;
        const float c0v[3] = {c0[0], c0[1], c0[2]}, c1v[3] = {c1[0], c1[1], c1[2]};
        const float q[3] = {a.qs[ov], a.qs[ov + 1], a.qs[ov + 2]};
        const int n2 = a.rlen[f];
        const float *tx = a.rsoa + (size_t)f * 3 * a.Ppad, *ty = tx + a.Ppad, *tz = ty + a.Ppad;
        // a record names a block only if it is finite, in range and 8-aligned; a block is rescanned once, up to the set's length
        int bb[3], nv[3];
#pragma unroll
        for (int cb = 0; cb < 3; ++cb) {
            const float m = a.pd[ov + cb];
            const int blk = a.pi[ov + cb];
            const bool ok = m < INFINITY && (unsigned)blk <= (unsigned)(a.Ppad - 8) && (blk & 7) == 0;
            bb[cb] = ok ? blk : -1;
#pragma unroll
            for (int cp = 0; cp < cb; ++cp) bb[cb] = bb[cb] == bb[cp] ? -1 : bb[cb];
            nv[cb] = bb[cb] < 0 ? 0 : min(8, n2 - bb[cb]);
        }
        // the three nearest targets lie inside the three best blocks: one exact rescan with the full (distance, index) key
        float kd[3];
        int ki[3];
        reart_rescan3(q, tx, ty, tz, bb, nv, kd, ki);
        // fewer than three finite candidates (non-finite coordinates, a set below three points): index 0, as the records of
        // reart_knn_cuda beyond a set's length
        float dk[3];
        int jk[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool ok = ki[k] != 0x7fffffff;          // then 0 <= ki < n2 <= Ppad
            jk[k] = ok ? ki[k] : 0;
            const float d = a.euclidean ? sqrtf(kd[k]) : kd[k];
            dk[k] = ok ? d : 0.0f;
        }
        float gtf[3];
        const bool m = reart_blend_point(dk, jk, 3, a.rflow + (size_t)f * a.Ppad * 3, gtf[0], gtf[1], gtf[2]);
        const float pred[3] = {c1v[0] - c0v[0], c1v[1] - c0v[1], c1v[2] - c0v[2]};      // pred_flow (run_robot.py:207)
        float gr[3];
        const double t = reart_flow_point(gtf, pred, m, a.robust, a.smooth, gr);
        if (live) {
            term = t;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                a.seed[ov + k] = ki[k] != 0x7fffffff ? ki[k] : -1;
                // device-scope: read back by whichever workgroup of the column finishes last, on any XCD
                __hip_atomic_store(&a.gp[ov + k], gr[k] * a.weight, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (a.gt) a.gt[oc + k] = gtf[k];
                if (a.dists) a.dists[oc + k] = dk[k];
                if (a.idx) a.idx[oc + k] = (int64_t)jk[k];
            }
            if (a.mask) a.mask[(size_t)f * a.N + p] = m ? 1 : 0;
        }
    }
    // The hand-off to the last workgroup of the column and of the launch.  Everything handed off (gp, the partials) is written by
    // agent-scope (write-through) stores and read by agent-scope loads, so no cache has to be written back or invalidated:
    // every wave waits until its stores have left it (a barrier waits for no memory counter), the workgroup meets in the block sum (which stores to LDS only), and
    // thread 0 -- after its own partial has left too -- signals with relaxed agent-scope adds.  A release here would write back
    // the XCD's whole L2, twice per workgroup.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    term = reart_block_sum_d<FT_BS>(term, s_red);
    const int total = nbx * a.B;
    if (tid == 0) {
        __hip_atomic_store(&a.part[(size_t)f * nbx + bx], term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int kc = __hip_atomic_fetch_add(&a.col[bx], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_lastcol = (kc == (unsigned int)(a.B - 1));
        const unsigned int k = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (k == (unsigned int)(total - 1));
    }
    __syncthreads();                                       // the loads below are issued after the tickets have come back
    if (s_lastcol && live) {
        // d loss / d comp[j] = gp[j - 1] - gp[j] (pred = comp[1:] - comp[:-1]); a term that does not exist is dropped, the
        // canonical frame takes none
        float prev[3] = {0.f, 0.f, 0.f};
        for (int j = 0; j <= a.B; ++j) {
            float next[3] = {0.f, 0.f, 0.f};
            if (j < a.B) {
                const size_t o = ((size_t)j * a.N + i) * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) next[k] = __hip_atomic_load(&a.gp[o + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (j != a.c) {
                float *g = a.G + ((size_t)(j < a.c ? j : j - 1) * a.N + p) * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float dlt = prev[k] - next[k];
                    g[k] = a.accumulate ? g[k] + dlt : dlt;
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) prev[k] = next[k];
        }
    }
    if (!s_last || !a.loss) return;
    if (tid < 64) {
        const double t = reart_partials_sum_d(a.part, total);      // fixed order, one rounding to float
        if (tid == 0) a.loss[0] = a.weight * (float)t;
    }
}

extern "C" int reart_flow_term(const float *pc_trans, const float *cano, const int32_t *order, int B, int N, int cano_idx,
                               int euclidean, int robust, float smooth_weight, float weight, int32_t *seed, float *gt_flow,
                               uint8_t *mask, float *dists, int64_t *idx, float *loss, float *G, int accumulate, void *workspace,
                               size_t workspace_bytes, void *stream) {
    if (B < 1 || N < 1 || cano_idx < 0 || cano_idx > B) return REART_ERR_INVALID_ARG;
    if (!flow_term_served(B, N, 3)) return REART_ERR_UNSUPPORTED;
    if (!pc_trans || !cano || !seed || !G || !workspace) return REART_ERR_INVALID_ARG;
    FlowTermCall c;
    flow_term_call_layout(B, N, &c);
    // the padded reference length this workspace was sized (and prepared) for
    FlowTermRef r;
    int lo = 1, hi = FT_MAX_POINTS / NN_BOX, Ppad = 0;
    while (lo <= hi) {
        const int mid = lo + (hi - lo) / 2;
        flow_term_ref_layout(B, mid * NN_BOX, &r);
        if (r.total + c.total == workspace_bytes) { Ppad = mid * NN_BOX; break; }
        if (r.total + c.total < workspace_bytes) lo = mid + 1; else hi = mid - 1;
    }
    if (!Ppad) return REART_ERR_INVALID_ARG;              // not a size reart_flow_term_workspace_bytes(B, N, .) returns
    if ((long long)B * Ppad > FT_MAX_ROWS) return REART_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace, *wc = ws + r.total;
    FlowTermArgs a = {};
    a.X = pc_trans; a.cano = cano; a.order = order; a.B = B; a.N = N; a.c = cano_idx; a.Ppad = Ppad;
    a.euclidean = euclidean ? 1 : 0; a.robust = robust ? 1 : 0; a.accumulate = accumulate ? 1 : 0;
    a.smooth = smooth_weight; a.weight = weight;
    a.qs = (float *)(wc + c.o_q); a.pd = (const float *)(wc + c.o_pd); a.pi = (const int *)(wc + c.o_pi);
    a.rsoa = (const float *)(ws + r.o_soa); a.rflow = (const float *)(ws + r.o_flow); a.rlen = (const int *)(ws + r.o_len);
    a.seed = seed; a.gt = gt_flow; a.mask = mask; a.dists = dists; a.idx = idx;
    a.gp = (float *)(wc + c.o_gp); a.G = G; a.part = (double *)(wc + c.o_part);
    a.col = (unsigned int *)(wc + c.o_col); a.ticket = (unsigned int *)(wc + c.o_ticket); a.loss = loss;
    const dim3 grid(c.nbx, B);
    hipLaunchKernelGGL(flow_stage_kernel, grid, dim3(FT_BS), 0, st, a);
    REART_CHECK_LAUNCH();
    SearchArgs sr = {};
    KnnJob &jb = sr.k3;
    jb.q = a.qs; jb.tsoa = a.rsoa; jb.boxes = (const float *)(ws + r.o_box); jb.tlen = a.rlen; jb.seed = seed;
    jb.P1 = N; jb.P2 = Ppad; jb.Ppad = Ppad; jb.L = 0; jb.nqg = reart_div_up(N, NN_BS);
    jb.pd = (float *)(wc + c.o_pd); jb.pi = (int *)(wc + c.o_pi);
    int S = 4;                                            // waves per search workgroup: as reart_knn_points_idx_warm
    while (S > 1 && reart_div_up(Ppad, S) < 64) S -= 1;
    sr.n3 = 1; sr.G = B * jb.nqg; sr.S1 = sr.S3 = S; sr.sparse = 40; sr.share = 2;
    const int rc = reart_search_launch(sr, st);
    if (rc != REART_OK) return rc;
    hipLaunchKernelGGL(flow_term_kernel, grid, dim3(FT_BS), 0, st, a);
    REART_CHECK_LAUNCH();
    return REART_OK;
}
