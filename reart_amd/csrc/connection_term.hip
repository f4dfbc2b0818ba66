// reart_amd/csrc/connection_term.hip -- the connection term of the reference (networks/loss.py compute_connection_loss
// :60-78) for gfx950: per edge (a, b) the k closest (point of part a, its nearest point of part b) pairs of the canonical
// cloud, and the mean squared distance of those pairs in every predicted frame, with its gradient.
//
// reart_connection_select, three launches:
//   cs_members_kernel  one workgroup per part p, 16 waves, each walking a contiguous run of the labels twice: count, then
//                      write the part's points in ascending index behind those of the parts below it (a stable counting
//                      sort by label; the part's offset is the number of points with a label in [0, p), counted alongside).
//   cs_search_kernel   workgroup (edge e, slot g): 256 sources of part a per pass, one per thread, the members of part b
//                      gathered into LDS 1024 at a time and scanned in ascending index with a strict <, so that the lowest
//                      index attaining the minimum stays.  A source's key is (bits of d) << 32 | i << 16 | j (N <= 65 536:
//                      both indices fit; (d, i) order, i unique per edge); every wave keeps the k smallest keys it has seen
//                      in LDS (knn_keys.h), wave 0 merges the four lists and writes the workgroup's partial list.
//   cs_merge_kernel    one wave per edge merges the partial lists of the slots that had sources and writes the tables.
// reart_connection_term, three launches with a gradient, two without:
//   reart_invlist_kernel<512, 16, CtRecords> (invlist_dev.h, shared with pointnet_grad.hip)
//                      the records 2 (e k + r) + role (0 = source, 1 = target) of the valid edges, grouped by the point they
//                      name and ascending inside a group: a workgroup of 1024 threads per 512 points, one cloud.
//   ct_cost_kernel     one workgroup per edge: the T k squared pair distances added in double (reart_block_sum_d, common.h).
//   ct_grad_kernel     a thread per (frame, point) adds the point's records in ascending record number; workgroup (0, 0)
//                      also adds the edge costs (reart_loss_sum_d, common.h, the structure term's as well).  ct_loss_kernel
//                      does that alone when no gradient is asked for.
// No floating-point atomics, no host synchronisation, no allocation; every output entry has one writer.
#include "common.h"
#include "invlist_dev.h"
#include "knn_keys.h"

#define CS_MAX_N REART_CONN_MAX_N    // 65 536: two indices in the low 32 bits of a key
#define CS_MAX_K REART_CONN_MAX_K    // 64: a wave's list, one key per lane
#define CS_MAX_P 64       // as the structure term
#define CS_MAX_E 4096
#define CS_SRC 256        // sources per workgroup pass (one per thread)
#define CS_TILE 1024      // target members per LDS tile
#define CS_MAX_G 16       // workgroups per edge at most
#define CT_TILE 512       // points per workgroup of the index kernel
#define CT_WAVES 16

static bool cs_shape_ok(int N, int P, int E, int k) {
    return N >= 1 && N <= CS_MAX_N && P >= 1 && P <= CS_MAX_P && E >= 0 && E <= CS_MAX_E && k >= 1 && k <= CS_MAX_K;
}
static bool ct_shape_ok(int T, int N, int E, int k) {
    return T >= 1 && T <= REART_MAX_POSE_LEN && N >= 1 && N <= CS_MAX_N && E >= 0 && E <= CS_MAX_E && k >= 1 && k <= CS_MAX_K;
}
static int cs_slots(int N) { const int g = reart_div_up(N, CS_SRC); return g < CS_MAX_G ? g : CS_MAX_G; }
// select: the parts' member lists [N], their sizes and first members [2][CS_MAX_P], every slot's k best keys [E][slots][k]
struct CsWs { int *members, *count; u64 *partial; };
static size_t cs_ws_layout(int N, int E, int k, void *workspace, CsWs *w) {
    reart_arena ws(workspace);
    w->members = ws.take<int>((size_t)N);
    w->count = ws.take<int>(2 * CS_MAX_P);
    w->partial = ws.take<u64>((size_t)(E > 0 ? E : 1) * cs_slots(N) * k);
    return ws.off;
}
// term: the edges' costs in double [E], the points' record lists as offsets [N + 1] and records [2][E][k]
struct CtWs { double *cost_d; int *start, *list; };
static size_t ct_ws_layout(int N, int E, int k, void *workspace, CtWs *w) {
    reart_arena ws(workspace);
    w->cost_d = ws.take<double>(E > 0 ? E : 1);
    w->start = ws.take<int>((size_t)N + 1);
    w->list = ws.take<int>(2 * (size_t)(E > 0 ? E : 1) * k);
    return ws.off;
}

// items per wave when CT_WAVES waves share n items in contiguous runs, whole steps of 64
__device__ __forceinline__ int cs_run(int n) { return (n + CT_WAVES * 64 - 1) / (CT_WAVES * 64) * 64; }

// ---------------------------------------------------------------------------------------------------------- select
__global__ __launch_bounds__(1024) void cs_members_kernel(const int64_t *__restrict__ seg, int N, int P, int *__restrict__ members,
                                                          int *__restrict__ count, int *__restrict__ base) {
    __shared__ int s_eq[CT_WAVES], s_lt[CT_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int run = cs_run(N);
    const int lo = min(N, w * run), hi = min(N, lo + run);
    int eq = 0, lt = 0;
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const int i = i0 + lane;
        const int64_t l = i < hi ? seg[i] : -1;
        eq += __popcll(__ballot(l == p));
        lt += __popcll(__ballot(l >= 0 && l < p));
    }
    if (lane == 0) { s_eq[w] = eq; s_lt[w] = lt; }
    __syncthreads();
    int first = 0, total = 0, off = 0;
    for (int v = 0; v < CT_WAVES; ++v) {
        first += s_lt[v];             // the parts below, every run
        total += s_eq[v];
        if (v < w) off += s_eq[v];    // this part, the runs before this wave's
    }
    off += first;
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const int i = i0 + lane;
        const bool mine = i < hi && seg[i] == p;
        const u64 m = __ballot(mine);
        if (mine) members[off + __popcll(m & reart_lanes_below(lane))] = i;
        off += __popcll(m);
    }
    if (tid == 0) { count[p] = total; base[p] = first; }
}

// the two parts of edge e and whether it is valid: both in [0,P), |a| >= k, |b| >= 1
__device__ __forceinline__ bool cs_edge(const int32_t *pairs, const int *count, int P, int k, int e, int &a, int &b) {
    a = pairs[2 * e];
    b = pairs[2 * e + 1];
    if (a < 0 || a >= P || b < 0 || b >= P) return false;
    return count[a] >= k && count[b] >= 1;
}

__global__ __launch_bounds__(CS_SRC) void cs_search_kernel(const float *__restrict__ cano, const int32_t *__restrict__ pairs,
                                                           const int *__restrict__ members, const int *__restrict__ count,
                                                           const int *__restrict__ base, int P, int k, u64 *__restrict__ partial) {
    __shared__ float4 s_t[CS_TILE];
    __shared__ u64 s_lst[CS_SRC / 64][64];
    __shared__ u64 s_cand[CS_SRC / 64][64];
    // edge fastest: the slots that have sources (the low ones) are neighbours in the grid, which the dispatcher deals
    // round-robin over the XCDs; slot fastest would put every slot 0 on one XCD whenever the slots are a multiple of 8
    const int e = blockIdx.x, g = blockIdx.y, G = gridDim.y, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    int a, b;
    if (!cs_edge(pairs, count, P, k, e, a, b)) return;
    const int na = count[a], nb = count[b];
    if (g * CS_SRC >= na) return;                       // cs_merge_kernel skips this slot
    const int *ma = members + base[a], *mb = members + base[b];
    s_lst[w][lane] = kl_none<u64>();
    reart_wave_sync();
    u64 thr = kl_none<u64>();
    for (int c = g; c * CS_SRC < na; c += G) {
        const int sp = c * CS_SRC + tid;
        const bool has = sp < na;
        const int i = has ? ma[sp] : 0;
        const float qx = cano[3 * i], qy = cano[3 * i + 1], qz = cano[3 * i + 2];
        float best = __int_as_float(0x7f800000);        // +inf: a distance that is not below it keeps position 0, a member
        int bpos = 0;
        for (int t0 = 0; t0 < nb; t0 += CS_TILE) {
            const int n = min(CS_TILE, nb - t0);
            __syncthreads();                            // the previous tile has been read
            for (int u = tid; u < n; u += CS_SRC) {
                const int j = mb[t0 + u];
                s_t[u] = make_float4(cano[3 * j], cano[3 * j + 1], cano[3 * j + 2], 0.f);
            }
            __syncthreads();
#pragma unroll 4
            for (int u = 0; u < n; ++u) {     // every lane reads the same address: a broadcast; four reads in flight
                const float4 t = s_t[u];
                const float d = reart_sqdist3(qx, qy, qz, t.x, t.y, t.z);
                if (d < best) { best = d; bpos = t0 + u; }
            }
        }
        const int j = mb[bpos];
        const u64 key = ((u64)__float_as_uint(best) << 32) | ((u64)(unsigned)i << 16) | (unsigned)j;
        const bool acc = has && key < thr;
        const u64 m = __ballot(acc);
        if (m) {
            const u64 v = kl_sort64(acc ? key : kl_none<u64>(), lane);
            thr = kl_merge<1>(s_lst[w], s_cand[w], k, v, __popcll(m), lane);
        }
    }
    __syncthreads();
    if (w == 0) {
        for (int o = 1; o < CS_SRC / 64; ++o) {
            const u64 v = lane < k ? s_lst[o][lane] : kl_none<u64>();       // ascending, the empty slots last
            const int c = __popcll(__ballot(v != kl_none<u64>()));
            if (c) kl_merge<1>(s_lst[0], s_cand[0], k, v, c, lane);
        }
        if (lane < k) partial[((size_t)e * G + g) * k + lane] = s_lst[0][lane];
    }
}

__global__ __launch_bounds__(64) void cs_merge_kernel(const int32_t *__restrict__ pairs, const int *__restrict__ count, int P, int k,
                                                      int G, const u64 *__restrict__ partial, int32_t *__restrict__ src_idx,
                                                      int32_t *__restrict__ tgt_idx, float *__restrict__ sel_dist,
                                                      uint8_t *__restrict__ valid) {
    __shared__ u64 s_lst[64];
    __shared__ u64 s_cand[64];
    const int e = blockIdx.x, lane = threadIdx.x;
    int a, b;
    const bool ok = cs_edge(pairs, count, P, k, e, a, b);
    u64 key = 0;                                        // an invalid edge: indices 0, distance +0
    if (ok) {
        const int ng = min(G, (count[a] + CS_SRC - 1) / CS_SRC);
        s_lst[lane] = lane < k ? partial[((size_t)e * G) * k + lane] : kl_none<u64>();
        reart_wave_sync();
        for (int g = 1; g < ng; ++g) {
            const u64 v = lane < k ? partial[((size_t)e * G + g) * k + lane] : kl_none<u64>();
            const int c = __popcll(__ballot(v != kl_none<u64>()));
            if (c) kl_merge<1>(s_lst, s_cand, k, v, c, lane);
        }
        key = s_lst[lane];
    }
    if (lane < k) {
        src_idx[e * k + lane] = (int32_t)((key >> 16) & 0xffffu);
        tgt_idx[e * k + lane] = (int32_t)(key & 0xffffu);
        if (sel_dist) sel_dist[e * k + lane] = __uint_as_float((unsigned)(key >> 32));
    }
    if (lane == 0) valid[e] = ok ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ term
struct CtTables {
    const int32_t *src, *tgt;    // [E,k]
    const uint8_t *valid;        // [E]
    int N, E, k;
};

// pair `rec` = e k + r takes part: its edge is valid and both indices are points of the cloud
__device__ __forceinline__ bool ct_live(const CtTables &c, int rec, int &s, int &g) {
    s = c.src[rec];
    g = c.tgt[rec];
    return c.valid[rec / c.k] != 0 && (unsigned)s < (unsigned)c.N && (unsigned)g < (unsigned)c.N;
}

// the records of reart_invlist_kernel: q = 2 (e k + r) + role names the pair's source (role 0) or target (role 1)
struct CtRecords {
    CtTables c;
    __device__ int count() const { return 2 * c.E * c.k; }
    __device__ int points() const { return c.N; }
    __device__ bool point(int, int q, int &pt) const {
        int s, g;
        const bool live = ct_live(c, q >> 1, s, g);
        pt = (q & 1) ? g : s;
        return live;
    }
};

__global__ __launch_bounds__(256) void ct_cost_kernel(const float *__restrict__ pc, CtTables c, int T, double *__restrict__ cost_d,
                                                      float *__restrict__ edge_cost) {
    __shared__ double s_w[4];
    const int e = blockIdx.x, tid = threadIdx.x;
    double acc = 0.0;
    for (int x = tid; x < T * c.k; x += 256) {
        const int t = x / c.k, rec = e * c.k + x % c.k;
        int s, g;
        if (!ct_live(c, rec, s, g)) continue;
        const float *ps = pc + ((size_t)t * c.N + s) * 3, *pg = pc + ((size_t)t * c.N + g) * 3;
        acc += (double)reart_sqdist3(ps[0], ps[1], ps[2], pg[0], pg[1], pg[2]);
    }
    const double tot = reart_block_sum_d<256>(acc, s_w) / (double)c.k;
    if (tid == 0) {
        cost_d[e] = tot;
        if (edge_cost) edge_cost[e] = (float)tot;
    }
}

__global__ __launch_bounds__(256) void ct_loss_kernel(const double *cost_d, int E, float weight, float *loss) {
    __shared__ double s_w[4];
    reart_loss_sum_d<256>(cost_d, E, weight, loss, s_w);
}

// grad[t,n] = sum over the records naming n, ascending record number, of +-(2 weight / k)(p[t,src] - p[t,tgt])
__global__ __launch_bounds__(256) void ct_grad_kernel(const float *__restrict__ pc, CtTables c, float scale, const int *__restrict__ start,
                                                      const int *__restrict__ list, float *__restrict__ grad,
                                                      const double *__restrict__ cost_d, float weight, float *__restrict__ loss) {
    __shared__ double s_w[4];
    const int n = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (n < c.N) {
        const float *p = pc + (size_t)t * c.N * 3;
        float gx = 0.f, gy = 0.f, gz = 0.f;
        const int q1 = start[n + 1];
        for (int u = start[n]; u < q1; ++u) {
            const int q = list[u], rec = q >> 1;
            const int s = c.src[rec], g = c.tgt[rec];
            const float dx = scale * (p[3 * s] - p[3 * g]), dy = scale * (p[3 * s + 1] - p[3 * g + 1]),
                        dz = scale * (p[3 * s + 2] - p[3 * g + 2]);
            if (q & 1) { gx -= dx; gy -= dy; gz -= dz; } else { gx += dx; gy += dy; gz += dz; }
        }
        float *o = grad + ((size_t)t * c.N + n) * 3;
        o[0] = gx; o[1] = gy; o[2] = gz;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0) reart_loss_sum_d<256>(cost_d, c.E, weight, loss, s_w);
}

// ------------------------------------------------------------------------------------------------------------ host
extern "C" size_t reart_connection_select_workspace_bytes(int N, int P, int E, int k) {
    CsWs w;
    return cs_shape_ok(N, P, E, k) ? cs_ws_layout(N, E, k, nullptr, &w) : 0;
}

extern "C" int reart_connection_select(const float *cano, const int64_t *seg, int N, int P, const int32_t *pairs, int E, int k,
                                       int32_t *src_idx, int32_t *tgt_idx, float *sel_dist, uint8_t *valid, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    if (!cano || !seg || N <= 0 || P <= 0 || E < 0 || k <= 0 || (E > 0 && (!pairs || !src_idx || !tgt_idx || !valid)))
        return REART_ERR_INVALID_ARG;
    if (!cs_shape_ok(N, P, E, k)) return REART_ERR_UNSUPPORTED;
    CsWs w;
    if (!workspace || workspace_bytes < cs_ws_layout(N, E, k, workspace, &w)) return REART_ERR_INVALID_ARG;
    if (E == 0) return REART_OK;
    hipStream_t st = (hipStream_t)stream;
    int *count = w.count, *base = count + CS_MAX_P;
    const int G = cs_slots(N);
    hipLaunchKernelGGL(cs_members_kernel, dim3(P), dim3(CT_WAVES * 64), 0, st, seg, N, P, w.members, count, base);
    hipLaunchKernelGGL(cs_search_kernel, dim3(E, G), dim3(CS_SRC), 0, st, cano, pairs, w.members, count, base, P, k, w.partial);
    hipLaunchKernelGGL(cs_merge_kernel, dim3(E), dim3(64), 0, st, pairs, count, P, k, G, w.partial, src_idx, tgt_idx, sel_dist, valid);
    REART_CHECK_LAUNCH();
    return REART_OK;
}

extern "C" size_t reart_connection_term_workspace_bytes(int T, int N, int E, int k) {
    CtWs w;
    return ct_shape_ok(T, N, E, k) ? ct_ws_layout(N, E, k, nullptr, &w) : 0;
}

extern "C" int reart_connection_term(const float *pc_trans, const int32_t *src_idx, const int32_t *tgt_idx, const uint8_t *valid,
                                     int T, int N, int E, int k, float weight, float *loss, float *edge_cost, float *grad,
                                     void *workspace, size_t workspace_bytes, void *stream) {
    if (!pc_trans || !loss || T <= 0 || N <= 0 || E < 0 || k <= 0 || (E > 0 && (!src_idx || !tgt_idx || !valid)))
        return REART_ERR_INVALID_ARG;
    if (!ct_shape_ok(T, N, E, k)) return REART_ERR_UNSUPPORTED;
    CtWs w;
    if (!workspace || workspace_bytes < ct_ws_layout(N, E, k, workspace, &w)) return REART_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    const CtTables c{src_idx, tgt_idx, valid, N, E, k};
    if (E > 0) hipLaunchKernelGGL(ct_cost_kernel, dim3(E), dim3(256), 0, st, pc_trans, c, T, w.cost_d, edge_cost);
    if (grad) {     // E == 0: every list is empty, the gradient is written as zeros
        hipLaunchKernelGGL((reart_invlist_kernel<CT_TILE, CT_WAVES, CtRecords>), dim3(reart_div_up(N, CT_TILE)), dim3(CT_WAVES * 64), 0, st,
                           CtRecords{c}, w.start, w.list);
        hipLaunchKernelGGL(ct_grad_kernel, dim3(reart_div_up(N, 256), T), dim3(256), 0, st, pc_trans, c, 2.0f * weight / (float)k,
                           w.start, w.list, grad, w.cost_d, weight, loss);
    } else {
        hipLaunchKernelGGL(ct_loss_kernel, dim3(1), dim3(256), 0, st, w.cost_d, E, weight, loss);
    }
    REART_CHECK_LAUNCH();
    return REART_OK;
}
