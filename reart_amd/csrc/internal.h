// reart_amd/csrc/internal.h -- argument blocks shared between the operator files and the
// fused relaxation step (step.hip).  Not part of the C ABI.
#pragma once
#include "common.h"

struct BaseFwdArgs {
    const float *cano;
    const float *W1, *b1, *W2, *p6d, *pt;
    const float *gumbel;        // [N,P] injected noise, or NULL -> Philox(seed, *iter)
    const float *tau_ptr;       // device scalar, or NULL -> tau
    const int64_t *iter_ptr;    // device counter used as Philox offset (nullable -> 0)
    uint64_t seed;
    float tau;
    int N, P, B, H, Npad;
    float *out;                 // [B,N,3]
    float *out_soa;             // [B,3,Npad] nullable (+INF beyond N), for the K-NN kernels
    int64_t *seg_part;          // [N] nullable
    float *trans_list;          // [B,P,4,4] nullable
    float *yT;                  // [P,N] nullable
    float *hT;                  // [H,N] nullable
    int *hard_idx;              // [N] nullable
    float *rt_table;            // [B*P][12] nullable: [R|t] rows for the backward's scalar loads
    float *boxes;               // [B][Npad/64][8] nullable: AABB of every 64 output points per frame
    int pts;                    // points per forward workgroup: 64 or 32 (0: the default, 32)
};

struct BaseBwdArgs {
    const float *cano, *W2, *p6d, *pt;
    const float *yT, *hT;       // hT == NULL: the block kernel re-evaluates the hidden layer from cano and W1 | b1
    const float *W1, *b1;       // read only where hT == NULL
    const int *hard_idx;
    const float *tau_ptr;
    float tau;
    const float *G;             // [B,N,3]
    const float *rt_table;      // [B*P][12] or NULL (built into the workspace)
    // fused step only: the tile load adds the flow-loss terms of the two adjacent frame pairs
    const float *gpf;           // [B,N,3] d(lambda*flow)/d pred_flow or NULL
    int cano_idx;
    int N, P, B, H;
    int nchunk;                 // ceil(N / cpts)
    int cpts;                   // points per backward workgroup: 64, 32 or 16 (0: the default, 32)
    int dp_sep;                 // set by the launcher: the hidden gradient has an LDS tile of its own (else it overwrites the h tile)
    float *partial;             // [nchunk][n_out]
    // fused step only: the Adam step sizes the finalize launch BEHIND this block launch reads (FinalizeAdam::step) are
    // promoted here, from the slot the previous finalize launch's bookkeeping workgroup wrote.  NULL: no promotion
    const float *step_next;     // [4]
    float *step_cur;            // [4]
    // finalize
    float *gW1, *gb1, *gW2, *g6d, *gt;
};

struct AdamSeg { float *p; const float *g; float *m; float *v; int n; float lr; };
struct AdamArgs { AdamSeg seg[8]; int nseg; float beta1, beta2, eps; const int64_t *step_ptr; int step; };

// Several independent instances of one shape in ONE launch (relax batch): the kernels of the fused step take their
// argument block K times and pick theirs by the grid's last dimension (blockIdx.y where the kernel's own grid is a row,
// blockIdx.z for the stand-alone consumers of step.hip, whose own grid is a plane); with one instance they are instantiated
// to read block 0.  6 blocks of the largest (SearchArgs) stay within the 4 KB kernel-argument segment with room for the
// runtime's hidden arguments.
#define REART_BATCH_MAX 6
template <class A>
struct Batched { A a[REART_BATCH_MAX]; };
template <class A>
static inline Batched<A> reart_batched(const A *a, int K) {
    Batched<A> b = {};
    for (int k = 0; k < K && k < REART_BATCH_MAX; ++k) b.a[k] = a[k];
    return b;
}
// force_long: take the long path (model_long.hip) also where the pose table fits in LDS (reart_relax_config.tune_long)
int reart_base_forward_launch(const BaseFwdArgs *a, int K, hipStream_t st, int force_long);   // same shapes, 1 <= K <= REART_BATCH_MAX
struct FinalizeAdam {
    int enabled;
    float *W1, *b1, *W2, *p6d, *pt;   // parameters (updated in place)
    float *m, *v;                     // moments, order W1|b1|W2|p6d|pt
    float seg_lr, trans_lr, beta1, beta2, eps;
    float weight_decay;               // torch.optim.Adam's L2 form: g += weight_decay * p
    const int64_t *step_ptr;
    // device [4], the step sizes of THIS step (with bc1 = 1 - beta1^step, bc2 = sqrt(1 - beta2^step) in double):
    // (float)((double)seg_lr / bc1), (float)((double)trans_lr / bc1), (float)bc2, unused
    const float *step;
};

// Fused step only: end-of-iteration bookkeeping (loss log, iteration counter, next temperature and
// Adam step sizes), done by ONE EXTRA workgroup of the finalize kernel (the last blockIdx.x).  No other
// workgroup of that launch reads `iter` or `tau`; the step sizes they do read (FinalizeAdam::step) are
// another slot than the one written here (`step_next`), which the next backward block launch promotes.
struct StepBook {
    int enabled;
    const double *frame_loss; int n_frame_part;
    const double *flow_part; int n_flow_part;
    int64_t *iter; float *tau; float *losses;
    float *step_next;          // [4]: FinalizeAdam::step of the NEXT step
    int ring, n_iter;
    float lambda_flow, fixed_tau, end_tau, start_tau, beta1, beta2, seg_lr, trans_lr;
    // recon_with_assign: the assignment partials (each times lambda_assign already) that go on top of frame_loss in row[0];
    // n_assign_part = 0 in every other mode.  losses_assign: nullable [ring], the assignment term alone (0 in the other modes)
    const double *assign_part; int n_assign_part;
    float *losses_assign;
};
int reart_base_backward_launch(const BaseBwdArgs *args, const FinalizeAdam *adam, const StepBook *book, void *const *workspaces,
                               size_t workspace_bytes, int K, hipStream_t st, int force_long);     // adam / book: arrays of K, or NULL
// ---- the same model for pose tables that do not fit in LDS (model_long.hip); which shapes: reart_base_path (model.hip)
int reart_base_forward_long_launch(const BaseFwdArgs *a, int K, hipStream_t st);
// the block kernel of the backward only (args as reart_base_backward_launch has prepared them: cpts, nchunk, partial, rt_table)
int reart_base_backward_long_launch(const BaseBwdArgs *a, int K, hipStream_t st);
// frames per LDS tile of that kernel (0: not even one fits); cpts = 0: without a hidden-gradient tile of its own
int reart_base_bwd_long_tile(int P, int B, int H, int cpts, int *dp_sep, size_t *lds);
#ifdef __HIPCC__
// cosine schedule of utils/model_utils.py:33-37 evaluated in double like the host code
__device__ __forceinline__ float reart_tau_schedule(long cur_iter, int n_iter, float end_t, float start_t) {
    const double c = cos(3.14159265358979323846 * (double)cur_iter / (double)n_iter);
    return (float)((double)end_t + ((double)start_t - (double)end_t) * (c + 1.0) * 0.5);
}
#endif
int reart_adam_ex(const AdamArgs &a, hipStream_t st);

// ---- kinematic.hip, shared with transform_grad.hip ---------------------------------------
#define PG_SLICES (256 / 12)   // point slices of pose_grad_kernel: twelve threads walk each, the slices are added in ascending order
// the slices' partial sums [B][PG_SLICES][P*12] of sum_{n in p} [G[t,n] x_n^T | G[t,n]] (N >= 1, B >= 1; launch only)
int reart_pose_grad_launch(const float *x, const int64_t *part, const float *G, int N, int P, int B, float *partial, hipStream_t st);
// reart_fk_backward with an upstream g_trans [B,P,4,4] (nullable) on the forward's `trans`; N = 0: x, part, G may be NULL
int reart_fk_backward_launch(const float *x, const int64_t *part, const float *G, int N, const int32_t *parent,
                             const int32_t *edge_of_part, const int32_t *order, int P, const float *axis, const float *moment,
                             const float *theta, const float *distance, int B, int E, const float *trans, const float *g_trans,
                             float *g_axis, float *g_moment, float *g_theta, float *g_distance, void *workspace,
                             size_t workspace_bytes, hipStream_t st);

// generic K-NN driver (knn.hip): njobs in {1,2}; job j searches q[j] ([N,P1[j],3] AoS) in t[j]
// ([N,P2[j],3] AoS); outputs dists/idx [N,P1[j],K].  Workspace: see knn_plan().
int reart_knn_run(int njobs, const float *const *q, const float *const *t,
                  const int64_t *const *lenq, const int64_t *const *lent, int N, const int *P1,
                  const int *P2, int K, int euclidean, float *const *dists, int64_t *const *idx,
                  void *workspace, size_t workspace_bytes, hipStream_t st);

// ---- K-NN internals (knn.hip) -----------------------------------------------------------
#define NN_BS 64   // threads per workgroup (one wave)
#define NN_UB 16   // targets per unrolled block; slice lengths are multiples of this
struct SoaJob {
    const float *src;
    const int64_t *len;  // nullable
    float *dst;
    int P, Ppad;
};
struct SoaArgs {
    SoaJob job[2];
};

// The members a search wave of prune.hip needs come first and are contiguous (q ... tlen, 88 bytes: SearchHot in prune.hip mirrors
// them): the search kernel picks its job at run time and fetches that run in one batch of wide scalar loads at its entry, instead of
// member by member where each is first used.
struct KnnJob {
    const float *q;        // [N,P1,3] AoS queries
    const float *q_alt;    // fused step: query cloud used where qmap[b] < 0
    const float *tsoa;     // [N,3,Ppad] SoA targets
    const float *boxes;    // nullable [N][Ppad/NN_BOX][8]: AABB (lo xyz, hi xyz, pad) of every NN_BOX targets
    const int *seed;       // pruned search only: [N][P1][KK] candidate neighbour indices (warm start); K = 1: may alias pi
    float *pd;             // partial dists [S][N][P1][KK]   (S > 1)
    int *pi;               // partial idx   [S][N][P1][KK]
    unsigned int *cost;    // pruned search only, nullable: [N * nqg] work done for the pair at each launch position
                           // (boxes tested and scanned, all waves), input of the next launch's order
    int P1, Ppad;          // Ppad = S*L, L % NN_UB == 0
    int nqg;               // ceil(P1/64)
    int P2;
    const int *tlen;       // nullable per-batch target count (ragged SoA rows, stride Ppad)
    unsigned int nqg_rcp;  // pruned search only: reart_div_magic(nqg), set by the search launcher (the wave splits its pair
                           // b * nqg + g with one multiply-high, reart_div_by_magic below)
    int L;
    // ---- not read by a search wave whose launch has item words (SearchArgs::item)
    const int *qmap;       // nullable per-batch query frame index into q
    const int64_t *lenq;   // nullable, rows >= lenq[n] produce zeros
    const int64_t *lent;   // nullable, number of valid targets
    const int *border;     // pruned search only, nullable: [N * nqg] (batch, query group) pair = b * nqg + g handled at
                           // launch position k (launches without item words; with them the word holds the pair)
    float *dists;          // final [N,P1,K]
    int64_t *idx;          // final [N,P1,K]
};
struct KnnArgs {
    KnnJob job[2];
    int N, S, K, euclidean;
    int items0;            // work items belonging to job 0
    int items;             // total work items
};

int reart_knn_launch_slices(const KnnArgs &a, int KK, hipStream_t st);
int reart_soa_launch(const SoaArgs &sa, int maxPpad, int N, int njobs, hipStream_t st);
int reart_knn_pick_split(long waves, int P2, int K);

// ---- K-NN for REART_MAX_K < K <= REART_MAX_K_LIST (knn_list.hip) ---------------------------
size_t reart_knn_list_workspace_bytes(int N, int P1, int P2, int K);
int reart_knn_list_run(const float *q, const float *t, const int64_t *lenq, const int64_t *lent, int N, int P1,
                       int P2, int K, int euclidean, float *dists, int64_t *idx, void *workspace,
                       size_t workspace_bytes, hipStream_t st);
// ---- K-NN for 1 <= D <= REART_MAX_D, T = float (D != 3) or double (knn_anyd.hip) -----------
template <class T>
int reart_knn_anyd_run(const T *q, const T *t, const int64_t *lenq, const int64_t *lent, int N, int P1, int P2, int D,
                       int K, int euclidean, T *dists, int64_t *idx, void *workspace, size_t workspace_bytes,
                       hipStream_t st);
#ifndef NN_BOX
#define NN_BOX 16   // targets per bounding box of the block-skip test (16, 32 or 64; measured 4545 / 4438 / 4321 it/s)
#endif
int reart_boxes_launch(const float *soa, int N, int Ppad, float *boxes, hipStream_t st);
// One launch position of a search job as ONE word, written by whoever lays the order down (relax_init_kernel; the counting
// sort of post_kernel moves the words as they are): the (batch, query group) pair that runs there in the low bits and the
// batch's query frame -- qmap[b], or b where the job has no map -- above them, plus one so that -1 (q_alt) is 0.  A search
// workgroup then has its query cloud after one load instead of border[pos] followed by qmap[b].  (A 16-byte record that
// also held the batch's target count was the first design; the step's workspace has 4 bytes per position and its size is
// part of the library's contract, and the count is a scalar load of tlen[b] that travels beside the query and the seeds.)
#define SEARCH_ITEM_PAIR_BITS 21
#define SEARCH_ITEM_PAIR_MASK ((1u << SEARCH_ITEM_PAIR_BITS) - 1u)
#if defined(__HIPCC__)
#define REART_HD __host__ __device__
#else
#define REART_HD
#endif
REART_HD static inline bool reart_search_items_fit(long pairs, int frames) {   // else: border / qmap (KnnJob), as the stand-alone operators
    return pairs <= (long)SEARCH_ITEM_PAIR_MASK && frames + 1 < (1 << (32 - SEARCH_ITEM_PAIR_BITS));
}
REART_HD static inline unsigned int reart_search_item(int pair, int qb) { return (unsigned int)pair | ((unsigned int)(qb + 1) << SEARCH_ITEM_PAIR_BITS); }
// n / d without a division where d is known in front of the launch: m = floor((2^32 - 1) / d) (the host, once), then
// q' = high word of n * m and ONE correction.  m >= (2^32 - d) / d, so n * m / 2^32 >= n / d - n / 2^32 > n / d - 1 for every
// n < 2^32, and m <= 2^32 / d, so q' <= n / d: q' is the quotient or one below it, whatever d >= 1 -- exact for every query-group
// count and every pair an item word or an order array can hold (tests/test_search_item_div_cpu.py walks them).  A software
// division is ~ 45 instructions with a v_rcp_iflag_f32 and a v_readfirstlane on a search wave's dependent chain.
REART_HD static inline unsigned int reart_div_magic(unsigned int d) { return 0xFFFFFFFFu / d; }
REART_HD static inline unsigned int reart_div_by_magic(unsigned int n, unsigned int d, unsigned int m) {
    const unsigned int q = (unsigned int)(((unsigned long long)n * m) >> 32);
    return q + (n - q * d >= d ? 1u : 0u);
}
// Frame offsets of a search job in 32 bits: true when the largest BYTE offset a search wave forms from a frame's base --
// queries [frames][P1][3], seeds and records [B][P1][K] (4 bytes each), targets [B][3][Ppad], boxes [B][Ppad / NN_BOX][8] --
// stays below 2^31 for the job (a frame's index times its stride is then an s_mul_i32 and one 64-bit add to the base).
// B: batches; q holds one query cloud per batch (qmap and the item words permute them: a query frame is < B).
REART_HD static inline bool reart_search_off32(long long B, long long P1, long long Ppad, int K) {
    const long long lim = 1ll << 31;
    return B * P1 * 3 * 4 < lim && B * P1 * K * 4 < lim && B * 3 * Ppad * 4 < lim && B * (Ppad / NN_BOX) * 8 * 4 < lim;
}
// exact search with box pruning + warm start (prune.hip): ONE launch for up to two K = 1 jobs (the Chamfer
// directions) and one K = 3 job (the flow search); one workgroup per (job, batch, query group), S waves each.
// The words that pick a workgroup's item and its record come first (one scalar load), the jobs behind them.
struct SearchArgs {
    int n1, n3;                    // K = 1 jobs k1[0 .. n1) (0, 1 or 2: the Chamfer directions) and K = 3 job k3 (0 or 1: the flow search)
    int G;                         // (batch, query group) pairs per job = B * nqg (the same for every job)
    int per;                       // pairs per XCD chunk = ceil(G / 8) (set by the launcher)
    int S1, S3;                    // waves per workgroup of a K = 1 / K = 3 item (1..4)
    int interleave;                // 0: XCD x runs the positions [x*per, (x+1)*per) (a run of frames per L2); 1: positions
                                   // x, x+8, ... (every XCD sees every frame: balanced whatever the frames cost)
    int sparse;                    // boxes needed by <= sparse queries of a wave go through the (query, box) queue (0: dense only)
    const unsigned int *item;      // nullable: [3][G] item words (reart_search_item) by launch position, row j for k1[j], row 2 for
                                   // k3.  NULL: the item comes from the job's border / qmap (the stand-alone warm operators)
    unsigned long long *prof;      // nullable: [grid][2] wall-clock stamps of every workgroup (start, end)
    unsigned int *prof_pairs;      //           [grid] distance evaluations executed by the workgroup
    int share;                     // 1: every lane's bound also takes the seeds of the 15 other lanes of its row (neighbour seeds)
    int cloud_resident;            // 1: when the target clouds fit in LDS, one workgroup of 16 waves per (job, batch, 16
                                   // query groups) with the cloud copied into LDS (knn_cloud_kernel); S1 / S3 then unused
    int cloud_slices;              // cloud-resident form: box slices per query group, 1 | 2 | 4 | 8 (0: the default, 4)
    int k_nqg;                     // query groups per batch (set by the launcher)
    int wide;                      // 1: 64-bit frame offsets also where 32 bits would do (the form very large clouds take; tests)
    KnnJob k1[2];                  // K = 1 jobs; results pd / pi [B][P1] (pi int32: also the next seed)
    KnnJob k3;                     // K = 3 job; results pd / pi [B][P1][3]: the three best 8-target BLOCKS
                                   // (block minimum, first index), rescanned with the exact key by the consumer
};
int reart_search_launch(const SearchArgs &a, hipStream_t st);
int reart_search_launch_batch(const SearchArgs *a, int K, hipStream_t st);          // group form only, same shapes
int reart_search_grid(int n1, int n3, int G);   // workgroups of that launch (an upper bound for both forms)
int reart_search_grid_cloud(int n1, int n3, int G, int nqg, int slices);
int reart_search_workgroups(const SearchArgs &a);   // of the form reart_search_launch will pick for `a`

#ifdef __HIPCC__
// branch-free insertion of key (d, j) into an ascending top-3 list ordered by (distance, index)
__device__ __forceinline__ void reart_top3_insert(float (&kd)[3], int (&ki)[3], float d, int j) {
    const bool l0 = (d < kd[0]) | ((d == kd[0]) & (j < ki[0]));
    const bool l1 = (d < kd[1]) | ((d == kd[1]) & (j < ki[1]));
    const bool l2 = (d < kd[2]) | ((d == kd[2]) & (j < ki[2]));
    kd[2] = l1 ? kd[1] : (l2 ? d : kd[2]);
    ki[2] = l1 ? ki[1] : (l2 ? j : ki[2]);
    kd[1] = l0 ? kd[0] : (l1 ? d : kd[1]);
    ki[1] = l0 ? ki[0] : (l1 ? j : ki[1]);
    kd[0] = l0 ? d : kd[0];
    ki[0] = l0 ? j : ki[0];
}
#endif

// ---- exact grid search over static target sets (grid.hip) -----------------------------------
struct GridBuildArgs {
    const float *pts;         // AoS points; set e starts at pts + 3 * off(e)
    const int *offsets;       // [E+1] prefix offsets (ragged) or NULL -> e * N
    int N;                    // points per set when offsets == NULL; max set size otherwise
    int stride;               // row stride of the sorted SoA arrays (>= max set size)
    float *gx, *gy, *gz;      // [E][stride] coordinates sorted by cell
    int *gorig;               // [E][stride] original index of each sorted point
    int *cell_start;          // [E][GR_CELLS + 1]
    float *meta;              // [E][GR_META]
    int *scratch;             // [E][3 * stride] ints: cell id | sort ping | pong
};

struct GridQueryArgs {
    const float *q;           // [E][nq][3] AoS queries
    const float *q_alt;       // used where qmap[e] < 0
    const int *qmap;          // nullable per-set query frame index
    int nq, E, stride, euclid_unused;
    const float *gx, *gy, *gz;
    const int *gorig, *cell_start;
    const float *meta;
    float *od;                // [E][nq][KK] squared distances, ascending
    int *oi;                  // [E][nq][KK] original indices
};

size_t reart_grid_bytes(int E, int stride);
void reart_grid_layout(void *mem, int E, int stride, GridBuildArgs *b);
int reart_grid_build_launch(const GridBuildArgs &b, int E, hipStream_t st);
int reart_grid_query_launch(const GridQueryArgs &q, int K, hipStream_t st);
