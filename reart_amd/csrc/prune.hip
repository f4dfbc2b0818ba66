// reart_amd/csrc/prune.hip -- EXACT nearest-neighbour search with bounding-box pruning and a
// warm start, for the relaxation loop (reference run_robot.py:154-221: every iteration repeats the
// Chamfer search of utils/chamfer.py:78-94 and the k=3 search of utils/flow_utils.py:158 on clouds
// that moved a little since the previous iteration).
//
// Same answer, bit for bit, as the brute-force kernels of knn.hip (same distance expression,
// strict '<', ties -> lowest index); what changes is how many targets are looked at.
//
//   * Clouds are stored in the leaf order of a balanced k-d tree (host side, relax.kd_order), so 16
//     consecutive targets form a compact box and the 64 queries of a wave are neighbours.
//   * Warm start: the neighbour indices of the PREVIOUS iteration (any valid indices would do)
//     give each query an upper bound thr on its K-th neighbour distance before anything is
//     scanned:  thr = max_k d(q, t[seed_k])  over K distinct seeds.
//   * Coarse filter, one box per lane: the wave's queries are summarised by 4 group boxes
//     (16 lanes each) with the group's largest thr; a target box survives if its box-to-box
//     lower bound is <= that thr for some group.  One ballot gives the survivor mask of 64 boxes.
//   * Precise filter, one query per lane: point-to-box lower bound against the lane's own thr
//     (which keeps shrinking as better candidates are found); the box is scanned if any lane
//     needs it.  Scanning is the brute-force inner loop of knn.hip in packed fp32; the 48 coordinates
//     of a scanned box are fetched through the vector memory path (lane l < 48 loads one float) into
//     a small LDS buffer and read back as broadcasts (a chain of scalar loads per scanned box -- the
//     brute-force kernel's operand path -- stalled on scalar-cache misses here: boxes are visited in
//     a data-dependent order and each is one cache line per axis).
//
// Exactness.  Both lower bounds are evaluated with the operations of the distance itself,
//   lb = ((ex*ex)+(ey*ey))+(ez*ez),  e = max(lo - q, q - hi, 0)  per axis,
// and fp32 subtraction, multiplication and addition are monotone, so lb <= d(q,t) for every
// target t inside the box (and the box-to-box bound is <= the point-to-box bound of every query
// of the group).  A box is dropped only when lb > thr strictly; a target that beats or TIES the
// current K-th candidate has d <= thr and therefore sits in a box that is scanned.
//
// Launch shape.  One WORKGROUP per (job, batch b, query group g of 64): its S waves take the boxes
// round-robin (slice s = boxes base + lane*S + s), keep their candidates in registers, meet once in LDS,
// and wave 0 merges them by the full (distance, index) key, does the ONE exact rescan of the winning half
// box and writes ONE record per query -- no per-slice partial lists in memory, nothing for the consumer to
// merge.  The K = 1 record (int32 index) is also the next iteration's warm-start seed, in place.
// Launch positions are dealt to the XCDs round-robin (workgroup L runs on XCD L % 8 and takes every 8th (batch, group)
// pair: every XCD sees every frame, which balances the chip whatever the frames cost; a contiguous run of frames per
// XCD -- `interleave = 0`, tune_xcd -- was measured slower: frames differ 10x in work), heaviest pairs first (counting
// sort of last iteration's work counts, step.hip).
//
//   * The head of a search workgroup (knn_group_kernel; read off the emitted gfx950 code, hipcc -S).  Entry: the words that
//     pick the item (n1 ... sparse, the item pointer, prof, share) in ONE batch of scalar loads and one wait; scalar
//     arithmetic on blockIdx gives (job, launch position).  Then, still in front of the opening barrier, everything else is
//     requested: the position's item word (a scalar load -- the previous launch wrote it, the longest wait of the head; it
//     holds the (batch, query group) pair AND the batch's query frame, internal.h) and the job's members by value (KnnJob
//     keeps them contiguous: s_load_dwordx16 + x8 at the job's offset).  One wait, at the barrier.  Behind it the
//     batch's target count (scalar load of tlen[b], only the flow job has one), the query (one global_load_dwordx3 through a
//     uniform base + 32-bit lane offset) and the K seeds are requested together; the count is wanted when the seeds are in.
//     All 3 K seed targets are gathered through the clamped index before the first LDS store (+inf is chosen at the store).
//     Global round trips from entry to the neighbour-seed bound: item word -> {query, seeds, count} -> seed targets, for
//     both kinds of item.  Before: the job's members one scalar load and one wait each where first used (about a dozen), the
//     order array as a vector load + v_readfirstlane, for the flow job qmap[b] the same way behind it, the count as a
//     flat_load, and the K = 3 seed targets in three dependent groups (2 + 4 + 3 loads) -- six round trips for a flow item.
//     Launches without item words (SearchArgs::item == NULL, the stand-alone warm operators) keep border[pos] -> qmap[b].
//   * The filter loop of a search wave (knn_pruned_wave; read off the emitted gfx950 code as well, counts in
//     profiles/filter_stream_isa_counts.txt).  The launch is bound by what a SIMD can issue, and most of what it issues is the
//     filter: coarse rounds, precise steps, queue appends.  In the group form (BOXL) a precise step of two boxes is 20 VALU
//     instructions, 18 of arithmetic and one v_mov_b32 per box for the LDS address: the coarse round parks a box's bounds as
//     (lo0, lo1) | (hi0, hi1) | (lo2, -hi2), the three register pairs the step works on.  The wave index is a scalar
//     (readfirstlane at the kernel's entry), so box addresses, the box number of an enqueue and the statistics counter are
//     SALU work.  The loop that judges boxes only enqueues; a dense scan or a drain is done outside it, so the candidates
//     are loop-invariant where most boxes pass, and it has ONE exit on one scalar (the survivor mask): a box no lane needs
//     costs 1 VALU, an enqueued one 5.  Before: 31 per step (nine register shuffles, two 64-bit multiply-adds for the
//     addresses), a v_add per counter event, and 14 copies of the candidates per enqueued box of a K = 3 item.  Per launch
//     of the headline shape 12.7 M -> 9.5 M VALU instructions, 32.5 -> 29.1 us.  The cloud-resident form (BOXL = false: bounds in the lanes of the coarse
//     round, read with v_readlane) keeps the per-box pairing it had -- it sits at 80 VGPRs and the axis form cost it a
//     resident wave -- and takes the same loop structure and the one-block coarse round.  Every form evaluates the same
//     operations in the same order: the filter's decisions, and with them the executed pairs, are bit for bit the same.
//   * The fixed part of a search wave (everything outside the filter loop; counts per region in
//     profiles/search_fixed_isa_counts.txt, tools/isa_regions.py).  Nearly half of the ~ 1 560 instructions a wave issues are set-up
//     and wrap-up that every wave repeats in the same form.  Cut where the result does not need them: the (batch, query group)
//     pair is split by a reciprocal of nqg the launcher puts beside it in the job (reart_div_by_magic, internal.h: one
//     s_mul_hi_u32 and one correction where a software division took ~ 45 instructions with a v_rcp_iflag_f32 and a
//     v_readfirstlane_b32 on the wave's chain); the frame bases are s_mul_i32 products where the launcher finds every offset
//     below 2^31 bytes (template parameter OFF32, reart_search_off32; the 64-bit form stays for larger clouds); the order array
//     and the query map of launches without item words are scalar loads (as vector loads they made the query frame a vector
//     value for every launch: two v_mul_lo_u32 and two v_readfirstlane_b32 in front of the query load); the counter's seed term
//     is counted in the bound loop (it was a second software division); the partial bounds of the workgroup's waves are
//     exchanged by four reads at fixed offsets, two selects on S and a v_min3_f32 + v_min_f32 (the loop over S was ~ 76
//     instructions, two canonicalising v_max per fminf); the six coordinate summaries of the rows are ONE block of 24 DPP
//     steps taken across the values (1 s_nop for 24).  Per wave ~ 120 of ~ 650 fixed instructions; every operation that
//     decides anything is the same in the same order.
//   * Neighbour seeds (round 3).  A lane's own seed is a poor bound exactly when it matters: every iteration a fifth of
//     the points re-sample their part label and jump (queries of the x -> y search, targets of the y -> x search), their
//     old neighbour is then far away, and those lanes -- 23 % of them -- used to produce 78 % of all (query, box)
//     pairs.  But the 16 lanes of a row are neighbours on the canonical shape, and the lanes that landed next to a
//     jumped point hold seeds next to ITS new neighbour.  So the lanes of a row park their seed targets in LDS and
//     every lane takes  thr = min over the row's lanes l' of  max_k d(q, t[seed_{l',k}])  -- any K distinct targets
//     bound the K-th neighbour distance, whoever found them.  Measured on dumped states (tools/sim_filter.py):
//     (query, box) pairs per wave 675 -> 194 (x -> y), 1219 -> 508 (y -> x), 983 -> 305 (flow); boxes some lane needs
//     76 -> 34; coarse survivors 112 -> 70.
#include "common.h"
#include "internal.h"
#include <math.h>
#include <string.h>
#include <stddef.h>

typedef float f2 __attribute__((ext_vector_type(2)));
// the members of a job a search wave needs, as KnnJob lays them out (internal.h): copied by value at the kernel's entry
struct SearchHot {
    const float *q, *q_alt, *tsoa, *boxes;
    const int *seed;
    float *pd;
    int *pi;
    unsigned int *cost;
    int P1, Ppad, nqg, P2;
    const int *tlen;
    unsigned int nqg_rcp;
    int L;                 // not used: fills the run to 24 words (s_load_dwordx16 + x8)
};
static_assert(sizeof(SearchHot) == 96 && offsetof(KnnJob, tlen) == offsetof(SearchHot, tlen) && offsetof(KnnJob, q) == 0 && offsetof(KnnJob, q_alt) == offsetof(SearchHot, q_alt) &&
              offsetof(KnnJob, nqg_rcp) == offsetof(SearchHot, nqg_rcp) &&
              offsetof(KnnJob, tsoa) == offsetof(SearchHot, tsoa) && offsetof(KnnJob, boxes) == offsetof(SearchHot, boxes) &&
              offsetof(KnnJob, seed) == offsetof(SearchHot, seed) && offsetof(KnnJob, pd) == offsetof(SearchHot, pd) &&
              offsetof(KnnJob, pi) == offsetof(SearchHot, pi) && offsetof(KnnJob, cost) == offsetof(SearchHot, cost) &&
              offsetof(KnnJob, P1) == offsetof(SearchHot, P1) && offsetof(KnnJob, Ppad) == offsetof(SearchHot, Ppad) &&
              offsetof(KnnJob, nqg) == offsetof(SearchHot, nqg) && offsetof(KnnJob, P2) == offsetof(SearchHot, P2),
              "SearchHot mirrors the head of KnnJob");
// a wave-uniform word that no launch writes while this one runs (the previous launch wrote it): a scalar load, whatever the
// compiler can prove about the pointer -- as a plain load it came out as a vector load, a wait and a v_readfirstlane
__device__ __forceinline__ int pr_uniform_word(const void *p) { return *(const __attribute__((address_space(4))) int *)p; }
#define PR_SMAX 4       // most waves (box slices) per search workgroup
// (a box's targets are fetched when it is scanned: prefetching every coarse survivor eight at a time was measured -- more
// instructions, loads for the 60 % of the boxes the precise test rejects, no gain; DESIGN_HISTORY.md)
#define PR_QCAP 640     // words of a wave's queue space: the first 384 hold box bounds, 256 (query, box) entries (768: one
                        // workgroup less per compute unit, 32.9 vs 32.3 us; 512: drains too small and too many, 33.7 us)
#define PR_WPE 6         // waves per SIMD the compiler must allow for (register budget: 85 -> 80 VGPRs; the kernel sat at the
                         // edge -- 78 under this bound, 82 without it, no spills either way -- and the sixth wave is worth 7 %;
                         // with the wave index in a scalar register it needs 70 and the bound is also its maximum, see below)
// LDS per wave: staged box of a dense scan [64 floats] | the wave's queries [64][4] | result slots [3][64] u64 | queue
// The precise filter reads a surviving box's bounds back from LDS (broadcast ds_read, the LDS pipe is idle) instead of twelve
// v_readlane per box pair on the VALU, which bounds this kernel: 45.0 -> 43.6 us per launch.  The 1.5 KB come out of the
// queue's space (768 -> 384 entries); with LDS of their own a workgroup less fits a compute unit: 48.6 us.
#define PR_LDS_WAVE_BYTES (64 * 4 + 64 * 16 + 3 * 64 * 8 + PR_QCAP * 4)

#ifdef REART_PRUNE_STATS   // diagnostic build only (tools/prune_stats.py): how much the filters let through
__device__ unsigned long long g_prune_stats[8];
extern "C" int reart_debug_prune_stats(unsigned long long *out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prune_stats), sizeof(g_prune_stats)) != hipSuccess) return REART_ERR_LAUNCH;
    if (reset) { unsigned long long z[8] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_prune_stats), z, sizeof(z)); }
    return REART_OK;
}
#define PRUNE_STAT(k, v) do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_prune_stats[k], (unsigned long long)(v)); } while (0)
// events of the filter loop per kind of item (row 0: K = 1, row 1: K = 3), summed over waves (tools/filter_events.py): 0 coarse
// rounds, 1 boxes passing the coarse filter, 2 precise steps (two boxes each, the last of a round may hold one), 3 boxes some
// lane needs, 4 of them enqueued, 5 densely scanned, 6 drain steps, 7 waves
__device__ unsigned long long g_prune_events[2][8];
extern "C" int reart_debug_prune_events(unsigned long long *out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prune_events), sizeof(g_prune_events)) != hipSuccess) return REART_ERR_LAUNCH;
    if (reset) { unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_prune_events), z, sizeof(z)); }
    return REART_OK;
}
#define PRUNE_EVENT(k, v) do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_prune_events[KK == 1 ? 0 : 1][k], (unsigned long long)(v)); } while (0)
#else
#define PRUNE_STAT(k, v) do { } while (0)
#define PRUNE_EVENT(k, v) do { } while (0)
#endif
#ifdef REART_PRUNE_PHASE   // diagnostic build only (tools/phase_prof.py; make -C reart_amd/csrc phase)
// phase clocks of the search waves (s_memtime ticks summed over waves): 0 prologue (seeds, group summaries), 1 coarse
// filter, 2 precise tests, 3 dense scans, 4 queue appends, 5 queue drains, 6 barrier wait + merge + rescan, 7 waves
__device__ unsigned long long g_prune_phase[8];
extern "C" int reart_debug_prune_phase(unsigned long long *out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prune_phase), sizeof(g_prune_phase)) != hipSuccess) return REART_ERR_LAUNCH;
    if (reset) { unsigned long long z[8] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_prune_phase), z, sizeof(z)); }
    return REART_OK;
}
#define PH_DECL unsigned long long ph_t = __builtin_amdgcn_s_memtime(), ph_acc[7] = {0, 0, 0, 0, 0, 0, 0}
#define PH(k) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); ph_acc[k] += n_ - ph_t; ph_t = n_; } while (0)
#define PH_FLUSH(from, to) do { if ((threadIdx.x & 63) == 0) for (int k_ = from; k_ <= to; ++k_) atomicAdd(&g_prune_phase[k_], ph_acc[k_]); } while (0)
// the head of a search wave, K = 1 items in row 0 and K = 3 items in row 1 (ticks summed over waves): 0 kernel entry -> call of
// knn_pruned_wave (item decode, arguments, record), then inside the prologue 1 -> query in registers, 2 -> seeds in registers,
// 3 -> seed targets parked in LDS, 4 the whole prologue (phase 0 above), 5 entry -> end of the wave's search, 6 waves.
// A stamp makes its values an operand of an empty asm, so the compiler waits for them there: the stamps serialise what
// they measure and belong to this build only.  Everything is added to the counters at the END of the wave's search: vmcnt
// counts atomics too, and an atomic in front of a stamp would make the stamp wait for 10 944 waves' contention on one word.
__device__ unsigned long long g_prune_head[2][8];
extern "C" int reart_debug_prune_head(unsigned long long *out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prune_head), sizeof(g_prune_head)) != hipSuccess) return REART_ERR_LAUNCH;
    if (reset) { unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_prune_head), z, sizeof(z)); }
    return REART_OK;
}
#define PH_HEAD_DECL unsigned long long hd_t = ph_t, hd_acc[3] = {0, 0, 0}
#define PH_STAMP(k, ...) do { asm volatile("" :: __VA_ARGS__); const unsigned long long n_ = __builtin_amdgcn_s_memtime(); hd_acc[k] = n_ - hd_t; hd_t = n_; } while (0)
#define PH_HEAD_FLUSH(row) do { if ((threadIdx.x & 63) == 0) { for (int k_ = 0; k_ < 3; ++k_) atomicAdd(&g_prune_head[row][1 + k_], hd_acc[k_]); \
                                atomicAdd(&g_prune_head[row][4], ph_acc[0]); atomicAdd(&g_prune_head[row][6], 1ull); } } while (0)
#define PH_ENTRY const unsigned long long hd_entry = __builtin_amdgcn_s_memtime(); unsigned long long hd_head = 0ull
#define PH_HEAD_END do { hd_head = __builtin_amdgcn_s_memtime() - hd_entry; } while (0)
#define PH_ENTRY_FLUSH(row) do { if ((threadIdx.x & 63) == 0) { atomicAdd(&g_prune_head[row][0], hd_head); \
                                 atomicAdd(&g_prune_head[row][5], __builtin_amdgcn_s_memtime() - hd_entry); } } while (0)
#else
#define PH_DECL do { } while (0)
#define PH(k) do { } while (0)
#define PH_FLUSH(from, to) do { } while (0)
#define PH_HEAD_DECL do { } while (0)
#define PH_STAMP(k, ...) do { } while (0)
#define PH_HEAD_FLUSH(row) do { } while (0)
#define PH_ENTRY do { } while (0)
#define PH_HEAD_END do { } while (0)
#define PH_ENTRY_FLUSH(row) do { } while (0)
#endif

// -DREART_PRUNE_MARKS (tools/isa_regions.py): a comment line in the emitted code where a region of a search wave's fixed part
// begins -- no instruction, but the scheduler may move arithmetic across it, so region counts are good to a few instructions
#ifdef REART_PRUNE_MARKS
#define PR_MARK(name) asm volatile("; PRMARK " name)
#else
#define PR_MARK(name) do { } while (0)
#endif

#define PR_WORK(w) ((unsigned)(w) << 20)   // the work count lives in bits 20..31 of a wave's statistics counter, the pairs below

// min / max of a lane's value with a DPP-permuted copy in ONE instruction (v_min_f32_dpp).  Written through the compiler
// the same step is three (v_mov_b32_dpp, a canonicalising v_max v,v -- fminf of a value of unknown origin -- and the
// v_min); the item prologue alone has 28 such steps.  Only used where EXEC is full (every source lane is live); the
// s_nop covers the two wait states a DPP read needs after a VALU write of the same register, which the hazard
// recogniser does not insert for inline assembly.  No signalling NaNs exist here; quiet NaNs behave like fminf / fmaxf.
#define PR_DPP_OP(NAME, OP, CTRLTXT)                                                                              \
    __device__ __forceinline__ float NAME(float v) {                                                              \
        float r;                                                                                                  \
        asm("s_nop 1\n\t" OP " %0, %1, %1 " CTRLTXT " row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v));            \
        return r;                                                                                                 \
    }
PR_DPP_OP(pr_min_q1, "v_min_f32_dpp", "quad_perm:[1,0,3,2]")
PR_DPP_OP(pr_min_q2, "v_min_f32_dpp", "quad_perm:[2,3,0,1]")
PR_DPP_OP(pr_min_hm, "v_min_f32_dpp", "row_half_mirror")
PR_DPP_OP(pr_min_rm, "v_min_f32_dpp", "row_mirror")
PR_DPP_OP(pr_max_q1, "v_max_f32_dpp", "quad_perm:[1,0,3,2]")
PR_DPP_OP(pr_max_q2, "v_max_f32_dpp", "quad_perm:[2,3,0,1]")
PR_DPP_OP(pr_max_hm, "v_max_f32_dpp", "row_half_mirror")
PR_DPP_OP(pr_max_rm, "v_max_f32_dpp", "row_mirror")
__device__ __forceinline__ float pr_row16_min(float v) { return pr_min_rm(pr_min_hm(pr_min_q2(pr_min_q1(v)))); }
__device__ __forceinline__ float pr_row16_max(float v) { return pr_max_rm(pr_max_hm(pr_max_q2(pr_max_q1(v)))); }
// The six row summaries of the query's coordinates (minimum and maximum per axis) in ONE block: the four steps are taken
// across the six values, so five instructions stand between a write and the DPP read of it and the block needs one s_nop
// (for whatever wrote the inputs) where six chains of pr_row16_* issue 24.  Outputs are early-clobber: the inputs are read
// by steps behind the first writes.  Same instructions, same operands per value: the same bits.
#define PR_ROW6_STEP(A, B, C, CTRLTXT)                                                                            \
    "v_min_f32_dpp %0, " A ", " A " " CTRLTXT " row_mask:0xf bank_mask:0xf\n\t"                                   \
    "v_min_f32_dpp %1, " B ", " B " " CTRLTXT " row_mask:0xf bank_mask:0xf\n\t"                                   \
    "v_min_f32_dpp %2, " C ", " C " " CTRLTXT " row_mask:0xf bank_mask:0xf\n\t"
#define PR_ROW6_STEPX(A, B, C, CTRLTXT)                                                                           \
    "v_max_f32_dpp %3, " A ", " A " " CTRLTXT " row_mask:0xf bank_mask:0xf\n\t"                                   \
    "v_max_f32_dpp %4, " B ", " B " " CTRLTXT " row_mask:0xf bank_mask:0xf\n\t"                                   \
    "v_max_f32_dpp %5, " C ", " C " " CTRLTXT " row_mask:0xf bank_mask:0xf\n\t"
__device__ __forceinline__ void pr_row16_box(float x, float y, float z, float &l0, float &l1, float &l2, float &h0, float &h1, float &h2) {
    asm("s_nop 1\n\t"
        PR_ROW6_STEP("%6", "%7", "%8", "quad_perm:[1,0,3,2]") PR_ROW6_STEPX("%6", "%7", "%8", "quad_perm:[1,0,3,2]")
        PR_ROW6_STEP("%0", "%1", "%2", "quad_perm:[2,3,0,1]") PR_ROW6_STEPX("%3", "%4", "%5", "quad_perm:[2,3,0,1]")
        PR_ROW6_STEP("%0", "%1", "%2", "row_half_mirror") PR_ROW6_STEPX("%3", "%4", "%5", "row_half_mirror")
        PR_ROW6_STEP("%0", "%1", "%2", "row_mirror") PR_ROW6_STEPX("%3", "%4", "%5", "row_mirror")
        : "=&v"(l0), "=&v"(l1), "=&v"(l2), "=&v"(h0), "=&v"(h1), "=&v"(h2) : "v"(x), "v"(y), "v"(z));
}
// minimum of three / two floats that are never NaN, in ONE instruction each: fminf of a value the compiler has not computed
// itself (an LDS read) is wrapped in a canonicalising v_max x,x per operand
__device__ __forceinline__ float pr_min3(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float pr_min2(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a frame's base inside an array of 4-byte elements, n1 * n2 elements per frame.  OFF32 (the launcher: reart_search_off32):
// every such offset of the launch is below 2^31 bytes, so it is s_mul_i32 products and a 64-bit add; otherwise every
// product is formed in 64 bits from the first factor on (s_mul_i32 + s_mul_hi_u32 + the cross terms per factor)
template <bool OFF32>
__device__ __forceinline__ const char *pr_frame(const void *base, int frame, int n1, int n2) {
    if (OFF32) return (const char *)base + (size_t)(4u * (unsigned)frame * (unsigned)n1 * (unsigned)n2);
    return (const char *)base + 4 * ((size_t)frame * (size_t)n1 * (size_t)n2);
}

__device__ __forceinline__ float rl(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

__device__ __forceinline__ float box_lb(float lo0, float lo1, float lo2, float hi0, float hi1, float hi2,
                                        float qlo0, float qlo1, float qlo2, float qhi0, float qhi1, float qhi2) {
    const float ex = fmaxf(fmaxf(lo0 - qhi0, qlo0 - hi0), 0.f);
    const float ey = fmaxf(fmaxf(lo1 - qhi1, qlo1 - hi1), 0.f);
    const float ez = fmaxf(fmaxf(lo2 - qhi2, qlo2 - hi2), 0.f);
    return (ex * ex + ey * ey) + ez * ez;
}

// One WAVE of a search workgroup: the 64 queries of group g of batch b against the boxes of slice s (boxes
// base + lane * S + s of every round).  Leaves, per lane (= query): KK = 1 the smallest distance found and the
// half box (8 targets) that holds it; KK = 3 the three best 8-target blocks by (minimum, first index).
// `pairs` counts the query-target distance evaluations the wave executed (lanes x targets, dense and sparse forms).
// LDSV: `cloud` / `boxes_p` point at a copy of the batch's target cloud (SoA rows of `cstride` floats) and of its boxes in
// LDS (knn_cloud_kernel); otherwise at the global images.  QCAP: entries of the wave's queue.
// share: neighbour seeds (parked in the queue's space, which is free until the first coarse round: s_bb | s_q when BOXL,
// s_q otherwise; skipped when that space is too small for KK x 3 x 64 floats).
// The caller has resolved what depends on the batch: `qcloud` the query cloud [P1][3] of batch b (q + qmap[b] * P1 * 3, or
// q_alt), `seed_p` the job's seeds, `n2` the batch's target count -- nothing here waits for a per-batch word.
template <int KK, bool LDSV, int QCAP, bool BOXL, bool OFF32>
__device__ __forceinline__ void knn_pruned_wave(const float *qcloud, const int *seed_p, const int P1, const int n2,
                                                const int S, const int sparse, const int b, const int g,
                                                const int s, const float *cloud, const int cstride, const float *boxes_p,
                                                float *s_tg, float *s_qc, unsigned int *s_q, float *s_bb, const int share, float *s_xthr,
                                                unsigned long long *s_key, float &qx_o, float &qy_o, float &qz_o,
                                                float (&bm)[KK], int (&bb)[KK], int &work_o, unsigned int &pairs_o) {
    struct { int S, sparse; } a = {S, sparse};
    const int lane = threadIdx.x & 63;
    PH_DECL;
    PH_HEAD_DECL;

    const int i = g * NN_BS + lane;
    const int ic = i < P1 ? i : P1 - 1;
    // (wave-uniform base) + (32-bit lane offset in bytes), as in the drain: no 64-bit lane address to build or keep
    const float *qp = (const float *)((const char *)qcloud + 12u * (unsigned)ic);
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    PR_MARK("seeds");
    PH_STAMP(0, "v"(qx), "v"(qy), "v"(qz));
    const f2 qx2 = {qx, qx}, qy2 = {qy, qy}, qz2 = {qz, qz};
    const f2 qxy = {qx, qy}, qzn = {-qz, qz};             // the precise filter's operands (paired by axis)

    const float *tx = cloud;
    const float *ty = tx + cstride;
    const float *tz = ty + cstride;
    const int nbox = (n2 + NN_BOX - 1) / NN_BOX;
    const float *bx = boxes_p;

    // ---- warm start
    float thr = 0.f;
    unsigned int wp = 0u;             // statistics counter, see PR_WORK below
    {
        const int *sd = (const int *)(pr_frame<OFF32>(seed_p, b, P1, KK) + 4u * KK * (unsigned)ic);
        int sj[KK];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < KK; ++k) {
            sj[k] = sd[k];
            ok = ok && sj[k] >= 0 && sj[k] < n2;
#pragma unroll
            for (int k2 = 0; k2 < k; ++k2) ok = ok && sj[k] != sj[k2];
        }
        PH_STAMP(1, "v"(sj[0]), "v"(sj[KK - 1]), "s"(n2));
        // scratch for the neighbour seeds: the result slots (s_key, 384 floats, initialised after this block) and the queue's
        // space behind them (box bounds | queue) are contiguous and idle until the first coarse round
        constexpr bool SCR_JOINT = BOXL;                         // s_bb | s_q contiguous
        constexpr bool SCR_FITS = (384 + QCAP + (SCR_JOINT ? 384 : 0)) >= KK * 3 * 64;
        if (SCR_FITS && share) {
            // ---- neighbour seeds: the K seed targets of every lane of this row of 16 (the lane's own among them), two lanes
            // per packed step.  A lane without usable seeds parks +inf (its candidates bound nothing -- but it still takes its
            // neighbours' bound); LDS operations of a wave complete in order, and every lane reads only its own row.
            // All 3 K gathers are in flight before the first LDS store: the index is clamped, so the loads need no guard, and
            // the +inf is chosen at the store.  (Guarded loads -- ok ? tx[j] : INFINITY -- were compiled into one exec-mask
            // block per seed, each waiting for its own loads before its stores: three round trips for a K = 3 item.)
            float *s_scr = (float *)s_key;
            float sx[KK], sy[KK], sz[KK];
#pragma unroll
            for (int k = 0; k < KK; ++k) {
                // (wave-uniform row) + (32-bit lane offset in bytes), as the query's load: no 64-bit lane address per row
                const unsigned jo = 4u * (unsigned)(ok ? sj[k] : 0);
                sx[k] = *(const float *)((const char *)tx + jo); sy[k] = *(const float *)((const char *)ty + jo);
                sz[k] = *(const float *)((const char *)tz + jo);
            }
            if (!LDSV) __builtin_amdgcn_sched_barrier(0);      // the scheduler must not sink a gather below a store
#pragma unroll
            for (int k = 0; k < KK; ++k) {
                s_scr[(3 * k + 0) * 64 + lane] = ok ? sx[k] : INFINITY;
                s_scr[(3 * k + 1) * 64 + lane] = ok ? sy[k] : INFINITY;
                s_scr[(3 * k + 2) * 64 + lane] = ok ? sz[k] : INFINITY;
            }
            PH_STAMP(2, "v"(lane));
            PR_MARK("bound");
            thr = INFINITY;
            const float *row = s_scr + (lane & 48);
            // s_xthr (the workgroup's exchange array [S][64]): the S waves of the workgroup hold the same 64 queries, so each
            // evaluates every S-th candidate pair and the partial bounds meet after ONE barrier (at the start of the waves'
            // lives, where they still run side by side); without it every wave evaluates all 16 candidates
            const bool split = s_xthr != nullptr && a.S > 1;
            const int c0 = split ? 2 * s : 0, cstep = split ? 2 * a.S : 2;
#pragma unroll 1      // rolled: unrolled, the 72 LDS loads of a K = 3 item in flight cost 25 VGPRs, i.e. two resident waves per SIMD
            for (int c = c0; c < 16; c += cstep) {
                f2 far = {0.f, 0.f};
#pragma unroll
                for (int k = 0; k < KK; ++k) {
                    const f2 dx = qx2 - *(const f2 *)(row + (3 * k + 0) * 64 + c);
                    const f2 dy = qy2 - *(const f2 *)(row + (3 * k + 1) * 64 + c);
                    const f2 dz = qz2 - *(const f2 *)(row + (3 * k + 2) * 64 + c);
                    const f2 d = (dx * dx + dy * dy) + dz * dz;
                    far = f2{fmaxf(far.x, d.x), fmaxf(far.y, d.y)};
                }
                thr = fminf(thr, fminf(far.x, far.y));
                wp += 64u * KK * 2u;                 // the seed candidates this wave evaluates: counted where they are, one s_add a
                                                     // trip (as (16 - c0 + cstep - 1) / cstep in front of the loop: a software division)
            }
            PR_MARK("exchange");
            if (split) {
                s_xthr[64 * s + lane] = thr;
                __syncthreads();                     // every live wave of the workgroup runs this prologue (waves >= S have left)
                // The minimum over the S live waves' slots, the wave's own among them: four reads at fixed offsets, the slots of
                // waves that do not exist (never written: any bits) replaced by +inf on a uniform condition, two instructions of
                // minima.  (As `for (t < a.S) thr = fminf(thr, s_xthr[..])` the loop was unrolled by two with exit flags and every
                // fminf canonicalised both operands: ~ 76 instructions.)  No operand is ever NaN: a partial bound is a
                // fminf / fmaxf of squared distances, and fmaxf(0, NaN) = 0 drops the NaN a NaN or infinite query produces --
                // that query is dealt with below, by the test on the query itself.  The minimum of a set of non-NaN floats
                // does not depend on the order they are taken in, and +0 / -0 cannot both occur (distances are >= +0): the
                // same bits as the loop's.
                const float x0 = s_xthr[lane], x1 = s_xthr[64 + lane], x2 = s_xthr[128 + lane], x3 = s_xthr[192 + lane];
                thr = pr_min2(pr_min3(x0, x1, a.S > 2 ? x2 : INFINITY), a.S > 3 ? x3 : INFINITY);
            }
            // a NaN query: fmaxf / fminf drop the NaN distances (fmaxf(0, NaN) = 0), so the bound would come out 0, not NaN --
            // test the query itself and prune nothing for it (its lower bounds are NaN and fail every compare: index -1)
            if (!(qx == qx && qy == qy && qz == qz)) thr = INFINITY;
        } else {
#pragma unroll
            for (int k = 0; k < KK; ++k) {
                const int j = ok ? sj[k] : 0;
                thr = fmaxf(thr, reart_sqdist3(qx, qy, qz, tx[j], ty[j], tz[j]));
            }
            wp = 64u * KK;
            if (!ok || !(thr >= 0.f)) thr = INFINITY;   // unusable seeds / NaN: no pruning for this lane
        }
    }

    // ---- group summaries: 4 groups of 16 lanes
    PR_MARK("rows");
    float gl0, gl1, gl2, gh0, gh1, gh2;
    pr_row16_box(qx, qy, qz, gl0, gl1, gl2, gh0, gh1, gh2);
    const float gt = pr_row16_max(thr);
    float G[4][7];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        G[q][0] = rl(gl0, 16 * q); G[q][1] = rl(gl1, 16 * q); G[q][2] = rl(gl2, 16 * q);
        G[q][3] = rl(gh0, 16 * q); G[q][4] = rl(gh1, 16 * q); G[q][5] = rl(gh2, 16 * q);
        G[q][6] = rl(gt, 16 * q);
    }

#pragma unroll
    for (int k = 0; k < KK; ++k) { bm[k] = INFINITY; bb[k] = -1; }
    const float *tx_g = tx;
    // ONE uniform counter for both statistics (a scalar register less, one s_add per event): bits 0..19 the distance
    // evaluations, bits 20..31 the work count that orders the next launch (a heuristic: overflow is harmless).  `pairs` is
    // the evaluation count only while a wave stays below 2^20 of them, i.e. while it scans or drains fewer than 16 384 targets:
    // every cloud of the headline shapes, warm or cold.  A cold wave over a larger slice (65 536 targets at S = 4) carries into
    // the work count and reports the count modulo 2^20; no result depends on either field (the order of the next launch does,
    // through buckets clamped to 255 -- tests/test_search_large_gpu.py runs such clouds, profiled and not, bit for bit)
    wp |= PR_WORK(16);                                                   // prologue ~ 16 tests

    const int queue_max = a.sparse;   // boxes needed by at most this many queries go through the (query, box) queue (0: off)
    int qcnt = 0;                     // entries in the wave's queue (uniform)
    // the wave's queries, parked once for the drain steps (a lane then evaluates ANOTHER lane's query)
    ((float4 *)s_qc)[lane] = make_float4(qx, qy, qz, 0.f);
    if (KK == 1) s_key[lane] = ~0ull;
    else { s_key[lane] = ~0ull; s_key[64 + lane] = ~0ull; s_key[128 + lane] = ~0ull; }
    // Drain: 64 entries per step, one per lane.  The lane's 16 targets come straight from the SoA rows (three 64-byte
    // lines per lane); the distance expression is the contract's.  K = 1: the (minimum, half box) of the entry meets the
    // query's other entries in an LDS atomic minimum on the 64-bit key (distance bits, block start) -- distances are
    // non-negative, so the integer order is the (distance, index) order and the result does not depend on the order of
    // arrival.  K = 3: both half-box minima go through three such minima in a row, the loser of each level moving on to
    // the next: the three slots end as the three smallest keys, again whatever the order.  Afterwards every lane folds
    // its query's slots into its registers (and its bound) and clears them.
    auto drain_queue = [&]() {
        for (int e0 = 0; e0 < qcnt; e0 += 64) {
            wp += PR_WORK(6);
            PRUNE_EVENT(6, 1);
            const int e = e0 + lane;
            const bool valid = e < qcnt;
            const unsigned ent = s_q[valid ? e : e0];
            const int ql = (int)(ent & 63u), j0 = (int)(ent >> 6) * NN_BOX;
            wp += (unsigned)__builtin_popcountll(__ballot(valid)) * NN_BOX;
            const float4 qc = ((const float4 *)s_qc)[ql];
            // rows addressed as (wave-uniform base) + (32-bit lane offset): the scalar-base form of global_load keeps three
            // 64-bit lane pointers (and their adds) out of the VGPRs
            const float *rx = tx_g, *ry = tx_g + cstride, *rz = tx_g + 2 * (size_t)cstride;
            const f2 cx = {qc.x, qc.x}, cy = {qc.y, qc.y}, cz = {qc.z, qc.z};
            float mh[2] = {INFINITY, INFINITY};
            // one half box (8 targets: six 16-byte loads) at a time: the twelve loads of a whole box in flight cost 24 more
            // VGPRs than the rest of the kernel needs, i.e. a resident wave per SIMD
#pragma unroll 1
            for (int hf = 0; hf < 2; ++hf) {
                float4 X[2], Y[2], Z[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const unsigned ob = 4u * ((unsigned)j0 + 8u * hf + 4u * u);          // BYTE offset: zext(ob) is the address form
                    X[u] = *(const float4 *)((const char *)rx + ob);
                    Y[u] = *(const float4 *)((const char *)ry + ob);
                    Z[u] = *(const float4 *)((const char *)rz + ob);
                }
                float m = INFINITY;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const f2 dxa = cx - f2{X[u].x, X[u].y}, dya = cy - f2{Y[u].x, Y[u].y}, dza = cz - f2{Z[u].x, Z[u].y};
                    const f2 dxb = cx - f2{X[u].z, X[u].w}, dyb = cy - f2{Y[u].z, Y[u].w}, dzb = cz - f2{Z[u].z, Z[u].w};
                    const f2 da = (dxa * dxa + dya * dya) + dza * dza;
                    const f2 db = (dxb * dxb + dyb * dyb) + dzb * dzb;
                    m = fminf(fminf(m, fminf(da.x, da.y)), fminf(db.x, db.y));
                }
                if (hf == 0) mh[0] = m; else mh[1] = m;
            }
            if (KK == 1) {
                const float m = fminf(mh[0], mh[1]);
                const unsigned long long key = ((unsigned long long)__float_as_uint(m) << 32) | (unsigned)(j0 + (mh[1] < mh[0] ? 8 : 0));
                if (valid) atomicMin(&s_key[ql], key);
            } else if (valid) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    unsigned long long key = ((unsigned long long)__float_as_uint(mh[h]) << 32) | (unsigned)(j0 + 8 * h);
#pragma unroll
                    for (int lv = 0; lv < 3; ++lv) {
                        const unsigned long long old = atomicMin(&s_key[64 * lv + ql], key);
                        key = old > key ? old : key;
                    }
                }
            }
        }
        qcnt = 0;
        // fold the slots of this lane's own query into its registers
        if (KK == 1) {
            const unsigned long long k = s_key[lane];
            const float m = __uint_as_float((unsigned)(k >> 32));
            const int blk = (int)(unsigned)k;
            if (k != ~0ull && ((m < bm[0]) || (m == bm[0] && blk < bb[0]))) { bm[0] = m; bb[0] = blk; }
            thr = fminf(thr, bm[0]);
            s_key[lane] = ~0ull;
        } else {
            float kd[3];
            int ki[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { kd[c] = bm[c]; ki[c] = bb[c] >= 0 ? bb[c] : 0x7fffffff; }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned long long k = s_key[64 * c + lane];
                s_key[64 * c + lane] = ~0ull;
                if (k != ~0ull) reart_top3_insert(kd, ki, __uint_as_float((unsigned)(k >> 32)), (int)(unsigned)k);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) { bm[c] = kd[c]; bb[c] = ki[c] == 0x7fffffff ? -1 : ki[c]; }
            thr = fminf(thr, bm[KK - 1]);
        }
    };
    const int per = 64 * a.S;
    PH(0);
    PR_MARK("filter");
    for (int base = 0; base < nbox; base += per) {
        // ---- coarse filter: lane l looks at box base + l*S + s
        const int bid = base + lane * a.S + s;
        bool pass = false;
        float lo0 = INFINITY, lo1 = INFINITY, lo2 = INFINITY, hi0 = INFINITY, hi1 = INFINITY, hi2 = INFINITY;
        if (bid < nbox) {
            const float4 A = *(const float4 *)(bx + (size_t)bid * 8);
            const float4 Bv = *(const float4 *)(bx + (size_t)bid * 8 + 4);
            lo0 = A.x; lo1 = A.y; lo2 = A.z; hi0 = A.w; hi1 = Bv.x; hi2 = Bv.y;
            if (BOXL) {        // the precise filter reads a surviving box's bounds back as LDS broadcasts (not VALU readlanes),
                // in the pairs it works on: (lo0, lo1) | (hi0, hi1) | (lo2, -hi2).  hi2 is parked NEGATED: the filter forms
                // {lo2 - qz, qz - hi2} as {lo2, -hi2} + {-qz, qz}, one packed add without a modifier to build
                float *o = s_bb + 6 * lane;
                o[0] = lo0; o[1] = lo1; o[2] = hi0; o[3] = hi1; o[4] = lo2; o[5] = -hi2;
            }
            // two query sub-groups per packed instruction (same operation order per sub-group as box_lb).  Both halves in ONE
            // basic block ('|', not '||'): the lane's bound is then broadcast by the op_sel of the packed add in both -- behind
            // a branch the second half assembled its operands with eight v_mov_b32 (the branch was taken only when all 64
            // boxes of a round passed in the first half)
            const f2 bl0 = {lo0, lo0}, bl1 = {lo1, lo1}, bl2 = {lo2, lo2}, bh0 = {hi0, hi0}, bh1 = {hi1, hi1}, bh2 = {hi2, hi2};
#pragma unroll
            for (int q = 0; q < 4; q += 2) {
                const f2 ql0 = {G[q][0], G[q + 1][0]}, ql1 = {G[q][1], G[q + 1][1]}, ql2 = {G[q][2], G[q + 1][2]};
                const f2 qh0 = {G[q][3], G[q + 1][3]}, qh1 = {G[q][4], G[q + 1][4]}, qh2 = {G[q][5], G[q + 1][5]};
                const f2 a0 = bl0 - qh0, c0 = ql0 - bh0, a1 = bl1 - qh1, c1 = ql1 - bh1, a2 = bl2 - qh2, c2 = ql2 - bh2;
                const f2 e0 = {fmaxf(fmaxf(a0.x, c0.x), 0.f), fmaxf(fmaxf(a0.y, c0.y), 0.f)};
                const f2 e1 = {fmaxf(fmaxf(a1.x, c1.x), 0.f), fmaxf(fmaxf(a1.y, c1.y), 0.f)};
                const f2 e2 = {fmaxf(fmaxf(a2.x, c2.x), 0.f), fmaxf(fmaxf(a2.y, c2.y), 0.f)};
                const f2 lb = (e0 * e0 + e1 * e1) + e2 * e2;
                pass = pass | (lb.x <= G[q][6]) | (lb.y <= G[q + 1][6]);
            }
        }
        unsigned long long mask = __ballot(pass);
        PH(1);
        PRUNE_STAT(KK == 1 ? 0 : 3, 0);                                  // coarse rounds (K = 1)
        PRUNE_EVENT(0, 1);
        PRUNE_EVENT(1, __builtin_popcountll(mask));
        if (KK == 1) PRUNE_STAT(1, __builtin_popcountll(mask));          // boxes passing the coarse filter
        if (KK == 1) PRUNE_STAT(3, __builtin_popcountll(__ballot(thr == INFINITY)));  // lanes without a bound
        // scan of one box: the brute-force inner loop of knn.hip on its 16 targets
        auto scan_box = [&](const int bit) {
            wp += PR_WORK(5) | (64u * NN_BOX);                           // a scan costs about five tests
            if (KK == 1) PRUNE_STAT(2, 1);                               // boxes scanned
            PRUNE_EVENT(5, 1);
            const int j0 = (base + bit * a.S + s) * NN_BOX;
            // the box's 16 targets are staged in the wave's LDS slot (x[16] | y[16] | z[16]); all lanes read
            // the same addresses (broadcast) -- the operands of the packed ops are VGPR pairs
            if (!LDSV) {
                const int l = lane < 48 ? lane : 47;
                const float v = tx_g[(size_t)(l >> 4) * cstride + j0 + (l & 15)];
                if (lane < 48) s_tg[lane] = v;
            }
            // LDSV: the cloud itself is in LDS -- the broadcast reads go straight to it
            const float *tx = LDSV ? tx_g : s_tg - j0;
            const float *ty = tx + (LDSV ? cstride : 16), *tz = ty + (LDSV ? cstride : 16);
            if (KK == 1) {
                // minimum of each half of the box: the final rescan then looks at 8 targets instead of 16
                float mh[2] = {INFINITY, INFINITY};
#pragma unroll
                for (int u = 0; u < NN_BOX; u += 2) {
                    const f2 dx = qx2 - *(const f2 *)(tx + j0 + u);
                    const f2 dy = qy2 - *(const f2 *)(ty + j0 + u);
                    const f2 dz = qz2 - *(const f2 *)(tz + j0 + u);
                    const f2 d = (dx * dx + dy * dy) + dz * dz;
                    mh[u >> 3] = fminf(fminf(mh[u >> 3], d.x), d.y);
                }
                const float m = fminf(mh[0], mh[1]);
                // ascending visits: ties keep the lower box, and inside a box the lower half
                if (m < bm[0]) { bm[0] = m; bb[0] = j0 + (mh[1] < mh[0] ? 8 : 0); }
                thr = fminf(thr, m);
            } else {
                constexpr int UBK = 8;
#pragma unroll
                for (int h = 0; h < NN_BOX; h += UBK) {
                    float m = INFINITY;
#pragma unroll
                    for (int u = 0; u < UBK; u += 2) {
                        const f2 dx = qx2 - *(const f2 *)(tx + j0 + h + u);
                        const f2 dy = qy2 - *(const f2 *)(ty + j0 + h + u);
                        const f2 dz = qz2 - *(const f2 *)(tz + j0 + h + u);
                        const f2 d = (dx * dx + dy * dy) + dz * dz;
                        m = fminf(fminf(m, d.x), d.y);
                    }
#pragma unroll
                    for (int c = KK - 1; c >= 0; --c) {
                        const int cp = c > 0 ? c - 1 : 0;
                        const bool lt_prev = (c > 0) && (m < bm[cp]);
                        const bool lt_cur = m < bm[c];
                        bm[c] = lt_prev ? bm[cp] : (lt_cur ? m : bm[c]);
                        bb[c] = lt_prev ? bb[cp] : (lt_cur ? j0 + h : bb[c]);
                    }
                }
                // KK distinct blocks hold KK distinct targets no farther than bm[KK-1]
                thr = fminf(thr, bm[KK - 1]);
            }
        };
        // (query, box) work queue.  Most scanned boxes are needed by a FEW of the wave's 64 queries (one to three is
        // typical: noisy points with large bounds drive the per-wave union), so walking a box with all 64 lanes for
        // their sake wastes the wave.  Such a box is not scanned here: every needing lane appends (box, lane) to the
        // wave's queue in LDS -- its rank among the needers (mbcnt of the ballot) is its slot -- and the queue is
        // drained 64 entries at a time with ONE entry per lane (drain_queue below): every lane then evaluates one
        // query against the 16 targets of one box, whatever mix of queries and boxes the entries hold.
        auto enqueue_box = [&](const int bit, const unsigned long long need, const bool nd, const int nneed) {
            wp += PR_WORK(1);
            if (KK == 1) PRUNE_STAT(2, 1);
            PRUNE_EVENT(4, 1);
            const int bid = base + bit * a.S + s;
            const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
            if (nd) s_q[qcnt + rank] = ((unsigned)bid << 6) | (unsigned)lane;
            qcnt += nneed;
        };
        // (Targets used to come through scalar loads, s_load_dwordx16 x 3 per scanned box: one dependent scalar-cache
        // miss chain per scan; measured 95 -> 80 us for the launch with the vector path of scan_box alone.)
        // ---- precise filter with the lane's current bound, two boxes per step in packed fp32 (same operation order per box
        // as box_lb; the second box is judged after the first one's scan).
        // The candidates (bm, bb, thr) pass three kinds of box: not needed and enqueued (the common ones: neither touches them)
        // and densely scanned / drained (rare: new candidates are computed beside the old ones).  With all three in one loop
        // body the compiler merged them in a block of copies that the common paths ran too: 14 v_mov_b32 per enqueued box of
        // a K = 3 item (7 + 7; 3 + 4 for K = 1).  So the loop is split: the INNER loop takes steps, judges both boxes and
        // enqueues, and the candidates are loop-invariant in it (it only reads thr); a box to scan or a full queue leaves it
        // with the box's number in `rare`, and the outer loop does the rare work at its ONE site (a second copy of the scan
        // costs registers).  When that happens at a step's first box the second one stays in the mask and leads the next
        // step: it is judged against the bound the rare work may just have lowered, as before, from the same lower bound
        // (evaluated again: the rare path pays).  The order of the evaluations is what it was.
        // The work count: two tests per step, and a round of n survivors takes (n + 1) / 2 steps when none is re-done --
        // counted once per round, so that the sum is the one this loop always reported whatever steps are re-done.
        wp += PR_WORK(2 * ((__builtin_popcountll(mask) + 1) >> 1));
        // a box some lane needs: enqueued, or `rare` says what the outer loop has to do (>= 0 scan this box, -2 drain the queue)
#define PR_NEEDED_BOX(BIT, NEED, ND)                                                                              \
        PRUNE_EVENT(3, 1);                                                                                        \
        const int nneed = __builtin_popcountll(NEED);                                                             \
        if (nneed > queue_max) { rare = (BIT); left = cm; cm = 0ull; }                                            \
        else { enqueue_box((BIT), (NEED), (ND), nneed); PH(4);                                                    \
               if (qcnt > QCAP - 64) { rare = -2; left = cm; cm = 0ull; } }   /* uniform: qcnt is a wave-wide count */
        unsigned long long cm = mask;                                    // every surviving box of the round
        for (;;) {
            int rare = -1;
            unsigned long long left = 0ull;                              // the boxes still to judge when the loop is left for rare work
            // ONE exit, at the head, on ONE scalar: every `break` out of a loop is a flag the compiler sets, merges and tests on
            // all paths; the rare paths empty the mask instead and park the rest of it in `left`
            while (cm != 0) {
                const int bA = __builtin_ctzll(cm);
                const unsigned long long restA = cm & (cm - 1);          // without box A
                const bool hasB = restA != 0;
                const int bB = hasB ? __builtin_ctzll(restA) : bA;
                f2 lb;
                if constexpr (BOXL) {
                    // Paired by AXIS, not by box: per box (lo0, lo1), (hi0, hi1) and (lo2, -hi2) are three aligned register pairs as
                    // the LDS reads deliver them (the coarse round parks them in this order), so no operand of a packed
                    // instruction is assembled from two boxes' registers (that took nine v_mov_b32 per step).  Per box the
                    // operations of box_lb in its order: {lo0, lo1} - {qx, qy}; {qx, qy} - {hi0, hi1}; {lo2, -hi2} + {-qz, qz}
                    // (negation is exact and addition commutes: the bits of lo2 - qz and qz - hi2); max3 per axis; {ex, ey}^2
                    // packed; (ex^2 + ey^2) + ez^2.  The two boxes are independent chains that share the packed square of
                    // {ezA, ezB} and the last packed add.  s_bb is wave-uniform for the compiler too (the caller's wave index
                    // is a scalar), so 24 * bA is SALU work.
                    const f2 *pA = (const f2 *)(s_bb + 6 * bA), *pB = (const f2 *)(s_bb + 6 * bB);
                    const f2 LA = pA[0], HA = pA[1], ZA = pA[2];
                    const f2 LB = pB[0], HB = pB[1], ZB = pB[2];
                    const f2 aA = LA - qxy, cA = qxy - HA, zA = ZA + qzn;
                    const f2 aB = LB - qxy, cB = qxy - HB, zB = ZB + qzn;
                    const f2 eA = {fmaxf(fmaxf(aA.x, cA.x), 0.f), fmaxf(fmaxf(aA.y, cA.y), 0.f)};
                    const f2 eB = {fmaxf(fmaxf(aB.x, cB.x), 0.f), fmaxf(fmaxf(aB.y, cB.y), 0.f)};
                    const f2 ez = {fmaxf(fmaxf(zA.x, zA.y), 0.f), fmaxf(fmaxf(zB.x, zB.y), 0.f)};
                    const f2 sA = eA * eA, sB = eB * eB;
                    float tA = sA.x + sA.y, tB = sB.x + sB.y;
                    asm("" : "+v"(tA), "+v"(tB));     // two scalar adds: packed across the boxes they cost three v_mov_b32 to pair up
                    lb = f2{tA, tB} + ez * ez;
                } else {
                    // the cloud-resident form keeps the bounds in the lanes of the coarse round and pairs box A with box B per axis
                    // (twelve v_readlane per step): the form this filter had before, unchanged
                    const f2 L0 = f2{rl(lo0, bA), rl(lo0, bB)}, L1 = f2{rl(lo1, bA), rl(lo1, bB)}, L2 = f2{rl(lo2, bA), rl(lo2, bB)};
                    const f2 H0 = f2{rl(hi0, bA), rl(hi0, bB)}, H1 = f2{rl(hi1, bA), rl(hi1, bB)}, H2 = f2{rl(hi2, bA), rl(hi2, bB)};
                    const f2 a0 = L0 - qx2, c0 = qx2 - H0, a1 = L1 - qy2, c1 = qy2 - H1, a2 = L2 - qz2, c2 = qz2 - H2;
                    const f2 e0 = {fmaxf(fmaxf(a0.x, c0.x), 0.f), fmaxf(fmaxf(a0.y, c0.y), 0.f)};
                    const f2 e1 = {fmaxf(fmaxf(a1.x, c1.x), 0.f), fmaxf(fmaxf(a1.y, c1.y), 0.f)};
                    const f2 e2 = {fmaxf(fmaxf(a2.x, c2.x), 0.f), fmaxf(fmaxf(a2.y, c2.y), 0.f)};
                    lb = (e0 * e0 + e1 * e1) + e2 * e2;
                }
                PRUNE_EVENT(2, 1);
                PH(2);
#ifdef REART_PRUNE_STATS   // how many of the 64 queries need a scanned box: 1 | 2-3 | 4-7 | 8+  (K = 1 only)
                if (KK == 1) {
                    const int nl = __builtin_popcountll(__ballot(lb.x <= thr));
                    if (nl) PRUNE_STAT(nl == 1 ? 4 : (nl < 4 ? 5 : (nl < 8 ? 6 : 7)), 1);
                }
#endif
                cm = restA;
                const bool ndA = lb.x <= thr;
                const unsigned long long needA = __ballot(ndA);
                if (needA) { PR_NEEDED_BOX(bA, needA, ndA) }
                if (cm == 0) continue;                                   // the round's last box; or rare work first (box B is in `left`)
                cm = restA & (restA - 1);
#ifdef REART_PRUNE_STATS
                if (KK == 1) {
                    const int nl = __builtin_popcountll(__ballot(lb.y <= thr));
                    if (nl) PRUNE_STAT(nl == 1 ? 4 : (nl < 4 ? 5 : (nl < 8 ? 6 : 7)), 1);
                }
#endif
                const bool ndB = lb.y <= thr;
                const unsigned long long needB = __ballot(ndB);
                if (needB) { PR_NEEDED_BOX(bB, needB, ndB) }
            }
            if (rare == -1) break;
            if (rare >= 0) { scan_box(rare); PH(3); }
            else { drain_queue(); PH(5); }
            cm = left;
        }
#undef PR_NEEDED_BOX
    }

    PRUNE_EVENT(7, 1);
    PH(2);
    if (qcnt > 0) drain_queue();
    PH(5);
    PH_FLUSH(0, 5);
    PH_HEAD_FLUSH(KK == 1 ? 0 : 1);
    PR_MARK("park");
    qx_o = qx; qy_o = qy; qz_o = qz;
    work_o = (int)(wp >> 20); pairs_o = wp & 0xFFFFFu;
}


// ------------------------------------------------------------------------------------------------------------
// The search launch: up to two K = 1 jobs (the Chamfer directions) and one K = 3 job (the flow search);
// SearchArgs is declared in internal.h.
// Exactly PR_WPE waves per SIMD, as a minimum AND a maximum: with the wave index in a scalar register the kernel needs 70
// VGPRs, which the hardware would run at seven -- a ninth resident workgroup per compute unit by LDS, a residency this kernel was not
// tuned at (the seventh wave was measured to buy nothing, DESIGN_HISTORY.md).  The maximum makes the allocation 73..80.
template <bool BATCH, bool OFF32>
__global__ __launch_bounds__(64 * PR_SMAX) __attribute__((amdgpu_waves_per_eu(PR_WPE, PR_WPE))) void knn_group_kernel(Batched<SearchArgs> ab) {
    // instance of a batch (gridDim.x is a multiple of 8: blockIdx.x & 7 is still the XCD); a single one reads at a fixed offset
    PH_ENTRY;
    const SearchArgs &a_ = ab.a[BATCH ? blockIdx.y : 0];
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];      // blockDim.x / 64 x PR_LDS_WAVE_BYTES
    // where wave t parks its candidates for the merge: its own result slots (s_key, 3 x 64 x 8 bytes), dead once its search
    // is over -- as static arrays they cost 6 KB per workgroup, i.e. the sixth resident workgroup of a compute unit
#define PARK_M(t) ((float *)(s_dyn + (size_t)(t) * PR_LDS_WAVE_BYTES + 64 * 4 + 64 * 16))
#define PARK_B(t) ((int *)(s_dyn + (size_t)(t) * PR_LDS_WAVE_BYTES + 64 * 4 + 64 * 16 + 3 * 64 * 4))
    __shared__ unsigned int s_wk[PR_SMAX][2];
    __shared__ float s_xthr[PR_SMAX][64];   // the waves' partial neighbour-seed bounds (written once, read after one barrier)
    __shared__ unsigned int s_ticket;
    __shared__ unsigned long long s_t0;
    // ---- which item: scalar arithmetic on blockIdx and the first words of the argument block, fetched in one load
    struct { int n1, n3, G, per, S1, S3, interleave, sparse; } a = {a_.n1, a_.n3, a_.G, a_.per, a_.S1, a_.S3, a_.interleave, a_.sparse};
    const unsigned int *const items = a_.item;
    unsigned long long *const prof = a_.prof;
    const int share = a_.share;
    asm volatile("" :: "s"(a.n1), "s"(a.n3), "s"(a.G), "s"(a.per), "s"(a.S1), "s"(a.S3), "s"(a.interleave), "s"(a.sparse), "s"(items), "s"(prof), "s"(share));
    const int L = blockIdx.x, x = L & 7, r = L >> 3;
    // the wave index as a SCALAR: threadIdx.x >> 6 is the same in all lanes of a wave, but divergent as far as the compiler can
    // tell -- and with it the wave's LDS base (every box address of the precise filter was a 64-bit VALU multiply-add), the
    // statistics counter (a v_add per event) and the box number of an enqueue
    const int s = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    // XCD-local item r: two K = 1 items alternate with one K = 3 item while both kinds last
    const int items1 = a.n1 * a.per, items3 = a.n3 * a.per;
    const int mixed = (a.n1 == 2 && a.n3) ? 3 * a.per : 0;
    int kind, idx;
    if (r < mixed) {
        const int q = r / 3, rr = r - 3 * q;
        kind = rr < 2 ? 1 : 3;
        idx = rr < 2 ? 2 * q + rr : q;
    } else {
        const int d1 = mixed ? 2 * a.per : 0, d3 = mixed ? a.per : 0;
        const int v = r - mixed, left1 = items1 - d1;
        kind = v < left1 ? 1 : 3;
        idx = v < left1 ? d1 + v : d3 + (v - left1);
    }
    // two K = 1 jobs share the K = 1 items: job idx & 1, position idx >> 1.  The shift count in integer arithmetic on `kind` as
    // a WORD (1 or 3) and n1 (0, 1 or 2): as the 1-bit value the compiler makes of (kind == 1 && n1 == 2) each use of it as a
    // number went v_cndmask_b32 + v_readfirstlane_b32
    asm("" : "+s"(kind));
    const int sh = (a.n1 >> 1) & ((3 - kind) >> 1);
    const int j = idx & sh;
    const int p = idx >> sh;
    const int pos = a.interleave ? p * 8 + x : x * a.per + p;   // launch position: XCD x owns a contiguous chunk, or every 8th
    const bool live = p < a.per && pos < a.G && (kind == 1 ? idx < items1 : idx < items3);
    // ---- everything the workgroup needs to know is requested HERE, in front of the opening barrier: the item word (one
    // scalar load whose address depends on blockIdx and a.item only; the previous launch wrote it, so it misses the local
    // L2 and is the longest wait of the head) and the job's members (one batch of wide scalar loads of the argument segment
    // at the job's offset).  A padding position (!live) reads word 0 of its row.
    const KnnJob *jp = kind == 1 ? &a_.k1[j] : &a_.k3;
    int rec = pos;
    if (items) rec = pr_uniform_word(items + ((size_t)(kind == 1 ? j : 2) * a.G + (live ? pos : 0)));
    SearchHot h;
    __builtin_memcpy(&h, jp, sizeof(SearchHot));
    if (threadIdx.x == 0) { s_ticket = 0u; s_t0 = prof ? wall_clock64() : 0ull; }
    __syncthreads();                        // at the start, where all waves of the workgroup arrive together
    PR_MARK("query");
    // the values are wanted in registers at this point: keeps the compiler from moving a load down to its first use
    asm volatile("" :: "s"(rec), "s"(h.tlen), "s"(h.q), "s"(h.q_alt), "s"(h.tsoa), "s"(h.boxes), "s"(h.seed), "s"(h.pd),
                 "s"(h.pi), "s"(h.cost), "s"(h.P1), "s"(h.Ppad), "s"(h.nqg), "s"(h.P2), "s"(h.nqg_rcp), "s"(h.L));
    const unsigned long long t0 = s_t0;
    if (!live) {                                                        // padding of the last chunk (uniform per workgroup)
        if (prof && threadIdx.x == 0) { prof[2 * (size_t)L] = t0; prof[2 * (size_t)L + 1] = t0; a_.prof_pairs[L] = 0u; }
        return;
    }
    const int S = kind == 1 ? a.S1 : a.S3;
    if (s >= S) return;                                                 // the other kind of item uses more waves
    // without item words (the stand-alone warm operators): the order array, then the query map
    // (both as scalar loads: as plain loads they were global_load + v_readfirstlane, and the query frame -- a phi of a scalar and
    // a vector value -- took the frame's base through two v_mul_lo_u32 and two v_readfirstlane for launches WITH item words too)
    const int grp = items ? (int)((unsigned)rec & SEARCH_ITEM_PAIR_MASK) : (jp->border ? pr_uniform_word(jp->border + pos) : pos);
    // the pair -> (batch, query group) without a division: the job carries the reciprocal of nqg beside it (internal.h)
    const int b = (int)reart_div_by_magic((unsigned)grp, (unsigned)h.nqg, h.nqg_rcp), g = grp - b * h.nqg;
    const int qb = items ? (int)((unsigned)rec >> SEARCH_ITEM_PAIR_BITS) - 1 : (jp->qmap ? pr_uniform_word(jp->qmap + b) : b);
    const int n2 = h.tlen ? pr_uniform_word(h.tlen + b) : h.P2;       // beside the query and the seeds; wanted when the seeds are in
    const float *qcloud = qb < 0 ? h.q_alt : (const float *)pr_frame<OFF32>(h.q, qb, h.P1, 3);
    const float *cloud = (const float *)pr_frame<OFF32>(h.tsoa, b, 3, h.Ppad);
    float qx = 0.f, qy = 0.f, qz = 0.f;
    float bm[3] = {INFINITY, INFINITY, INFINITY};
    int bb[3] = {-1, -1, -1};
    int work = 0;
    unsigned int pairs = 0u;
    {
        unsigned char *wl = s_dyn + (size_t)s * PR_LDS_WAVE_BYTES;
        float *s_tg = (float *)wl;
        float *s_qc = (float *)(wl + 64 * 4);
        unsigned long long *s_key = (unsigned long long *)(wl + 64 * 4 + 64 * 16);
        // the queue space's offset as ONE scalar the compiler cannot take apart: a box's three pairs are then read through one
        // address register (s_bb + 24 * box, offsets 0 / 8 / 16); as base + 2816 the constant did not fit ds_read2_b64's
        // offset field and every box took a second v_mov_b32
        int q_off = s * PR_LDS_WAVE_BYTES + (64 * 4 + 64 * 16 + 3 * 64 * 8);
        asm("" : "+s"(q_off));
        unsigned int *s_q = (unsigned int *)(s_dyn + q_off);
        static_assert(384 + PR_QCAP >= 3 * 3 * 64, "neighbour seeds of a K = 3 item: 9 x 64 floats in the result slots + the queue's space");
        static_assert(PR_QCAP >= 384 + 128, "box bounds of a coarse round + at least two drain steps of queue");
        float *s_bb = (float *)s_q;          // the bounds of a coarse round's 64 boxes take the first 384 entries of the queue's space
        s_q += 384;
        constexpr int QC = PR_QCAP - 384;
        const float *boxes_p = (const float *)pr_frame<OFF32>(h.boxes, b, (int)((unsigned)h.Ppad / NN_BOX), 8);
        PH_HEAD_END;
        if (kind == 1) {
            float m1[1]; int b1[1];
            knn_pruned_wave<1, false, QC, true, OFF32>(qcloud, h.seed, h.P1, n2, S, a.sparse, b, g, s, cloud, h.Ppad, boxes_p, s_tg, s_qc, s_q, s_bb, share, share > 1 ? &s_xthr[0][0] : nullptr, s_key,
                                               qx, qy, qz, m1, b1, work, pairs);
            bm[0] = m1[0]; bb[0] = b1[0];
        } else {
            knn_pruned_wave<3, false, QC, true, OFF32>(qcloud, h.seed, h.P1, n2, S, a.sparse, b, g, s, cloud, h.Ppad, boxes_p, s_tg, s_qc, s_q, s_bb, share, share > 1 ? &s_xthr[0][0] : nullptr, s_key,
                                               qx, qy, qz, bm, bb, work, pairs);
        }
        PH_ENTRY_FLUSH(kind == 1 ? 0 : 1);
    }
    // ---- the LAST wave to finish merges (no barrier: a wave that is done leaves at once and frees its slot; measured with
    // a barrier here, 17 % of a wave's life was waiting for its slowest sibling).  Every wave parks its candidates, then
    // takes a ticket; LDS operations of a wave complete in order, so the ticket holder S-1 sees all of them.
    if (S > 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { PARK_M(s)[k * 64 + lane] = bm[k]; PARK_B(s)[k * 64 + lane] = bb[k]; }
        if (lane == 0) { s_wk[s][0] = (unsigned int)work; s_wk[s][1] = pairs; }
        __threadfence_block();
        int ticket = 0;
        if (lane == 0) ticket = (int)atomicAdd(&s_ticket, 1u);
        ticket = __builtin_amdgcn_readfirstlane(ticket);
#ifdef REART_PRUNE_PHASE
        if (lane == 0) atomicAdd(&g_prune_phase[7], 1ull);
#endif
        if (ticket != S - 1) return;
        __threadfence_block();
        work = 0; pairs = 0u;
        for (int t = 0; t < S; ++t) { work += (int)s_wk[t][0]; pairs += s_wk[t][1]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) { bm[k] = PARK_M(0)[k * 64 + lane]; bb[k] = PARK_B(0)[k * 64 + lane]; }
    }
    PR_MARK("merge");
    // ---- merge the slices' candidates by (minimum, first index): distinct slices hold distinct boxes, so the lower block
    // start is the lower index
    const int i = g * NN_BS + lane;
    const float *tx = cloud, *ty = tx + h.Ppad, *tz = ty + h.Ppad;
    if (kind == 1) {
        float m = bm[0];
        int blk = bb[0];
        for (int t = 1; t < S; ++t) {
            const float mt = PARK_M(t)[lane];
            const int bt = PARK_B(t)[lane];
            const bool take = bt >= 0 && ((mt < m) || (mt == m && (blk < 0 || bt < blk)));
            m = take ? mt : m; blk = take ? bt : blk;
        }
        // exact (lowest) index inside the winning half box: ONE rescan per query
        int bi = 0x7fffffff;
        if (blk >= 0) {
#pragma unroll
            for (int u = NN_BOX / 2 - 1; u >= 0; --u) {
                const float d = reart_sqdist3(qx, qy, qz, tx[blk + u], ty[blk + u], tz[blk + u]);
                if (d == m) bi = blk + u;
            }
        }
        pairs += 64u * (NN_BOX / 2);
        if (i < h.P1) {
            // (wave-uniform frame base) + (32-bit lane offset), as the loads of the prologue
            *(float *)(pr_frame<OFF32>(h.pd, b, h.P1, 1) + 4u * (unsigned)i) = m;
            *(int *)(pr_frame<OFF32>(h.pi, b, h.P1, 1) + 4u * (unsigned)i) = bi;
        }
    } else {
        float kd[3] = {INFINITY, INFINITY, INFINITY};
        int ki[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff};
#pragma unroll
        for (int k = 0; k < 3; ++k) reart_top3_insert(kd, ki, bm[k], bb[k] >= 0 ? bb[k] : 0x7fffffff);
        for (int t = 1; t < S; ++t) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int bt = PARK_B(t)[k * 64 + lane];
                reart_top3_insert(kd, ki, PARK_M(t)[k * 64 + lane], bt >= 0 ? bt : 0x7fffffff);
            }
        }
        if (i < h.P1) {
            float *od = (float *)(pr_frame<OFF32>(h.pd, b, h.P1, 3) + 12u * (unsigned)i);
            int *oi = (int *)(pr_frame<OFF32>(h.pi, b, h.P1, 3) + 12u * (unsigned)i);
#pragma unroll
            for (int k = 0; k < 3; ++k) { od[k] = kd[k]; oi[k] = kd[k] < INFINITY ? ki[k] : -1; }
        }
    }
    if (lane == 0) {
        if (h.cost) h.cost[pos] = (unsigned int)work;
        if (prof) {
            prof[2 * (size_t)L] = t0; prof[2 * (size_t)L + 1] = wall_clock64();
            a_.prof_pairs[L] = pairs;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// Cloud-resident form of the same search.  Measured on the kernel above (tools/phase_prof.py): a search wave is a CHAIN
// of dependent memory round trips -- seeds -> seed targets -> boxes -> (per scanned box / per drain step) targets ->
// rescan -- and spends its life waiting for them, not computing.  A target cloud of the loop is 48 KB (4096 points,
// SoA) + 8 KB of boxes: it fits in LDS.  Here one workgroup of PC_WAVES waves copies the cloud and the boxes of ITS
// (job, batch) into LDS once (coalesced 16-byte loads); its waves are PC_WAVES / S query groups x S box slices, every
// target / box read is served by LDS, the slices of a group meet in LDS as 64-bit (distance, block) keys and the
// slice-0 wave merges them, rescans once and writes the record.  What is left of the chain in global memory: the
// query, its seeds, and the record written at the end.
// Falls back to knn_group_kernel when a cloud does not fit (reart_search_launch decides).
#define PC_WAVES 16
#define PC_QCAP 256
#define PC_WAVE_BYTES (64 * 16 + 3 * 64 * 8 + PC_QCAP * 4)      // the wave's queries | result slots | queue
__global__ __launch_bounds__(64 * PC_WAVES) void knn_cloud_kernel(SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    const int L = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long t0 = 0ull;
    if (a.prof && threadIdx.x == 0) t0 = wall_clock64();
    // workgroup -> (job, batch, block of PC_WAVES query groups); jobs innermost so that neighbours differ in kind
    const int njobs = a.n1 + a.n3;
    const int jsel = L % njobs;
    const int rest = L / njobs;
    const int B = a.G / a.k_nqg;
    const int b = rest % B, blk = rest / B;
    const int kind = jsel < a.n1 ? 1 : 3;
    const KnnJob &jb = kind == 1 ? a.k1[jsel] : a.k3;
    const int S = a.cloud_slices, gpw = PC_WAVES / S;             // slices per group, groups per workgroup
    // ---- stage the batch's target cloud and boxes
    const int Ppad = jb.Ppad, nboxp = Ppad / NN_BOX;
    float *cl = (float *)s_dyn;                                   // [3][Ppad]
    float *bxs = cl + 3 * (size_t)Ppad;                           // [nboxp][8]
    {
        const float4 *src = (const float4 *)(jb.tsoa + (size_t)b * 3 * Ppad);
        float4 *dst = (float4 *)cl;
        const int n4 = 3 * Ppad / 4;
        for (int e = threadIdx.x; e < n4; e += 64 * PC_WAVES) dst[e] = src[e];
        const float4 *sb = (const float4 *)(jb.boxes + (size_t)b * nboxp * 8);
        float4 *db = (float4 *)bxs;
        for (int e = threadIdx.x; e < 2 * nboxp; e += 64 * PC_WAVES) db[e] = sb[e];
    }
    __syncthreads();
    const int g = blk * gpw + w / S, sl = w % S;
    unsigned int pairs = 0u;
    int work = 0;
    unsigned char *wbase = s_dyn + (size_t)(3 * Ppad + 8 * nboxp) * 4;
    unsigned long long *s_key = (unsigned long long *)(wbase + (size_t)w * PC_WAVE_BYTES + 64 * 16);
    float qx = 0.f, qy = 0.f, qz = 0.f;
    float bm[3] = {INFINITY, INFINITY, INFINITY};
    int bb[3] = {-1, -1, -1};
    if (g < jb.nqg) {
        unsigned char *wl = wbase + (size_t)w * PC_WAVE_BYTES;
        float *s_qc = (float *)wl;
        unsigned int *s_q = (unsigned int *)(wl + 64 * 16 + 3 * 64 * 8);
        const int qb = jb.qmap ? jb.qmap[b] : b;
        const float *qcloud = qb < 0 ? jb.q_alt : jb.q + (size_t)qb * jb.P1 * 3;
        const int n2 = jb.tlen ? jb.tlen[b] : jb.P2;
        if (kind == 1) {
            float m1[1]; int b1[1];
            knn_pruned_wave<1, true, PC_QCAP, false, false>(qcloud, jb.seed, jb.P1, n2, S, a.sparse, b, g, sl, cl, Ppad, bxs, nullptr, s_qc, s_q, nullptr, a.share, nullptr, s_key, qx, qy, qz,
                                              m1, b1, work, pairs);
            bm[0] = m1[0]; bb[0] = b1[0];
        } else {
            knn_pruned_wave<3, true, PC_QCAP, false, false>(qcloud, jb.seed, jb.P1, n2, S, a.sparse, b, g, sl, cl, Ppad, bxs, nullptr, s_qc, s_q, nullptr, a.share, nullptr, s_key, qx, qy, qz,
                                              bm, bb, work, pairs);
        }
        if (S > 1 && sl > 0) {
            // the slice's candidates as (distance bits, block) keys in its own (now idle) result slots
#pragma unroll
            for (int k = 0; k < 3; ++k)
                s_key[64 * k + lane] = bb[k] >= 0 ? (((unsigned long long)__float_as_uint(bm[k]) << 32) | (unsigned)bb[k]) : ~0ull;
            if (lane == 0) { s_key[192] = (unsigned long long)(unsigned)work; s_key[193] = (unsigned long long)pairs; }   // queue area
        }
    }
    if (S > 1) __syncthreads();
    if (g < jb.nqg && sl == 0) {
        // ---- slice 0 merges its group's slices by the full (distance, block) key: distinct slices hold distinct boxes
        for (int t = 1; t < S; ++t) {
            const unsigned long long *ok = (const unsigned long long *)(wbase + (size_t)(w + t) * PC_WAVE_BYTES + 64 * 16);
            work += (int)(unsigned)ok[192]; pairs += (unsigned)ok[193];
            if (kind == 1) {
                const unsigned long long k = ok[lane];
                const float m = __uint_as_float((unsigned)(k >> 32));
                const int bt = (int)(unsigned)k;
                if (k != ~0ull && ((m < bm[0]) || (m == bm[0] && (bb[0] < 0 || bt < bb[0])))) { bm[0] = m; bb[0] = bt; }
            } else {
                float kd[3];
                int ki[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) { kd[c] = bm[c]; ki[c] = bb[c] >= 0 ? bb[c] : 0x7fffffff; }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const unsigned long long k = ok[64 * c + lane];
                    if (k != ~0ull) reart_top3_insert(kd, ki, __uint_as_float((unsigned)(k >> 32)), (int)(unsigned)k);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) { bm[c] = kd[c]; bb[c] = ki[c] == 0x7fffffff ? -1 : ki[c]; }
            }
        }
        const int i = g * NN_BS + lane;
        if (kind == 1) {
            // exact (lowest) index inside the winning half box
            int bi = 0x7fffffff;
            if (bb[0] >= 0) {
                const float *tx = cl, *ty = cl + Ppad, *tz = cl + 2 * (size_t)Ppad;
#pragma unroll
                for (int u = NN_BOX / 2 - 1; u >= 0; --u) {
                    const float d = reart_sqdist3(qx, qy, qz, tx[bb[0] + u], ty[bb[0] + u], tz[bb[0] + u]);
                    if (d == bm[0]) bi = bb[0] + u;
                }
            }
            pairs += 64u * (NN_BOX / 2);
            if (i < jb.P1) {
                const size_t o = (size_t)b * jb.P1 + i;
                jb.pd[o] = bm[0]; jb.pi[o] = bi;
            }
        } else if (i < jb.P1) {
            const size_t o = ((size_t)b * jb.P1 + i) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) { jb.pd[o + k] = bm[k]; jb.pi[o + k] = bm[k] < INFINITY ? bb[k] : -1; }
        }
        if (lane == 0 && jb.cost) jb.cost[b * jb.nqg + g] = (unsigned int)work;
    } else {
        pairs = 0u;                       // counted by the group's slice-0 wave
    }
    if (a.prof) {
        __shared__ unsigned int s_pairs[PC_WAVES];
        if (lane == 0) s_pairs[w] = pairs;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int tot = 0u;
            for (int k = 0; k < PC_WAVES; ++k) tot += s_pairs[k];
            a.prof[2 * (size_t)L] = t0; a.prof[2 * (size_t)L + 1] = wall_clock64();
            a.prof_pairs[L] = tot;
        }
    }
}

// LDS bytes of the cloud-resident form for the largest target cloud of the launch; 0 = does not fit
static size_t search_cloud_lds(const SearchArgs &a) {
    int Ppad = 0;
    for (int j = 0; j < a.n1; ++j) Ppad = a.k1[j].Ppad > Ppad ? a.k1[j].Ppad : Ppad;
    if (a.n3) Ppad = a.k3.Ppad > Ppad ? a.k3.Ppad : Ppad;
    const size_t need = (size_t)(3 * Ppad + 8 * (Ppad / NN_BOX)) * 4 + (size_t)PC_WAVES * PC_WAVE_BYTES + 256;
    return need <= 152 * 1024 ? need : 0;
}

static int search_check(SearchArgs &a) {
    if (a.n1 < 0 || a.n1 > 2 || a.n3 < 0 || a.n3 > 1 || a.n1 + a.n3 == 0 || a.G < 1) return REART_ERR_INVALID_ARG;
    if ((a.n1 && (a.S1 < 1 || a.S1 > PR_SMAX)) || (a.n3 && (a.S3 < 1 || a.S3 > PR_SMAX))) return REART_ERR_INVALID_ARG;
    for (int j = 0; j < a.n1; ++j)
        if (!a.k1[j].boxes || !a.k1[j].seed || !a.k1[j].pd || !a.k1[j].pi) return REART_ERR_INVALID_ARG;
    if (a.n3 && (!a.k3.boxes || !a.k3.seed || !a.k3.pd || !a.k3.pi)) return REART_ERR_INVALID_ARG;
    a.per = reart_div_up(a.G, 8);
    a.k_nqg = a.n1 ? a.k1[0].nqg : a.k3.nqg;
    for (int j = 0; j < a.n1; ++j) {
        if (a.k1[j].nqg < 1) return REART_ERR_INVALID_ARG;
        a.k1[j].nqg_rcp = reart_div_magic((unsigned)a.k1[j].nqg);
    }
    if (a.n3) {
        if (a.k3.nqg < 1) return REART_ERR_INVALID_ARG;
        a.k3.nqg_rcp = reart_div_magic((unsigned)a.k3.nqg);
    }
    return REART_OK;
}
// every frame offset of every job of the launch in 32 bits (reart_search_off32): picks the kernel's instantiation.
// The batch count is G / nqg: every caller lays out G = B * nqg pairs (SearchArgs::G), which is checked here.
static bool search_off32(const SearchArgs &a) {
    bool ok = !a.wide;
    for (int j = 0; j < a.n1; ++j) ok = ok && a.G % a.k1[j].nqg == 0;
    if (a.n3) ok = ok && a.G % a.k3.nqg == 0;
    for (int j = 0; j < a.n1; ++j) ok = ok && reart_search_off32(a.G / a.k1[j].nqg, a.k1[j].P1, a.k1[j].Ppad, 1);
    if (a.n3) ok = ok && reart_search_off32(a.G / a.k3.nqg, a.k3.P1, a.k3.Ppad, 3);
    return ok;
}

int reart_search_launch(const SearchArgs &a_in, hipStream_t st) {
    SearchArgs a = a_in;
    const int rc = search_check(a);
    if (rc != REART_OK) return rc;
    const size_t cl_lds = a.cloud_resident ? search_cloud_lds(a) : 0;
    a.cloud_slices = (a.cloud_slices == 1 || a.cloud_slices == 2 || a.cloud_slices == 4 || a.cloud_slices == 8) ? a.cloud_slices : 4;
    if (cl_lds) {
        if (hipFuncSetAttribute((const void *)knn_cloud_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024) != hipSuccess)
            return REART_ERR_LAUNCH;
        hipLaunchKernelGGL(knn_cloud_kernel, dim3(reart_search_grid_cloud(a.n1, a.n3, a.G, a.k_nqg, a.cloud_slices)), dim3(64 * PC_WAVES),
                           cl_lds, st, a);
        REART_CHECK_LAUNCH();
        return REART_OK;
    }
    return reart_search_launch_batch(&a, 1, st);
}
// K searches of one geometry in one launch (group form): instance k is the grid's row k
int reart_search_launch_batch(const SearchArgs *ak, int K, hipStream_t st) {
    if (K < 1 || K > REART_BATCH_MAX) return REART_ERR_INVALID_ARG;
    Batched<SearchArgs> ab = {};
    for (int k = 0; k < K; ++k) {
        ab.a[k] = ak[k];
        const int rc = search_check(ab.a[k]);
        if (rc != REART_OK) return rc;
        const SearchArgs &a = ab.a[k], &a0 = ab.a[0];
        if (a.n1 != a0.n1 || a.n3 != a0.n3 || a.G != a0.G || a.S1 != a0.S1 || a.S3 != a0.S3) return REART_ERR_INVALID_ARG;
    }
    const SearchArgs &a = ab.a[0];
    const int S = (a.n1 ? a.S1 : 0) > (a.n3 ? a.S3 : 0) ? a.S1 : a.S3;
    const size_t lds = (size_t)S * PR_LDS_WAVE_BYTES;
    bool off32 = true;
    for (int k = 0; k < K; ++k) off32 = off32 && search_off32(ab.a[k]);
    const dim3 grid1(reart_search_grid(a.n1, a.n3, a.G)), gridK(reart_search_grid(a.n1, a.n3, a.G), K);
    if (K == 1 && off32) hipLaunchKernelGGL((knn_group_kernel<false, true>), grid1, dim3(64 * S), lds, st, ab);
    else if (K == 1) hipLaunchKernelGGL((knn_group_kernel<false, false>), grid1, dim3(64 * S), lds, st, ab);
    else if (off32) hipLaunchKernelGGL((knn_group_kernel<true, true>), gridK, dim3(64 * S), lds, st, ab);
    else hipLaunchKernelGGL((knn_group_kernel<true, false>), gridK, dim3(64 * S), lds, st, ab);
    REART_CHECK_LAUNCH();
    return REART_OK;
}
// workgroups the launch of `a` will have (the form is chosen exactly as in reart_search_launch)
int reart_search_workgroups(const SearchArgs &a) {
    const int nqg = a.n1 ? a.k1[0].nqg : a.k3.nqg;
    const int cs = (a.cloud_slices == 1 || a.cloud_slices == 2 || a.cloud_slices == 4 || a.cloud_slices == 8) ? a.cloud_slices : 4;
    if (a.cloud_resident && search_cloud_lds(a)) return reart_search_grid_cloud(a.n1, a.n3, a.G, nqg, cs);
    return reart_search_grid(a.n1, a.n3, a.G);
}
int reart_search_grid(int n1, int n3, int G) { return 8 * (n1 + n3) * reart_div_up(G, 8); }
int reart_search_grid_cloud(int n1, int n3, int G, int nqg, int slices) {
    return (n1 + n3) * (G / nqg) * reart_div_up(nqg, PC_WAVES / slices);
}

// ---------------------------------------------------------------------------------------------
// Stand-alone entry: warm-started exact K-NN (K = 1 or 3) through the C ABI.
// ---------------------------------------------------------------------------------------------
// merge the S slice partials of one query by the (distance, index) key; K = 3 partials are blocks of
// 8 targets (block minimum, first index) that are rescanned here with the exact key
template <int KK>
__global__ __launch_bounds__(256) void knn_warm_finish_kernel(KnnArgs a) {
    const KnnJob jb = a.job[0];
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= jb.P1) return;
    float kd[KK];
    int ki[KK];
#pragma unroll
    for (int k = 0; k < KK; ++k) { kd[k] = INFINITY; ki[k] = 0x7fffffff; }
    auto insert = [&](float d, int j) {
#pragma unroll
        for (int s = KK - 1; s >= 0; --s) {
            const int sp = s > 0 ? s - 1 : 0;
            const bool lp = (s > 0) && ((d < kd[sp]) | ((d == kd[sp]) & (j < ki[sp])));
            const bool lc = (d < kd[s]) | ((d == kd[s]) & (j < ki[s]));
            kd[s] = lp ? kd[sp] : (lc ? d : kd[s]);
            ki[s] = lp ? ki[sp] : (lc ? j : ki[s]);
        }
    };
    {
        const size_t o = ((size_t)b * jb.P1 + i) * KK;                   // one merged record per query
#pragma unroll
        for (int k = 0; k < KK; ++k) {
            const float d = jb.pd[o + k];
            const int q = jb.pi[o + k];
            insert(d, (d < INFINITY && q >= 0) ? q : 0x7fffffff);
        }
    }
    if (KK > 1) {
        const float *qp = jb.q + ((size_t)b * jb.P1 + i) * 3;
        const float qx = qp[0], qy = qp[1], qz = qp[2];
        const float *tx = jb.tsoa + (size_t)b * 3 * jb.Ppad, *ty = tx + jb.Ppad, *tz = ty + jb.Ppad;
        int blk[KK];
#pragma unroll
        for (int k = 0; k < KK; ++k) { blk[k] = kd[k] < INFINITY ? ki[k] : -1; kd[k] = INFINITY; ki[k] = 0x7fffffff; }
#pragma unroll
        for (int c = 0; c < KK; ++c) {
            if (blk[c] < 0) continue;
            for (int u = 0; u < 8; ++u) {
                const int jj = blk[c] + u;
                const float d = reart_sqdist3(qx, qy, qz, tx[jj], ty[jj], tz[jj]);
                insert(d, d < INFINITY ? jj : 0x7fffffff);
            }
        }
    }
    const int n2 = jb.P2;
    const int valid = KK < n2 ? KK : n2;
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        const bool ok = k < valid && ki[k] != 0x7fffffff;
        const size_t o = ((size_t)b * jb.P1 + i) * KK + k;
        jb.dists[o] = ok ? kd[k] : 0.0f;
        jb.idx[o] = ok ? (int64_t)ki[k] : (int64_t)0;
        ((int *)jb.seed)[o] = ok ? ki[k] : -1;     // warm start of the next call
    }
}

struct WarmPlan { int S, Ppad; size_t o_soa, o_box, o_pd, o_pi, total; };
static int warm_plan(int N, int P1, int P2, int K, WarmPlan *p) {
    if (N < 0 || P1 < 0 || P2 < 0 || (K != 1 && K != 3)) return REART_ERR_INVALID_ARG;
    p->S = 4;                                                             // waves per search workgroup
    while (p->S > 1 && reart_div_up(P2, p->S) < 64) p->S -= 1;
    p->Ppad = (int)reart_align_up((size_t)(P2 > 0 ? P2 : 1), NN_BOX);
    reart_arena ws;
    p->o_soa = ws.take_bytes(sizeof(float) * 3 * (size_t)N * p->Ppad);
    p->o_box = ws.take_bytes(sizeof(float) * 8 * (size_t)N * (p->Ppad / NN_BOX));
    p->o_pd = ws.take_bytes(sizeof(float) * (size_t)N * P1 * K);
    p->o_pi = ws.take_bytes(sizeof(int) * (size_t)N * P1 * K);
    p->total = ws.off;
    return REART_OK;
}

extern "C" size_t reart_knn_points_warm_workspace_bytes(int N, int P1, int P2, int K) {
    WarmPlan p;
    return warm_plan(N, P1, P2, K, &p) == REART_OK ? p.total : 0;
}

extern "C" int reart_knn_points_idx_warm(const float *p1, const float *p2, int N, int P1, int P2, int K,
                                         int32_t *seed, float *dists, int64_t *idx, void *workspace,
                                         size_t workspace_bytes, void *stream) {
    WarmPlan p;
    int rc = warm_plan(N, P1, P2, K, &p);
    if (rc != REART_OK) return rc;
    if (N == 0 || P1 == 0) return REART_OK;
    if (!p1 || !p2 || !seed || !dists || !idx || P2 < 1) return REART_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < p.total) return REART_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    SoaArgs sa = {};
    for (int j = 0; j < 2; ++j) {
        sa.job[j].src = p2; sa.job[j].len = nullptr; sa.job[j].dst = (float *)(ws + p.o_soa);
        sa.job[j].P = P2; sa.job[j].Ppad = p.Ppad;
    }
    rc = reart_soa_launch(sa, p.Ppad, N, 1, st);
    if (rc != REART_OK) return rc;
    rc = reart_boxes_launch((const float *)(ws + p.o_soa), N, p.Ppad, (float *)(ws + p.o_box), st);
    if (rc != REART_OK) return rc;
    KnnArgs a = {};
    a.N = N; a.S = p.S; a.K = K; a.euclidean = 0;
    KnnJob &jb = a.job[0];
    jb.q = p1; jb.tsoa = (const float *)(ws + p.o_soa); jb.boxes = (const float *)(ws + p.o_box);
    jb.seed = seed; jb.P1 = P1; jb.P2 = P2; jb.Ppad = p.Ppad; jb.L = 0; jb.nqg = reart_div_up(P1, NN_BS);
    jb.pd = (float *)(ws + p.o_pd); jb.pi = (int *)(ws + p.o_pi); jb.dists = dists; jb.idx = idx;
    a.job[1] = jb;
    SearchArgs sr = {};
    sr.G = N * jb.nqg; sr.S1 = sr.S3 = p.S; sr.sparse = 40; sr.share = 2;
    if (K == 1) { sr.k1[0] = jb; sr.n1 = 1; } else { sr.k3 = jb; sr.n3 = 1; }
    rc = reart_search_launch(sr, st);
    if (rc != REART_OK) return rc;
    const dim3 fg(reart_div_up(P1, 256), N);
    if (K == 1) hipLaunchKernelGGL((knn_warm_finish_kernel<1>), fg, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((knn_warm_finish_kernel<3>), fg, dim3(256), 0, st, a);
    REART_CHECK_LAUNCH();
    return REART_OK;
}
