// reart_amd/csrc/invlist_dev.h -- the inverse lists of the operators' gradients: which records name point p of cloud b?
// One definition of the stable counting sort behind ConnectionTerm (connection_term.hip: records = the two ends of the
// selected pairs) and the PointNet++ gradients (pointnet_grad.hip: records = gathered rows, (fine point, neighbour) pairs).
//
// A cloud has rec.count() records and rec.points() points; rec.point(b, q, pt) says whether record q of cloud b is live
// (a record that is not takes no place) and which point it names.  Output, absolute numbers throughout: start
// [B][points + 1] offsets into list, list the record numbers b * count + q -- the records of a point in ascending order, the
// points of a cloud in order, the clouds one after another from b * count on.  Workgroup (x, b) of WAVES waves owns points [x TILE, (x + 1) TILE)
// of cloud b and reads all of the cloud's records twice (count per (wave, point), then place), every wave a contiguous run
// in whole steps of 64.  Integer atomics on LDS counters only: any order, one result.
#pragma once
#include "common.h"

template <int TILE, int WAVES, class Rec>
__global__ __launch_bounds__(WAVES * 64) void reart_invlist_kernel(Rec rec, int *__restrict__ start, int *__restrict__ list) {
    __shared__ int s_cnt[WAVES][TILE];
    __shared__ int s_start[TILE];
    __shared__ int s_below[WAVES], s_wsum[WAVES];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, b = blockIdx.y;
    static_assert(TILE <= WAVES * 64, "a thread owns at most one point of the tile");
    const bool owner = tid < TILE;
    const int Npts = rec.points(), lo = blockIdx.x * TILE, hi = min(Npts, lo + TILE);
    const int R = rec.count(), base = b * R;
    const int run = (R + WAVES * 64 - 1) / (WAVES * 64) * 64;
    const int q_lo = min(R, w * run), q_hi = min(R, q_lo + run);
    int *__restrict__ start_b = start + (size_t)b * (Npts + 1);
    for (int u = tid; u < WAVES * TILE; u += WAVES * 64) (&s_cnt[0][0])[u] = 0;
    __syncthreads();
    int below = 0;
    for (int q0 = q_lo; q0 < q_hi; q0 += 64) {
        const int q = q0 + lane;
        int pt = 0;
        const bool live = q < q_hi && rec.point(b, q, pt);
        below += __popcll(__ballot(live && pt < lo));
        if (live && pt >= lo && pt < hi) atomicAdd(&s_cnt[w][pt - lo], 1);
    }
    if (lane == 0) s_below[w] = below;
    __syncthreads();
    // a point's list: the waves' runs behind each other; the tile's lists behind each other; the tile behind the points below
    int tot = 0;
    if (owner)
        for (int v = 0; v < WAVES; ++v) {
            const int n = s_cnt[v][tid];
            s_cnt[v][tid] = tot;
            tot += n;
        }
    int inc = tot;
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    if (lane == 63) s_wsum[w] = inc;
    __syncthreads();
    int first = 0, all = 0;
    for (int v = 0; v < WAVES; ++v) {
        first += s_below[v];
        all += s_wsum[v];
        if (v < w) first += s_wsum[v];
    }
    if (owner) {
        s_start[tid] = first + inc - tot;
        if (lo + tid < hi) start_b[lo + tid] = base + first + inc - tot;
    }
    if (tid == 0 && hi == Npts) start_b[Npts] = base + first + all;      // wave 0: first = the records below the tile
    __syncthreads();
    for (int q0 = q_lo; q0 < q_hi; q0 += 64) {
        const int q = q0 + lane;
        int pt = 0;
        const bool live = q < q_hi && rec.point(b, q, pt);
        bool todo = live && pt >= lo && pt < hi;
        unsigned long long m;
        while ((m = __ballot(todo)) != 0) {               // one point per turn: its records of this step, in lane order
            const int lp = __shfl(pt, __ffsll((long long)m) - 1, 64) - lo;
            const bool mine = todo && pt - lo == lp;
            const unsigned long long same = __ballot(mine);
            const int at = s_cnt[w][lp];
            if (mine) list[base + s_start[lp] + at + __popcll(same & reart_lanes_below(lane))] = base + q;
            reart_wave_sync();
            if (lane == 0) s_cnt[w][lp] = at + __popcll(same);
            reart_wave_sync();
            todo = todo && !mine;
        }
    }
}
