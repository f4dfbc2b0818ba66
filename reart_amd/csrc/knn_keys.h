// reart_amd/csrc/knn_keys.h -- the per-query ranked list of the LDS-list K-NN kernels (knn_list.hip,
// knn_anyd.hip).
//
// A list holds a query's K best targets so far as K ascending keys in LDS.  The fp32 searches use a 64-bit key,
// (bits of the fp32 distance) << 32 | j; the fp64 search uses KeyF64, the pair (bits of the fp64 distance, j) in
// lexicographic order.  Distances are >= +0, so either order is (distance, index) order and every key is distinct.
// A wave that found candidates (keys below the list's K-th key) sorts them across its 64 lanes and merges them in:
// every candidate and every list entry finds its new slot by counting the other side's smaller keys (binary
// searches), and entries pushed past K fall off.  The helpers are templates over the key type; a key type brings
// kl_sel, kl_shfl_xor, kl_cas, operator< and a kl_none specialisation (the all-ones key, above every real key).
#pragma once
#include "common.h"

typedef unsigned long long u64;

// fp64 search key: distance bits, then index; 16 B in LDS
struct __attribute__((aligned(16))) KeyF64 {
    u64 d;
    unsigned j, pad;
};

__device__ __forceinline__ bool operator<(const KeyF64 &a, const KeyF64 &b) {
    return a.d < b.d || (a.d == b.d && a.j < b.j);
}

// c ? a : b, per component (a select of whole structs goes through scratch memory)
__device__ __forceinline__ u64 kl_sel(bool c, u64 a, u64 b) { return c ? a : b; }
__device__ __forceinline__ KeyF64 kl_sel(bool c, KeyF64 a, KeyF64 b) {
    return KeyF64{c ? a.d : b.d, c ? a.j : b.j, 0u};
}

// one compare-exchange of the bitonic network: min(o, v) if keep_min, else max(o, v)
__device__ __forceinline__ u64 kl_cas(bool keep_min, u64 o, u64 v) {
    return keep_min ? (o < v ? o : v) : (o > v ? o : v);
}
__device__ __forceinline__ KeyF64 kl_cas(bool keep_min, KeyF64 o, KeyF64 v) {
    return kl_sel(keep_min ? o < v : v < o, o, v);
}

template <class Key>
__device__ __forceinline__ Key kl_none();
template <>
__device__ __forceinline__ u64 kl_none<u64>() { return ~0ull; }
template <>
__device__ __forceinline__ KeyF64 kl_none<KeyF64>() { return KeyF64{~0ull, ~0u, 0u}; }

__device__ __forceinline__ u64 kl_shfl_xor(u64 v, int m) {
    const int lo = __shfl_xor((int)(unsigned)v, m, 64), hi = __shfl_xor((int)(unsigned)(v >> 32), m, 64);
    return ((u64)(unsigned)hi << 32) | (unsigned)lo;
}

__device__ __forceinline__ KeyF64 kl_shfl_xor(KeyF64 v, int m) {
    return KeyF64{kl_shfl_xor(v.d, m), (unsigned)__shfl_xor((int)v.j, m, 64), 0u};
}

// ascending across the 64 lanes (bitonic network)
template <class Key>
__device__ __forceinline__ Key kl_sort64(Key v, int lane) {
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const Key o = kl_shfl_xor(v, j);
            const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
            v = kl_cas(keep_min, o, v);
        }
    }
    return v;
}

// number of entries of the ascending array a[0..n) below v
template <class Key>
__device__ __forceinline__ int kl_count_below(const Key *a, int n, Key v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Merge c sorted candidates into the list lst[0..K) (NE = list entries per lane, K <= 64 * NE).  v: this lane's
// candidate, ascending across the lanes, lanes >= c hold kl_none; cand: 64 keys of LDS scratch.  Called by the
// whole wave; returns the list's new K-th key.
template <int NE, class Key>
__device__ __forceinline__ Key kl_merge(Key *lst, Key *cand, int K, Key v, int c, int lane) {
    cand[lane] = v;
    Key old[NE];
#pragma unroll
    for (int u = 0; u < NE; ++u) old[u] = (lane + 64 * u < K) ? lst[lane + 64 * u] : kl_none<Key>();
    reart_wave_sync();
    // new slots: a candidate moves up by the list entries below it, an entry by the candidates below it
    const int cpos = lane < c ? lane + kl_count_below(lst, K, v) : K;
    int npos[NE];
#pragma unroll
    for (int u = 0; u < NE; ++u) npos[u] = lane + 64 * u + kl_count_below(cand, c, old[u]);
    reart_wave_sync();
#pragma unroll
    for (int u = 0; u < NE; ++u)
        if (lane + 64 * u < K && npos[u] < K) lst[npos[u]] = old[u];
    if (cpos < K) lst[cpos] = v;
    reart_wave_sync();
    return lst[K - 1];
}
