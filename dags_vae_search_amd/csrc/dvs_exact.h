// Exact structure search: the globally optimal DAG of a local-score table by the subset dynamic programme
// of Silander and Myllymaki (2006).  Included by k_bic.hip after dvs_cpdag.h.  fp64 compares and one fp64 addition per
// candidate, every choice by a total order: two runs give equal bytes (semantics: include/dvs.h, dvs_exact_search).
//
//   k_exact_best       best parents: a subset-max transform under (value descending, mask ascending).  A pass takes nb <=
//                      8 bits lo .. lo + nb - 1 of S: a workgroup holds the 2^nb rows that differ in those bits (all n
//                      columns, value and mask, 12 bytes a cell: at most 48 KB) in LDS and folds S ^ (1 << i) into every S
//                      with bit i, one barrier per bit.  The first pass (lo = 0: consecutive S, the tile is one contiguous
//                      run of the [S][v] layout) reads the caller's table and applies admissibility; later passes read and
//                      write best / arg in rows n cells long, 2^lo rows apart.  n bits take ceil(n / 8) passes of
//                      near-equal width, one launch each.  Cells with v in S are carried along (they never feed a cell
//                      with v not in S) and end up unspecified but deterministic.
//   k_exact_sinks      R and sink, level by level in popcount: a thread takes the W of its level among 2^n, walks its bits
//                      upwards and keeps the first largest R[W ^ s] + best[W ^ s][s].  n <= 9: one workgroup per table and
//                      one launch, a barrier between levels (measured: 12 - 17 us at n = 8 against 7.5 us a launch); above,
//                      one launch per level (one workgroup takes 122 us at n = 11 and 238 us at n = 12, 13 launches 97 us).
//   k_exact_backtrack  n serial steps, one thread per table.
#pragma once
#include "dvs_bn_common.h"

constexpr int EX_TILE_BITS = 8;              // bits of S per LDS pass
constexpr int EX_ONE_WG_VARS = 9;            // k_exact_sinks: up to here one workgroup walks all levels of a table
constexpr uint32_t EX_NO_ARG = 0xffffffffu;

__device__ __forceinline__ double ex_neg_inf() { return __longlong_as_double((long long)0xfff0000000000000ull); }

__global__ __launch_bounds__(256) void k_exact_best(ExactArgs a, int lo, int nb, int first) {
    DVS_DYN_LDS(smem);
    const int n = a.n, cells = n << nb, rest = n - nb;
    double* val = (double*)smem;
    uint32_t* arg = (uint32_t*)(smem + (size_t)cells * 8);
    const uint32_t t = blockIdx.x >> rest, q = blockIdx.x & ((1u << rest) - 1u);
    const uint32_t base = (q & ((1u << lo) - 1u)) | ((q >> lo) << (lo + nb));      // the tile's S with bits lo .. lo+nb-1 clear
    const size_t tab = (size_t)t << n;
    for (int c = threadIdx.x; c < cells; c += 256) {
        const int j = c / n, v = c - j * n;
        const uint32_t S = base | ((uint32_t)j << lo);
        const size_t g = (tab + S) * n + v;
        if (first) {
            const double x = a.table[g];
            const bool ok = !((S >> v) & 1u) && (a.max_parents <= 0 || __popc(S) <= a.max_parents) &&
                            !(a.forbidden && (a.forbidden[v] & (uint64_t)S)) && x == x;
            val[c] = ok ? x : ex_neg_inf();
            arg[c] = ok ? S : EX_NO_ARG;
        } else {
            val[c] = a.best[g];
            arg[c] = a.arg[g];
        }
    }
    __syncthreads();
    for (int i = 0; i < nb; ++i) {
        for (int c = threadIdx.x; c < cells; c += 256) {
            if (!(((c / n) >> i) & 1)) continue;
            const int d = c - (n << i);                          // row j ^ (1 << i): not written in this sweep
            const double x = val[d], y = val[c];
            const uint32_t px = arg[d];
            if (x > y || (x == y && px < arg[c])) {
                val[c] = x;
                arg[c] = px;
            }
        }
        __syncthreads();
    }
    for (int c = threadIdx.x; c < cells; c += 256) {
        const int j = c / n, v = c - j * n;
        const size_t g = (tab + (base | ((uint32_t)j << lo))) * n + v;
        a.best[g] = val[c];
        a.arg[g] = arg[c];
    }
}

// levels k_lo .. k_hi of every table; wgs workgroups share a table.  More than one level per launch needs wgs == 1: the
// barrier orders a level's stores before the next level's loads within the workgroup only.
__global__ __launch_bounds__(256) void k_exact_sinks(ExactArgs a, int k_lo, int k_hi, int wgs) {
    const int n = a.n;
    const uint32_t t = blockIdx.x / wgs, full = 1u << n, stride = (uint32_t)wgs * 256u;
    const size_t tab = (size_t)t << n;
    for (int k = k_lo; k <= k_hi; ++k) {
        for (uint32_t W = (blockIdx.x % wgs) * 256u + threadIdx.x; W < full; W += stride) {
            if (W == 0u) {
                if (k == 1) {
                    a.R[tab] = 0.0;
                    a.sink[tab] = -1;
                }
                continue;
            }
            if (__popc(W) != k) continue;
            double top = 0.0;
            int sink = -1;
            for (uint32_t m = W; m; m &= m - 1u) {
                const int s = __ffs((int)m) - 1;
                const uint32_t prev = W ^ (1u << s);
                const double r = prev ? a.R[tab + prev] : 0.0;
                const double cand = r + a.best[(tab + prev) * n + s];
                if (sink < 0 || cand > top) {
                    top = cand;
                    sink = s;
                }
            }
            a.R[tab + W] = top;
            a.sink[tab + W] = sink;
        }
        if (k < k_hi) __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_exact_backtrack(ExactArgs a) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.B) return;
    const int n = a.n;
    const size_t tab = (size_t)t << n, row = (size_t)t * n;
    uint32_t W = (1u << n) - 1u;
    const double score = a.R[tab + W];
    const bool none = score == ex_neg_inf();
    a.score[t] = score;
    a.flags[t] = none ? 1 : 0;
    if (none) {
        for (int v = 0; v < n; ++v) {
            a.parents[row + v] = 0ull;
            a.order[row + v] = -1;
        }
        return;
    }
    for (int k = n - 1; k >= 0; --k) {
        const int s = a.sink[tab + W];                           // always a bit of W
        W ^= 1u << s;
        a.order[row + k] = s;
        a.parents[row + s] = (uint64_t)a.arg[(tab + W) * n + s];
    }
}

void dvs_launch_exact(const ExactArgs& a, dvs_stream_t st) {
    const int n = a.n, passes = (n + EX_TILE_BITS - 1) / EX_TILE_BITS;
    for (int p = 0, lo = 0; p < passes; ++p) {
        const int nb = n / passes + (p < n % passes ? 1 : 0);
        const size_t lds = ((size_t)n << nb) * 12;
        DVS_LAUNCH(k_exact_best, dim3((unsigned)a.B << (n - nb)), dim3(256), lds, st, a, lo, nb, p == 0 ? 1 : 0);
        lo += nb;
    }
    if (n <= EX_ONE_WG_VARS) {
        DVS_LAUNCH(k_exact_sinks, dim3((unsigned)a.B), dim3(256), 0, st, a, 1, n, 1);
    } else {
        const int wgs = 1 << (n - 8);
        for (int k = 1; k <= n; ++k) DVS_LAUNCH(k_exact_sinks, dim3((unsigned)a.B * wgs), dim3(256), 0, st, a, k, k, wgs);
    }
    DVS_LAUNCH(k_exact_backtrack, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, st, a);
}
