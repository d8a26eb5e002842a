// Exact posterior arc probabilities: P(u -> v | data) summed over every DAG, by the subset dynamic programme
// of Koivisto and Sood (2004) with the feature step of Koivisto (2006).  Included by k_bic.hip after dvs_exact.h, whose
// lattice walks it repeats with log-sum-exp in place of max.  Natural logs in fp64 throughout, only exp and log, no
// floating-point atomics, every sum in a fixed order: two runs give equal bytes (semantics: include/dvs.h,
// dvs_arc_posterior).  The prior is order-modular (uniform over orders), NOT uniform over DAGs: a DAG weighs in with its
// number of linear extensions.
//
//   k_post_lse      a log-sum transform over the subset lattice, the tiling of k_exact_best: a pass takes nb <= 8 bits of S, a
//                   workgroup holds the 2^nb rows x n columns (8 bytes a cell: at most 40 KB) in LDS and folds one bit per
//                   barrier with a pairwise log-add.  Down (up == 0) folds S ^ bit into S: subset sums; its first pass reads
//                   the caller's table and applies admissibility and size_prior; the result is alpha.  Up folds S | bit into
//                   S: superset sums; its first pass forms L[S] + Rb[V \ S \ v] on the fly (-inf where v in S), so that
//                   array never exists in memory; the result, gamma, overwrites alpha, which is dead after the chains.
//   k_post_chain    L and Rb level by level in popcount, the shape of k_exact_sinks with its thresholds (one workgroup per
//                   table up to n = 9, one launch per level above: measured for k_exact_sinks, not re-measured here).  A cell
//                   is one max, <= n exp in ascending v, one log.
//   k_post_arcs     family = exp(f + gamma - log_z) and the arc sums: thread (row, v) walks its P with n register
//                   accumulators (P's bit u adds to accumulator u), the rows of a workgroup are added in row order through
//                   LDS, one partial [n][n] per workgroup goes to the workspace.
//   k_post_finish   adds the partials of a table in a fixed order, one workgroup per arc; writes prob, log_z and flags.
#pragma once
#include "dvs_bn_common.h"

constexpr int POST_MAX_VARS = 20;

// log(exp(x) + exp(y)); -inf for two -inf, never NaN for operands < +inf
__device__ __forceinline__ double post_logadd(double x, double y) {
    const double hi = x > y ? x : y, lo = x > y ? y : x;
    if (lo == ex_neg_inf()) return hi;                           // also two -inf; the same bytes as the formula, without exp and log
    return hi + log(1.0 + exp(lo - hi));
}

// f(v, P) of include/dvs.h: the cell plus size_prior[popcount(P)], -inf where P is not admissible for v
__device__ __forceinline__ double post_cell(const PosteriorArgs& a, double x, uint32_t S, int v) {
    const int k = __popc(S);
    const bool ok = !((S >> v) & 1u) && (a.max_parents <= 0 || k <= a.max_parents) &&
                    !(a.forbidden && (a.forbidden[v] & (uint64_t)S)) && x == x;
    if (!ok) return ex_neg_inf();
    return a.size_prior ? x + a.size_prior[k] : x;
}

__global__ __launch_bounds__(256) void k_post_lse(PosteriorArgs a, int lo, int nb, int first, int up) {
    DVS_DYN_LDS(smem);
    const int n = a.n, cells = n << nb, rest = n - nb;
    double* val = (double*)smem;
    const uint32_t t = blockIdx.x >> rest, q = blockIdx.x & ((1u << rest) - 1u), full = (1u << n) - 1u;
    const uint32_t base = (q & ((1u << lo) - 1u)) | ((q >> lo) << (lo + nb));      // the tile's S with bits lo .. lo+nb-1 clear
    const size_t tab = (size_t)t << n;
    for (int c = threadIdx.x; c < cells; c += 256) {
        const int j = c / n, v = c - j * n;
        const uint32_t S = base | ((uint32_t)j << lo);
        const size_t g = (tab + S) * n + v;
        if (!first)
            val[c] = a.alpha[g];
        else if (!up)
            val[c] = post_cell(a, a.table[g], S, v);
        else
            val[c] = ((S >> v) & 1u) ? ex_neg_inf() : a.L[tab + S] + a.Rb[tab + (full ^ S ^ (1u << v))];
    }
    __syncthreads();
    for (int i = 0; i < nb; ++i) {
        for (int c = threadIdx.x; c < cells; c += 256) {
            const int has = ((c / n) >> i) & 1;
            if (has == up) continue;
            const int d = up ? c + (n << i) : c - (n << i);      // row j ^ (1 << i): not written in this sweep
            val[c] = post_logadd(val[c], val[d]);
        }
        __syncthreads();
    }
    for (int c = threadIdx.x; c < cells; c += 256) {
        const int j = c / n, v = c - j * n;
        a.alpha[((tab + (base | ((uint32_t)j << lo))) * n + v)] = val[c];
    }
}

// One cell of a chain: lse over the bits s of W of own[W ^ s] + alpha[at(W ^ s)][s], the terms in ascending s.
// REVERSED: alpha is taken at the complement of W (Rb), otherwise at W ^ s (L).  own[0] is the constant 0 and is not read:
// level 1 runs beside the thread that stores it.
template <bool REVERSED>
__device__ __forceinline__ double post_chain_term(const PosteriorArgs& a, const double* own, size_t tab, uint32_t W, uint32_t outside, int s) {
    const uint32_t prev = W ^ (1u << s);
    return (prev ? own[tab + prev] : 0.0) + a.alpha[(tab + (REVERSED ? outside : prev)) * a.n + s];
}
template <bool REVERSED>
__device__ __forceinline__ double post_chain_cell(const PosteriorArgs& a, const double* own, size_t tab, uint32_t W, uint32_t full) {
    const uint32_t outside = full ^ W;
    double top = ex_neg_inf();
    for (uint32_t m = W; m; m &= m - 1u) {
        const double term = post_chain_term<REVERSED>(a, own, tab, W, outside, __ffs((int)m) - 1);
        top = term > top ? term : top;
    }
    if (top == ex_neg_inf()) return top;
    double sum = 0.0;
    for (uint32_t m = W; m; m &= m - 1u) sum += exp(post_chain_term<REVERSED>(a, own, tab, W, outside, __ffs((int)m) - 1) - top);
    return top + log(sum);
}

// levels k_lo .. k_hi of every table; wgs workgroups share a table.  More than one level per launch needs wgs == 1: the
// barrier orders a level's stores before the next level's loads within the workgroup only.
__global__ __launch_bounds__(256) void k_post_chain(PosteriorArgs a, int k_lo, int k_hi, int wgs) {
    const int n = a.n;
    const uint32_t t = blockIdx.x / wgs, total = 1u << n, stride = (uint32_t)wgs * 256u;
    const size_t tab = (size_t)t << n;
    for (int k = k_lo; k <= k_hi; ++k) {
        for (uint32_t W = (blockIdx.x % wgs) * 256u + threadIdx.x; W < total; W += stride) {
            if (W == 0u) {
                if (k == 1) {
                    a.L[tab] = 0.0;
                    a.Rb[tab] = 0.0;
                }
                continue;
            }
            if (__popc(W) != k) continue;
            a.L[tab + W] = post_chain_cell<false>(a, a.L, tab, W, total - 1u);
            a.Rb[tab + W] = post_chain_cell<true>(a, a.Rb, tab, W, total - 1u);
        }
        if (k < k_hi) __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_post_arcs(PosteriorArgs a) {
    DVS_DYN_LDS(smem);
    double* part = (double*)smem;                                // [rows][n (u)][n (v)]
    const int n = a.n, nn = n * n;
    const uint32_t t = blockIdx.x / a.groups, g = blockIdx.x % a.groups, total = 1u << n;
    const size_t tab = (size_t)t << n;
    const int r = threadIdx.x / n, v = threadIdx.x - r * n;
    const double log_z = a.L[tab + total - 1u];
    const bool none = log_z == ex_neg_inf();
    double acc[POST_MAX_VARS];
#pragma unroll
    for (int u = 0; u < POST_MAX_VARS; ++u) acc[u] = 0.0;
    if (r < a.rows) {
        for (int i = 0; i < a.sweeps; ++i) {
            const uint64_t at = ((uint64_t)g * a.sweeps + i) * a.rows + r;
            if (at >= total) break;
            const uint32_t P = (uint32_t)at;
            const size_t c = (tab + P) * n + v;
            const double f = post_cell(a, a.table[c], P, v);
            const double fam = (none || f == ex_neg_inf()) ? 0.0 : exp(f + a.alpha[c] - log_z);
            if (a.family) a.family[c] = fam;
#pragma unroll
            for (int u = 0; u < POST_MAX_VARS; ++u)
                if ((P >> u) & 1u) acc[u] += fam;
        }
#pragma unroll
        for (int u = 0; u < POST_MAX_VARS; ++u)
            if (u < n) part[r * nn + u * n + v] = acc[u];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nn; e += 256) {
        double s = 0.0;
        for (int row = 0; row < a.rows; ++row) s += part[row * nn + e];
        a.partial[((size_t)t * a.groups + g) * nn + e] = s;
    }
}

// one workgroup per (table, arc): thread i adds the partials i, i + 256, ... in that order, the 256 sums meet in the fixed tree
// of dvs_block_sum256
__global__ __launch_bounds__(256) void k_post_finish(PosteriorArgs a) {
    __shared__ double red[256];
    const int n = a.n, nn = n * n, t = blockIdx.x / nn, e = blockIdx.x - t * nn, tid = threadIdx.x;
    const double* p = a.partial + (size_t)t * a.groups * nn + e;
    double s = 0.0;
    for (int g = tid; g < a.groups; g += 256) s += p[(size_t)g * nn];
    red[tid] = s;
    __syncthreads();
    dvs_block_sum256(tid, red);
    if (tid == 0) {
        a.prob[(size_t)t * nn + e] = red[0];
        if (e == 0) {
            const size_t tab = (size_t)t << n, all = ((size_t)1 << n) - 1;
            const double log_z = a.L[tab + all];
            a.log_z[2 * t] = log_z;
            a.log_z[2 * t + 1] = a.Rb[tab + all];
            a.flags[t] = log_z == ex_neg_inf() ? 1 : 0;
        }
    }
}

void dvs_launch_arc_posterior(const PosteriorArgs& in, dvs_stream_t st) {
    PosteriorArgs a = in;
    const PosteriorSplit split = dvs_posterior_split(a.n);
    a.rows = split.rows;
    a.sweeps = split.sweeps;
    a.groups = split.groups;
    const int n = a.n, passes = (n + EX_TILE_BITS - 1) / EX_TILE_BITS;
    const auto transform = [&](const char* name, int up) {
        for (int p = 0, lo = 0; p < passes; ++p) {
            const int nb = n / passes + (p < n % passes ? 1 : 0);
            DVS_LAUNCH_AS(name, k_post_lse, dim3((unsigned)a.B << (n - nb)), dim3(256), ((size_t)n << nb) * 8, st, a, lo, nb,
                          p == 0 ? 1 : 0, up);
            lo += nb;
        }
    };
    transform("k_post_lse_down", 0);
    if (n <= EX_ONE_WG_VARS) {
        DVS_LAUNCH(k_post_chain, dim3((unsigned)a.B), dim3(256), 0, st, a, 1, n, 1);
    } else {
        const int wgs = 1 << (n - 8);
        for (int k = 1; k <= n; ++k) DVS_LAUNCH(k_post_chain, dim3((unsigned)a.B * wgs), dim3(256), 0, st, a, k, k, wgs);
    }
    transform("k_post_lse_up", 1);
    DVS_LAUNCH(k_post_arcs, dim3((unsigned)a.B * a.groups), dim3(256), (size_t)a.rows * n * n * 8, st, a);
    DVS_LAUNCH(k_post_finish, dim3((unsigned)a.B * n * n), dim3(256), 0, st, a);
}
