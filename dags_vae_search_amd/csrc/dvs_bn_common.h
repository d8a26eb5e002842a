// What the Bayesian-network kernels of k_bic.hip share: the packed data set and a packed row in registers,
// the layout of a family's dense table, the dense count, and the launchers' table size and family dispatch.  k_bic.hip
// includes it first; dvs_hillclimb.h, dvs_tabu.h, dvs_cpdag.h, dvs_citest.h, dvs_fitted.h (what the fitted-network kernels
// share on top of it), dvs_infer.h, dvs_exact.h, dvs_posterior.h and dvs_strength.h include it for what they use.  The lane
// and workgroup primitives that are not about networks (64-bit broadcasts and shuffles, wave reductions, dvs_block_sum256)
// are in dvs_device.h.  Everything here is forced inline.
#pragma once
#include "dvs_search_args.h"

// ---- packed data: 4-bit level codes, 16 variables per 64-bit word, sample-major ------------------------------------------
constexpr int BIC_MAX_BINS = 36864;          // q_v * r_v histogram bins that fit LDS (144 KB of u32 counters)
static_assert(DVS_CI_MAX_CELLS == BIC_MAX_BINS, "the CI table shares the scorer's LDS budget");

static inline int bic_words(int n) { return (n + 15) / 16; }
static inline size_t bn_table_lds() { return (size_t)BIC_MAX_BINS * sizeof(unsigned); }      // dynamic LDS of a dense table

__device__ __forceinline__ double bn_lgamma(double x) {
#ifdef DVS_EMU
    int sign;                    // the emulator runs workgroups on several host threads: libm's lgamma writes a global
    return lgamma_r(x, &sign);
#else
    return lgamma(x);
#endif
}
__device__ __forceinline__ double bn_nan() { return __longlong_as_double(0x7ff8000000000000LL); }      // the quiet NaN of a refusal

__device__ __forceinline__ int bic_level(const uint64_t* row, int var) { return (int)((row[var >> 4] >> (4 * (var & 15))) & 15ull); }

// sample s of a structure's data set is row rows[s] of the data (dvs_strength.h: the *_rows kernels)
__device__ __forceinline__ const int* rs_rows(const RowSetArgs& r, int dag) {
    const int set = r.set_of != nullptr ? r.set_of[dag] : dag;
    return r.rows + (size_t)set * (size_t)r.set_size;
}

// One row (n <= 48: at most three words) in registers.
struct BnRow {
    uint64_t w0, w1, w2;
};
__device__ __forceinline__ BnRow bn_row_load(const uint64_t* src, int words) {
    return BnRow{src[0], words > 1 ? src[1] : 0ull, words > 2 ? src[2] : 0ull};
}
__device__ __forceinline__ void bn_row_store(uint64_t* dst, const BnRow& x, int words) {
    dst[0] = x.w0;
    if (words > 1) dst[1] = x.w1;
    if (words > 2) dst[2] = x.w2;
}
__device__ __forceinline__ int bn_level(const BnRow x, int v) {
    const uint64_t w0 = x.w0, w1 = x.w1, w2 = x.w2;          // a choice among values: among the fields it is an indexed
    const uint64_t w = v < 16 ? w0 : v < 32 ? w1 : w2;       // load, and the row leaves the registers
    return (int)((w >> (4 * (v & 15))) & 15ull);
}
// x with `level` in the nibble of v, which x holds as zero
__device__ __forceinline__ BnRow bn_row_with(const BnRow x, int v, uint64_t level) {
    const uint64_t l = level << (4 * (v & 15));
    return BnRow{v < 16 ? x.w0 | l : x.w0, v >= 16 && v < 32 ? x.w1 | l : x.w1, v >= 32 ? x.w2 | l : x.w2};
}
// the mixed-radix configuration of the parents pm in row x, lowest variable id fastest: the key of the CPT layout
__device__ __forceinline__ int bn_row_config(const BnRow& x, uint64_t pm, const unsigned char* card) {
    int cfg = 0, stride = 1;
    for (; pm; pm &= pm - 1ull) {
        const int p = dvs_ctz64(pm);
        cfg += bn_level(x, p) * stride;
        stride *= card[p];
    }
    return cfg;
}
// the level a 31-bit draw h selects among the r cumulative thresholds T (k_bn_sample_prep wrote them)
__device__ __forceinline__ uint64_t bn_draw_level(const uint32_t* T, int r, uint32_t h) {
    uint64_t level = 0ull;
    for (int k = 0; k < r - 1; ++k) level += h >= T[k] ? 1ull : 0ull;
    return level;
}
// what the per-row kernels keep in LDS of variable `tid` of family `fam`: where its table starts behind offsets[0], its level
// count, its parents without itself
__device__ __forceinline__ void bn_stage_var(int tid, size_t fam, const long long* offsets, const uint8_t* card, const uint64_t* parents,
                                             int* s_base, unsigned char* s_card, uint64_t* s_par) {
    s_base[tid] = (int)(offsets[fam] - offsets[0]);
    s_card[tid] = card[tid];
    s_par[tid] = parents[fam] & ~(1ull << tid);
}

// One wave per structure, lane = variable, the lane's parent row one u64 -> the lane's ancestors (bit-row Warshall: after
// round k every path through 0 .. k is in)
__device__ __forceinline__ uint64_t bn_closure(uint64_t row, int n) {
    uint64_t reach = row;
    for (int k = 0; k < n; ++k) {
        const uint64_t rk = dvs_bcast64(reach, k);
        if ((reach >> k) & 1ull) reach |= rk;
    }
    return reach;
}

// ---- the dense table of a family -------------------------------------------------------------------------------------------
// The set bits of pm (the parents, the variable's own bit masked off by the caller) as (id, mixed-radix stride) pairs, lowest
// id fastest, and q, the product of their level counts, as far as q * r stays within `limit` cells; r is what a
// configuration holds (the levels of the variable; for a CI test those of x times those of y; below 1 it counts as 1 and the
// caller refuses).  Returns the number of parents, or -1 for a bit >= n or a table beyond the limit (*q_out is then not
// written).  The light form, bn_family_layout<false>, gives q and the refusal only and takes null for the arrays.  One thread
// calls it.
template <bool IDS = true>
__device__ __forceinline__ int bn_family_layout(uint64_t pm, const int n, const uint8_t* card, long long r, const long long limit,
                                                int* par_id, int* par_stride, long long* q_out) {
    if (r < 1) r = 1;
    long long q = 1;
    int np = 0;
    for (; pm; pm &= pm - 1ull) {
        const int p = dvs_ctz64(pm);
        if (p >= n) return -1;
        if (IDS) {
            par_id[np] = p;
            par_stride[np] = (int)q;
        }
        q *= card[p];
        if (q * r > limit) return -1;
        ++np;
    }
    *q_out = q;
    return q * r > limit ? -1 : np;
}

// Counts the samples into the dense table: zero `bins` counters, then one integer atomic per sample at cell(row, key), key
// the configuration of the np parents; barriers in between and after.  ROWS: sample s is row rows[s].  GUARD: a sample whose
// cell is >= bins (a level code >= its level count) is left out; without it the caller vouches for the codes.  Every thread of
// the workgroup calls it.
template <bool ROWS, bool GUARD, class Cell>
__device__ __forceinline__ void bn_dense_count(unsigned* hist, const int bins, const uint64_t* data, const int words, const int S,
                                               const int* rows, const int np, const int* par_id, const int* par_stride, Cell&& cell) {
    for (int i = threadIdx.x; i < bins; i += blockDim.x) hist[i] = 0u;
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += blockDim.x) {
        const uint64_t* row = data + (size_t)(ROWS ? rows[s] : s) * words;
        int key = 0;
        for (int i = 0; i < np; ++i) key += bic_level(row, par_id[i]) * par_stride[i];
        const int idx = cell(row, key);
        if (!GUARD || idx < bins) atomicAdd(&hist[idx], 1u);
    }
    __syncthreads();
}

// ---- launchers -----------------------------------------------------------------------------------------------------------
// One launch of kernel<0> (the penalised likelihoods: type <= DVS_SCORE_BIC) or kernel<1> (the Dirichlet scores) over a dense
// table's LDS, under the profile name of its family (bench_hillclimb.py, bench_tabu.py and profiles/*.json look them up).
#define BN_LAUNCH_FAMILY(type, kernel, name0, name1, grid, st, args)                                      \
    do {                                                                                                  \
        if ((type) <= DVS_SCORE_BIC) {                                                                    \
            DVS_SET_LDS(kernel<0>, bn_table_lds());                                                       \
            DVS_LAUNCH_AS(name0, kernel<0>, grid, dim3(256), bn_table_lds(), st, args);                   \
        } else {                                                                                          \
            DVS_SET_LDS(kernel<1>, bn_table_lds());                                                       \
            DVS_LAUNCH_AS(name1, kernel<1>, grid, dim3(256), bn_table_lds(), st, args);                   \
        }                                                                                                 \
    } while (0)
