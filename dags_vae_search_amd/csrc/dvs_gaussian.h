// Gaussian Bayesian networks, next to the discrete scorers whose search layer they share.  Included by
// k_bic.hip after dvs_permtest.h.  Semantics, summation orders and refusals: include/dvs_gaussian.h.
//
//   k_gbn_colsum         one 256-thread workgroup per (set, chunk of DVS_GBN_CHUNK positions): the chunk's rows are staged in
//   k_gbn_mean           LDS (gathered through `rows` with a row set), thread i < n adds column i in position order;
//   k_gbn_cross          k_gbn_mean folds the chunk sums of a (set, column) in chunk order and divides.  k_gbn_cross stages the
//   k_gbn_fold           same rows, centres them in place, and every thread owns cells (i <= j) of the upper triangle, adding
//                        the rounded products in position order; k_gbn_fold adds a cell's chunk values in chunk order and writes
//                        both triangles.  No atomics: the bytes depend on nothing but the definitions.
//   k_gbn_local          one lane per family.  gbn_family is the one device function behind the scorer, the toggle pass and the
//   k_gbn_toggle         fit: it gathers M[Pa + v] from the set's moments (18 KB at n = 48, read through the caches: the lanes
//   k_gbn_fit            of a workgroup may belong to different row sets, so no workgroup-wide image is staged), factors it
//                        row by row into the lane's slice of LDS — element e of lane l at s_L[e * 64 + l], consecutive lanes
//                        in consecutive banks — and returns the squared pivots' sums.  Plain fp64 vector arithmetic: no f64 MFMA,
//                        no fused multiply-add (contraction is off in every function that rounds).
#pragma once
#include "dvs_bn_common.h"

constexpr int GBN_LANES = 64;                                                        // one wave per workgroup of the family kernels
constexpr int GBN_FACTOR = (DVS_GBN_MAX_PARENTS + 1) * (DVS_GBN_MAX_PARENTS + 2) / 2;    // packed lower triangle, v's row last
constexpr size_t GBN_FACTOR_LDS = (size_t)GBN_FACTOR * GBN_LANES * sizeof(double);
static_assert(DVS_GBN_MAX_PARENTS >= 8, "the cap on a family's parents is at least 8");
static_assert(4 * GBN_FACTOR_LDS <= 160 * 1024, "four family workgroups (a wave per SIMD) share a compute unit's 160 KiB of LDS");
static_assert(GBN_FACTOR_LDS <= 64 * 1024, "the factor slices are static LDS");
static_assert((size_t)DVS_GBN_CHUNK * DVS_WTOK * sizeof(double) <= 64 * 1024, "a staged chunk is static LDS");

// ---------------------------------------------------------------------------------------------------------
// Moments
// ---------------------------------------------------------------------------------------------------------
// The chunk routines.  dvs_mixed.h runs the same ones over the segments of a partition (a segment list instead of a set), so
// a block of dvs_cg_moments and a row set of dvs_gbn_moments are one summation.
// stages `len` rows [len][n] into x: row r is data row rows[r], or p0 + r with rows null.  Every thread of the workgroup calls
// it; a barrier follows.
__device__ __forceinline__ void gbn_stage_rows(const double* data, int n, const int* rows, int p0, int len, double* x) {
    for (int e = threadIdx.x; e < len * n; e += blockDim.x) {
        const int r = e / n, c = e - r * n;
        const size_t src = rows != nullptr ? (size_t)rows[r] : (size_t)(p0 + r);
        x[e] = data[src * n + c];
    }
    __syncthreads();
}
// stages chunk `chunk` of set `set`; returns its length
__device__ __forceinline__ int gbn_stage_chunk(const GbnMomentArgs& a, int set, int chunk, double* x) {
    const int p0 = chunk * DVS_GBN_CHUNK;
    const int len = a.set_size - p0 < DVS_GBN_CHUNK ? a.set_size - p0 : DVS_GBN_CHUNK;
    gbn_stage_rows(a.data, a.n, a.rows != nullptr ? a.rows + (size_t)set * (size_t)a.set_size + p0 : nullptr, p0, len, x);
    return len;
}
// pass 1 of a staged chunk: thread i < n adds column i in position order -> out[i]
__device__ __forceinline__ void gbn_chunk_colsum(const double* x, int len, int n, double* out) {
#pragma clang fp contract(off)
    const int i = threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int r = 0; r < len; ++r) s = s + x[r * n + i];
    out[i] = s;
}
// `chunks` chunk values, `stride` doubles apart, added in chunk order from +0
__device__ __forceinline__ double gbn_fold_chunks(const double* part, int chunks, size_t stride) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s = s + part[(size_t)c * stride];
    return s;
}
// cell q of the upper triangle in row-major order: row i holds n - i cells (i, i) .. (i, n - 1)
__device__ __forceinline__ void gbn_tri_cell(int q, int n, int* i_out, int* j_out) {
    int i = 0, at = q;
    while (at >= n - i) {
        at -= n - i;
        ++i;
    }
    *i_out = i;
    *j_out = i + at;
}
// pass 2 of a staged chunk: centres it in place, then every thread owns cells of the upper triangle -> out[tri].  Every thread
// of the 256-thread workgroup calls it (it holds a barrier).
__device__ __forceinline__ void gbn_chunk_cross(double* x, int len, int n, int tri, const double* mean, double* out) {
#pragma clang fp contract(off)
    for (int e = threadIdx.x; e < len * n; e += 256) x[e] = x[e] - mean[e % n];
    __syncthreads();
    for (int q = threadIdx.x; q < tri; q += 256) {
        int i, j;
        gbn_tri_cell(q, n, &i, &j);
        double s = 0.0;
        for (int r = 0; r < len; ++r) {
            const double prod = x[r * n + i] * x[r * n + j];
            s = s + prod;
        }
        out[q] = s;
    }
}

__global__ __launch_bounds__(256) void k_gbn_colsum(GbnMomentArgs a) {
    __shared__ double s_x[DVS_GBN_CHUNK * DVS_WTOK];
    const int set = blockIdx.x / a.chunks, chunk = blockIdx.x - set * a.chunks;
    const int len = gbn_stage_chunk(a, set, chunk, s_x);
    gbn_chunk_colsum(s_x, len, a.n, a.sums + (size_t)blockIdx.x * a.n);
}

__global__ __launch_bounds__(256) void k_gbn_mean(GbnMomentArgs a) {
#pragma clang fp contract(off)
    const int idx = blockIdx.x * 256 + threadIdx.x, n = a.n;
    if (idx >= a.n_sets * n) return;
    const int set = idx / n, i = idx - set * n;
    const double s = gbn_fold_chunks(a.sums + (size_t)set * a.chunks * n + i, a.chunks, (size_t)n);
    double* mom = a.moments + (size_t)set * DVS_GBN_STRIDE(n);
    const double m = (double)a.set_size;
    if (i == 0) mom[0] = m;
    mom[1 + i] = s / m;
}

__global__ __launch_bounds__(256) void k_gbn_cross(GbnMomentArgs a) {
    __shared__ double s_x[DVS_GBN_CHUNK * DVS_WTOK];
    const int set = blockIdx.x / a.chunks, chunk = blockIdx.x - set * a.chunks, n = a.n;
    const int len = gbn_stage_chunk(a, set, chunk, s_x);
    gbn_chunk_cross(s_x, len, n, a.tri, a.moments + (size_t)set * DVS_GBN_STRIDE(n) + 1, a.cells + (size_t)blockIdx.x * a.tri);
}

__global__ __launch_bounds__(256) void k_gbn_fold(GbnMomentArgs a) {
    const int idx = blockIdx.x * 256 + threadIdx.x, n = a.n;
    if (idx >= a.n_sets * a.tri) return;
    const int set = idx / a.tri, q = idx - set * a.tri;
    int i, j;
    gbn_tri_cell(q, n, &i, &j);
    const double s = gbn_fold_chunks(a.cells + (size_t)set * a.chunks * a.tri + q, a.chunks, (size_t)a.tri);
    double* C = a.moments + (size_t)set * DVS_GBN_STRIDE(n) + 1 + n;
    C[i * n + j] = s;
    C[j * n + i] = s;
}

void dvs_launch_gbn_moments(const GbnMomentArgs& in, dvs_stream_t st) {
    GbnMomentArgs a = in;
    const GbnMomentLayout l = dvs_gbn_moment_layout(a.n, a.n_sets, a.set_size);
    a.chunks = (int)l.chunks;
    a.tri = (int)l.tri;
    const dim3 per_chunk((unsigned)(a.n_sets * a.chunks));
    DVS_LAUNCH(k_gbn_colsum, per_chunk, dim3(256), 0, st, a);
    DVS_LAUNCH(k_gbn_mean, dim3((unsigned)((a.n_sets * a.n + 255) / 256)), dim3(256), 0, st, a);
    DVS_LAUNCH(k_gbn_cross, per_chunk, dim3(256), 0, st, a);
    DVS_LAUNCH(k_gbn_fold, dim3((unsigned)((a.n_sets * a.tri + 255) / 256)), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// One family
// ---------------------------------------------------------------------------------------------------------
struct GbnFamily {
    int p;                       // parents; -1: refused
    double m, ldp, rss;          // the set's size, ln det M[Pa], the last squared pivot
};

// element (i, j), j <= i, of the lane's packed factor
__device__ __forceinline__ double& gbn_L(double* L, int i, int j) { return L[(i * (i + 1) / 2 + j) * GBN_LANES]; }

// one row of the factor: variable ai against the first i parents of pm, then its own pivot -> the squared pivot; the caller
// checks it before the next row reads L[i][i]
__device__ __forceinline__ double gbn_factor_row(const double* C, int n, uint64_t pm, int i, int ai, double t, double* L, double* diag) {
#pragma clang fp contract(off)
    uint64_t mj = pm;
    for (int j = 0; j < i; ++j, mj &= mj - 1ull) {
        double s = C[ai * n + dvs_ctz64(mj)];
        for (int k = 0; k < j; ++k) {
            const double prod = gbn_L(L, i, k) * gbn_L(L, j, k);
            s = s - prod;
        }
        gbn_L(L, i, j) = s / gbn_L(L, j, j);
    }
    double s = C[ai * n + ai] + t;                           // t = 0 outside bge: x + 0 is x
    *diag = s;
    for (int k = 0; k < i; ++k) {
        const double prod = gbn_L(L, i, k) * gbn_L(L, i, k);
        s = s - prod;
    }
    gbn_L(L, i, i) = sqrt(s);
    return s;
}

// the pivot rule of include/dvs_gaussian.h: finite, and beyond rounding of zero
__device__ __forceinline__ bool gbn_pivot_ok(double d2, double diag, int p) {
#pragma clang fp contract(off)
    const double eps = 2.220446049250313e-16;                // 2^-52
    return d2 - d2 == 0.0 && d2 > ((double)(p + 2) * eps) * diag;
}

// Factors the family (v, pm) of the set at `mom` into the lane's slice L.  likelihood: refuse m - p - 1 < 1.
__device__ __forceinline__ GbnFamily gbn_family(const double* mom, int n, int v, uint64_t pm, double t, bool likelihood, double* L) {
#pragma clang fp contract(off)
    GbnFamily f;
    f.p = -1;
    f.m = mom[0];
    f.ldp = 0.0;
    f.rss = 0.0;
    pm &= ~(1ull << v);
    const int p = __popcll(pm);
    if ((pm >> n) != 0ull || p > DVS_GBN_MAX_PARENTS) return f;
    if (likelihood && f.m - (double)p - 1.0 < 1.0) return f;
    const double* C = mom + 1 + n;
    double ldp = 0.0, diag;
    uint64_t mi = pm;
    for (int i = 0; i < p; ++i, mi &= mi - 1ull) {
        const double d2 = gbn_factor_row(C, n, pm, i, dvs_ctz64(mi), t, L, &diag);
        if (!gbn_pivot_ok(d2, diag, p)) return f;
        ldp = ldp + log(d2);
    }
    const double d2 = gbn_factor_row(C, n, pm, p, v, t, L, &diag);
    if (!gbn_pivot_ok(d2, diag, p)) return f;
    f.p = p;
    f.ldp = ldp;
    f.rss = d2;
    return f;
}

// the local score of include/dvs_gaussian.h from a factored family; NaN for a refused one
__device__ __forceinline__ double gbn_local(const GbnScoreArgs& a, const GbnFamily& f) {
#pragma clang fp contract(off)
    if (f.p < 0) return bn_nan();
    const double m = f.m, p = (double)f.p;
    if (a.type != DVS_GSCORE_BGE) {
        const double dof = m - p - 1.0;
        const double s2 = f.rss / dof;
        const double ll = -(0.5 * m) * log(6.283185307179586 * s2) - 0.5 * dof;
        if (a.type == DVS_GSCORE_LOGLIK) return ll;
        const double k = a.arg != a.arg ? log(m) / 2.0 : a.arg;
        return ll - k * (p + 2.0);
    }
    const double g = a.arg2 - (double)a.n + p;
    const double ldf = f.ldp + log(f.rss);
    double s = -(0.5 * m) * log(3.141592653589793);
    s = s + 0.5 * log(a.arg / (a.arg + m));
    s = s + bn_lgamma(0.5 * (m + g + 1.0));
    s = s - bn_lgamma(0.5 * (g + 1.0));
    s = s + (0.5 * (g + p + 1.0)) * log(a.t);
    s = s - (0.5 * (m + g + 1.0)) * ldf;
    s = s + (0.5 * (m + g)) * f.ldp;
    return s;
}

__device__ __forceinline__ const double* gbn_set(const GbnScoreArgs& a, int b) {
    return a.moments + (size_t)(a.set_of != nullptr ? a.set_of[b] : 0) * DVS_GBN_STRIDE(a.n);
}

// the score of family (b, v) with parent set pm; a refusal sets bit 4 of status
__device__ __forceinline__ double gbn_family_score(const GbnScoreArgs& a, int b, int v, uint64_t pm, double* L) {
    const GbnFamily f = gbn_family(gbn_set(a, b), a.n, v, pm, a.type == DVS_GSCORE_BGE ? a.t : 0.0, a.type != DVS_GSCORE_BGE, L);
    if (f.p < 0) atomicOr(a.status, 16);
    return gbn_local(a, f);
}

__global__ __launch_bounds__(GBN_LANES) void k_gbn_local(GbnScoreArgs a) {
    __shared__ double s_L[GBN_FACTOR * GBN_LANES];
    const long long fam = (long long)blockIdx.x * GBN_LANES + threadIdx.x;
    if (fam >= (long long)a.B * a.n) return;
    const int b = (int)(fam / a.n), v = (int)(fam - (long long)b * a.n);
    a.local[fam] = gbn_family_score(a, b, v, a.parents[fam], s_L + threadIdx.x);
}

// out[b] = local[b][0] + ... + local[b][n - 1], from +0 in that order
__global__ __launch_bounds__(256) void k_gbn_total(GbnScoreArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    double s = 0.0;
    for (int v = 0; v < a.n; ++v) s = s + a.local[(size_t)b * a.n + v];
    a.out[b] = s;
}

void dvs_launch_gbn_scores(const GbnScoreArgs& a, dvs_stream_t st) {
    const long long fams = (long long)a.B * a.n;
    DVS_LAUNCH(k_gbn_local, dim3((unsigned)((fams + GBN_LANES - 1) / GBN_LANES)), dim3(GBN_LANES), 0, st, a);
    DVS_LAUNCH(k_gbn_total, dim3((unsigned)((a.B + 255) / 256)), dim3(256), 0, st, a);
}

// One lane per cell (row, u) of the rows a pass covers: the two worklist slots of every structure, or all its n rows.
__global__ __launch_bounds__(GBN_LANES) void k_gbn_toggle(GbnToggleArgs t) {
    __shared__ double s_L[GBN_FACTOR * GBN_LANES];
    const GbnScoreArgs& a = t.s;
    const int n = a.n;
    const long long rows = t.worklist != nullptr ? 2ll * a.B : (long long)a.B * n;
    const long long idx = (long long)blockIdx.x * GBN_LANES + threadIdx.x;
    if (idx >= rows * n) return;
    const int row = (int)(idx / n), u = (int)(idx - (long long)row * n);
    int b, v;
    if (t.worklist != nullptr) {
        v = t.worklist[row];
        b = row >> 1;
        if (v < 0 || v >= n || u == v) return;       // empty slot; L of a moved row is the T cell of the move (k_hc_step)
    } else {
        v = row % n;
        b = row / n;
    }
    const size_t cell = (size_t)b * n + v;
    const double score = gbn_family_score(a, b, v, a.parents[cell] ^ (u == v ? 0ull : 1ull << u), s_L + threadIdx.x);
    if (u == v) {
        a.local[cell] = score;
        t.toggles[cell * n + u] = bn_nan();
    } else {
        t.toggles[cell * n + u] = score;
    }
}

void dvs_launch_gbn_toggle(const GbnToggleArgs& t, dvs_stream_t st) {
    const long long rows = t.worklist != nullptr ? 2ll * t.s.B : (long long)t.s.B * t.s.n;
    DVS_LAUNCH(k_gbn_toggle, dim3((unsigned)((rows * t.s.n + GBN_LANES - 1) / GBN_LANES)), dim3(GBN_LANES), 0, st, t);
}

// the backward solve of include/dvs_gaussian.h over the last row of a factored family, in place: L[p][i] becomes beta_i
__device__ __forceinline__ void gbn_backsolve(double* L, int p) {
#pragma clang fp contract(off)
    for (int i = p - 1; i >= 0; --i) {
        double s = gbn_L(L, p, i);
        for (int k = i + 1; k < p; ++k) {
            const double prod = gbn_L(L, k, i) * gbn_L(L, p, k);
            s = s - prod;
        }
        gbn_L(L, p, i) = s / gbn_L(L, i, i);
    }
}

// One lane per family: the factor, then the backward solve over the last row in place.
__global__ __launch_bounds__(GBN_LANES) void k_gbn_fit(GbnFitArgs t) {
#pragma clang fp contract(off)
    __shared__ double s_L[GBN_FACTOR * GBN_LANES];
    const GbnScoreArgs& a = t.s;
    const int n = a.n;
    const long long fam = (long long)blockIdx.x * GBN_LANES + threadIdx.x;
    if (fam >= (long long)a.B * n) return;
    const int b = (int)(fam / n), v = (int)(fam - (long long)b * n);
    double* L = s_L + threadIdx.x;
    const double* mom = gbn_set(a, b);
    const uint64_t pm = a.parents[fam] & ~(1ull << v);
    const GbnFamily f = gbn_family(mom, n, v, pm, 0.0, true, L);
    double* coef = t.coef + (size_t)fam * n;
    if (f.p < 0) {
        atomicOr(a.status, 16);
        for (int u = 0; u < n; ++u) coef[u] = bn_nan();
        t.intercept[fam] = bn_nan();
        t.sd[fam] = bn_nan();
        return;
    }
    const int p = f.p;
    gbn_backsolve(L, p);
    for (int u = 0; u < n; ++u) coef[u] = 0.0;
    double c0 = mom[1 + v];
    uint64_t mi = pm;
    for (int i = 0; i < p; ++i, mi &= mi - 1ull) {
        const int u = dvs_ctz64(mi);
        const double beta = gbn_L(L, p, i);
        coef[u] = beta;
        const double prod = beta * mom[1 + u];
        c0 = c0 - prod;
    }
    t.intercept[fam] = c0;
    t.sd[fam] = sqrt(f.rss / (f.m - (double)p - 1.0));
}

void dvs_launch_gbn_fit(const GbnFitArgs& t, dvs_stream_t st) {
    const long long fams = (long long)t.s.B * t.s.n;
    DVS_LAUNCH(k_gbn_fit, dim3((unsigned)((fams + GBN_LANES - 1) / GBN_LANES)), dim3(GBN_LANES), 0, st, t);
}
