// A multivariate normal conditioned on the observed part of every row: the posterior of the missing variables,
// the log-density of the observed ones, their sum and the summed conditional covariance, by one partial Cholesky factorisation
// per missingness pattern.  Included by k_bic.hip after dvs_mixed_params.h.  Semantics, operation orders and refusals:
// include/dvs_gaussian_incomplete.h.  Plain fp64 vector arithmetic: no f64 MFMA, no fused multiply-add (contraction is off in every
// function that rounds), no floating-point atomics.  The image of 256 rows, the chunk length and the two levels of the sum are
// dvs_fitted.h's.
//
//   k_gbn_condition          one workgroup per chunk of 256 positions of `order`.  The chunk's rows are gathered into the
//                            lane-interleaved image (t_i of position r at t[i * GPAR_LD + r]: a lane's own column is
//                            conflict-free); three packed lower triangles sit next to it: cov, the working A and the chunk's
//                            covariance sum.  The workgroup walks the chunk's runs of equal masks in order.  It factors a run's
//                            pattern once, together: per pivot one thread per variable takes l_i, then the threads stride over the
//                            trailing cells.  The factor stays in A (l_i of pivot j in cell (i, j), d in s_d).  The lanes that own
//                            the run's rows then substitute, reading l_i as LDS broadcasts.  Rows that arrive sorted by mask cost
//                            one factorisation per pattern and chunk and O(n^2) each; a chunk whose rows all differ factors 256
//                            times.  Nothing per row lives in a thread-private array: a row is indexed by variable id at run time.
//   k_gbn_condition_finish   one workgroup per covariance cell adds the chunks' values as k_bn_loglik_sum adds chunk sums and
//                            writes both triangles; the last workgroup adds the chunks' refused rows.
#pragma once
#include "dvs_gaussian_params.h"

constexpr int GINC_TRI = DVS_WTOK * (DVS_WTOK + 1) / 2;      // the cells of a packed lower triangle at n = 48
static_assert((size_t)GPAR_LD * DVS_WTOK * sizeof(double) + 3 * GINC_TRI * sizeof(double) + 12 * 1024 <= 160 * 1024,
              "the image, the three triangles and the per-position words fit a compute unit's LDS");

__device__ __forceinline__ int ginc_tri(int i, int h) { return i * (i + 1) / 2 + h; }                 // i >= h
__device__ __forceinline__ int ginc_sym(int i, int j) { return i >= j ? ginc_tri(i, j) : ginc_tri(j, i); }

__global__ __launch_bounds__(GPAR_ROWS) void k_gbn_condition(GbnConditionArgs a) {
#pragma clang fp contract(off)
    DVS_DYN_LDS(smem);
    __shared__ double s_C[GINC_TRI], s_A[GINC_TRI], s_acc[GINC_TRI];
    __shared__ double s_mean[DVS_WTOK], s_d[DVS_WTOK], s_l[DVS_WTOK], s_ld;
    __shared__ uint64_t s_mask[GPAR_ROWS];
    __shared__ int s_row[GPAR_ROWS], s_bad[GPAR_ROWS], s_refused;
    __shared__ unsigned short s_cell[GINC_TRI];              // cell -> (i << 8) | h
    double* t = (double*)smem;
    const int tid = threadIdx.x, n = a.n, chunk = blockIdx.x, cells = n * (n + 1) / 2;
    const bool full = a.cvar != nullptr || a.ccov != nullptr;            // false: the M x M cells are never read, so not updated
    const uint64_t low = (1ull << n) - 1ull;
    const int len = fit_chunk_len(a.rows, chunk);
    const long long pos0 = (long long)chunk * GPAR_ROWS;

    for (int e = tid; e < n * n; e += GPAR_ROWS) {
        const int i = e / n, h = e - i * n;
        if (h > i) continue;
        const int c = ginc_tri(i, h);
        s_cell[c] = (unsigned short)((i << 8) | h);
        s_C[c] = a.cov[e];
        s_acc[c] = 0.0;
    }
    if (tid < n) s_mean[tid] = a.mean[tid];
    if (tid == 0) s_refused = 0;
    if (tid < len) {
        const int row = a.order != nullptr ? a.order[pos0 + tid] : (int)(pos0 + tid);
        const uint64_t m = a.observed[row];
        s_row[tid] = row;
        s_mask[tid] = m;
        s_bad[tid] = (m >> n) != 0ull ? 1 : 0;
    }
    __syncthreads();
    for (int e = tid; e < len * n; e += GPAR_ROWS) {
        const int r = e / n, c = e - r * n;
        double v = 0.0;
        if ((s_mask[r] >> c) & 1ull) {
            const double xv = a.x[(size_t)s_row[r] * n + c];
            if (!gpar_finite(xv)) s_bad[r] = 1;              // every writer stores the same word
            v = xv - s_mean[c];
        }
        t[c * GPAR_LD + r] = v;
    }
    __syncthreads();

    double term = 0.0;                                       // this position's logp, +0 when refused or absent
    int start = 0;
    while (start < len) {                                    // uniform: every thread walks the same runs
        const uint64_t m = s_mask[start];
        int end = start + 1, cnt = s_bad[start] ? 0 : 1;
        while (end < len && s_mask[end] == m) {
            cnt += s_bad[end] ? 0 : 1;
            ++end;
        }
        const uint64_t obs = m & low, mis = low & ~obs;
        const int k = __popcll(obs);
        bool ok = (m >> n) == 0ull && cnt > 0;
        if (ok) {
            for (int c = tid; c < cells; c += GPAR_ROWS) s_A[c] = s_C[c];
            if (tid == 0) s_ld = 0.0;
            __syncthreads();
            uint64_t rem = low;                              // the variables not yet pivoted
            for (uint64_t pm = obs; pm; pm &= pm - 1ull) {
                const int j = dvs_ctz64(pm);
                const double ajj = s_A[ginc_tri(j, j)];
                const double thr = ((double)(k + 1) * 2.220446049250313e-16) * s_C[ginc_tri(j, j)];
                if (!gpar_finite(ajj) || ajj <= thr) {       // uniform, and no barrier of this pivot has been met
                    ok = false;
                    break;
                }
                const double d = sqrt(ajj);
                rem &= ~(1ull << j);
                if (tid == 0) {
                    s_ld = s_ld + log(ajj);
                    s_d[j] = d;
                }
                if (tid < n && ((rem >> tid) & 1ull)) {
                    const int c = ginc_sym(tid, j);
                    const double l = s_A[c] / d;
                    s_l[tid] = l;
                    s_A[c] = l;                              // the factor stays where the cell was: row and column j are done
                }
                __syncthreads();
                for (int c = tid; c < cells; c += GPAR_ROWS) {
                    const int i = s_cell[c] >> 8, h = s_cell[c] & 255;
                    if (!((rem >> i) & 1ull) || !((rem >> h) & 1ull)) continue;
                    if (!full && !(((obs >> i) | (obs >> h)) & 1ull)) continue;
                    const double prod = s_l[i] * s_l[h];
                    s_A[c] = s_A[c] - prod;
                }
                __syncthreads();
            }
        }
        __syncthreads();
        if (tid >= start && tid < end) {
            const bool bad = !ok || s_bad[tid] != 0;
            double q = bn_nan(), lp = bn_nan();
            if (!bad) {
                q = 0.0;
                uint64_t rem = low;
                for (uint64_t pm = obs; pm; pm &= pm - 1ull) {
                    const int j = dvs_ctz64(pm);
                    const double y = t[j * GPAR_LD + tid] / s_d[j];
                    const double yy = y * y;
                    q = q + yy;
                    rem &= ~(1ull << j);
                    for (uint64_t rm = a.completed != nullptr ? rem : rem & obs; rm; rm &= rm - 1ull) {
                        const int i = dvs_ctz64(rm);
                        const double prod = s_A[ginc_sym(i, j)] * y;
                        t[i * GPAR_LD + tid] = t[i * GPAR_LD + tid] - prod;
                    }
                }
                const double kc = (double)k * 0.9189385332046727;
                const double hl = 0.5 * s_ld;
                const double norm = kc + hl;
                const double hq = 0.5 * q;
                lp = -(norm + hq);
                term = lp;
            } else {
                atomicAdd(&s_refused, 1);
            }
            if (a.quad != nullptr) a.quad[s_row[tid]] = q;
            a.logp[s_row[tid]] = lp;
        }
        __syncthreads();
        if (a.completed != nullptr || a.cvar != nullptr)
            for (int e = tid; e < (end - start) * n; e += GPAR_ROWS) {
                const int r = start + e / n, c = e % n;
                const bool bad = !ok || s_bad[r] != 0, o = ((obs >> c) & 1ull) != 0ull;
                const size_t at = (size_t)s_row[r] * n + c;
                if (a.completed != nullptr) {
                    double v = bn_nan();
                    if (!bad) v = o ? a.x[at] : s_mean[c] - t[c * GPAR_LD + r];
                    a.completed[at] = v;
                }
                if (a.cvar != nullptr) {
                    double v = bn_nan();
                    if (!bad) v = o ? 0.0 : s_A[ginc_tri(c, c)];
                    a.cvar[at] = v;
                }
            }
        if (a.ccov != nullptr && ok)
            for (int c = tid; c < cells; c += GPAR_ROWS) {
                const int i = s_cell[c] >> 8, h = s_cell[c] & 255;
                if (!((mis >> i) & 1ull) || !((mis >> h) & 1ull)) continue;
                const double prod = (double)cnt * s_A[c];
                s_acc[c] = s_acc[c] + prod;
            }
        __syncthreads();                                     // the next run overwrites A
        start = end;
    }
    fit_chunk_sum(term, &a.partials[chunk]);
    if (tid == 0) {
        a.refused[chunk] = s_refused;
        if (s_refused) atomicOr(a.status, 16);
    }
    if (a.ccov != nullptr)
        for (int c = tid; c < cells; c += GPAR_ROWS) a.cov_partials[(size_t)c * a.chunks + chunk] = s_acc[c];
}

__global__ __launch_bounds__(256) void k_gbn_condition_finish(GbnConditionArgs a) {
    __shared__ long long s_cnt[256];
    const int tid = threadIdx.x, cell = blockIdx.x;
    if (cell == (int)gridDim.x - 1) {                        // the refused rows: integers, any order
        long long s = 0;
        for (int c = tid; c < a.chunks; c += 256) s += a.refused[c];
        s_cnt[tid] = s;
        __syncthreads();
        dvs_block_sum256(tid, s_cnt);
        if (tid == 0 && a.counts != nullptr) *a.counts = s_cnt[0];
        return;
    }
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= cell) ++i;
    const int h = cell - i * (i + 1) / 2;
    const double* p = a.cov_partials + (size_t)cell * a.chunks;
    double s = 0.0;
    for (int c = tid; c < a.chunks; c += 256) s += p[c];
    fit_chunk_sum(s, &a.ccov[(size_t)i * a.n + h]);
    if (tid == 0 && i != h) a.ccov[(size_t)h * a.n + i] = a.ccov[(size_t)i * a.n + h];
}

void dvs_launch_gbn_condition(const GbnConditionArgs& a, dvs_stream_t st) {
    DVS_SET_LDS(k_gbn_condition, gpar_image_lds(DVS_WTOK));
    DVS_LAUNCH(k_gbn_condition, dim3((unsigned)a.chunks), dim3(GPAR_ROWS), gpar_image_lds(a.n), st, a);
    fit_launch_loglik_sum(1, a.chunks, a.partials, a.loglik, st);
    const int cells = a.ccov != nullptr ? a.n * (a.n + 1) / 2 : 0;
    DVS_LAUNCH(k_gbn_condition_finish, dim3((unsigned)cells + 1), dim3(256), 0, st, a);
}
