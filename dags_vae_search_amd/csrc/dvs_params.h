// Parameters of a discrete Bayesian network on the device (definitions in include/dvs.h): the conditional
// probability tables of a structure, forward sampling from them and the log-likelihood of held-out rows.  Included by
// k_bic.hip after dvs_citest.h.  Integer counts and fp64 arithmetic, every sum in a fixed order, no atomics but the integer LDS
// histogram adds and the status atomicOr: two runs give equal bytes.  The order and the two levels of the sum are dvs_fitted.h's.
//
//   k_bn_fit             one workgroup per (structure, variable): the dense (configuration, level) table in dynamic LDS, counted
//                        by the scorer's routine (bn_dense_count, here with the range guard); the thread that owns configuration
//                        j takes N_j and writes its r cells.  No sort path: a table above 36 864 cells is refused.
//   k_bn_sample_prep     one workgroup: thread 0 checks the slots and orders the variables (fit_order); all threads then check
//                        the rows of the tables and write their u32 thresholds.
//   k_bn_sample          one thread per row: the variables in the prep's order, the row's levels in registers (BnRow), one
//                        counter-based draw per (row, variable); thresholds from LDS when the tables fit DVS_BN_SAMPLE_LDS_CELLS.
//   k_bn_loglik_prep     one workgroup per (structure, variable): checks the slot and writes log(theta) of its cells.
//   k_bn_loglik_rows     one thread per row, one workgroup per 256 rows of one structure: the row term, then a fixed tree
//                        (fit_chunk_sum); k_bn_loglik_sum of dvs_fitted.h adds the chunk partials of a structure.
#pragma once
#include "dvs_fitted.h"

// ---------------------------------------------------------------------------------------------------------
// k_bn_fit
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bn_fit(BnFitArgs a) {
    DVS_DYN_LDS(smem);
    __shared__ int par_id[48], par_stride[48];
    __shared__ int s_np, s_q;
    const int v = blockIdx.x % a.n, tid = threadIdx.x;
    const size_t fam = blockIdx.x;                           // = structure * n + v
    const int r = a.card[v];
    if (tid == 0) {
        long long q = 0;
        int np = bn_family_layout(a.parents[fam] & ~(1ull << v), a.n, a.card, r, BIC_MAX_BINS, par_id, par_stride, &q);
        const long long lo = a.offsets[fam], hi = a.offsets[fam + 1];
        if (np >= 0 && (r < 1 || lo < 0 || hi - lo != q * r || hi > a.cpt_cells)) np = -1;
        s_np = np;
        s_q = (int)q;
    }
    __syncthreads();
    const int np = s_np;
    if (np < 0) {
        if (tid == 0) atomicOr(a.status, 16);
        return;
    }
    unsigned* hist = (unsigned*)smem;
    const int q = s_q, bins = q * r;
    // guarded: a level code >= card is never written out of the table
    bn_dense_count<false, true>(hist, bins, a.data, a.words, a.S, nullptr, np, par_id, par_stride,
                                [&](const uint64_t* row, int key) { return key * r + bic_level(row, v); });
    double* out = a.cpt + a.offsets[fam];
    {
#pragma clang fp contract(off)
        const double dr = (double)r;
        const double alpha = a.method == 1 ? a.iss / (dr * (double)q) : 0.0;
        const double ralpha = dr * alpha;
        for (int j = tid; j < q; j += blockDim.x) {
            unsigned nj = 0;
            for (int k = 0; k < r; ++k) nj += hist[j * r + k];
            const double dn = (double)nj;
            for (int k = 0; k < r; ++k) {
                const double c = (double)hist[j * r + k];
                double th;
                if (a.method == 1) th = (c + alpha) / (dn + ralpha);
                else if (nj) th = c / dn;
                else th = a.unobserved ? 1.0 / dr : bn_nan();
                out[(size_t)j * r + k] = th;
            }
        }
    }
}

void dvs_launch_bn_fit(const BnFitArgs& in, dvs_stream_t st) {
    BnFitArgs a = in;
    a.words = bic_words(a.n);
    DVS_SET_LDS(k_bn_fit, bn_table_lds());
    DVS_LAUNCH(k_bn_fit, dim3((unsigned)a.B * a.n), dim3(256), bn_table_lds(), st, a);
}

// ---------------------------------------------------------------------------------------------------------
// k_bn_sample_prep, k_bn_sample
// ---------------------------------------------------------------------------------------------------------
constexpr int BN_HDR_DRAWABLE = 48;                          // header word after order [48]

__global__ __launch_bounds__(256) void k_bn_sample_prep(BnSampleArgs a) {
    __shared__ int s_state, s_bad;                           // s_state: 0 go on, else the status bits that stop the call
    const int tid = threadIdx.x, n = a.n;
    const long long base = a.offsets[0];
    if (tid == 0) {
        int state = 0;
        for (int v = 0; v < n && !state; ++v) {              // the slots: every table as long as its family says
            long long q = 0;
            const long long r = a.card[v], lo = a.offsets[v] - base, hi = a.offsets[v + 1] - base;
            const bool ok = r >= 1 && r <= 16 && lo >= 0 && hi <= a.n_cells &&
                            bn_family_layout<false>(a.parents[v] & ~(1ull << v), n, a.card, r, a.n_cells, nullptr, nullptr, &q) >= 0;
            if (!ok || hi - lo != q * r) state = 16;
        }
        if (!state && a.offsets[n] - base != a.n_cells) state = 16;
        // the slots have refused a parent bit >= n
        if (!state && !fit_order(n, [&](int v) { return a.parents[v] & ~(1ull << v); }, a.header)) state = 1;
        s_state = state;
        s_bad = 0;
    }
    __syncthreads();
    if (s_state) {
        if (tid == 0) {
            atomicOr(a.status, s_state);
            a.header[BN_HDR_DRAWABLE] = 0;
        }
        return;
    }
    int bad = 0;
    for (int v = 0; v < n; ++v) {
        const long long lo = a.offsets[v] - base;
        const int r = a.card[v], q = (int)((a.offsets[v + 1] - base - lo) / r);
        for (int j = tid; j < q; j += blockDim.x) {
            const double* th = a.cpt + base + lo + (size_t)j * r;
            uint32_t* T = a.thr + lo + (size_t)j * r;
            double c = 0.0;
            int last = -1;                                   // the last level with theta > 0
            for (int k = 0; k < r; ++k) {
                const double t = th[k];
                if (!(t >= 0.0) || !(t <= 1.7976931348623157e308)) bad = 1;          // NaN, negative, infinite
                if (t > 0.0) last = k;
                c += t;
                const double x = floor(c * 2147483648.0);
                T[k] = x >= 2147483648.0 ? 0x80000000u : x >= 0.0 ? (uint32_t)x : 0u;
            }
            if (!(fabs(c - 1.0) <= 1e-9)) bad = 1;
            for (int k = last < 0 ? 0 : last; k < r; ++k) T[k] = 0x80000000u;
        }
    }
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    if (tid == 0) {
        if (s_bad) atomicOr(a.status, 64);
        a.header[BN_HDR_DRAWABLE] = s_bad ? 0 : 1;
    }
}

template <bool STAGED>
__global__ __launch_bounds__(256) void k_bn_sample(BnSampleArgs a) {
    DVS_DYN_LDS(smem);
    __shared__ int s_order[48], s_base[48];
    __shared__ unsigned char s_card[48];
    __shared__ uint64_t s_par[48];
    const int tid = threadIdx.x, n = a.n;
    if (!a.header[BN_HDR_DRAWABLE]) return;                  // uniform: the prep refused the network
    if (tid < n) {
        s_order[tid] = a.header[tid];
        bn_stage_var(tid, tid, a.offsets, a.card, a.parents, s_base, s_card, s_par);
    }
    const uint32_t* thr = a.thr;
    if (STAGED) {
        uint32_t* lt = (uint32_t*)smem;
        for (int i = tid; i < (int)a.n_cells; i += blockDim.x) lt[i] = a.thr[i];
        thr = lt;
    }
    __syncthreads();
    const long long row = (long long)blockIdx.x * 256 + tid;
    if (row >= a.rows) return;
    const uint32_t g = a.row_offset + (uint32_t)row;
    const uint32_t key = dvs_site_key(a.seed_lo, a.seed_hi, DVS_SITE_BN_SAMPLE, g);
    BnRow x = {0ull, 0ull, 0ull};
    for (int i = 0; i < n; ++i) {
        const int v = s_order[i], r = s_card[v];
        const int cfg = bn_row_config(x, s_par[v], s_card);
        const uint32_t* T = thr + s_base[v] + cfg * r;
        const uint32_t h = dvs_draw(key, (uint32_t)v) >> 1;
        x = bn_row_with(x, v, bn_draw_level(T, r, h));
    }
    bn_row_store(a.out + (size_t)row * a.words, x, a.words);
}

void dvs_launch_bn_sample(const BnSampleArgs& in, uint64_t seed, dvs_stream_t st) {
    BnSampleArgs a = in;
    a.words = bic_words(a.n);
    dvs_seed_split(a, seed);
    DVS_LAUNCH(k_bn_sample_prep, dim3(1), dim3(256), 0, st, a);
    const unsigned grid = (unsigned)((a.rows + 255) / 256);
    if (a.n_cells <= DVS_BN_SAMPLE_LDS_CELLS) {
        const size_t lds = (size_t)DVS_BN_SAMPLE_LDS_CELLS * sizeof(uint32_t);
        DVS_LAUNCH_AS("k_bn_sample_lds", k_bn_sample<true>, dim3(grid), dim3(256), lds, st, a);
    } else {
        DVS_LAUNCH_AS("k_bn_sample_global", k_bn_sample<false>, dim3(grid), dim3(256), 0, st, a);
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_bn_loglik_prep, k_bn_loglik_rows
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bn_loglik_prep(BnLoglikArgs a) {
    __shared__ long long s_cells;
    const int v = blockIdx.x % a.n, tid = threadIdx.x;
    const size_t fam = blockIdx.x;
    const long long base = a.offsets[0], lo = a.offsets[fam] - base, hi = a.offsets[fam + 1] - base;
    if (tid == 0) {
        long long q = 0;
        const int np = bn_family_layout<false>(a.parents[fam] & ~(1ull << v), a.n, a.card, a.card[v], 0x7fffffffLL, nullptr, nullptr, &q);
        const bool ok = np >= 0 && a.card[v] >= 1 && lo >= 0 && hi - lo == q * a.card[v] && hi <= a.log_cells;
        s_cells = ok ? hi - lo : -1;
        a.fam_ok[fam] = ok ? 1 : 0;
        if (!ok) atomicOr(a.status, 16);
    }
    __syncthreads();
    const long long cells = s_cells;
    for (long long i = tid; i < cells; i += blockDim.x) a.logs[lo + i] = log(a.cpt[base + lo + i]);
}

__global__ __launch_bounds__(256) void k_bn_loglik_rows(BnLoglikArgs a) {
    __shared__ int s_base[48], s_ok;
    __shared__ unsigned char s_card[48];
    __shared__ uint64_t s_par[48];
    const int tid = threadIdx.x, n = a.n;
    const int b = blockIdx.x / a.chunks, chunk = blockIdx.x - b * a.chunks;
    if (tid == 0) s_ok = 1;
    __syncthreads();
    if (tid < n) {
        const size_t fam = (size_t)b * n + tid;
        bn_stage_var(tid, fam, a.offsets, a.card, a.parents, s_base, s_card, s_par);
        if (!a.fam_ok[fam]) s_ok = 0;
    }
    __syncthreads();
    const long long row = (long long)chunk * 256 + tid;
    double term = 0.0;
    if (row < a.rows) {
        const BnRow x = bn_row_load(a.data + (size_t)row * a.words, a.words);
        bool ok = s_ok != 0;
        for (int v = 0; v < n; ++v)
            if (bn_level(x, v) >= s_card[v]) ok = false;
        if (!ok) {
            if (s_ok) atomicOr(a.status, 16);                // a level code >= card; a refused family has said so already
            term = bn_nan();
        } else {
            for (int v = 0; v < n; ++v) {
                const int cfg = bn_row_config(x, s_par[v], s_card);
                term += a.logs[s_base[v] + cfg * (int)s_card[v] + bn_level(x, v)];
            }
        }
        if (a.per_row) a.per_row[(size_t)b * a.rows + row] = term;
    }
    fit_chunk_sum(term, &a.partials[(size_t)b * a.chunks + chunk]);
}

void dvs_launch_bn_loglik(const BnLoglikArgs& in, dvs_stream_t st) {
    BnLoglikArgs a = in;
    a.words = bic_words(a.n);
    DVS_LAUNCH(k_bn_loglik_prep, dim3((unsigned)a.B * a.n), dim3(256), 0, st, a);
    DVS_LAUNCH(k_bn_loglik_rows, dim3((unsigned)a.B * a.chunks), dim3(256), 0, st, a);
    fit_launch_loglik_sum(a.B, a.chunks, a.partials, a.out, st);
}
