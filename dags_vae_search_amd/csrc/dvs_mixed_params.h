// A fitted conditional Gaussian network on the device: forward sampling of its real columns, the continuous
// part of the log-likelihood of held-out rows and prediction.  Included by k_bic.hip after dvs_mixed.h and
// dvs_gaussian_params.h.  Semantics, operation orders and refusals: include/dvs_mixed_params.h.  Plain fp64 vector arithmetic:
// no f64 MFMA, no fused multiply-add (contraction is off in every function that rounds), no floating-point atomics.  What makes
// an all-continuous network give the Gaussian entry points' bytes is dvs_fitted.h's: the order, the image, the noise draw, the
// density term, the blanket update and the two levels of the sum (k_bn_loglik_sum adds the chunk sums).
//
//   k_cgbn_prep          one wave: the rules on card / parents / offset and the topological order, into the workspace header.
//   k_cgbn_cells         one thread per (continuous variable, configuration): the rule on the cell's parameters (bit 6) and
//                        c = log(sd) + log(sqrt(2 pi)); an empty configuration (sd NaN) is skipped.
//   k_cgbn_sample        one thread per row, 256 rows per workgroup, the row's packed words in registers, its real values in the
//   k_cgbn_loglik_rows   image of dvs_fitted.h (column c of row r at x[c * GPAR_LD + r]: coalesced global traffic and
//   k_cgbn_predict       conflict-free LDS writes both ways).  k_cgbn_loglik_rows ends in dvs_bn_loglik's tree.
// The network's arcs are a compact list in LDS (cgbn_stage): for every continuous variable its discrete parents with their radix
// multipliers, its continuous parents with their columns of x, and its first cell.  The per-configuration parameters do not fit
// LDS at q = 4096: a row reads them from global memory at cell * n + u, for its parents only.
#pragma once
#include "dvs_gaussian_params.h"

constexpr int CGBN_HDR_SOUND = 48;                           // header word after order [48], as dvs_bn_sample's
constexpr int CGBN_HDR_BAD_CELL = 49;                        // set by k_cgbn_cells: a cell broke bit 6

struct alignas(16) CgbnLists {
    int off[DVS_WTOK + 1];                                   // the entries of v: off[v] .. off[v + 1], discrete parents first
    int nd[DVS_WTOK];                                        // how many of them are discrete
    int cell0[DVS_WTOK];                                     // offset[v]
    unsigned short aux[GPAR_MAX_ARCS];                       // a discrete parent: its radix multiplier; a continuous one: its column
    unsigned char idx[GPAR_MAX_ARCS];
    unsigned char col[DVS_WTOK], card[DVS_WTOK];
    uint64_t par[DVS_WTOK];                                  // Pa(v) of a continuous v, the self bit off; 0 for a discrete v
};
static_assert((size_t)GPAR_LD * DVS_WTOK * sizeof(double) + sizeof(CgbnLists) + 16 * GPAR_ROWS * sizeof(double) + 1024 <= 160 * 1024,
              "the image, the lists and mode 2's a_k fit a compute unit's LDS");

__device__ __forceinline__ bool cgbn_sound(const int* header) { return header[CGBN_HDR_SOUND] != 0 && header[CGBN_HDR_BAD_CELL] == 0; }

// ---------------------------------------------------------------------------------------------------------
// The rules and the order
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_cgbn_prep(CgbnRowArgs a) {
    __shared__ uint64_t s_par[DVS_WTOK];
    __shared__ int s_card[DVS_WTOK], s_order[DVS_WTOK], s_state;
    const int tid = threadIdx.x, n = a.net.n;
    const uint64_t low = (1ull << n) - 1ull;                 // n <= 48
    if (tid == 0) s_state = 0;
    if (tid < n) {
        s_par[tid] = a.net.parents[tid] & ~(1ull << tid);
        s_card[tid] = a.net.card[tid];
    }
    __syncthreads();
    int bad = 0;
    if (tid < n) {
        const uint64_t pm = s_par[tid];
        const int c = s_card[tid];
        if ((pm >> n) != 0ull || c > 16) bad = 16;
        long long q = c > 0 ? 0 : 1;
        for (uint64_t m = pm & low; m; m &= m - 1ull) {
            const int u = dvs_ctz64(m), cu = s_card[u];
            if (c > 0 && cu == 0) bad = 16;                  // a continuous parent of a discrete variable
            if (c == 0 && cu > 0 && q <= DVS_CG_MAX_CONFIGS) q *= cu;
        }
        if (q > DVS_CG_MAX_CONFIGS || a.net.offset[tid + 1] - a.net.offset[tid] != q) bad = 16;
    }
    if (tid == 0) {
        int zeros = 0;
        for (int v = 0; v < n; ++v) zeros += s_card[v] == 0;
        if (zeros != a.net.nc || a.net.offset[0] != 0 || a.net.offset[n] != a.net.cells) bad = 16;
        // the target is of the kind the mode needs
        if (a.target >= 0 && (s_card[a.target] > 0) != (a.mode == DVS_CGBN_PREDICT_CLASS)) bad = 16;
    }
    if (bad) atomicOr(&s_state, bad);
    __syncthreads();
    if (tid == 0) {
        if (!fit_order(n, [&](int v) { return s_par[v] & low; }, s_order)) s_state |= 1;
    }
    __syncthreads();
    const int state = s_state;
    if (tid == 0) {
        if (state) atomicOr(a.net.status, state);
        a.header[CGBN_HDR_SOUND] = state ? 0 : 1;
        a.header[CGBN_HDR_BAD_CELL] = 0;
    }
    if (!state && tid < n) a.header[tid] = s_order[tid];
}

// grid (ceil(min(cells, DVS_CG_MAX_CONFIGS) / 256), n): the configurations of variable blockIdx.y
__global__ __launch_bounds__(256) void k_cgbn_cells(CgbnRowArgs a) {
    if (!a.header[CGBN_HDR_SOUND]) return;                   // uniform: the offsets are not to be trusted
    const int n = a.net.n, v = blockIdx.y;
    if (a.net.card[v] != 0) return;
    const long long lo = a.net.offset[v], q = a.net.offset[v + 1] - lo, z = (long long)blockIdx.x * 256 + threadIdx.x;
    if (z >= q) return;
    const size_t cell = (size_t)(lo + z);
    const double sd = a.net.sd[cell];
    if (sd != sd) {                                          // an empty configuration: nothing else of it is read
        if (a.c != nullptr) a.c[cell] = bn_nan();
        return;
    }
    bool bad = !gpar_finite(a.net.intercept[cell]) || !gpar_finite(sd) || !(sd > 0.0);
    for (uint64_t m = a.net.parents[v] & ~(1ull << v); m; m &= m - 1ull) {
        const int u = dvs_ctz64(m);
        if (a.net.card[u] == 0 && !gpar_finite(a.net.coef[cell * n + u])) bad = true;
    }
    if (bad) {
        atomicOr(a.net.status, 64);
        atomicOr(&a.header[CGBN_HDR_BAD_CELL], 1);
    }
    if (a.c != nullptr) a.c[cell] = fit_log_norm(sd);
}

static void cgbn_launch_prep(const CgbnRowArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_cgbn_prep, dim3(1), dim3(64), 0, st, a);
    const long long widest = a.net.cells < DVS_CG_MAX_CONFIGS ? a.net.cells : DVS_CG_MAX_CONFIGS;
    DVS_LAUNCH(k_cgbn_cells, dim3((unsigned)((widest + 255) / 256), (unsigned)a.net.n), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// The network's arcs as compact lists in LDS
// ---------------------------------------------------------------------------------------------------------
// Stages a sound network (at most GPAR_MAX_ARCS arcs, every q within DVS_CG_MAX_CONFIGS).  Every thread calls it; a barrier follows.
__device__ __forceinline__ void cgbn_stage(const CgbnNet& net, CgbnLists* s) {
    const int n = net.n, tid = threadIdx.x;
    if (tid < n) {
        const int c = net.card[tid];
        s->card[tid] = (unsigned char)c;
        s->par[tid] = c == 0 ? net.parents[tid] & ~(1ull << tid) : 0ull;
        s->cell0[tid] = (int)net.offset[tid];
    }
    __syncthreads();
    if (tid <= n) {
        int at = 0, col = 0;
        for (int u = 0; u < tid; ++u) {
            at += __popcll(s->par[u]);
            col += s->card[u] == 0;
        }
        s->off[tid] = at;
        if (tid < n) s->col[tid] = (unsigned char)col;
    }
    __syncthreads();
    if (tid < n) {
        int e = s->off[tid], mul = 1, nd = 0;
        for (uint64_t m = s->par[tid]; m; m &= m - 1ull) {
            const int u = dvs_ctz64(m), cu = s->card[u];
            if (cu == 0) continue;
            s->idx[e] = (unsigned char)u;
            s->aux[e] = (unsigned short)mul;
            mul *= cu;
            ++e;
            ++nd;
        }
        for (uint64_t m = s->par[tid]; m; m &= m - 1ull) {
            const int u = dvs_ctz64(m);
            if (s->card[u] != 0) continue;
            s->idx[e] = (unsigned char)u;
            s->aux[e] = s->col[u];
            ++e;
        }
        s->nd[tid] = nd;
    }
    __syncthreads();
}

// the cell of the continuous v in the row r; -1: a discrete parent's level is at or above its card.  The level of parent
// `set` (-1: none) is `level` and its nibble is not read.
__device__ __forceinline__ int cgbn_cell(const CgbnLists* s, const BnRow r, int v, int set, int level) {
    int z = 0;
    bool bad = false;
    const int e0 = s->off[v], e1 = e0 + s->nd[v];
    for (int e = e0; e < e1; ++e) {
        const int u = s->idx[e];
        const int l = u == set ? level : bn_level(r, u);
        if (l >= (int)s->card[u]) bad = true;
        z += l * (int)s->aux[e];
    }
    return bad ? -1 : s->cell0[v] + z;
}

// mu_{v,z} at the image's row `lane`, the term of variable `skip` (-1: none) left out
__device__ __forceinline__ double cgbn_mu(const CgbnLists* s, const CgbnNet& net, const double* x, int lane, int v, int cell, int skip) {
#pragma clang fp contract(off)
    double mu = net.intercept[cell];
    const double* cf = net.coef + (size_t)cell * net.n;
    for (int e = s->off[v] + s->nd[v]; e < s->off[v + 1]; ++e) {
        const int u = s->idx[e];
        if (u == skip) continue;
        const double prod = cf[u] * x[(int)s->aux[e] * GPAR_LD + lane];
        mu = mu + prod;
    }
    return mu;
}

// ---------------------------------------------------------------------------------------------------------
// Forward sampling of the real columns
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GPAR_ROWS) void k_cgbn_sample(CgbnRowArgs a) {
#pragma clang fp contract(off)
    DVS_DYN_LDS(smem);
    __shared__ CgbnLists s_net;
    __shared__ int s_order[DVS_WTOK];
    double* x = (double*)smem;
    const int tid = threadIdx.x, n = a.net.n;
    if (!cgbn_sound(a.header)) return;                       // uniform: the preparation refused the network
    if (tid < n) s_order[tid] = a.header[tid];
    cgbn_stage(a.net, &s_net);
    const long long row0 = (long long)blockIdx.x * GPAR_ROWS;
    int flags = 0;
    const int len = fit_chunk_len(a.rows, blockIdx.x);
    if (tid < len) {
        const BnRow r = bn_row_load(a.packed + (size_t)(row0 + tid) * a.words, a.words);
        const uint32_t g = a.row_offset + (uint32_t)(row0 + tid);
        const uint32_t key = dvs_site_key(a.seed_lo, a.seed_hi, DVS_SITE_GBN_SAMPLE, g);
        for (int i = 0; i < n; ++i) {
            const int v = s_order[i];
            if (s_net.card[v] != 0) continue;                // uniform
            const int cell = cgbn_cell(&s_net, r, v, -1, 0);
            double value = bn_nan();
            if (cell < 0) flags |= 16;
            else {
                const double sd = a.net.sd[cell];
                if (sd != sd) flags |= 128;
                else {
                    const double mu = cgbn_mu(&s_net, a.net, x, tid, v, cell, -1);
                    const double noise = sd * fit_noise(key, v);
                    value = mu + noise;
                }
            }
            x[(int)s_net.col[v] * GPAR_LD + tid] = value;
        }
    }
    if (flags) atomicOr(a.net.status, flags);
    fit_image_store(a.per_row, len, a.net.nc, blockIdx.x, x);
}

void dvs_launch_cgbn_sample(const CgbnRowArgs& in, uint64_t seed, dvs_stream_t st) {
    CgbnRowArgs a = in;
    dvs_seed_split(a, seed);
    a.words = bic_words(a.net.n);
    a.target = -1;
    a.c = nullptr;
    cgbn_launch_prep(a, st);
    DVS_SET_LDS(k_cgbn_sample, gpar_image_lds(DVS_WTOK));
    DVS_LAUNCH(k_cgbn_sample, dim3((unsigned)((a.rows + GPAR_ROWS - 1) / GPAR_ROWS)), dim3(GPAR_ROWS), gpar_image_lds(a.net.nc), st, a);
}

// ---------------------------------------------------------------------------------------------------------
// The continuous part of the held-out log-likelihood
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GPAR_ROWS) void k_cgbn_loglik_rows(CgbnRowArgs a) {
#pragma clang fp contract(off)
    DVS_DYN_LDS(smem);
    __shared__ CgbnLists s_net;
    double* x = (double*)smem;
    const int tid = threadIdx.x, n = a.net.n, chunk = blockIdx.x;
    const bool sound = cgbn_sound(a.header);                 // uniform
    const int len = fit_image_load(a.x, a.rows, a.net.nc, chunk, x);
    if (sound) cgbn_stage(a.net, &s_net);
    const long long row = (long long)chunk * GPAR_ROWS + tid;
    double term = 0.0;
    int flags = 0;
    if (tid < len) {
        if (!sound) term = bn_nan();
        else {
            const BnRow r = bn_row_load(a.packed + (size_t)row * a.words, a.words);
            for (int v = 0; v < n; ++v) {
                if (s_net.card[v] != 0) continue;            // uniform
                const int cell = cgbn_cell(&s_net, r, v, -1, 0);
                if (cell < 0) {
                    flags |= 16;
                    continue;
                }
                const double sd = a.net.sd[cell];
                if (sd != sd) {
                    flags |= 128;
                    continue;
                }
                const double xv = x[(int)s_net.col[v] * GPAR_LD + tid];
                term = fit_log_density(term, xv, cgbn_mu(&s_net, a.net, x, tid, v, cell, -1), sd, a.c[cell]);
            }
            if (flags) term = bn_nan();
        }
        if (a.per_row) a.per_row[row] = term;
    }
    if (flags) atomicOr(a.net.status, flags);
    fit_chunk_sum(term, &a.partials[chunk]);
}

void dvs_launch_cgbn_loglik(const CgbnRowArgs& in, dvs_stream_t st) {
    CgbnRowArgs a = in;
    a.words = bic_words(a.net.n);
    a.target = -1;
    cgbn_launch_prep(a, st);
    DVS_SET_LDS(k_cgbn_loglik_rows, gpar_image_lds(DVS_WTOK));
    DVS_LAUNCH(k_cgbn_loglik_rows, dim3((unsigned)a.chunks), dim3(GPAR_ROWS), gpar_image_lds(a.net.nc), st, a);
    fit_launch_loglik_sum(1, a.chunks, a.partials, a.out, st);                       // the one row of chunk sums
}

// ---------------------------------------------------------------------------------------------------------
// Prediction
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GPAR_ROWS) void k_cgbn_predict(CgbnRowArgs a) {
#pragma clang fp contract(off)
    DVS_DYN_LDS(smem);
    __shared__ CgbnLists s_net;
    __shared__ double s_a[16 * GPAR_ROWS];                   // mode 2: a_k of row r at s_a[k * 256 + r]
    double* x = (double*)smem;
    const int tid = threadIdx.x, n = a.net.n, t = a.target, chunk = blockIdx.x;
    const bool sound = cgbn_sound(a.header);                 // uniform
    const int len = fit_image_load(a.x, a.rows, a.net.nc, chunk, x);
    if (sound) cgbn_stage(a.net, &s_net);
    const long long row = (long long)chunk * GPAR_ROWS + tid;
    if (tid >= len) return;                                  // no barrier from here on
    int flags = 0;
    if (a.mode != DVS_CGBN_PREDICT_CLASS) {
        double pred = bn_nan(), var = bn_nan();
        if (sound) {
            const BnRow r = bn_row_load(a.packed + (size_t)row * a.words, a.words);
            const int cell = cgbn_cell(&s_net, r, t, -1, 0);
            const double sd = cell < 0 ? 0.0 : a.net.sd[cell];
            if (cell < 0) flags |= 16;
            else if (sd != sd) flags |= 128;
            else {
                const double s = sd * sd;
                pred = cgbn_mu(&s_net, a.net, x, tid, t, cell, -1);
                var = s;
                if (a.mode == DVS_CGBN_PREDICT_EXACT) {
                    fit_blanket(n, s, pred, var, [&](int c, double& beta, double& sdc, double& res) {
                        if (c == t || !((s_net.par[c] >> t) & 1ull)) return false;   // uniform: c is no child of t
                        const int cc = cgbn_cell(&s_net, r, c, -1, 0);
                        if (cc < 0) {
                            flags |= 16;
                            return false;
                        }
                        sdc = a.net.sd[cc];
                        if (sdc != sdc) {
                            flags |= 128;
                            return false;
                        }
                        beta = a.net.coef[(size_t)cc * n + t];
                        res = x[(int)s_net.col[c] * GPAR_LD + tid] - cgbn_mu(&s_net, a.net, x, tid, c, cc, t);
                        return true;
                    });
                    if (flags) pred = var = bn_nan();
                }
            }
        }
        a.per_row[row] = pred;
        a.out[row] = var;
    } else {
        // a refused network: the row of posterior is as wide as card[target] says, 16 at the most
        const int levels = sound ? (int)s_net.card[t] : a.net.card[t] < 16 ? (int)a.net.card[t] : 16;
        int label = 255;
        if (!sound && a.posterior != nullptr)
            for (int k = 0; k < levels; ++k) a.posterior[(size_t)row * levels + k] = bn_nan();
        if (sound) {
            const BnRow r = bn_row_load(a.packed + (size_t)row * a.words, a.words);
            for (int k = 0; k < levels; ++k) s_a[k * GPAR_ROWS + tid] = a.prior != nullptr ? log(a.prior[(size_t)row * levels + k]) : 0.0;
            for (int c = 0; c < n; ++c) {
                if (!((s_net.par[c] >> t) & 1ull)) continue; // uniform: c is no continuous child of t
                const double xc = x[(int)s_net.col[c] * GPAR_LD + tid];
                for (int k = 0; k < levels; ++k) {
                    const int cc = cgbn_cell(&s_net, r, c, t, k);
                    double ak = bn_nan();
                    if (cc < 0) flags |= 16;
                    else {
                        const double sdc = a.net.sd[cc];
                        if (sdc != sdc) flags |= 128;
                        else ak = fit_log_density(s_a[k * GPAR_ROWS + tid], xc, cgbn_mu(&s_net, a.net, x, tid, c, cc, -1), sdc, a.c[cc]);
                    }
                    s_a[k * GPAR_ROWS + tid] = ak;
                }
            }
            double M = s_a[tid];
            bool any_nan = M != M;
            label = 0;
            for (int k = 1; k < levels; ++k) {
                const double ak = s_a[k * GPAR_ROWS + tid];
                if (ak != ak) any_nan = true;
                else if (ak > M) {
                    M = ak;
                    label = k;
                }
            }
            if (any_nan) label = 255;
            else {
                double W = 0.0;
                for (int k = 0; k < levels; ++k) {
                    const double w = exp(s_a[k * GPAR_ROWS + tid] - M);
                    s_a[k * GPAR_ROWS + tid] = w;
                    W = W + w;
                }
                if (a.posterior != nullptr)
                    for (int k = 0; k < levels; ++k) a.posterior[(size_t)row * levels + k] = s_a[k * GPAR_ROWS + tid] / W;
            }
            if (any_nan && a.posterior != nullptr)
                for (int k = 0; k < levels; ++k) a.posterior[(size_t)row * levels + k] = bn_nan();
        }
        a.label[row] = (uint8_t)label;
    }
    if (flags) atomicOr(a.net.status, flags);
}

void dvs_launch_cgbn_predict(const CgbnRowArgs& in, dvs_stream_t st) {
    CgbnRowArgs a = in;
    a.words = bic_words(a.net.n);
    cgbn_launch_prep(a, st);
    DVS_SET_LDS(k_cgbn_predict, gpar_image_lds(DVS_WTOK));
    DVS_LAUNCH(k_cgbn_predict, dim3((unsigned)a.chunks), dim3(GPAR_ROWS), gpar_image_lds(a.net.nc), st, a);
}
