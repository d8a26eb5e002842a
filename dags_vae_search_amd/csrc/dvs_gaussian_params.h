// A fitted Gaussian network on the device: its joint distribution, forward sampling, the log-likelihood of
// held-out rows and prediction.  Included by k_bic.hip after dvs_gaussian_ci.h.  Semantics, operation orders and refusals:
// include/dvs_gaussian_params.h.  Plain fp64 vector arithmetic: no f64 MFMA, no fused multiply-add (contraction is off in every
// function that rounds), no floating-point atomics.  The order, the image of 256 rows and its load, the quantile, the density
// term, the blanket update and the two levels of the sum are dvs_fitted.h's, shared with the other fitted networks; k_gbn_sample
// spells out the noise draw and the write-out that k_cgbn_sample takes from there (the reason is at the kernel).
//
//   k_gbn_joint          one wave per network: lane 0 orders the variables, then for v in that order the lanes take the
//                        variables u placed before v, one cov[v][u] each; the matrix lives in LDS (18 KB at n = 48).
//   k_gbn_quantiles      one thread per value: gpar_quantile, the function the sampler calls.
//   k_gbn_sample_prep    one wave: the three rules and the order, into the workspace header.
//   k_gbn_sample         one thread per row, 256 rows per workgroup.  A row's values are indexed by parent id at run time, so
//                        they live in LDS, lane-interleaved as gbn_L lays a lane's factor out: value v of row r at
//                        s_x[v * GPAR_LD + r], consecutive rows in consecutive banks.  The finished image is written out
//                        contiguously (element e of the chunk by thread e mod 256).
//   k_gbn_params_prep    one wave per network: the three rules -> ok[b]; c[b][v] = log(sd) + log(sqrt(2 pi)).
//   k_gbn_loglik_rows    one workgroup per (chunk of 256 rows, part of the batch): the chunk is staged once through the same
//   k_gbn_predict        image (coalesced reads, the transposing LDS writes conflict-free by GPAR_LD = 257) and the structures
//                        of the part are looped over inside the workgroup, so a row is read from memory once per part, not
//                        once per structure.  k_gbn_loglik_rows ends in dvs_bn_loglik's tree (fit_chunk_sum), and the
//                        launcher's second level is dvs_bn_loglik's too (k_bn_loglik_sum).
// Every network's parents are kept once per workgroup as a compact (index, coefficient) list in LDS (gpar_stage_net): a DAG
// on 48 variables has at most 1128 arcs, and only networks the rules passed are staged.
#pragma once
#include "dvs_fitted.h"

constexpr int GPAR_MAX_ARCS = DVS_WTOK * (DVS_WTOK - 1) / 2;
static_assert((size_t)GPAR_LD * DVS_WTOK * sizeof(double) + 20 * 1024 <= 160 * 1024, "the image and the lists fit a compute unit's LDS");

__device__ __forceinline__ bool gpar_finite(double x) { return x - x == 0.0; }

// The three rules of include/dvs_gaussian_params.h and the topological order of one network.  Every thread of the workgroup
// calls it (it holds barriers); returns the status bits, 0 for a sound network, whose order is then in s_order[0 .. n).
__device__ __forceinline__ int gpar_check(int n, const uint64_t* parents, const double* coef, const double* intercept, const double* sd,
                                          int* s_state, int* s_order) {
    __shared__ uint64_t s_par[DVS_WTOK];
    const int tid = threadIdx.x;
    if (tid == 0) *s_state = 0;
    if (tid < n) s_par[tid] = parents[tid];
    __syncthreads();
    int bad = 0;
    for (int cell = tid; cell < n * n; cell += blockDim.x) {
        const int v = cell / n, u = cell - v * n;
        const uint64_t pm = parents[v] & ~(1ull << v);
        if (u == 0) {
            if ((pm >> n) != 0ull) bad |= 16;
            if (!gpar_finite(intercept[v]) || !gpar_finite(sd[v]) || !(sd[v] > 0.0)) bad |= 64;
        }
        if (((pm >> u) & 1ull) && !gpar_finite(coef[cell])) bad |= 64;
    }
    if (bad) atomicOr(s_state, bad);
    __syncthreads();
    if (tid == 0) {
        const uint64_t low = n == 64 ? ~0ull : (1ull << n) - 1ull;
        if (!fit_order(n, [&](int v) { return s_par[v] & low & ~(1ull << v); }, s_order)) *s_state |= 1;
    }
    __syncthreads();
    return *s_state;
}

// ---------------------------------------------------------------------------------------------------------
// The joint distribution
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_gbn_joint(GbnJointArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_cov[DVS_WTOK * DVS_WTOK], s_mean[DVS_WTOK];
    __shared__ int s_order[DVS_WTOK], s_state;
    const int n = a.net.n, b = blockIdx.x, tid = threadIdx.x;
    const uint64_t* parents = a.net.parents + (size_t)b * n;
    const double* coef = a.net.coef + (size_t)b * n * n;
    const double* intercept = a.net.intercept + (size_t)b * n;
    const double* sd = a.net.sd + (size_t)b * n;
    double* mean = a.mean + (size_t)b * n;
    double* cov = a.cov + (size_t)b * n * n;
    const int state = gpar_check(n, parents, coef, intercept, sd, &s_state, s_order);
    if (state) {
        if (tid == 0) atomicOr(a.net.status, state);
        for (int e = tid; e < n * n; e += 64) cov[e] = bn_nan();
        for (int e = tid; e < n; e += 64) mean[e] = bn_nan();
        return;
    }
    for (int i = 0; i < n; ++i) {
        const int v = s_order[i];
        const uint64_t pm = parents[v] & ~(1ull << v);
        const double* cv = coef + (size_t)v * n;
        for (int j = tid; j < i; j += 64) {
            const int u = s_order[j];
            double s = 0.0;
            for (uint64_t m = pm; m; m &= m - 1ull) {
                const int k = dvs_ctz64(m);
                const double prod = cv[k] * s_cov[k * n + u];
                s = s + prod;
            }
            s_cov[v * n + u] = s;
            s_cov[u * n + v] = s;
        }
        __syncthreads();
        if (tid == 0) {
            double s = sd[v] * sd[v], mu = intercept[v];
            for (uint64_t m = pm; m; m &= m - 1ull) {
                const int k = dvs_ctz64(m);
                const double prod = cv[k] * s_cov[v * n + k];
                s = s + prod;
                const double pmu = cv[k] * s_mean[k];
                mu = mu + pmu;
            }
            s_cov[v * n + v] = s;
            s_mean[v] = mu;
        }
        __syncthreads();
    }
    for (int e = tid; e < n * n; e += 64) cov[e] = s_cov[e];
    for (int e = tid; e < n; e += 64) mean[e] = s_mean[e];
}

void dvs_launch_gbn_joint(const GbnJointArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_gbn_joint, dim3((unsigned)a.net.B), dim3(64), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// The quantile function (gpar_quantile, dvs_fitted.h) on its own
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gbn_quantiles(GbnQuantileArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < a.count) a.z[i] = gpar_quantile(a.k[i]);
}

void dvs_launch_gbn_quantiles(const GbnQuantileArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_gbn_quantiles, dim3((unsigned)((a.count + 255) / 256)), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// One network's parents as a compact list in LDS
// ---------------------------------------------------------------------------------------------------------
struct GparNet {
    int off[DVS_WTOK + 1];                                   // the entries of v: off[v] .. off[v + 1]
    unsigned char idx[GPAR_MAX_ARCS];
    double coef[GPAR_MAX_ARCS], intercept[DVS_WTOK], sd[DVS_WTOK];
    uint64_t par[DVS_WTOK];                                  // Pa(v) as a mask, the self bit off
};

// Stages network b (sound: the rules passed, so it has at most GPAR_MAX_ARCS arcs): the masks first, the offsets from them by
// popcounts in LDS, then the n^2 cells.  Every thread calls it; a barrier follows.
__device__ __forceinline__ void gpar_stage_net(const GbnNet& net, int b, GparNet* s) {
    const int n = net.n, tid = threadIdx.x;
    const uint64_t* parents = net.parents + (size_t)b * n;
    const double* coef = net.coef + (size_t)b * n * n;
    if (tid < n) {
        s->par[tid] = parents[tid] & ~(1ull << tid);
        s->intercept[tid] = net.intercept[(size_t)b * n + tid];
        s->sd[tid] = net.sd[(size_t)b * n + tid];
    }
    __syncthreads();
    if (tid <= n) {
        int at = 0;
        for (int u = 0; u < tid; ++u) at += __popcll(s->par[u]);
        s->off[tid] = at;
    }
    __syncthreads();
    for (int cell = tid; cell < n * n; cell += blockDim.x) {
        const int v = cell / n, u = cell - v * n;
        const uint64_t pm = s->par[v];
        if ((pm >> u) & 1ull) {
            const int at = s->off[v] + __popcll(pm & ((1ull << u) - 1ull));
            s->idx[at] = (unsigned char)u;
            s->coef[at] = coef[cell];
        }
    }
    __syncthreads();
}

// mu_v at the image's row `lane`, the term of variable `skip` (-1: none) left out
__device__ __forceinline__ double gpar_mu(const GparNet* s, const double* x, int lane, int v, int skip) {
#pragma clang fp contract(off)
    double mu = s->intercept[v];
    for (int e = s->off[v]; e < s->off[v + 1]; ++e) {
        const int u = s->idx[e];
        if (u == skip) continue;
        const double prod = s->coef[e] * x[u * GPAR_LD + lane];
        mu = mu + prod;
    }
    return mu;
}

// ---------------------------------------------------------------------------------------------------------
// Forward sampling
// ---------------------------------------------------------------------------------------------------------
constexpr int GPAR_HDR_DRAWABLE = 48;                        // header word after order [48], as dvs_bn_sample's

__global__ __launch_bounds__(64) void k_gbn_sample_prep(GbnSampleArgs a) {
    __shared__ int s_order[DVS_WTOK], s_state;
    const int state = gpar_check(a.net.n, a.net.parents, a.net.coef, a.net.intercept, a.net.sd, &s_state, s_order);
    if (threadIdx.x == 0) {
        if (state) atomicOr(a.net.status, state);
        a.header[GPAR_HDR_DRAWABLE] = state ? 0 : 1;
    }
    if (!state && (int)threadIdx.x < a.net.n) a.header[threadIdx.x] = s_order[threadIdx.x];
}

__global__ __launch_bounds__(GPAR_ROWS) void k_gbn_sample(GbnSampleArgs a) {
#pragma clang fp contract(off)
    DVS_DYN_LDS(smem);
    __shared__ GparNet s_net;
    __shared__ int s_order[DVS_WTOK];
    double* x = (double*)smem;
    const int tid = threadIdx.x, n = a.net.n;
    if (!a.header[GPAR_HDR_DRAWABLE]) return;                // uniform: the prep refused the network
    if (tid < n) s_order[tid] = a.header[tid];
    gpar_stage_net(a.net, 0, &s_net);
    // The draw, the row count and the write-out are spelled out here as fit_noise, fit_chunk_len and fit_image_store spell them
    // (k_cgbn_sample calls those): through the helpers the compiler allocates this kernel's registers another way and
    // gaussian_sample at n = 37 measured 2.5 % slower, with this text it is the instruction stream it was.
    const long long row0 = (long long)blockIdx.x * GPAR_ROWS;
    const int len = a.rows - row0 < GPAR_ROWS ? (int)(a.rows - row0) : GPAR_ROWS;
    if (tid < len) {
        const uint32_t g = a.row_offset + (uint32_t)(row0 + tid);
        const uint32_t key = dvs_site_key(a.seed_lo, a.seed_hi, DVS_SITE_GBN_SAMPLE, g);
        for (int i = 0; i < n; ++i) {
            const int v = s_order[i];
            const double mu = gpar_mu(&s_net, x, tid, v, -1);
            const uint32_t h1 = dvs_draw(key, 2u * (uint32_t)v), h2 = dvs_draw(key, 2u * (uint32_t)v + 1u);
            const uint64_t k = ((uint64_t)(h1 >> 6) << 26) + (uint64_t)(h2 >> 6);
            const double noise = s_net.sd[v] * gpar_quantile(k);
            x[v * GPAR_LD + tid] = mu + noise;
        }
    }
    __syncthreads();
    double* out = a.out + (size_t)row0 * n;
    for (int e = tid; e < len * n; e += GPAR_ROWS) {
        const int r = e / n, c = e - r * n;
        out[e] = x[c * GPAR_LD + r];
    }
}

void dvs_launch_gbn_sample(const GbnSampleArgs& in, uint64_t seed, dvs_stream_t st) {
    GbnSampleArgs a = in;
    dvs_seed_split(a, seed);
    DVS_LAUNCH(k_gbn_sample_prep, dim3(1), dim3(64), 0, st, a);
    const size_t lds = gpar_image_lds(a.net.n);
    DVS_SET_LDS(k_gbn_sample, gpar_image_lds(DVS_WTOK));
    DVS_LAUNCH(k_gbn_sample, dim3((unsigned)((a.rows + GPAR_ROWS - 1) / GPAR_ROWS)), dim3(GPAR_ROWS), lds, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// Held-out log-likelihood and prediction
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_gbn_params_prep(GbnRowArgs a) {
#pragma clang fp contract(off)
    __shared__ int s_order[DVS_WTOK], s_state;
    const int n = a.net.n, b = blockIdx.x, tid = threadIdx.x;
    const double* sd = a.net.sd + (size_t)b * n;
    const int state = gpar_check(n, a.net.parents + (size_t)b * n, a.net.coef + (size_t)b * n * n, a.net.intercept + (size_t)b * n, sd,
                                 &s_state, s_order);
    if (tid == 0) {
        if (state) atomicOr(a.net.status, 16);
        a.ok[b] = state ? 0 : 1;
    }
    if (a.c != nullptr && !state && tid < n) a.c[(size_t)b * n + tid] = fit_log_norm(sd[tid]);
}

__global__ __launch_bounds__(GPAR_ROWS) void k_gbn_loglik_rows(GbnRowArgs a) {
#pragma clang fp contract(off)
    DVS_DYN_LDS(smem);
    __shared__ GparNet s_net;
    __shared__ double s_c[DVS_WTOK];
    double* x = (double*)smem;
    const int tid = threadIdx.x, n = a.net.n;
    const int chunk = blockIdx.x / a.bsplit, part = blockIdx.x - chunk * a.bsplit;
    const int len = fit_image_load(a.data, a.rows, n, chunk, x);
    const long long row = (long long)chunk * GPAR_ROWS + tid;
    for (int b = part; b < a.net.B; b += a.bsplit) {
        const bool ok = a.ok[b] != 0;                        // uniform
        __syncthreads();                                     // the lists and the tree of the structure before
        if (ok) {
            if (tid < n) s_c[tid] = a.c[(size_t)b * n + tid];
            gpar_stage_net(a.net, b, &s_net);
        }
        double term = 0.0;
        if (tid < len) {
            if (!ok) term = bn_nan();
            else
                for (int v = 0; v < n; ++v)
                    term = fit_log_density(term, x[v * GPAR_LD + tid], gpar_mu(&s_net, x, tid, v, -1), s_net.sd[v], s_c[v]);
            if (a.per_row) a.per_row[(size_t)b * a.rows + row] = term;
        }
        fit_chunk_sum(term, &a.partials[(size_t)b * a.chunks + chunk]);
    }
}

// the parts the batch is cut into: enough workgroups for the device when the rows alone give few chunks
static int gpar_bsplit(const GbnRowArgs& a) {
    const int want = (1024 + a.chunks - 1) / a.chunks;
    return want < a.net.B ? want : a.net.B;
}

void dvs_launch_gbn_loglik(const GbnRowArgs& in, dvs_stream_t st) {
    GbnRowArgs a = in;
    a.bsplit = gpar_bsplit(a);
    DVS_LAUNCH(k_gbn_params_prep, dim3((unsigned)a.net.B), dim3(64), 0, st, a);
    DVS_SET_LDS(k_gbn_loglik_rows, gpar_image_lds(DVS_WTOK));
    DVS_LAUNCH(k_gbn_loglik_rows, dim3((unsigned)a.chunks * a.bsplit), dim3(GPAR_ROWS), gpar_image_lds(a.net.n), st, a);
    fit_launch_loglik_sum(a.net.B, a.chunks, a.partials, a.out, st);
}

__global__ __launch_bounds__(GPAR_ROWS) void k_gbn_predict(GbnRowArgs a) {
#pragma clang fp contract(off)
    DVS_DYN_LDS(smem);
    __shared__ GparNet s_net;
    __shared__ int s_child[DVS_WTOK];                        // the entry of t in c's list, -1: c is no child of t
    double* x = (double*)smem;
    const int tid = threadIdx.x, n = a.net.n, t = a.target;
    const int chunk = blockIdx.x / a.bsplit, part = blockIdx.x - chunk * a.bsplit;
    const int len = fit_image_load(a.data, a.rows, n, chunk, x);
    const long long row = (long long)chunk * GPAR_ROWS + tid;
    for (int b = part; b < a.net.B; b += a.bsplit) {
        const bool ok = a.ok[b] != 0;                        // uniform
        __syncthreads();                                     // the lists of the structure before
        double pred = bn_nan(), var = bn_nan();
        if (ok) {
            gpar_stage_net(a.net, b, &s_net);
            if (a.mode == DVS_GBN_PREDICT_EXACT) {
                if (tid < n) {
                    int at = -1;
                    for (int e = s_net.off[tid]; e < s_net.off[tid + 1]; ++e)
                        if (s_net.idx[e] == t) at = e;
                    s_child[tid] = at;
                }
                __syncthreads();
            }
            const double s = s_net.sd[t] * s_net.sd[t];
            pred = gpar_mu(&s_net, x, tid, t, -1);
            var = s;
            if (a.mode == DVS_GBN_PREDICT_EXACT)
                fit_blanket(n, s, pred, var, [&](int c, double& beta, double& sdc, double& res) {
                    const int at = s_child[c];
                    if (at < 0) return false;                // uniform: c is no child of t
                    beta = s_net.coef[at];
                    sdc = s_net.sd[c];
                    res = x[c * GPAR_LD + tid] - gpar_mu(&s_net, x, tid, c, t);
                    return true;
                });
        }
        if (tid < len) a.per_row[(size_t)b * a.rows + row] = pred;
        if (chunk == 0 && tid == 0) a.out[b] = var;
    }
}

void dvs_launch_gbn_predict(const GbnRowArgs& in, dvs_stream_t st) {
    GbnRowArgs a = in;
    a.bsplit = gpar_bsplit(a);
    DVS_LAUNCH(k_gbn_params_prep, dim3((unsigned)a.net.B), dim3(64), 0, st, a);
    DVS_SET_LDS(k_gbn_predict, gpar_image_lds(DVS_WTOK));
    DVS_LAUNCH(k_gbn_predict, dim3((unsigned)a.chunks * a.bsplit), dim3(GPAR_ROWS), gpar_image_lds(a.net.n), st, a);
}
