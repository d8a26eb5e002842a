// Native BIC scorer for discrete Bayesian networks: replaces the per-graph `Rscript bnlearn` subprocess
// of BNLearnWrapper.score (src/problem/bn/bnlearn.py:27-61, bnlearn_scripts/bnlearn_score.R:25-39) by a batched
// contingency-count kernel.  bnlearn's discrete BIC is decomposable:
//   BIC(G) = sum_v [ sum_{j,k} N_vjk log(N_vjk / N_vj) - (log S / 2)(r_v - 1) q_v ]
// One workgroup per (DAG, variable): the S samples (4-bit level codes, 16 variables per 64-bit word, sample-major:
// one coalesced 8-byte load per lane and word; the whole asia / sachs data set is 40 KB and lives in L2) are binned
// into an LDS histogram over (parent configuration, state) with integer atomics (or, for parent sets whose table does
// not fit LDS, sorted as 64-bit keys), then the log-likelihood terms are summed in fp64 in a fixed order (integer
// counts are exact, so the score does not depend on the atomics' order).
// Integer/byte work bound by LDS atomics and L2 reads — no MFMA.
//
// The same counts give bnlearn's other decomposable discrete scores (dvs_bn_scores; definitions in include/dvs.h).  The
// kernel is a template over the score FAMILY, which selects the per-cell term and what is added to the sum:
//   family 0, penalised log-likelihood (loglik, aic, bic):  sum_{j,k} N_jk log(N_jk / N_j) - k (r - 1) q
//   family 1, Bayesian Dirichlet (bde, bds, k2, bdj):
//       sum_j [ lgamma(a_j) - lgamma(a_j + N_j) + sum_k ( lgamma(a_jk + N_jk) - lgamma(a_jk) ) ],  a_j = r a_jk
// Only occupied cells (N_jk > 0) and observed configurations (N_j > 0) are visited — every other cell contributes exactly
// zero to each of these scores — so the sort path serves both families.  bds needs the number of observed configurations
// before the sum: one more pass over the table rows (dense) or over the sorted keys (sort), an integer count.  lgamma is
// the device math library's, in fp64; its two arguments that do not depend on the cell, lgamma(a_j) and lgamma(a_jk), are
// taken once per workgroup.  Family 1 is VALU-bound by lgamma (two per occupied cell and row) — no MFMA there either.
#include "dvs_bn_common.h"

constexpr int BIC_MAX_SORT = 16384;          // samples the sort path can hold in LDS (64-bit keys)

__device__ __forceinline__ int bic_bits(int card) {   // bits needed for a level code 0 .. card-1
    int b = 0;
    while ((1 << b) < card) ++b;
    return b;
}
// first index in sorted keys[0..n) with keys[i] >= x
__device__ __forceinline__ int bic_lower_bound(const uint64_t* keys, int n, uint64_t x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Family 1's prior, once per workgroup after the counting pass (all threads call it: it holds two barriers).
//   bde: a_j = iss / q    bds: a_j = iss / (observed configurations)    k2: a_jk = 1    bdj: a_jk = 1/2;    a_j = r a_jk
__device__ __forceinline__ void bn_prior(const BicArgs& a, int r, double q, const int* qobs, double* aj, double* ajk,
                                         double* lg_aj, double* lg_ajk) {
    __syncthreads();
    if (threadIdx.x == 0) {
        double x, y;
        if (a.type == DVS_SCORE_K2 || a.type == DVS_SCORE_BDJ) {
            y = a.type == DVS_SCORE_K2 ? 1.0 : 0.5;
            x = y * (double)r;
        } else {
            x = a.arg / (a.type == DVS_SCORE_BDS ? (double)*qobs : q);
            y = x / (double)r;
        }
        *aj = x;
        *ajk = y;
        *lg_aj = bn_lgamma(x);
        *lg_ajk = bn_lgamma(y);
    }
    __syncthreads();
}

// Two counting strategies, chosen per (DAG, variable):
//   histogram: q_v * r_v <= BIC_MAX_BINS cells fit LDS -> integer atomics into the dense table (the common case);
//   sort:      larger parent sets (sachs: >= 9 ternary parents) are sparse — at most S cells are occupied — so the
//              bit-packed 64-bit (configuration, state) keys of the S samples are bitonic-sorted in LDS and the counts
//              are run lengths found by binary search.
//
// bn_family_score is the whole of that for one (variable, parent set): the local score of variable v under the parent mask
// (*pmask ^ flip) with v's own bit masked off.  Every thread of the workgroup calls it (it holds barriers); thread 0 gets
// the score, NaN (and status bit 4) when the family is refused.  k_bic_local calls it with flip = 0 for the mask as it
// stands, k_bn_toggle (dvs_hillclimb.h) with one bit flipped: one function, so the two kernels give equal bytes for equal
// parent sets.  It walks the mask itself instead of calling bn_family_layout: the same walk lays out the sort keys and
// keeps q (as a double) past the dense limit, where the shared routine stops.
//
// ROWS (the *_rows kernels of dvs_strength.h): sample s of the workgroup's data set is row rows[s] of a.data and a.S is the
// set's size; nothing else changes, and the counts do not depend on the order of the rows, so the score is, bit for bit,
// that of the gathered data set.  The instantiations without ROWS never read `rows`.
template <int FAMILY, bool ROWS = false>
__device__ __forceinline__ double bn_family_score(const BicArgs& a, const int v, const uint64_t* pmask, const uint64_t flip,
                                                  char* smem, const int* rows = nullptr) {
    __shared__ double red[256];
    __shared__ int par_id[48], par_stride[48], par_shift[48];
    __shared__ int s_np, s_mode, s_rbits;
    __shared__ double s_q;
    __shared__ int s_qobs;                                   // family 1, bds: parent configurations observed in the data
    __shared__ double s_aj, s_ajk, s_lg_aj, s_lg_ajk;        // family 1: the prior's a_j, a_jk and their lgamma
    const int r = a.card[v];
    if (threadIdx.x == 0) {
        uint64_t pm = (*pmask ^ flip) & ~(1ull << v);
        double q = 1.0;
        long long qi = 1;
        int np = 0, bits = bic_bits(r), mode = 0;          // mode 0 histogram, 1 sort, -1 unsupported
        for (; pm; pm &= pm - 1) {
            const int p = __builtin_ctzll(pm);
            if (p >= a.n) { mode = -1; break; }
            par_id[np] = p;
            par_stride[np] = (int)qi;                      // histogram: mixed radix, lowest variable id fastest
            par_shift[np] = bits;                          // sort: bit-packed above the state's bits
            bits += bic_bits(a.card[p]);
            q *= a.card[p];
            if (mode == 0) {
                qi *= a.card[p];
                if (qi * r > BIC_MAX_BINS) mode = 1;
            }
            ++np;
        }
        if (mode == 1 && (bits > 63 || a.S > BIC_MAX_SORT)) mode = -1;
        s_np = np;
        s_q = q;
        s_mode = mode;
        s_rbits = bic_bits(r);
        if (FAMILY == 1) s_qobs = 0;
    }
    __syncthreads();
    const int np = s_np, mode = s_mode;
    if (mode < 0) {
        if (threadIdx.x == 0) atomicOr(a.status, 16);
        return bn_nan();
    }
    double acc = 0.0;
    if (mode == 0) {
        unsigned* hist = (unsigned*)smem;
        const int q = (int)s_q, bins = q * r;
        bn_dense_count<ROWS, false>(hist, bins, a.data, a.words, a.S, rows, np, par_id, par_stride,
                                    [&](const uint64_t* row, int key) { return key * r + bic_level(row, v); });
        if constexpr (FAMILY == 0) {
            for (int j = threadIdx.x; j < q; j += blockDim.x) {
                unsigned nj = 0;
                for (int k = 0; k < r; ++k) nj += hist[j * r + k];
                if (nj == 0) continue;
                const double dn = (double)nj;
                for (int k = 0; k < r; ++k) {
                    const unsigned c = hist[j * r + k];
                    if (c) acc += (double)c * log((double)c / dn);
                }
            }
        } else {
            if (a.type == DVS_SCORE_BDS) {
                int seen = 0;
                for (int j = threadIdx.x; j < q; j += blockDim.x) {
                    unsigned nj = 0;
                    for (int k = 0; k < r; ++k) nj += hist[j * r + k];
                    seen += nj != 0;
                }
                if (seen) atomicAdd(&s_qobs, seen);
            }
            bn_prior(a, r, s_q, &s_qobs, &s_aj, &s_ajk, &s_lg_aj, &s_lg_ajk);
            const double aj = s_aj, ajk = s_ajk, lg_aj = s_lg_aj, lg_ajk = s_lg_ajk;
            for (int j = threadIdx.x; j < q; j += blockDim.x) {
                unsigned nj = 0;
                for (int k = 0; k < r; ++k) nj += hist[j * r + k];
                if (nj == 0) continue;
                acc += lg_aj - bn_lgamma(aj + (double)nj);
                for (int k = 0; k < r; ++k) {
                    const unsigned c = hist[j * r + k];
                    if (c) acc += bn_lgamma(ajk + (double)c) - lg_ajk;
                }
            }
        }
    } else {
        uint64_t* keys = (uint64_t*)smem;
        const int S = a.S, rbits = s_rbits;
        int spad = 1;
        while (spad < S) spad <<= 1;
        for (int s = threadIdx.x; s < spad; s += blockDim.x) {
            uint64_t key = ~0ull;
            if (s < S) {
                const uint64_t* row = a.data + (size_t)(ROWS ? rows[s] : s) * a.words;
                key = (uint64_t)bic_level(row, v);
                for (int i = 0; i < np; ++i) key |= (uint64_t)bic_level(row, par_id[i]) << par_shift[i];
            }
            keys[s] = key;
        }
        __syncthreads();
        for (int k = 2; k <= spad; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = threadIdx.x; i < spad; i += blockDim.x) {
                    const int p = i ^ j;
                    if (p > i) {
                        const uint64_t x = keys[i], y = keys[p];
                        if ((x > y) == ((i & k) == 0)) {
                            keys[i] = y;
                            keys[p] = x;
                        }
                    }
                }
                __syncthreads();
            }
        if constexpr (FAMILY == 0) {
            for (int i = threadIdx.x; i < S; i += blockDim.x) {
                const uint64_t key = keys[i];
                if (i > 0 && keys[i - 1] == key) continue;                 // not the first sample of its (j, k) cell
                const int c = bic_lower_bound(keys, S, key + 1) - i;
                const uint64_t j0 = (key >> rbits) << rbits;
                const int nj = bic_lower_bound(keys, S, j0 + (1ull << rbits)) - bic_lower_bound(keys, S, j0);
                acc += (double)c * log((double)c / (double)nj);
            }
        } else {
            if (a.type == DVS_SCORE_BDS) {
                int seen = 0;
                for (int i = threadIdx.x; i < S; i += blockDim.x)
                    seen += i == 0 || (keys[i - 1] >> rbits) != (keys[i] >> rbits);   // first sample of its configuration
                if (seen) atomicAdd(&s_qobs, seen);
            }
            bn_prior(a, r, s_q, &s_qobs, &s_aj, &s_ajk, &s_lg_aj, &s_lg_ajk);
            const double aj = s_aj, ajk = s_ajk, lg_aj = s_lg_aj, lg_ajk = s_lg_ajk;
            for (int i = threadIdx.x; i < S; i += blockDim.x) {
                const uint64_t key = keys[i];
                if (i > 0 && keys[i - 1] == key) continue;                 // not the first sample of its (j, k) cell
                const int c = bic_lower_bound(keys, S, key + 1) - i;
                acc += bn_lgamma(ajk + (double)c) - lg_ajk;
                if (i > 0 && (keys[i - 1] >> rbits) == (key >> rbits)) continue;   // not the first cell of its configuration
                const uint64_t j0 = (key >> rbits) << rbits;
                const int nj = bic_lower_bound(keys, S, j0 + (1ull << rbits)) - i;
                acc += lg_aj - bn_lgamma(aj + (double)nj);
            }
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    dvs_block_sum256((int)threadIdx.x, red);
    double score = 0.0;
    if (threadIdx.x == 0) {
        if constexpr (FAMILY == 0) {
            const double k = a.arg != a.arg ? 0.5 * log((double)a.S) : a.arg;
            score = red[0] - k * (double)(r - 1) * s_q;
        } else {
            score = red[0];
        }
    }
    return score;
}

// k_bic_local and k_bic_local_rows (dvs_strength.h): one workgroup per (DAG, variable); r is read with ROWS only
template <int FAMILY, bool ROWS>
__device__ __forceinline__ void bic_local_cell(const BicArgs& a, const RowSetArgs* r) {
    DVS_DYN_LDS(smem);
    const int v = blockIdx.x % a.n, dag = blockIdx.x / a.n;
    const size_t cell = (size_t)dag * a.n + v;
    const double score = bn_family_score<FAMILY, ROWS>(a, v, a.parents + cell, 0ull, smem, ROWS ? rs_rows(*r, dag) : nullptr);
    if (threadIdx.x == 0) a.local[cell] = score;
}
template <int FAMILY>
__global__ __launch_bounds__(256) void k_bic_local(BicArgs a) {
    bic_local_cell<FAMILY, false>(a, nullptr);
}

__global__ __launch_bounds__(256) void k_bic_sum(BicArgs a) {
    const int dag = blockIdx.x * blockDim.x + threadIdx.x;
    if (dag >= a.B) return;
    double s = 0.0;
    for (int v = 0; v < a.n; ++v) s += a.local[(size_t)dag * a.n + v];
    a.out[dag] = s;
}

#include "dvs_hillclimb.h"
#include "dvs_tabu.h"
#include "dvs_cpdag.h"
#include "dvs_citest.h"
#include "dvs_local.h"
#include "dvs_permtest.h"
#include "dvs_gaussian.h"
#include "dvs_gaussian_ci.h"
#include "dvs_gaussian_params.h"
#include "dvs_mixed.h"
#include "dvs_params.h"
#include "dvs_mixed_params.h"
#include "dvs_gaussian_incomplete.h"
#include "dvs_infer.h"
#include "dvs_eliminate.h"
#include "dvs_incomplete.h"
#include "dvs_exact.h"
#include "dvs_posterior.h"
#include "dvs_ordermc.h"
#include "dvs_strength.h"
#include "dvs_available.h"

void dvs_launch_bic(const BicArgs& in, dvs_stream_t st) {
    BicArgs a = in;
    a.words = bic_words(a.n);
    BN_LAUNCH_FAMILY(a.type, k_bic_local, "k_bic_local", "k_bn_local_dirichlet", dim3((unsigned)a.B * a.n), st, a);
    DVS_LAUNCH(k_bic_sum, dim3((a.B + 255) / 256), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// GP predictor, predictive mean: mean(x*) = c + sum_m o exp(-|x* - z_m|^2 / (2 l^2)) alpha_m for the
// reference's SGPR model (src/predictors/gp.py:13-32: ConstantMean + InducingPointKernel(ScaleKernel(RBF))), with alpha
// solved once at fit time.  One wave per query: its 32-dim latent in registers (lane = dimension pair), the M inducing
// points streamed from global/L2 ([M][32] fp32 = 64 KB), fp64 accumulation: SGPR weights alternate in sign and are
// orders of magnitude larger than the result.  B x M x 32 MACs — tiny; the kernel exists so that the encode -> predict
// -> decode loop of latent-space search never leaves the device.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gp_predict(GpArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + wave;
    if (q >= a.B) return;
    // lane m-stride: each lane owns inducing points lane, lane + 64, ...; the query is read once per lane (L1 broadcast)
    double acc = 0.0;
    for (int m = lane; m < a.M; m += 64) {
        const float* zm = a.z + (size_t)m * a.D;
        const float* xq = a.x + (size_t)q * a.D;
        float d2 = 0.f;
        for (int k = 0; k < a.D; ++k) {
            const float d = xq[k] - zm[k];
            d2 = fmaf(d, d, d2);
        }
        acc += a.alpha[m] * exp(-(double)d2 * a.inv2l2);
    }
    acc = dvs_wave_sum(acc, lane);
    if (lane == 0) a.out[q] = a.constant + a.outputscale * acc;
}

void dvs_launch_gp_predict(const GpArgs& in, double lengthscale, dvs_stream_t st) {
    GpArgs a = in;
    a.inv2l2 = dvs_gp_inv2l2(lengthscale);
    DVS_LAUNCH(k_gp_predict, dim3((a.B + 3) / 4), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// GP predictor, hyper-parameter training (reference loop src/predictors/gp.py:55-81 =
// experiments/01_bn_asia/main.py:315-393: Adam on -ExactMarginalLogLikelihood of the SGPR model).  The two kernel-specific
// pieces of one training iteration; the dense M x M / M x n factorisations in between are library calls of the host side
// (predictor.py), the parameter update is dvs_clip_adam.
//   k_gp_kernel      K[a][b] = o exp(-|xa_a - xb_b|^2 / (2 l^2)), float64 (K_uu needs all of it: its Cholesky factor is
//                    ill-conditioned at M = 500), float32 points.
//   k_gp_kernel_bwd  given G = dF/dK: row a's pull-backs  dxa_a = sum_b G'_ab K_ab (xb_b - xa_a) / l^2  (G' = G + G^T when
//                    xa and xb are the same point set, K_uu) and the per-row partial sums of dF/dl = sum G K d^2 / l^3 and
//                    dF/do = sum G K / o.  One wave per row a, lanes stride over b, fixed-order reduction: bitwise
//                    reproducible.  K is recomputed from the points (a 32-dim distance) instead of read.
// ---------------------------------------------------------------------------------------------------------
constexpr int DVS_GP_MAXD = 32;
__global__ __launch_bounds__(256) void k_gp_kernel(GpKernArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.na * a.nb) return;
    const int ra = (int)(i / a.nb), rb = (int)(i - (size_t)ra * a.nb);
    const float* pa = a.xa + (size_t)ra * a.D;
    const float* pb = a.xb + (size_t)rb * a.D;
    double d2 = 0.0;
    for (int k = 0; k < a.D; ++k) {
        const double d = (double)pa[k] - (double)pb[k];
        d2 = fma(d, d, d2);
    }
    a.K[i] = a.outputscale * exp(-d2 * a.inv2l2);
}
__global__ __launch_bounds__(256) void k_gp_kernel_bwd(GpKernArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ra = blockIdx.x * 4 + wave;
    if (ra >= a.na) return;
    const float* pa = a.xa + (size_t)ra * a.D;
    double xa[DVS_GP_MAXD], acc[DVS_GP_MAXD];
#pragma unroll
    for (int k = 0; k < DVS_GP_MAXD; ++k) {
        xa[k] = k < a.D ? (double)pa[k] : 0.0;
        acc[k] = 0.0;
    }
    double sl = 0.0, so = 0.0;
    for (int rb = lane; rb < a.nb; rb += 64) {
        const float* pb = a.xb + (size_t)rb * a.D;
        double diff[DVS_GP_MAXD], d2 = 0.0;
#pragma unroll
        for (int k = 0; k < DVS_GP_MAXD; ++k) {
            diff[k] = k < a.D ? (double)pb[k] - xa[k] : 0.0;
            d2 = fma(diff[k], diff[k], d2);
        }
        const double Kab = a.outputscale * exp(-d2 * a.inv2l2);
        const double g = a.G[(size_t)ra * a.nb + rb];
        const double w = g * Kab;
        sl += w * d2;
        so += w;
        const double wr = a.symmetric ? (g + a.G[(size_t)rb * a.nb + ra]) * Kab : w;
#pragma unroll
        for (int k = 0; k < DVS_GP_MAXD; ++k) acc[k] = fma(wr, diff[k], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < DVS_GP_MAXD; ++k) {
        const double s = dvs_wave_sum(acc[k], lane);
        if (lane == 0 && k < a.D) a.dxa[(size_t)ra * a.D + k] = s * a.inv_l2;
    }
    sl = dvs_wave_sum(sl, lane);
    so = dvs_wave_sum(so, lane);
    if (lane == 0) {
        a.rows[2 * (size_t)ra] = sl * a.inv_l3;
        a.rows[2 * (size_t)ra + 1] = so * a.inv_o;
    }
}

static GpKernArgs gp_kern_derived(const GpKernArgs& in, double lengthscale) {
    GpKernArgs a = in;
    a.inv2l2 = dvs_gp_inv2l2(lengthscale);
    a.inv_l2 = dvs_gp_inv_l2(lengthscale);
    a.inv_l3 = 1.0 / (lengthscale * lengthscale * lengthscale);
    a.inv_o = 1.0 / a.outputscale;
    return a;
}
void dvs_launch_gp_kernel(const GpKernArgs& in, double lengthscale, dvs_stream_t st) {
    const GpKernArgs a = gp_kern_derived(in, lengthscale);
    const size_t n = (size_t)a.na * a.nb;
    DVS_LAUNCH(k_gp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
}
void dvs_launch_gp_kernel_bwd(const GpKernArgs& in, double lengthscale, dvs_stream_t st) {
    const GpKernArgs a = gp_kern_derived(in, lengthscale);
    DVS_LAUNCH(k_gp_kernel_bwd, dim3((unsigned)((a.na + 3) / 4)), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// Row codec -> BIC parent masks on the device (the relabelling of BNLearnWrapper.score, src/problem/bn/bnlearn.py:34-45:
// graph vertex v stands for data-set variable labels[v]): parents[b][labels[v]] = OR over predecessors u of (1 << labels[u]).
// One thread per (DAG, vertex).  status bit 5: the labels of a DAG are not a permutation of 0..n-1 (the reference asserts,
// bnlearn.py:35) — that DAG's masks are zeroed.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bic_parent_masks(BicMaskArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.B * a.n) return;
    const int b = i / a.n, v = i - b * a.n;
    const uint8_t* lab = a.labels + (size_t)b * a.n;
    uint64_t seen = 0;
    bool ok = true;
    for (int u = 0; u < a.n; ++u) {
        ok = ok && lab[u] < a.n;
        seen |= 1ull << (lab[u] & 63);
    }
    ok = ok && seen == (a.n == 64 ? ~0ull : (1ull << a.n) - 1ull);
    const uint64_t pr = a.wide ? ((const uint64_t*)a.preds)[i] : (uint64_t)((const uint16_t*)a.preds)[i];
    uint64_t m = 0;
    for (int u = 0; u < v; ++u)
        if ((pr >> u) & 1ull) m |= 1ull << (lab[u] & 63);
    if (!ok) {
        atomicOr(a.status, 32);
        a.parents[(size_t)b * a.n + v] = 0;
        return;
    }
    a.parents[(size_t)b * a.n + lab[v]] = m;
}
void dvs_launch_bic_parent_masks(const BicMaskArgs& a, dvs_stream_t st) {
    DVS_LAUNCH(k_bic_parent_masks, dim3((unsigned)((a.B * a.n + 255) / 256)), dim3(256), 0, st, a);
}
