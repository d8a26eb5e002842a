/* dvs_gaussian.h — sixth companion header of dvs.h: Gaussian Bayesian networks on real-valued data: the
 * moments of a data set or of many row sets of it, bnlearn's continuous scores loglik-g, aic-g, bic-g and bge from those
 * moments, the single-edge toggle pass over them, and the regression parameters of a structure.  dvs.h and the five companion
 * headers before this one stay what they are and DVS_VERSION stays 202: a pure addition.
 *
 * Arithmetic.  Everything is IEEE fp64, one rounded operation at a time: no fused multiply-add anywhere, no floating-point
 * atomics, every sum in the order stated here.  Two calls give equal bytes.
 *
 * ---- dvs_gbn_moments, dvs_gbn_moments_workspace_bytes -------------------------------------------------------------------------
 * data: device f64 [n_samples][n_vars], 1 <= n_vars <= 48.  rows: device i32 [n_sets][set_size] indices into data, NOT range
 * checked on the device (the caller checks them once), or null: then n_sets must be 1, set_size must be n_samples and the one
 * set holds all rows in order.  Sample s of set r is row rows[r][s].  moments: device f64 [n_sets][DVS_GBN_STRIDE(n_vars)],
 * DVS_GBN_STRIDE(n) = 1 + n + n * n doubles per set:
 *   [0]                 m = set_size, as a double
 *   [1 + i]             mean[i]
 *   [1 + n + i * n + j] C[i][j] = sum over the samples of (x_i - mean_i) (x_j - mean_j), both triangles written, equal bytes
 * Order.  The samples of a set are cut into chunks of DVS_GBN_CHUNK consecutive positions (the last one may be short).
 *   pass 1   a chunk's column sum starts at +0 and adds x_i in position order; sum_i starts at +0 and adds the chunk sums in
 *            ascending chunk order; mean_i = sum_i / m.
 *   pass 2   d_i = x_i - mean_i (one subtraction); a chunk's cell (i, j), i <= j, starts at +0 and adds the rounded product
 *            d_i * d_j in position order; C[i][j] starts at +0 and adds the chunk cells in ascending chunk order.
 * So a row-set result is, as bytes, the plain call on the gathered rows.  workspace holds the chunk values:
 * dvs_gbn_moments_workspace_bytes = 8 * n_sets * chunks * (n + n (n + 1) / 2), chunks = ceil(set_size / DVS_GBN_CHUNK); 0 is a
 * refusal.  Checked before anything is enqueued, in this order: n_sets, set_size, n_samples > 0 (2), n_vars in [1, 48] (3),
 * rows null with n_sets != 1 or set_size != n_samples (13), n_sets * chunks * n (n + 1) / 2 < 2^31 (2), null pointers (10),
 * workspace_bytes (14 with the needed size), moments_bytes < n_sets * DVS_GBN_STRIDE * 8 (14 with that size).
 *
 * ---- dvs_gbn_scores -----------------------------------------------------------------------------------------------------------
 * moments: device f64 [n_sets][DVS_GBN_STRIDE(n_vars)] as dvs_gbn_moments writes them; set_of: device i32 [batch], the set of
 * each structure, NOT range checked on the device, or null for all set 0; parents: device u64 [batch][n_vars], bit u of
 * parents[b][v] <=> u -> v (the self bit is ignored).  local: device f64 [batch][n_vars]; out: device f64 [batch], local added
 * over v ascending from +0 (NaN if any is); status: device i32, zeroed by the caller — the layout and meaning of dvs_bn_scores.
 * The family (v, Pa), p = |Pa|, a_0 < a_1 < ... < a_(p-1) the parents and a_p = v.  M = C for the likelihood scores and the
 * fit; for bge M = C off the diagonal and M[i][i] = C[i][i] + t (one addition).  Row-wise Cholesky of M[a][a]:
 *   for i = 0 .. p:  for j = 0 .. i:
 *     s = M[a_i][a_j];  for k = 0 .. j - 1:  s = s - L[i][k] * L[j][k]   (product rounded, then the subtraction)
 *     j < i:  L[i][j] = s / L[j][j]
 *     j = i:  d_i^2 = s, the squared pivot;  L[i][i] = sqrt(s)
 * ln det M[Pa] = ldp starts at +0 and adds log(d_k^2) for k = 0 .. p - 1; RSS = d_p^2.
 * Refusals: NaN in local[b][v] and bit 4 of status; the other families of the structure are scored.
 *   a parent bit at or above n_vars;  p > DVS_GBN_MAX_PARENTS (the factor is not spilled);
 *   m - p - 1 < 1, for the likelihood scores and the fit;
 *   a squared pivot that is not finite, or within rounding of zero: d_k^2 <= (p + 2) * 2^-52 * M[a_k][a_k] (the size of the
 *   Cholesky backward error on that diagonal entry: a smaller pivot cannot be told from a collinear column).
 * Scores, with m the set's size, dof = m - p - 1:
 *   DVS_GSCORE_LOGLIK   s2 = RSS / dof (the unbiased residual variance, bnlearn's as recalled: unpinned against an R run);
 *                       LL = -(0.5 * m) * log(6.283185307179586 * s2) - 0.5 * dof
 *   DVS_GSCORE_AIC      LL - k * (p + 2)          score_arg = k >= 0, default 1
 *   DVS_GSCORE_BIC      LL - k * (p + 2)          score_arg = k >= 0, default log(m) / 2 (taken on the device)
 *   DVS_GSCORE_BGE      Geiger and Heckerman's score with the correction of Kuipers, Moffa and Heckerman (2014), the prior
 *                       mean being the sample mean (bnlearn's default as recalled), so that R = t I + C:
 *                       score_arg = alpha_mu > 0, default 1; score_arg2 = alpha_w > n_vars + 1, default n_vars + 2;
 *                       t = alpha_mu * (alpha_w - n - 1) / (alpha_mu + 1);  g = alpha_w - n + p;  ldf = ldp + log(RSS);
 *                       local = ((((((-(0.5 * m) * log(pi)) + 0.5 * log(alpha_mu / (alpha_mu + m)))
 *                                + lgamma(0.5 * (m + g + 1))) - lgamma(0.5 * (g + 1))) + (0.5 * (g + p + 1)) * log(t))
 *                                - (0.5 * (m + g + 1)) * ldf) + (0.5 * (m + g)) * ldp,   log(pi) = log(3.141592653589793)
 * score_arg = NaN asks for the default; score_arg2 is read by bge only and must be NaN otherwise.  Checked before anything is
 * enqueued, in this order: batch, n_sets > 0 (2), n_vars in [1, 48] (3), score_type (12), the arguments (13), null pointers
 * (10).
 *
 * ---- dvs_gbn_toggle_scores ------------------------------------------------------------------------------------------------------
 * dvs_bn_toggle_scores over the moments: toggles[b][v][u] (device f64 [batch][n][n]) is, as bytes, local[v] of dvs_gbn_scores on
 * the structure with bit u of parents[b][v] flipped, NaN on the diagonal and where that family is refused (bit 4 of status: the
 * move is not available); local[b][v] is that call's bytes too.  worklist null: all rows.  worklist device i32 [2 * batch]:
 * slots 2b and 2b + 1 name the rows of structure b to recompute, -1 = none; only those rows of toggles are written and local
 * is left to dvs_hc_step.  Checks: those of dvs_gbn_scores with batch * n_vars^2 < 2^31 (2) next to n_vars, then local_bytes <
 * batch * n_vars * 8 and toggles_bytes < batch * n_vars^2 * 8 (14 with the needed size).
 *
 * ---- dvs_gbn_fit ----------------------------------------------------------------------------------------------------------------
 * The regression of v on its parents from the same factor (M = C): y = L[p][0 .. p - 1] is the forward solve; the backward one is
 *   for i = p - 1 .. 0:  s = y_i;  for k = i + 1 .. p - 1:  s = s - L[k][i] * beta_k;  beta_i = s / L[i][i]
 * coef[b][v][a_i] = beta_i and 0 elsewhere in the row (device f64 [batch][n][n]); intercept[b][v] = mean_v less the rounded
 * products beta_i * mean_(a_i), subtracted for i = 0 .. p - 1; sd[b][v] = sqrt(RSS / (m - p - 1)).  The refusal rules are the
 * likelihood scores'; a refused family has NaN in its whole coef row, its intercept and its sd, and sets bit 4 of status.
 * Checks: batch, n_sets > 0 (2), n_vars and batch * n_vars^2 < 2^31 (3, 2), null pointers (10), coef_bytes < batch * n^2 * 8
 * (14 with the needed size). */
#ifndef DVS_GAUSSIAN_H
#define DVS_GAUSSIAN_H

#include "dvs.h"

#define DVS_GBN_CHUNK 128
#define DVS_GBN_MAX_PARENTS 11
#define DVS_GBN_STRIDE(n) (1 + (n) + (n) * (n))

#ifdef __cplusplus
extern "C" {
#endif

typedef enum dvs_gscore_type {
    DVS_GSCORE_LOGLIK = 0,
    DVS_GSCORE_AIC = 1,
    DVS_GSCORE_BIC = 2,
    DVS_GSCORE_BGE = 3
} dvs_gscore_type;

size_t dvs_gbn_moments_workspace_bytes(int32_t n_vars, int32_t n_sets, int32_t set_size);

int dvs_gbn_moments(int32_t n_vars, int32_t n_samples, const double* data, const int32_t* rows, int32_t n_sets, int32_t set_size,
                    void* workspace, size_t workspace_bytes, double* moments, size_t moments_bytes, void* stream);

int dvs_gbn_scores(int32_t batch, int32_t n_vars, const double* moments, int32_t n_sets, const int32_t* set_of,
                   const uint64_t* parents, int32_t score_type, double score_arg, double score_arg2, double* local, double* out,
                   int32_t* status, void* stream);

int dvs_gbn_toggle_scores(int32_t batch, int32_t n_vars, const double* moments, int32_t n_sets, const int32_t* set_of,
                          const uint64_t* parents, int32_t score_type, double score_arg, double score_arg2,
                          const int32_t* worklist, double* local, size_t local_bytes, double* toggles, size_t toggles_bytes,
                          int32_t* status, void* stream);

int dvs_gbn_fit(int32_t batch, int32_t n_vars, const double* moments, int32_t n_sets, const int32_t* set_of,
                const uint64_t* parents, double* coef, size_t coef_bytes, double* intercept, double* sd, int32_t* status,
                void* stream);

#ifdef __cplusplus
}
#endif
#endif
