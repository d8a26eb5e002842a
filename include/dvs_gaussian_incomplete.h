/* dvs_gaussian_incomplete.h — eleventh companion header of dvs.h: a multivariate normal conditioned on the observed part of
 * every row.  One call gives, for rows with missing values, the posterior mean and variance of the missing
 * variables (exact imputation), the log-density of the observed part, its sum over the rows, and the summed conditional
 * covariance, which is what the E-step of EM on a Gaussian network needs.  dvs.h, the ten companion headers before this one and
 * DVS_VERSION = 202 stay what they are: a pure addition.
 *
 * Arithmetic.  IEEE fp64, one rounded operation at a time: no fused multiply-add anywhere, no matrix instructions, no
 * floating-point atomics, every sum in the order stated here.  Two calls give equal bytes.  log and sqrt are the platform's.
 *
 * ---- dvs_gbn_condition, dvs_gbn_condition_workspace_bytes ----------------------------------------------------------------------
 * Inputs.
 *   mean      device f64 [n_vars], cov: device f64 [n_vars][n_vars]: one multivariate normal as dvs_gbn_joint writes it
 *             (include/dvs_gaussian_params.h).  Only the cells cov[i][j] with i >= j are read; below, A_ij with i < j names
 *             the cell [j][i].
 *   x         device f64 [n_rows][n_vars].
 *   observed  device u64 [n_rows]: bit v set <=> x[r][v] is observed.  An unobserved cell never enters arithmetic, whatever it
 *             holds (NaN included): values are selected, not multiplied by 0.
 *   order     null or device i32 [n_rows], a permutation of the rows; null is the identity.  Position p holds row order[p].  It
 *             is not checked on the device.
 *
 * Per row.  O = the observed bits below n_vars, ascending; k = |O|; M = the other variables below n_vars.
 *   A = the lower triangle of cov.  t_i = x_i - mean_i for i in O, t_i = +0 for i in M.  ld = +0, q = +0.
 *   For each pivot j in O, ascending:
 *     1. the row is refused if A_jj is not finite or A_jj <= ((k + 1) * 2^-52) * cov[j][j]  (the backward error of a Cholesky
 *        factor of k rows on that diagonal entry, the argument of the pivot rule of include/dvs_gaussian.h);
 *     2. d = sqrt(A_jj);  ld = ld + log(A_jj);  y = t_j / d;  q = q + y * y;
 *     3. for every variable i not yet pivoted (the later members of O, and all of M):  l_i = A_ij / d;  t_i = t_i - l_i * y;
 *     4. for every pair i >= h of variables not yet pivoted:  A_ih = A_ih - l_i * l_h.
 *   Every product is rounded, then the addition or subtraction.  A cell receives exactly one update per pivot, in pivot order, so
 *   the factor and the trailing block depend on (cov, the mask) alone and a row's results on (mean, cov, its x, its mask) alone:
 *   not on order, on the launch geometry or on the rows it shares a workgroup with.
 *
 * Outputs (device; each may be null unless it says required).
 *   completed f64 [n_rows][n_vars]   x_i for i in O (its bits), mean_i - t_i for i in M: the conditional mean.
 *   cvar      f64 [n_rows][n_vars]   +0 on O, the final A_ii on M: the conditional variance.
 *   quad      f64 [n_rows]           q, the squared Mahalanobis distance of the observed part.
 *   logp      f64 [n_rows], required -((k * 0.9189385332046727 + 0.5 * ld) + 0.5 * q), the log-density of the observed part; a
 *                                    row with k = 0 has -0 here and the mean in completed.
 *   loglik    f64 [1], required      the sum of logp over the positions of order, in the two-level order of dvs_bn_loglik (as
 *                                    include/dvs_gaussian_params.h states it for dvs_gbn_loglik): chunks of 256 positions, a tree
 *                                    over a chunk's 256 terms, slot t of a second array adds the chunk sums t, t + 256, ... in
 *                                    ascending order, the same tree.  A refused row counts +0.
 *   ccov      f64 [n_vars][n_vars]   the sum over the rows of the conditional covariance: a row's cells are the final A_ih on
 *                                    M x M and +0 elsewhere.  The positions of order are cut into chunks of 256; within a chunk a
 *                                    run is a maximal stretch of consecutive positions with equal masks, and len the number of its
 *                                    rows that are not refused.  A chunk's cell starts at +0 and for each run with len > 0, in
 *                                    ascending position, on M x M:  cell = cell + (double)len * A_ih  (one product, one addition);
 *                                    a run whose rows are all refused adds nothing.  The chunk values are added cell by cell as
 *                                    loglik's chunk sums are.  Both triangles are written with equal bytes.
 *   counts    i64 [1]                the number of refused rows.
 *   With cvar and ccov both null the updates of step 4 on M x M may be left out; every cell is independent of the others, so the
 *   other outputs keep their bytes.
 *
 * Refusals.  A row is refused when a pivot fails rule 1, when a bit of its mask lies at or above n_vars, or when an observed
 * cell is not finite.  It has NaN in all its cells of every per-row output given, sets bit 4 of status (device i32, zeroed by the
 * caller) and is counted; the other rows are written as usual.
 *
 * workspace: dvs_gbn_condition_workspace_bytes(n_vars, n_rows) bytes of device memory (0 and dvs_last_error on a refusal): with
 * chunks = ceil(n_rows / 256), the chunk sums f64 [chunks], the refused rows per chunk i32 [chunks], then the chunks' covariance
 * cells f64 [n_vars (n_vars + 1) / 2][chunks], each array starting at a multiple of 256 bytes.
 * Checked before anything is enqueued, in this order: n_rows in [1, 2^31 - 1] (2), n_vars in [1, 48] (3), null pointers (10:
 * mean, cov, x, observed, logp, loglik, workspace, status), workspace_bytes (14 with the needed size). */
#ifndef DVS_GAUSSIAN_INCOMPLETE_H
#define DVS_GAUSSIAN_INCOMPLETE_H

#include "dvs_gaussian_params.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t dvs_gbn_condition_workspace_bytes(int32_t n_vars, int64_t n_rows);

int dvs_gbn_condition(int32_t n_vars, int64_t n_rows, const double* mean, const double* cov, const double* x,
                      const uint64_t* observed, const int32_t* order, double* completed, double* cvar, double* quad, double* logp,
                      double* loglik, double* ccov, int64_t* counts, void* workspace, size_t workspace_bytes, int32_t* status,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
