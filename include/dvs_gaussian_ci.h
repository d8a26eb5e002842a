/* dvs_gaussian_ci.h — seventh companion header of dvs.h: conditional-independence tests on real-valued data,
 * bnlearn's `cor`, `zf` and `mi-g`, from the moments dvs_gbn_moments writes (include/dvs_gaussian.h).  One Cholesky factor per
 * test and no pass over the rows.  dvs.h, the six companion headers before this one and DVS_VERSION = 202 stay what they are: a
 * pure addition.  The layouts of the tests and of the results are those of dvs_ci_tests (dvs.h) and dvs_ci_tests_group
 * (dvs_local.h), so dvs_pc_expand, dvs_pc_reduce, dvs_pc_orient and dvs_mmpc_update work on them unchanged.
 *
 * The three statistics and their p-values follow bnlearn's ci.test as recalled and are unpinned against an R run.
 *
 * Arithmetic.  IEEE fp64, one rounded operation at a time up to the squared pivots, r and 1 - r^2: no fused multiply-add, no
 * floating-point atomics, every sum in the order stated here.  Two calls give equal bytes.
 *
 * ---- dvs_gbn_ci_tests ---------------------------------------------------------------------------------------------------------
 * moments: device f64 [n_sets][DVS_GBN_STRIDE(n_vars)] as dvs_gbn_moments writes them; set_of: device i32 [n_tests], the set of
 * each test, NOT range checked on the device, or null for all set 0 (the meaning it has in dvs_gbn_scores).  pairs: device i32
 * [n_tests][2], (x, y); cond: device u64 [n_tests], bit z <=> z is in the conditioning set Z; out: device f64 [n_tests][3],
 * (statistic, df, p-value); status: device i32, zeroed by the caller — the layout of dvs_ci_tests.
 *
 * One test (x, y | Z), k = |Z|, m the size of its set, C its centred cross-products.  a_0 < a_1 < ... < a_(k-1) the members of Z,
 * a_k = x, a_(k+1) = y.  Row-wise Cholesky of C[a][a], the operation order of dvs_gbn_scores:
 *   for i = 0 .. k + 1:  for j = 0 .. i:
 *     s = C[a_i][a_j];  for t = 0 .. j - 1:  s = s - L[i][t] * L[j][t]   (product rounded, then the subtraction)
 *     j < i:  L[i][j] = s / L[j][j]
 *     j = i:  d_i^2 = s, the squared pivot;  L[i][i] = sqrt(s)
 * Every squared pivot passes the pivot rule of dvs_gaussian.h at p = k + 1: d_i^2 is finite and d_i^2 > ((k + 3) * 2^-52) *
 * C[a_i][a_i].  With l = L[k + 1][k] and d_y^2 = d_(k+1)^2:
 *   ll = l * l;  q = ll + d_y^2;  r = l / sqrt(q);  1 - r^2 = d_y^2 / q;  r^2 = ll / q
 * (r is the partial correlation of x and y given Z; 1 - r^2 is that quotient, never a subtraction from 1).
 * Cells, by test_type:
 *   DVS_GCI_COR    df = m - k - 2;  statistic = r * sqrt(df / (1 - r^2)), signed (Student's t);
 *                  p = I_(1 - r^2)(0.5 * df, 0.5), the regularised incomplete beta function (two-sided)
 *   DVS_GCI_ZF     the df cell holds m - k - 3;  statistic = (0.5 * log((1 + r) / (1 - r))) * sqrt(m - k - 3), signed (Fisher's z);
 *                  p = erfc(|statistic| / 1.4142135623730951)
 *   DVS_GCI_MI_G   statistic = -m * log(1 - r^2);  df = 1;  p = erfc(sqrt(statistic / 2))
 * Library functions.  log, sqrt and erfc are the platform's.  I_x(a, b) is a modified Lentz evaluation of the continued fraction
 * (Numerical Recipes' betacf: tiny = 1e-300, stops when |delta - 1| < 1e-15, at most 20 000 steps), on (a, b, x) when
 * x < (a + 1) / (a + b + 2) and as 1 - I_(1 - x)(b, a) otherwise, 1 - x being r^2 above; its lead factor is
 * exp(lgamma(a + b) - lgamma(a) - lgamma(b) + a * log(x) + b * log(1 - x)), lgamma the platform's.  The difference of the two
 * large lgamma values carries an absolute error of a few ulp of lgamma(a + b), so the relative error of a `cor` p-value grows
 * with df: measured below 1e-11 up to df = 5000 and about 2.4e-11 at df = 65 536; about 1e-9 is expected at
 * df = 10^6.  A property of the scheme, stated here, not a defect.
 * Refusals: three NaNs in the test's cells and bit 4 of status; the other tests of the call are evaluated.
 *   x = y;  x or y in Z;  x, y or a bit of cond at or above n_vars (or an index below 0);  k > DVS_GCI_MAX_COND (the factor is
 *   not spilled);  df < 1: m - k - 2 < 1 for cor and mi-g, m - k - 3 < 1 for zf;  a squared pivot that fails the rule above (a
 *   collinear conditioning set cannot be told from a rounding artefact; bnlearn's pseudo-inverse is not restated).
 * Checked before anything is enqueued, in this order: n_tests, n_sets > 0 (2), n_vars in [1, 48] (3), n_tests * 3 < 2^31 (2),
 * test_type (12), null pointers (10; set_of may be null), out_bytes < n_tests * 24 (14 with the needed size).
 *
 * ---- dvs_gbn_ci_tests_group -------------------------------------------------------------------------------------------------
 * target: device i32 [n_groups]; cond, candidates: device u64 [n_groups]; out: device f64 [n_groups][n_vars][3] — the layout of
 * dvs_ci_tests_group; set_of: device i32 [n_groups] or null.  Cell [g][c] is, byte for byte, what dvs_gbn_ci_tests gives for
 * the pair (x, y) = (target[g], c) given cond[g] on the set of group g, for every c < n_vars with bit c of candidates[g] set: the
 * rows of Z and of the target are factored once and every candidate's row is appended to them, the same operations in the same
 * order.  A refused candidate has three NaNs and sets bit 4 of status.  A cell whose c is not in candidates[g] is three NaNs and
 * sets no bit; bits of candidates at or above n_vars name no cell and are not read.
 * Checked before anything is enqueued, in this order: n_groups, n_sets > 0 (2), n_vars in [1, 48] (3), n_groups * n_vars * 3 <
 * 2^31 (2), test_type (12), null pointers (10; set_of may be null), out_bytes < n_groups * n_vars * 24 (14 with the needed
 * size). */
#ifndef DVS_GAUSSIAN_CI_H
#define DVS_GAUSSIAN_CI_H

#include "dvs_gaussian.h"

#define DVS_GCI_MAX_COND 10      /* |Z| + 2 rows fit the lane's factor slice of DVS_GBN_MAX_PARENTS + 1 rows */

#ifdef __cplusplus
extern "C" {
#endif

typedef enum dvs_gci_type {
    DVS_GCI_COR = 0,
    DVS_GCI_ZF = 1,
    DVS_GCI_MI_G = 2
} dvs_gci_type;

int dvs_gbn_ci_tests(int32_t n_tests, int32_t n_vars, const double* moments, int32_t n_sets, const int32_t* set_of,
                     const int32_t* pairs, const uint64_t* cond, int32_t test_type, double* out, size_t out_bytes,
                     int32_t* status, void* stream);

int dvs_gbn_ci_tests_group(int32_t n_groups, int32_t n_vars, const double* moments, int32_t n_sets, const int32_t* set_of,
                           const int32_t* target, const uint64_t* cond, const uint64_t* candidates, int32_t test_type,
                           double* out, size_t out_bytes, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
