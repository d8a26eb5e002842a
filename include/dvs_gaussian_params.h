/* dvs_gaussian_params.h — eighth companion header of dvs.h: what is done with a fitted Gaussian network: its
 * joint distribution, forward sampling, the log-likelihood of held-out rows and prediction of one variable, bnlearn's
 * gbn2mvnorm, rbn, logLik and predict on a Gaussian network.  dvs.h, the seven companion headers before this one and
 * DVS_VERSION = 202 stay what they are: a pure addition.  The quantile function and bnlearn parity are as recalled and are
 * unpinned against an R run.
 *
 * Arithmetic.  IEEE fp64, one rounded operation at a time: no fused multiply-add anywhere, no floating-point atomics, every sum
 * in the order stated here.  Two calls give equal bytes.  log and sqrt are the platform's.
 *
 * A network is laid out as dvs_gbn_fit writes it (include/dvs_gaussian.h): parents: device u64 [batch][n_vars], bit u of
 * parents[b][v] <=> u -> v (the self bit is ignored); coef: device f64 [batch][n_vars][n_vars], read at parent bits only;
 * intercept, sd: device f64 [batch][n_vars].  There is no cap on the number of parents: a variable may have n_vars - 1.
 * Pa(v) is the set of parent bits of v below n_vars without v.  The conditional mean of v at the values x:
 *   mu_v(x) = intercept_v, then for u in Pa(v) ascending: mu = mu + coef[v][u] * x_u   (the product rounded, then the addition)
 * The topological order is dvs_bn_sample's: the lowest variable all of whose parents are placed, repeatedly.
 * A network is malformed, with these bits of status (device i32, zeroed by the caller; several may be set), when
 *   bit 0   it has a cycle (no variable can be placed);
 *   bit 4   a parent bit lies at or above n_vars;
 *   bit 6   an intercept, an sd or a coefficient at a parent bit is not finite, or an sd is not > 0.
 *
 * ---- dvs_gbn_joint --------------------------------------------------------------------------------------------------------------
 * mean: device f64 [batch][n_vars]; cov: device f64 [batch][n_vars][n_vars] of the multivariate normal every network defines.
 * The variables are taken in topological order.  For v:
 *   mean_v = mu_v(mean)
 *   for every u placed before v:  s = +0, then for k in Pa(v) ascending: s = s + coef[v][k] * cov[k][u];  cov[v][u] = cov[u][v] = s
 *   s = sd_v * sd_v, then for k in Pa(v) ascending: s = s + coef[v][k] * cov[v][k];  cov[v][v] = s
 * Both triangles are written with equal bytes.  A malformed network sets its bits of status and has NaN in all its cells of
 * mean and cov; the other networks are written as usual.
 * Checked before anything is enqueued, in this order: batch > 0 (2), n_vars in [1, 48] (3), batch * n_vars^2 < 2^31 (2), null
 * pointers (10), cov_bytes < batch * n_vars^2 * 8 (14 with the needed size).
 *
 * ---- dvs_gbn_quantiles ------------------------------------------------------------------------------------------------------------
 * The sampler's map from an integer to a standard normal deviate, for count values: k: device u64 [count], z: device f64 [count].
 * k >= 2^52 gives NaN.  Otherwise u = (k + 0.5) * 2^-52 and uc = ((2^52 - 1 - k) + 0.5) * 2^-52 = 1 - u, both exact and in (0, 1);
 * q = u - 0.5, exact.  z is the normal quantile of u by Wichura's algorithm AS 241, PPND16:
 *   |q| <= 0.425   r = 0.180625 - q * q;                     z = q * A(r) / B(r)
 *   otherwise      p = min(u, uc);  r = sqrt(-log(p));
 *                  r <= 5:  r = r - 1.6;  z = C(r) / D(r)        r > 5:  r = r - 5;  z = E(r) / F(r);        q < 0:  z = -z
 * A polynomial is a Horner chain of rounded products and rounded additions: P(r) = p7, then for i = 6 .. 0: P = P * r; P = P + p_i.
 * The denominators have the constant term 1.  q * A(r) is one rounded product, divided by B(r).  The coefficients:
 *   a0 .. a7   3.3871328727963666080  1.3314166789178437745e+2  1.9715909503065514427e+3  1.3731693765509461125e+4
 *              4.5921953931549871457e+4  6.7265770927008700853e+4  3.3430575583588128105e+4  2.5090809287301226727e+3
 *   b1 .. b7   4.2313330701600911252e+1  6.8718700749205790830e+2  5.3941960214247511077e+3  2.1213794301586595867e+4
 *              3.9307895800092710610e+4  2.8729085735721942674e+4  5.2264952788528545610e+3
 *   c0 .. c7   1.42343711074968357734  4.63033784615654529590  5.76949722146069140550  3.64784832476320460504
 *              1.27045825245236838258  2.41780725177450611770e-1  2.27238449892691845833e-2  7.74545014278341407640e-4
 *   d1 .. d7   2.05319162663775882187  1.67638483018380384940  6.89767334985100004550e-1  1.48103976427480074590e-1
 *              1.51986665636164571966e-2  5.47593808499534494600e-4  1.05075007164441684324e-9
 *   e0 .. e7   6.65790464350110377720  5.46378491116411436990  1.78482653991729133580  2.96560571828504891230e-1
 *              2.65321895265761230930e-2  1.24266094738807843860e-3  2.71155556874348757815e-5  2.01033439929228813265e-7
 *   f1 .. f7   5.99832206555887937690e-1  1.36929880922735805310e-1  1.48753612908506148525e-2  7.86869131145613259100e-4
 *              1.84631831751005468180e-5  1.42151175831644588870e-7  2.04426310338993978564e-15
 * The central branch uses + - * / alone; a tail branch adds one log and one sqrt.  z(k) = -z(2^52 - 1 - k) as bytes.
 * Checked before anything is enqueued, in this order: count in [1, 2^31 - 1] (2), null pointers (10).
 *
 * ---- dvs_gbn_sample, dvs_gbn_sample_workspace_bytes -------------------------------------------------------------------------------
 * n_rows rows drawn from ONE network (parents u64 [n_vars], coef f64 [n_vars][n_vars], intercept, sd f64 [n_vars]) by forward
 * sampling.  data_out: device f64 [n_rows][n_vars], every cell written.  workspace: dvs_gbn_sample_workspace_bytes(n_vars)
 * bytes of device memory (0 and dvs_last_error for n_vars outside [1, 48]).  A preparation kernel orders the variables and
 * checks the network; each of the three status bits leaves data_out untouched.
 * Row i has the global index g = (row_offset + i) mod 2^32 and key = dvs_site_key(seed_lo, seed_hi, 510, g) of
 * csrc/dvs_device.h, seed_lo and seed_hi the halves of seed.  Variable v draws h1 = dvs_draw(key, 2 v), h2 = dvs_draw(key,
 * 2 v + 1), k = (h1 >> 6) * 2^26 + (h2 >> 6), z = the quantile above at k, and x_v = mu_v(x) + sd_v * z (one product, one
 * addition).  The variables are taken in topological order, but x depends on (seed, g, v) and the network alone: not on the
 * order, the launch geometry, or how a request is cut into calls with consecutive row_offset.
 * Checked before anything is enqueued, in this order: n_rows in [1, 2^31 - 1] (2), n_vars in [1, 48] (3), row_offset >= 0 (12),
 * null pointers (10), workspace_bytes (14 with the needed size).
 *
 * ---- dvs_gbn_loglik ---------------------------------------------------------------------------------------------------------------
 * The log-likelihood of n_rows rows (data: device f64 [n_rows][n_vars], any rows, not the fit's) under each of batch networks.
 * A preparation kernel takes c_v = log(sd_v) + 0.9189385332046727 once per (b, v).  The term of a row starts at +0; for v
 * ascending:  e = (x_v - mu_v(x)) / sd_v;  term = term - (c_v + 0.5 * (e * e)).
 * per_row: null or device f64 [batch][n_rows], the terms; out: device f64 [batch], their sum in the order of dvs_bn_loglik: the
 * rows are cut into chunks of 256 (absent rows count +0); the 256 terms of a chunk are added by a tree (for s = 128, 64 .. 1:
 * slot t < s adds slot t + s); slot t of a second array of 256 starts at +0 and adds the chunk sums t, t + 256, ... in ascending
 * order; the same tree gives out[b].  per_row given or null gives the same out.  Nothing is special-cased for the data: a NaN or
 * infinite cell propagates by IEEE arithmetic.  A malformed network has NaN in all its cells of per_row and in out[b] and sets
 * bit 4 of status (alone, whichever rule it breaks); the other networks are evaluated.
 * workspace: the chunk sums f64 [batch][chunks], flags i32 [batch][n_vars], then c f64 [batch][n_vars], each array starting at a
 * multiple of 256 bytes — the size dvs_bn_loglik's layout has before its tables plus batch * n_vars * 8.
 * Checked before anything is enqueued, in this order: batch > 0 (2), n_rows in [1, 2^31 - 1] (2), n_vars in [1, 48] (3),
 * batch * n_vars and batch * ceil(n_rows / 256) < 2^31 (2), null pointers (10; per_row may be null), workspace_bytes (14 with
 * the needed size).
 *
 * ---- dvs_gbn_predict --------------------------------------------------------------------------------------------------------------
 * The prediction of variable target for every row under each of batch networks; the target's own column is never read.
 * pred: device f64 [batch][n_rows]; var: device f64 [batch], the conditional variance, which does not depend on the row.
 *   mode 0   from the parents (bnlearn's predict(method = "parents")):  pred = mu_t(x);  var = sd_t * sd_t
 *   mode 1   the exact conditional given every other variable, closed-form over the Markov blanket:
 *            s = sd_t * sd_t;  prec = 1 / s;  num = mu_t(x) * prec;  then for the children c of t (t in Pa(c)) ascending:
 *              w = coef[c][t] / (sd_c * sd_c);  r = x_c - m_c, m_c = mu_c(x) with t's term left out of the sum;
 *              num = num + w * r;  prec = prec + coef[c][t] * w   (each product rounded, then the addition)
 *            pred = num / prec;  var = 1 / prec
 * A malformed network has NaN in its row of pred and in var[b] and sets bit 4 of status.  workspace: flags i32 [batch], rounded
 * up to a multiple of 256 bytes.
 * Checked before anything is enqueued, in this order: batch > 0 (2), n_rows in [1, 2^31 - 1] (2), n_vars in [1, 48] (3),
 * batch * n_vars and batch * ceil(n_rows / 256) < 2^31 (2), target in [0, n_vars) (13), mode 0 or 1 (12), null pointers (10), workspace_bytes (14 with the
 * needed size). */
#ifndef DVS_GAUSSIAN_PARAMS_H
#define DVS_GAUSSIAN_PARAMS_H

#include "dvs_gaussian.h"

#define DVS_GBN_PREDICT_PARENTS 0
#define DVS_GBN_PREDICT_EXACT 1

#ifdef __cplusplus
extern "C" {
#endif

int dvs_gbn_joint(int32_t batch, int32_t n_vars, const uint64_t* parents, const double* coef, const double* intercept,
                  const double* sd, double* mean, double* cov, size_t cov_bytes, int32_t* status, void* stream);

int dvs_gbn_quantiles(int64_t count, const uint64_t* k, double* z, void* stream);

size_t dvs_gbn_sample_workspace_bytes(int32_t n_vars);

int dvs_gbn_sample(int32_t n_vars, int64_t n_rows, const uint64_t* parents, const double* coef, const double* intercept,
                   const double* sd, uint64_t seed, int64_t row_offset, void* workspace, size_t workspace_bytes,
                   double* data_out, int32_t* status, void* stream);

int dvs_gbn_loglik(int32_t batch, int32_t n_vars, int64_t n_rows, const double* data, const uint64_t* parents, const double* coef,
                   const double* intercept, const double* sd, double* per_row, double* out, void* workspace,
                   size_t workspace_bytes, int32_t* status, void* stream);

int dvs_gbn_predict(int32_t batch, int32_t n_vars, int64_t n_rows, const double* data, const uint64_t* parents,
                    const double* coef, const double* intercept, const double* sd, int32_t target, int32_t mode, double* pred,
                    double* var, void* workspace, size_t workspace_bytes, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
