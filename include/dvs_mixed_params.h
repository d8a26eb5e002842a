/* dvs_mixed_params.h — tenth companion header of dvs.h: what is done with a fitted conditional Gaussian network:
 * forward sampling of its real columns, the continuous part of the log-likelihood of held-out rows, and prediction of one
 * variable, bnlearn's rbn, logLik and predict on a mixed network.  dvs.h, the nine companion headers before this one and
 * DVS_VERSION = 202 stay what they are: a pure addition.  bnlearn parity is as recalled and unpinned against an R run.
 *
 * Arithmetic.  IEEE fp64, one rounded operation at a time: no fused multiply-add anywhere, no floating-point atomics, every sum
 * in the order stated here.  Two calls give equal bytes.  log, exp and sqrt are the platform's.
 *
 * The network.  ONE network per call on n_vars <= 48 variables, n_cont >= 1 of them continuous.
 *   card       device u8 [n_vars]: the level count 1 .. 16 of a discrete variable, 0 for a continuous one (include/dvs_mixed.h)
 *   parents    device u64 [n_vars]: bit u of parents[v] <=> u -> v (the self bit is ignored)
 *   offset     device i64 [n_vars + 1]: the exclusive prefix over v of q_v; q_v = the product of the level counts of the discrete
 *              parents of a continuous v (1 for none) and q_v = 0 for a discrete v.  n_cells = offset[n_vars] as the host knows it
 *   coef       device f64 [n_cells][n_vars], read at continuous parent bits only;  intercept, sd: device f64 [n_cells]
 * These are the arrays dvs_cg_fit (include/dvs_mixed.h) writes when it is given the continuous families in ascending variable
 * order.  The tables of the discrete variables are not an argument: no entry point here reads a CPT, and the discrete half of
 * every quantity is composed by the caller with dvs_bn_sample / dvs_bn_loglik / dvs_bn_predict, the way dvs_cg_scores composes
 * with dvs_bn_scores.
 * Rows.  packed: device u64 [n_rows][ceil(n_vars / 16)], the level codes of dvs_bn_scores (the nibble of a continuous variable is
 * not read); x: device f64 [n_rows][n_cont], the continuous columns in ascending variable order.
 * The configuration z of a continuous v in a row is the mixed-radix number of the levels of its discrete parents, the lowest
 * variable id fastest (the key of dvs_cg_partition); its cell is offset[v] + z.  The conditional mean at the row's values:
 *   mu_{v,z}(x) = intercept[cell], then for the continuous parents u ascending: mu = mu + coef[cell][u] * x_u
 *   (the product rounded, then the addition)
 * A configuration is EMPTY exactly when its sd is NaN (what dvs_cg_fit writes for a configuration without rows); its other
 * parameters are then not read.  There is no cap on continuous parents: DVS_GBN_MAX_PARENTS belongs to the fit.
 * The network is malformed, with these bits of status (device i32, zeroed by the caller; several may be set), when
 *   bit 0   it has a cycle over all variables (no variable can be placed);
 *   bit 4   a parent bit lies at or above n_vars; a discrete variable has a continuous parent; a card is above 16; a q_v is above
 *           DVS_CG_MAX_CONFIGS; offset[0] is not 0 or offset[v + 1] - offset[v] is not q_v or offset[n_vars] is not n_cells; n_cont
 *           differs from the zeros of card;
 *   bit 6   a non-empty configuration has an intercept, an sd or a coefficient at a continuous parent bit that is not finite, or
 *           an sd that is not > 0.  (Looked at only when bits 0 and 4 are clear: the cells are found through offset.)
 * A malformed network leaves dvs_cgbn_sample's output untouched and gives NaN (255 in a u8 prediction) in every cell the two
 * row entry points write.
 * Rows that meet trouble.  A row in which a variable the entry point evaluates has an empty configuration is not an error: the
 * cell written for it is NaN (in the sampler: x_v, and from there by IEEE arithmetic every value computed from it) and bit 7 of
 * status is set as information.  A row whose level code for a discrete parent that is read is at or above its card gets NaN in the
 * same way and sets bit 4: the rule of dvs_bn_loglik, not the clamp of dvs_cg_partition.
 *
 * ---- dvs_cgbn_sample, dvs_cgbn_sample_workspace_bytes ----------------------------------------------------------------------------
 * packed holds the levels of n_rows rows, already drawn (dvs_bn_sample on the discrete sub-network, spread to the variables'
 * nibbles).  x_out: device f64 [n_rows][n_cont], every cell written.  workspace: dvs_cgbn_sample_workspace_bytes(n_vars) = 256
 * bytes of device memory (0 and dvs_last_error for n_vars outside [1, 48]).  Preparation kernels apply the rules above and find
 * the topological order, dvs_bn_sample's: the lowest variable all of whose parents are placed, repeatedly.  Then one thread per
 * row: row i has the global index g = (row_offset + i) mod 2^32 and key = dvs_site_key(seed_lo, seed_hi, 510, g) of
 * csrc/dvs_device.h.  A continuous variable v, by its id in the full numbering, draws h1 = dvs_draw(key, 2 v), h2 = dvs_draw(key,
 * 2 v + 1), k = (h1 >> 6) * 2^26 + (h2 >> 6), z = the AS 241 quantile of dvs_gbn_quantiles (include/dvs_gaussian_params.h) at k,
 * and x_v = mu_{v,z}(x) + sd * z (one product, one addition).  x depends on (seed, g, v), the row's levels and the network alone:
 * not on the order, the launch geometry, or how a request is cut into calls with consecutive row_offset.  Site 510 is
 * dvs_gbn_sample's on purpose: with every variable continuous the bytes are that entry point's on the same parameters.  (The
 * discrete half draws at site 500, in dvs_bn_sample.)
 * Checked before anything is enqueued, in this order: n_rows in [1, 2^31 - 1] and n_cells >= 1 with n_cells * n_vars < 2^31 (2),
 * n_vars in [1, 48] and n_cont in [1, n_vars] (3), row_offset >= 0 (12), null pointers (10), workspace_bytes (14 with the needed
 * size).
 *
 * ---- dvs_cgbn_loglik, dvs_cgbn_loglik_workspace_bytes ----------------------------------------------------------------------------
 * The continuous part of the log-likelihood of n_rows rows.  A preparation kernel takes c = log(sd) + 0.9189385332046727 once per
 * cell.  The term of a row starts at +0; for the continuous v ascending, z its configuration in the row:
 *   e = (x_v - mu_{v,z}(x)) / sd_{v,z};  term = term - (c_{v,z} + 0.5 * (e * e))
 * per_row: null or device f64 [n_rows], the terms; out: device f64 [1], their sum in the order of dvs_bn_loglik: chunks of 256
 * rows (absent rows count +0) added by a tree (for s = 128, 64 .. 1: slot t < s adds slot t + s); slot t of a second array of 256
 * starts at +0 and adds the chunk sums t, t + 256, ... in ascending order; the same tree gives out.  per_row given or null gives
 * the same out.  A NaN or infinite data cell propagates by IEEE arithmetic.  With every variable continuous the bytes are those
 * of dvs_gbn_loglik at batch 1.
 * workspace: a header of 256 bytes, the chunk sums f64 [ceil(n_rows / 256)] rounded up to a multiple of 256 bytes, then c f64
 * [n_cells]; dvs_cgbn_loglik_workspace_bytes gives the size, 0 and dvs_last_error on a refusal.
 * Checked before anything is enqueued, in this order: n_rows and n_cells as above (2), n_vars and n_cont (3), null pointers (10;
 * per_row may be null), workspace_bytes (14 with the needed size).
 *
 * ---- dvs_cgbn_predict, dvs_cgbn_predict_workspace_bytes ----------------------------------------------------------------------------
 * The prediction of variable target for every row; the target's own column of x or nibble of packed is never read.
 *   DVS_CGBN_PREDICT_PARENTS (0), a continuous target from its parents:  pred = mu_{t,z}(x);  var = sd_{t,z} * sd_{t,z}
 *   DVS_CGBN_PREDICT_EXACT (1), a continuous target given every other variable, dvs_gbn_predict's closed form over the Markov
 *     blanket with every child's parameters at that child's configuration in the row (the children of a continuous variable are
 *     all continuous):
 *       s = sd_t * sd_t;  prec = 1 / s;  num = mu_t(x) * prec;  then for the children c of t ascending, at c's cell:
 *         w = coef[c][t] / (sd_c * sd_c);  r = x_c - m_c, m_c = mu_c(x) with t's term left out of the sum;
 *         num = num + w * r;  prec = prec + coef[c][t] * w   (each product rounded, then the addition)
 *       pred = num / prec;  var = 1 / prec
 *     In both modes pred and var are device f64 [n_rows]; prior and posterior are not read.
 *   DVS_CGBN_PREDICT_CLASS (2), a discrete target t with r = card[t] levels given every other variable.  prior: null or device
 *     f64 [n_rows][r], the posterior of t over its discrete Markov blanket (null counts as all ones).  For k = 0 .. r - 1:
 *       a_k = log(prior_k)   (+0 for a null prior);  then for every continuous child c of t ascending, z the configuration of c in
 *       the row with t's level set to k and e as in the log-likelihood:  a_k = a_k - (c_{c,z} + 0.5 * (e * e))
 *     M = the largest a_k;  w_k = exp(a_k - M);  W = +0, then W = W + w_k for k ascending;  posterior (null or device f64
 *     [n_rows][r]) = w_k / W;  pred (device u8 [n_rows]) = the lowest k with a_k = M.  When any a_k is NaN, pred is 255 and the
 *     row of posterior is NaN.  var is not read.  The computation is in the log domain on purpose: the product of 47 Gaussian
 *     factors underflows in the linear domain.
 * With every variable continuous, modes 0 and 1 give dvs_gbn_predict's pred bytes.
 * workspace: a header of 256 bytes, then c f64 [n_cells]; dvs_cgbn_predict_workspace_bytes gives the size.
 * Checked before anything is enqueued, in this order: n_rows and n_cells as above (2), n_vars and n_cont (3), mode 0, 1 or 2 (12),
 * target in [0, n_vars) (13), null pointers (10; prior and posterior may be null; var may be null in mode 2), workspace_bytes (14
 * with the needed size).  A target of the wrong kind for the mode (card[target] > 0 in modes 0 and 1, = 0 in mode 2) is seen on
 * the device, where card lives: bit 4 of status and NaN / 255 everywhere, like a malformed network. */
#ifndef DVS_MIXED_PARAMS_H
#define DVS_MIXED_PARAMS_H

#include "dvs_mixed.h"

#define DVS_CGBN_PREDICT_PARENTS 0
#define DVS_CGBN_PREDICT_EXACT 1
#define DVS_CGBN_PREDICT_CLASS 2

#ifdef __cplusplus
extern "C" {
#endif

size_t dvs_cgbn_sample_workspace_bytes(int32_t n_vars);

int dvs_cgbn_sample(int32_t n_vars, int32_t n_cont, int64_t n_rows, int64_t n_cells, const uint8_t* card, const uint64_t* parents,
                    const int64_t* offset, const double* coef, const double* intercept, const double* sd, const uint64_t* packed,
                    uint64_t seed, int64_t row_offset, void* workspace, size_t workspace_bytes, double* x_out, int32_t* status,
                    void* stream);

size_t dvs_cgbn_loglik_workspace_bytes(int32_t n_vars, int64_t n_rows, int64_t n_cells);

int dvs_cgbn_loglik(int32_t n_vars, int32_t n_cont, int64_t n_rows, int64_t n_cells, const uint8_t* card, const uint64_t* parents,
                    const int64_t* offset, const double* coef, const double* intercept, const double* sd, const uint64_t* packed,
                    const double* x, double* per_row, double* out, void* workspace, size_t workspace_bytes, int32_t* status,
                    void* stream);

size_t dvs_cgbn_predict_workspace_bytes(int32_t n_vars, int64_t n_cells);

int dvs_cgbn_predict(int32_t n_vars, int32_t n_cont, int64_t n_rows, int64_t n_cells, const uint8_t* card, const uint64_t* parents,
                     const int64_t* offset, const double* coef, const double* intercept, const double* sd, const uint64_t* packed,
                     const double* x, int32_t target, int32_t mode, const double* prior, void* pred, double* var, double* posterior,
                     void* workspace, size_t workspace_bytes, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
