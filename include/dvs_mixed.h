/* dvs_mixed.h — ninth companion header of dvs.h: conditional Gaussian networks on data sets that hold factors and real columns
 * (DESIGN.md §32): the rows of a data set partitioned by the configuration of a set D of discrete variables, the moments of the
 * real columns of every configuration, bnlearn's mixed-data scores loglik-cg, aic-cg and bic-cg from those moments, and the
 * single-edge toggle pass over them.  dvs.h and the eight companion headers before this one stay what they are and
 * DVS_VERSION stays 202: a pure addition.
 *
 * Arithmetic.  Everything is IEEE fp64, one rounded operation at a time: no fused multiply-add anywhere, no floating-point
 * atomics, every sum in the order stated here.  Two calls give equal bytes.
 *
 * The data set.  n_vars <= 48 variables.  card: device u8 [n_vars]; card[v] in 1 .. 16 is the level count of a discrete
 * variable, card[v] = 0 marks a continuous one.  data: device u64 [n_samples][ceil(n_vars / 16)], the packed level codes of
 * dvs_bn_scores (the nibble of a continuous variable is not read; a code at or above its level count counts as the top level).
 * x: device f64 [n_samples][n_cont], the continuous columns in ascending variable order; n_cont is the number of zeros in card.
 * A discrete variable takes discrete parents only.  A continuous variable v takes discrete parents D (q = the product of their
 * level counts, 1 for none) and continuous parents G, p = |G| <= DVS_GBN_MAX_PARENTS: one linear regression on G for every
 * configuration of D.
 *
 * ---- dvs_cg_partition -----------------------------------------------------------------------------------------------------------
 * masks: device u64 [n_requests], each a set D.  A request is refused (bit 4 of status, count[r][0] = -1, nothing else of the
 * request written) when a bit of D is at or above n_vars or names a continuous variable, or when q > q_pitch; q_pitch itself
 * must lie in [1, DVS_CG_MAX_CONFIGS] (4096: three 16-level parents; a choice, not a measurement).  The configuration of a row
 * is the mixed-radix number of its levels over D, the lowest variable id fastest (the key of the CPT layout of dvs_bn_fit).
 *   count: device i32 [n_requests][q_pitch]   count[r][z] = the rows of configuration z (0 for q <= z < q_pitch)
 *   start: device i32 [n_requests][q_pitch]   the exclusive prefix of count[r]
 *   order: device i32 [n_requests][n_samples] the row indices sorted by (configuration, row index): a stable sort, which has
 *                                             exactly one result; how it is computed (integer atomics included) is free
 * Checked before anything is enqueued, in this order: n_requests, n_samples > 0 (2), n_vars in [1, 48] (3), q_pitch (13),
 * n_requests * max(q_pitch, n_samples) < 2^31 (2), null pointers (10), count_bytes < n_requests * q_pitch * 4 and order_bytes <
 * n_requests * n_samples * 4 (14 with the needed size).
 *
 * ---- dvs_cg_moments, dvs_cg_moments_workspace_bytes --------------------------------------------------------------------------
 * count, start, order: as dvs_cg_partition wrote them.  moments: device f64 [n_requests][q_pitch][DVS_GBN_STRIDE(n_cont)].  Block
 * (r, z) is, as bytes, what dvs_gbn_moments (include/dvs_gaussian.h) writes for the row set order[r][start[z] : start[z] +
 * count[z]] of x: chunks of DVS_GBN_CHUNK consecutive positions of that segment, two passes, the orders of that header.  An empty
 * configuration (and every z at or above q) has m = 0 and +0 everywhere else.  A refused request has m = NaN in its block 0 and
 * empty blocks otherwise.  workspace_bytes = 8 * ceil((q_pitch + 1) / 2) * n_requests + 8 * n_requests * slots * (n + n (n + 1)
 * / 2), slots = ceil(n_samples / DVS_GBN_CHUNK) + q_pitch (a bound on the chunks of one request), n = n_cont; 0 is a refusal.
 * Checks: n_requests, n_samples > 0 (2), n_cont in [1, 48] (3), q_pitch (13), n_requests * slots * n (n + 1) / 2 and n_requests
 * * q_pitch * n (n + 1) / 2 < 2^31 (2), null pointers (10), workspace_bytes, then moments_bytes (14 with the needed size).
 *
 * ---- dvs_cg_scores, dvs_cg_scores_workspace_bytes -------------------------------------------------------------------------------
 * parents: device u64 [batch][n_vars], bit u of parents[b][v] <=> u -> v (the self bit is ignored).  tables: device u64
 * [n_tables], each the device address of the moment blocks [q][DVS_GBN_STRIDE(n_cont)] of one set D (a request of
 * dvs_cg_moments; blocks of one table are contiguous); table_of: device i32 [batch][n_vars], the table of the discrete parents
 * of family (b, v), read for a continuous v only, -1 = none (the family is refused); NOT range checked on the device.  The
 * caller vouches that table_of names the table of D = parents[b][v] restricted to the discrete variables.  tables and table_of
 * may be null when n_cont = 0.  local: device f64 [batch][n_vars]; out: device f64 [batch], local added over v ascending from
 * +0; status: device i32, zeroed by the caller.
 * A continuous v, with a_0 < ... < a_(p-1) the continuous parents as columns of x:
 *   for every configuration z with m_z > 0, in ascending z: the row-wise Cholesky of C_z[G + v] of include/dvs_gaussian.h;
 *     dof_z = m_z - p - 1;  s2_z = RSS_z / dof_z;  LL_z = -(0.5 * m_z) * log(6.283185307179586 * s2_z) - 0.5 * dof_z
 *   LL starts at +0 and adds LL_z in ascending z (one lane; no tree);  local = LL - (k * q) * (p + 2)
 * q counts empty configurations too.  k = 0 for DVS_CGSCORE_LOGLIK, score_arg >= 0 (default 1) for DVS_CGSCORE_AIC and score_arg
 * >= 0 (default log(n_samples) / 2, taken on the device) for DVS_CGSCORE_BIC; NaN asks for the default and is what loglik takes.
 * With every variable continuous the bytes are dvs_gbn_scores' (loglik-g, aic-g, bic-g) on the moments of all rows.
 * Refusals, NaN in local[b][v] and bit 4 of status while the other families are scored: a parent bit at or above n_vars; q >
 * DVS_CG_MAX_CONFIGS; table_of < 0; p > DVS_GBN_MAX_PARENTS; a non-empty configuration with dof_z < 1; a pivot failing the pivot
 * rule of include/dvs_gaussian.h in some configuration.
 * A discrete v: a continuous parent bit is a refusal (the illegal arc); otherwise local[b][v] is, as bytes, local of
 * dvs_bn_scores (loglik / aic / bic with the same score_arg) on the same packed rows: the entry point runs that scorer on a copy
 * of the structures held in workspace and overwrites the other cells.  workspace_bytes = 8 * batch * n_vars + 64.
 * Three things follow bnlearn as recalled and are unpinned against an R run: the unbiased variance RSS_z / (m_z - p - 1) of
 * every configuration, the parameter count q (p + 2), and the treatment of sparse configurations (an empty one adds nothing to
 * LL and counts in q; one with 1 .. p + 1 rows refuses the family).
 * Checked before anything is enqueued, in this order: batch, n_samples > 0 (2), n_vars in [1, 48] and n_cont in [0, n_vars]
 * (3), score_type (12), score_arg (13), null pointers (10), workspace_bytes (14 with the needed size).  n_cont differing from
 * the zeros of card refuses every family on the device.
 *
 * ---- dvs_cg_toggle_scores, dvs_cg_toggle_workspace_bytes ------------------------------------------------------------------------
 * toggles[b][v][u] (device f64 [batch][n][n]) is, as bytes, local[v] of dvs_cg_scores on the structure with bit u of
 * parents[b][v] flipped; NaN on the diagonal, where that family is refused (bit 4 of status), and on every cell with a discrete
 * v and a continuous u (the illegal arc: no status bit, the move is not available).  local[b][v] is that call's bytes too.
 * worklist null: all rows, table_of device i32 [batch * n][n].  worklist device i32 [2 * batch]: slots 2b and 2b + 1 name the
 * rows of structure b to recompute, -1 = none; only those rows of toggles are written, local is left to dvs_hc_step, and
 * table_of is device i32 [2 * batch][n] by slot.  table_of[row][u] is the table of the flipped family's D; for a continuous u
 * (and u = v) that is the table of D as it stands.  workspace_bytes = 8 * batch * n_vars + 64 + 8 * batch.  Checks: those of
 * dvs_cg_scores with batch * n_vars^2 < 2^31 (2) next to n_vars, then local_bytes < batch * n_vars * 8 and toggles_bytes < batch
 * * n_vars^2 * 8 (14 with the needed size).
 *
 * ---- dvs_cg_fit -----------------------------------------------------------------------------------------------------------------
 * n_families continuous families in a flat layout.  var: device i32 [n_families] the variable, parents: device u64
 * [n_families] its parent mask, table: device u64 [n_families] the address of the table of its D, offset: device i64
 * [n_families + 1] the exclusive prefix of the families' q (the caller vouches for it).  One lane per (family, configuration):
 * the factor of dvs_cg_scores, then the backward solve of dvs_gbn_fit.  coef: device f64 [offset[n_families]][n_vars], the
 * coefficient of every continuous parent at its variable id and 0 elsewhere; intercept, sd, count: device f64
 * [offset[n_families]], as dvs_gbn_fit defines them on the configuration's block, count = m_z.  An empty configuration has NaN
 * in coef, intercept and sd and count 0 (no status bit).  A refused (family, configuration) has NaN as well and sets bit 4; a
 * discrete variable or a refused D refuses every configuration of the family.  n_cells = offset[n_families] as the host knows
 * it.  Checks: n_families, n_cells > 0 (2), n_vars and n_cont (3), n_cells * n_vars < 2^31 (2), null pointers (10), coef_bytes <
 * n_cells * n_vars * 8 (14 with the needed size). */
#ifndef DVS_MIXED_H
#define DVS_MIXED_H

#include "dvs_gaussian.h"

#define DVS_CG_MAX_CONFIGS 4096

#ifdef __cplusplus
extern "C" {
#endif

typedef enum dvs_cgscore_type {
    DVS_CGSCORE_LOGLIK = 0,
    DVS_CGSCORE_AIC = 1,
    DVS_CGSCORE_BIC = 2
} dvs_cgscore_type;

int dvs_cg_partition(int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card, int32_t n_requests,
                     const uint64_t* masks, int32_t q_pitch, int32_t* count, size_t count_bytes, int32_t* start, int32_t* order,
                     size_t order_bytes, int32_t* status, void* stream);

size_t dvs_cg_moments_workspace_bytes(int32_t n_cont, int32_t n_samples, int32_t n_requests, int32_t q_pitch);

int dvs_cg_moments(int32_t n_cont, int32_t n_samples, const double* x, int32_t n_requests, int32_t q_pitch, const int32_t* count,
                   const int32_t* start, const int32_t* order, void* workspace, size_t workspace_bytes, double* moments,
                   size_t moments_bytes, void* stream);

size_t dvs_cg_scores_workspace_bytes(int32_t batch, int32_t n_vars);

int dvs_cg_scores(int32_t batch, int32_t n_vars, int32_t n_cont, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                  const uint64_t* tables, const int32_t* table_of, const uint64_t* parents, int32_t score_type, double score_arg,
                  void* workspace, size_t workspace_bytes, double* local, double* out, int32_t* status, void* stream);

size_t dvs_cg_toggle_workspace_bytes(int32_t batch, int32_t n_vars);

int dvs_cg_toggle_scores(int32_t batch, int32_t n_vars, int32_t n_cont, int32_t n_samples, const uint64_t* data,
                         const uint8_t* card, const uint64_t* tables, const int32_t* table_of, const uint64_t* parents,
                         int32_t score_type, double score_arg, const int32_t* worklist, void* workspace, size_t workspace_bytes,
                         double* local, size_t local_bytes, double* toggles, size_t toggles_bytes, int32_t* status, void* stream);

int dvs_cg_fit(int32_t n_families, int32_t n_cells, int32_t n_vars, int32_t n_cont, const uint8_t* card, const int32_t* var,
               const uint64_t* parents, const uint64_t* table, const int64_t* offset, double* coef, size_t coef_bytes,
               double* intercept, double* sd, double* count, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
