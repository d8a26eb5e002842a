/* dvs_incomplete.h — second companion header of dvs.h: learning from incomplete data on a fitted discrete Bayesian network
 * (DESIGN.md §25): the expected counts of one EM step, the tables from such counts, and exact imputation, all on the step
 * executor of dvs_bn_eliminate (include/dvs_eliminate.h, whose plan words, limits and conventions apply).  dvs.h and
 * dvs_eliminate.h stay what they are and DVS_VERSION stays 202: a pure addition.
 *
 * ONE network: card, parents, offsets, cpt, n_cells as for dvs_bn_eliminate (the cell of level k of variable v under the parent
 * configuration key is cpt[offsets[v] + key * r + k], key mixed-radix with the lowest parent id fastest).  Arrays "in the CPT
 * layout" (counts, cpt_out) hold n_cells cells and the cell of cpt[offsets[v] + i] is their cell offsets[v] - offsets[0] + i.
 *
 * Incomplete data is (data, observed): data device u64 [n_rows][ceil(n_vars / 16)] packed 4-bit levels as everywhere in dvs.h,
 * observed device u64 [n_rows], bit v set <=> variable v is observed in that row; the nibble of an unobserved variable is
 * ignored.  The level masks of row r are built on the fly: an observed variable has the one bit of its level, an unobserved one
 * 0xFFFF.
 *
 * ---- dvs_bn_expected_counts: the E-step ------------------------------------------------------------------------------------
 * plans / plan_offsets: n_vars + 1 plans in the words of dvs_bn_eliminate.  Plan v keeps exactly the family of v, {v} and its
 * parents; plan n_vars keeps nothing (the evidence plan).  plan_words, arena_cells, out_cells and step_cells are the caller's
 * statements about them: the longest plan, the largest arena, the largest last step and the largest step output; a plan beyond
 * plan_words, arena_cells or out_cells is malformed.  The arena and the last step's cells of a row both live in LDS:
 * arena_cells + out_cells <= DVS_BN_ELIM_MAX_CELLS.
 *
 * row_z[r] (device f64 [n_rows]): z of the evidence plan on row r, computed exactly as dvs_bn_eliminate defines z (its one
 * cell); NaN for a row whose observed has a bit at or above n_vars or whose observed level is at or above its variable's level
 * count.  ok(r) <=> neither of those, and row_z[r] is finite and > 0.  A row that is not ok adds to nothing; it is counted in
 * skipped (device i64 [1]), and bit 4 of status is set for a bad level or bit, bit 7 for z = 0 or a z that is not finite
 * (information, as bit 7 of dvs_bn_lw is).
 *
 * counts (device f64 [n_cells], the CPT layout): for family v and cell j = key * r + k
 *   I_j    the integer number of ok rows in which the whole family is observed and whose levels index j;
 *   F_j    rows are cut into chunks of 256 (chunk c: rows 256 c .. 256 c + 255).  F_{c,j} starts at +0; for the ok rows of the
 *          chunk in ascending order whose family is not wholly observed, with out and z of plan v on that row (z the fixed tree
 *          over out): if z is finite and > 0, F_{c,j} += out[cell] / z — one division, then one addition, contraction off —
 *          where cell is j's place in the plan's lowest-id-fastest layout; otherwise nothing is added and bit 7 is set.
 *          F_j is the library's tree over the chunk values: slot t of 256 adds chunks t, t + 256, ... ascending from +0, then
 *          x[i] += x[i + s] for s = 128, 64, ..., 1.
 *   counts_j = (double)I_j + F_j, one addition.
 * Integer atomics count I; there are no floating-point atomics: two calls give equal bytes, and the bytes do not depend on
 * rows_per_group or on the launch geometry.
 *
 * loglik (device f64 [1]): the log-likelihood of the incomplete data, the sum over ok rows of log(row_z[r]) in the order of
 * dvs_bn_loglik (per chunk of 256 rows x[i] += x[i + s], s = 128 .. 1; then slot t adds the chunks t, t + 256, ... and the same
 * tree); a row that is not ok counts +0.
 *
 * Before anything of a plan is executed it is checked as dvs_bn_eliminate checks it, and in addition: the kept variables of
 * plan v < n_vars are exactly {v} and the parents of v and its out_cells are the q * r cells of v's table; plan n_vars keeps
 * nothing and has one cell.  (The kept list and the last step's scope are separate words: without the second test a last step
 * over more variables would leave the table.)  As for dvs_bn_eliminate, no words can make a kernel read or write out of
 * bounds.  A malformed family plan sets bit 4 and plan_flags[v] = 1 (device i32 [n_vars + 1], written); the counts of that
 * family are NaN and the other families are what they are without it.  A malformed evidence plan, or network (then every plan is flagged), leaves no row ok: counts, row_z and
 * loglik are NaN and skipped = n_rows.
 *
 * rows_per_group: 0 selects the rule of dvs_bn_eliminate, G = clamp(1024 / step_cells, 1, 64); either is then limited so that
 * G arenas, G last steps, the plan words and G mask rows fit the LDS of a workgroup.
 *
 * workspace: dvs_bn_expected_counts_workspace_bytes(n_cells, n_vars, n_rows) bytes (0: refused), contents unspecified on entry.
 *
 * Checked before anything is enqueued, in this order: n_vars in [1, 48] (3), n_cells in [n_vars, 2^31 - 1] (2), n_rows in
 * [1, 2^31 - 1] and ceil(n_rows / 256) * n_cells < 2^40 (2), plan_words in [7, DVS_BN_ELIM_MAX_WORDS] (12), arena_cells,
 * out_cells and step_cells in [1, DVS_BN_ELIM_MAX_CELLS] (12), arena_cells + out_cells <= DVS_BN_ELIM_MAX_CELLS (12),
 * rows_per_group in [0, 64] (12), null pointers (10), plans_bytes < (n_vars + 1) * 28 (14 with that size), workspace_bytes
 * below the workspace function's value (14 with that size).
 *
 * ---- dvs_bn_fit_counts: the M-step -----------------------------------------------------------------------------------------
 * counts (device f64 [n_cells], the CPT layout) -> cpt_out (the same layout).  N_j is the sum of N_jk over k ascending from +0.
 *   DVS_FIT_MLE    theta = N_jk / N_j; N_j = 0 gives NaN, or 1 / r with unobserved = 1.
 *   DVS_FIT_BAYES  theta = (N_jk + a) / (N_j + r * a) with a = iss / (r * q); the operations in exactly that order, none fused.
 * This is the arithmetic of dvs_bn_fit: on integer counts the bytes are those of dvs_bn_fit.  A family whose table does not lie
 * in offsets[0] .. offsets[0] + n_cells with q * r cells, or that holds a negative or non-finite count, sets bit 4 of status
 * and is NaN (every cell of its slot where the slot itself is sound, nothing where it is not).
 * Checked in this order: n_vars (3), n_cells (2), method is a dvs_fit_method (12), iss finite and > 0 with DVS_FIT_BAYES (13),
 * unobserved 0 or 1 (12), null pointers (10).
 *
 * ---- dvs_bn_impute: exact single imputation --------------------------------------------------------------------------------
 * n_vars plans, plan v keeping exactly {v} with out_cells = the level count of v (else malformed).  For row r and a variable v
 * it does not observe: out and z of plan v on that row; the level is the lowest k that maximises out[k] (no division; ties go to the lowest level, as dvs_bn_blanket_posterior
 * predicts; bnlearn breaks them at random).  The variable stays missing when the row has a bad level or observed bit (bit 4),
 * when plan v is malformed (bit 4, plan_flags[v] = 1), or when that z is not finite and > 0 (bit 7): its nibble is 0 and its bit
 * in observed_out is clear.  There is no evidence plan in this call: the z that decides is the z of plan v, which is P(evidence)
 * as well.  Observed nibbles are copied, every word of data_out (device u64 [n_rows][ceil(n_vars / 16)]) is written with zero
 * above n_vars, and observed_out[r] (device u64 [n_rows]) is observed[r] or-ed with the imputed bits.
 * workspace: dvs_bn_impute_workspace_bytes(n_vars, n_rows) bytes: the levels u8 [n_rows][n_vars], packed by a last kernel so
 * that no two workgroups write one word.
 * Checked in this order: n_vars (3), n_cells (2), n_rows in [1, 2^31 - 1] (2), plan_words (12), arena_cells and step_cells in
 * [1, DVS_BN_ELIM_MAX_CELLS] (12), arena_cells + 16 <= DVS_BN_ELIM_MAX_CELLS (12), rows_per_group in [0, 64] (12), null
 * pointers (10), plans_bytes < n_vars * 28 (14), workspace_bytes (14).
 *
 * Soft EM with exact expected counts is dvs_bn_expected_counts then dvs_bn_fit_counts, repeated; bnlearn's hard EM is impute
 * then fit.  Parity with bnlearn's `impute` and `bn.fit` on incomplete data is unpinned against an R run. */
#ifndef DVS_INCOMPLETE_H
#define DVS_INCOMPLETE_H

#include "dvs.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t dvs_bn_expected_counts_workspace_bytes(int64_t n_cells, int32_t n_vars, int64_t n_rows);

int dvs_bn_expected_counts(int32_t n_vars, int64_t n_rows, const uint8_t* card, const uint64_t* parents, const int64_t* offsets,
                           const double* cpt, int64_t n_cells, const int32_t* plans, size_t plans_bytes,
                           const int64_t* plan_offsets, int32_t plan_words, int32_t arena_cells, int32_t out_cells,
                           int32_t step_cells, const uint64_t* data, const uint64_t* observed, int32_t rows_per_group,
                           double* counts, double* row_z, double* loglik, int64_t* skipped, int32_t* plan_flags, void* workspace,
                           size_t workspace_bytes, int32_t* status, void* stream);

int dvs_bn_fit_counts(int32_t n_vars, const uint8_t* card, const uint64_t* parents, const int64_t* offsets, const double* counts,
                      int64_t n_cells, int32_t method, double iss, int32_t unobserved, double* cpt_out, int32_t* status,
                      void* stream);

size_t dvs_bn_impute_workspace_bytes(int32_t n_vars, int64_t n_rows);

int dvs_bn_impute(int32_t n_vars, int64_t n_rows, const uint8_t* card, const uint64_t* parents, const int64_t* offsets,
                  const double* cpt, int64_t n_cells, const int32_t* plans, size_t plans_bytes, const int64_t* plan_offsets,
                  int32_t plan_words, int32_t arena_cells, int32_t step_cells, const uint64_t* data, const uint64_t* observed,
                  int32_t rows_per_group, uint64_t* data_out, uint64_t* observed_out, int32_t* plan_flags, void* workspace,
                  size_t workspace_bytes, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
