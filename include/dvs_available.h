/* dvs_available.h — third companion header of dvs.h: available-case scoring of discrete Bayesian networks on incomplete data
 * (DESIGN.md §26): the node-average likelihood `nal` and its penalised form `pnal` (Balov 2013; Bodewes and Scutari 2021),
 * which score a family on exactly the rows in which that family is wholly observed and divide by their number.  The score is
 * decomposable, so dvs_hc_step / dvs_tabu_step run on its tables unchanged.  dvs.h, dvs_eliminate.h and dvs_incomplete.h stay
 * what they are and DVS_VERSION stays 202: a pure addition.
 *
 * Incomplete data is the pair (data, observed) of dvs_incomplete.h: data device u64 [n_samples][ceil(n_vars / 16)] packed 4-bit
 * levels, observed device u64 [n_samples], bit v set <=> variable v is observed in that row.  The nibble of an unobserved
 * variable is ignored; bits of observed at or above n_vars are ignored.  The level code of an observed variable must be below
 * its level count, as for dvs_bn_scores (not checked).
 *
 * ---- definitions -----------------------------------------------------------------------------------------------------------
 * Family mask.  For variable v under the parent mask P (parents[b][v] with v's own bit masked off; in the toggle pass with bit u
 * flipped first), F = bit(v) | P.
 * Rows that count.  Row s counts for the family iff (observed[s] & F) == F.  m is the number of such rows.
 * Counts and log-likelihood.  N_jk and N_j are the counts over those rows only, LL = sum N_jk log(N_jk / N_j) in exactly the
 * summation order of dvs_bn_scores with DVS_SCORE_LOGLIK on the data set of those m rows (any order: the counts do not depend on
 * it): LL is, as bytes, local[v] of that call.
 * Local score.  local = LL / m - (k * (r - 1)) * q, r the level count of v and q the product of its parents' level counts (a
 * double): one division, then the two products in that order, then one subtraction, none fused — the bytes of the same
 * expression in IEEE binary64.
 * k is passed as given and must be finite and >= 0.  nal is k = 0.  The library has no default: bnlearn's pnal default, as far as
 * recalled n_samples ^ -0.25 (the alpha = 1/4 of Bodewes and Scutari), is the caller's to compute; parity with bnlearn's nal /
 * pnal is unpinned against an R run.
 * m = 0.  The local score is -inf and bit 7 of status is set (information, as bit 7 of dvs_bn_lw is; not bit 4); used is 0.  A
 * move into such a family is never taken by dvs_hc_step, which needs delta > min_delta.
 * Refusals.  A family is refused (NaN, bit 4 of status, used 0) by the rules of dvs_bn_scores decided on n_samples, not on m: a
 * table beyond 36 864 cells with more than 16 384 samples, keys beyond 63 bits, a parent bit at or above n_vars.
 * Total.  out[b] is the sum of local[b][v] over v ascending from +0, as dvs_bn_scores adds it.
 * Integer atomics only: two calls give equal bytes.
 *
 * ---- dvs_bn_scores_avail ---------------------------------------------------------------------------------------------------
 * batch structures: parents device u64 [batch][n_vars] -> local device f64 [batch][n_vars], out device f64 [batch], used device
 * i32 [batch][n_vars] (m per family) or null, status device i32 [1] (or-ed into).
 * Checked before anything is enqueued, in this order: batch and n_samples > 0 (2), n_vars in [1, 48] (3), null pointers
 * (data, observed, card, parents, local, out, status: 10), k finite and >= 0 (13).
 *
 * ---- dvs_bn_toggle_scores_avail --------------------------------------------------------------------------------------------
 * The semantics of dvs_bn_toggle_scores: toggles[b][v][u] is the local score of v with bit u of parents[b][v] flipped, NaN on
 * the diagonal; local[b][v] the local score as it stands.  worklist null: a full pass; else i32 [2 batch] and only the rows it
 * names are written (slots 2 b and 2 b + 1 belong to structure b and hold a variable index, or anything outside [0, n_vars) for
 * none; local is not written in a worklist pass).  A cell is, as bytes, local[v] of dvs_bn_scores_avail on the structure with
 * that bit flipped.
 * Checked in this order: batch and n_samples > 0 (2), n_vars in [1, 48] (3), batch * n_vars^2 < 2^31 (2), null pointers (10), k
 * (13), local_bytes < batch * n_vars * 8 (14 with that size), toggles_bytes < batch * n_vars^2 * 8 (14 with that size). */
#ifndef DVS_AVAILABLE_H
#define DVS_AVAILABLE_H

#include "dvs.h"

#ifdef __cplusplus
extern "C" {
#endif

int dvs_bn_scores_avail(int32_t batch, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint64_t* observed,
                        const uint8_t* card, const uint64_t* parents, double k, double* local, double* out, int32_t* used,
                        int32_t* status, void* stream);

int dvs_bn_toggle_scores_avail(int32_t batch, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint64_t* observed,
                               const uint8_t* card, const uint64_t* parents, double k, const int32_t* worklist, double* local,
                               size_t local_bytes, double* toggles, size_t toggles_bytes, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
