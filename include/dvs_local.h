/* dvs_local.h — fourth companion header of dvs.h: local (per-target) constraint-based structure learning on discrete data
 * (DESIGN.md §27): conditional-independence tests grouped by (target, conditioning set), and the decisions of one round of
 * MMPC, the max-min parents and children search of Tsamardinos, Brown and Aliferis (2006).  dvs.h, dvs_eliminate.h,
 * dvs_incomplete.h and dvs_available.h stay what they are and DVS_VERSION stays 202: a pure addition.
 *
 * ---- dvs_ci_tests_group ----------------------------------------------------------------------------------------------------
 * Group g tests every variable x whose bit is set in candidates[g] against y = target[g] given the variables whose bits are set
 * in cond[g].  data, card, test_type and the statistics are those of dvs_ci_tests (dvs.h).
 * out device f64 [n_groups][n_vars][3], written whole.  Cell [g][x] of an x in candidates[g] is (statistic, df, p-value), byte
 * for byte what dvs_ci_tests writes for the test (x, y | Z) with the same test_type; the table of a test is laid out as there,
 * (key * r_x + level_x) * r_y + level_y.  Cell [g][x] of an x that is not in candidates[g] is three NaNs and sets no status bit.
 * Refusals.  A candidate is refused — three NaNs, bit 4 of status — by the rules of dvs_ci_tests: x = y, x in Z, y in Z, y or a
 * bit of Z outside [0, n_vars), a level count of 0, a table of more than lds_cells cells.  The last rule is decided candidate
 * by candidate.  A bit of candidates[g] at or above n_vars has no cell and sets bit 4.
 * lds_cells in [1, 36 864] is the launch's dynamic LDS in u32 counters.  One 256-thread workgroup owns a group; it takes the
 * group's accepted candidates in ascending order in passes, a pass holding as many consecutive tables as fit, and scans the
 * rows once per pass: one mixed-radix key per row, one integer LDS atomic per candidate of the pass.  Counts are integers and
 * the sums of a statistic are taken in the order of dvs_ci_tests, so the bytes depend neither on lds_cells (beyond the
 * refusals) nor on the number of passes, and two calls give equal bytes.
 * Checked before anything is enqueued, in this order: n_groups and n_samples > 0 (2), n_vars in [1, 48] (3), test_type (12),
 * lds_cells in [1, 36864] (13), n_groups * n_vars < 2^31 (2), null pointers (10), out_bytes < n_groups * n_vars * 24 (14 with
 * that size).
 *
 * ---- dvs_mmpc_update -------------------------------------------------------------------------------------------------------
 * What a round of grouped tests decides, for all n_vars targets in lock-step.  One wave per target t, lane = candidate x.
 * State (device): cpc u64 [n] the members so far, cand u64 [n] the candidates still open, last i32 [n] the member added last
 * or -1 when the target has finished, pmax f64 [n][n] (start: 0) the largest p-value seen of (t, x), smin f64 [n][n] (start:
 * +inf) the smallest statistic seen, sepset u64 [n][n] (cell [t][x]: the conditioning set that separated x from t).
 * The round: target, cond, candidates [n_groups] as given to dvs_ci_tests_group, out its output, group_offsets i64 [n + 1]: the
 * groups of target t are group_offsets[t] .. group_offsets[t + 1] - 1 (clamped to [0, n_groups]), walked in that order.
 * phase = 0, forward.  For a lane x in cand[t] and in the group's candidates that has not left in this round: a NaN p-value is
 * counted as refused and changes nothing; p > alpha: x leaves cand for good, sepset[t][x] = the group's cond, later groups of
 * the round are ignored for x; otherwise pmax = max(pmax, p), smin = min(smin, statistic).  Then F is the member left in cand
 * with the smallest pmax, values below 2^-1022 taken as 0; ties go to the largest smin, then to the lowest index.  With an F:
 * cpc_next = cpc | F, cand_next = cand without F and without those that left, last = F.  Without: last = -1.
 * phase = 1, backward.  cand is not used (cand_next = cand) and last, pmax, smin are not written.  A lane x in cpc[t] and in
 * the group's candidates with p > alpha leaves: cpc_next = cpc without those, sepset[t][x] = the first such group's cond.
 * Outputs: cpc_next, cand_next u64 [n], written whole, which may not alias cpc and cand; refused i32 [1], written: the NaN
 * cells counted; result i64 [n][2]: (F or -1, the candidates that left in this round).  Integers and comparisons only: two
 * calls give equal bytes.
 * Checked in this order: n_vars in [1, 48] (3), n_groups > 0 and n_groups * n_vars < 2^31 (2), phase 0 or 1 (13), alpha in
 * [0, 1] (13), null pointers (10), out_bytes < n_groups * n_vars * 24, state_bytes < n_vars^2 * 8 (what each of pmax, smin and
 * sepset holds), result_bytes < n_vars * 16 (14 with the needed size). */
#ifndef DVS_LOCAL_H
#define DVS_LOCAL_H

#include "dvs.h"

#ifdef __cplusplus
extern "C" {
#endif

int dvs_ci_tests_group(int32_t n_groups, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                       const int32_t* target, const uint64_t* cond, const uint64_t* candidates, int32_t test_type,
                       int32_t lds_cells, double* out, size_t out_bytes, int32_t* status, void* stream);

int dvs_mmpc_update(int32_t n_vars, int32_t n_groups, int32_t phase, const int32_t* target, const uint64_t* cond,
                    const uint64_t* candidates, const int64_t* group_offsets, const double* out, size_t out_bytes, double alpha,
                    const uint64_t* cpc, const uint64_t* cand, uint64_t* cpc_next, uint64_t* cand_next, int32_t* last,
                    double* pmax, double* smin, uint64_t* sepset, size_t state_bytes, int32_t* refused, int64_t* result,
                    size_t result_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
