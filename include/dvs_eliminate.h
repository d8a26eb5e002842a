/* dvs_eliminate.h — companion header of dvs.h: exact inference on a fitted discrete Bayesian network by bucket (variable)
 * elimination.  dvs.h stays the statement of the 64 entry points it has; what was added beside them is
 * declared here, in the same conventions (plain pointers and sizes, "device" memory owned by the caller, work enqueued on the
 * passed stream, return codes and dvs_last_error as in dvs.h).  DVS_VERSION stays 202: a pure addition.
 *
 * dvs_bn_eliminate: ONE network (card, parents, offsets, cpt, n_cells as for dvs_bn_lw; the CPT layout of dvs.h: the cell of
 * level k of variable v under the parent configuration key is cpt[offsets[v] + key * r + k], key mixed-radix with the lowest
 * parent id fastest), n_plans elimination plans and n_rows mask rows.  Every (plan, row) pair is computed.
 *
 * masks: device u16 [n_rows][n_vars]; bit k of masks[row][v] set <=> level k of variable v is allowed in that row.  An observed
 * variable has one bit set, an unconstrained one 0xFFFF; bits at or above card[v] are ignored; an empty allowed set is no error
 * (every term it would have summed is absent, so the sums are +0).
 *
 * A plan is a sequence of int32 words; plans (device i32, plans_bytes bytes) holds all of them, plan p being the words
 * plan_offsets[p] .. plan_offsets[p + 1] - 1 (plan_offsets: device i64 [n_plans + 1]).  The words of one plan:
 *   header   DVS_BN_ELIM_TAG, n_vars, n_steps, arena_cells, out_cells, n_keep, then the n_keep kept variables in ascending id
 *   step     x, out_offset, out_cells, n_scope, n_inputs, then the n_scope variables of the output scope in ascending id, then
 *            per input 4 + n_scope words: kind, offset, cells, stride_x, and one stride per scope variable (0 where the input
 *            does not hold it).
 * A factor is an array of fp64 cells over a scope, lowest variable id fastest.  kind = v >= 0: the table of variable v (offset
 * and cells are not read: the span is offsets[v] .. offsets[v + 1]); kind = -1: the span offset .. offset + cells - 1 of the
 * row's arena, which holds arena_cells fp64 cells and lives in LDS.  Every step but the last eliminates its x in [0, n_vars):
 * for every cell c of the output, decoded into one level l_i per scope variable (c = l_0 + card_0 * (l_1 + card_1 * ...)),
 *     acc = +0;  for k = 0, 1, ..., card[x] - 1 with bit k of masks[row][x] set:
 *         p = in_0[at_0];  p = p * in_1[at_1];  ... in the order of the inputs;   acc = acc + p
 *     with at_j = k * stride_x_j + sum_i l_i * stride_j_i,
 * and acc goes to cell out_offset + c of the arena.  The last step has x = -1 and out_offset = -1: it multiplies what is left
 * into the caller's out, one term per cell (k does not exist, stride_x is not read), and a cell with a level that the row's
 * mask does not allow for its scope variable is +0.  All of it is fp64 in the linear domain with contraction off; a product of
 * up to n_vars table cells below the range of fp64 underflows to 0 (a log-domain variant does not exist).
 * out (device f64 [n_plans][n_rows][out_stride]): the out_cells cells of the last step, unnormalised — P(the kept variables'
 * levels and the row's masks) — then +0 up to out_stride.  z (device f64 [n_plans][n_rows]): the sum of those out_cells cells
 * in the fixed order of this library: slot t of 256 adds the cells t, t + 256, ... in ascending order starting from +0, then
 * x[i] += x[i + s] for s = 128, 64, ..., 1; z is x[0].  No floating-point atomics: two calls give equal bytes, and the bytes
 * do not depend on rows_per_group or on the launch geometry.
 *
 * A workgroup owns one plan and a group of G rows, each row with an arena of its own; rows_per_group = 0 selects the library's
 * rule G = clamp(1024 / step_cells, 1, 64); a given value is taken as it is; either is then limited to
 * DVS_BN_ELIM_MAX_CELLS / arena_cells.  arena_cells, step_cells and plan_words are the caller's statements about the plans of
 * this call — the largest arena, the largest step output and the longest plan in words — which size the launch; a plan that
 * exceeds arena_cells or plan_words is malformed.
 *
 * The library guarantees memory safety for any plan words; the arithmetic of a hand-made plan is the caller's business.
 * Before anything of a plan is executed, one workgroup checks it: plan_offsets inside plans_bytes and at most plan_words
 * apart; the tag, n_vars and the counts (n_steps >= 1, 1 <= arena_cells <= the argument, 1 <= out_cells <= out_stride, n_keep
 * <= DVS_BN_ELIM_MAX_SCOPE, kept variables ascending and < n_vars); per step: the last one, and only it, has x = -1 and
 * out_offset = -1, and its out_cells are the header's; every other output span lies inside arena_cells; n_scope <=
 * DVS_BN_ELIM_MAX_SCOPE, scope variables ascending, < n_vars and not x, out_cells = the product of their level counts;
 * 1 <= n_inputs <= DVS_BN_ELIM_MAX_INPUTS; per input: kind -1 or a variable, an arena span inside arena_cells and disjoint
 * from the step's output span, no negative stride, and stride_x * (card[x] - 1) + sum_i stride_i * (card_i - 1) below the
 * span's (or the table's) size; the steps end where the plan ends.  It also checks the network as dvs_bn_blanket_posterior
 * does (level counts in 1..16, parent bits < n_vars, every table inside offsets[0] .. offsets[0] + n_cells and of q * r cells).
 * A malformed plan (or network: then every plan) sets bit 4 of status and plan_flags[p] = 1 (device i32 [n_plans], written: 0
 * for a plan that was executed); its out_stride cells of every row and its z are NaN and nothing of it is executed.  The
 * other plans of the call are computed as if it were not there.
 *
 * Checked before anything is enqueued, in this order: n_vars in [1, 48] (3), n_cells in [n_vars, 2^31 - 1] (2), n_plans and
 * n_rows in [1, 2^31 - 1] and n_plans * n_rows < 2^31 (2), plan_words in [7, DVS_BN_ELIM_MAX_WORDS] (12), arena_cells and
 * step_cells in [1, DVS_BN_ELIM_MAX_CELLS] (12), out_stride in [1, DVS_BN_ELIM_MAX_CELLS] (12), rows_per_group in [0, 64]
 * (12), null pointers (10), plans_bytes < n_plans * 28 (14 with that size), out_bytes < n_plans * n_rows * out_stride * 8 (14
 * with that size).
 *
 * The cap: DVS_BN_ELIM_MAX_CELLS = 16 384 fp64 cells = 128 KiB of LDS for the arena of one row.  There is no global-memory
 * fallback: a network whose elimination needs more is outside this entry point (DESIGN.md §24 says what that excludes). */
#ifndef DVS_ELIMINATE_H
#define DVS_ELIMINATE_H

#include "dvs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DVS_BN_ELIM_TAG 0x454C4D31       /* "ELM1": the first word of a plan */
#define DVS_BN_ELIM_MAX_CELLS 16384      /* fp64 cells of one row's arena, of one table, of out_stride */
#define DVS_BN_ELIM_MAX_WORDS 4096       /* int32 words of one plan (staged in LDS next to the arenas) */
#define DVS_BN_ELIM_MAX_SCOPE 16         /* variables of one step's output scope, and kept variables */
#define DVS_BN_ELIM_MAX_INPUTS 64        /* factors one step multiplies */

int dvs_bn_eliminate(int32_t n_vars, int32_t n_plans, int64_t n_rows, const uint8_t* card, const uint64_t* parents,
                     const int64_t* offsets, const double* cpt, int64_t n_cells, const int32_t* plans, size_t plans_bytes,
                     const int64_t* plan_offsets, int32_t plan_words, int32_t arena_cells, int32_t step_cells,
                     const uint16_t* masks, int32_t rows_per_group, int32_t out_stride, double* out, size_t out_bytes,
                     double* z, int32_t* plan_flags, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
