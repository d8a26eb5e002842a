/* dvs_permtest.h — fifth companion header of dvs.h: Monte Carlo permutation conditional-independence tests on discrete data
 * (DESIGN.md §28): bnlearn's mc-mi / mc-x2, the sequential smc-mi / smc-x2 and the semiparametric sp-mi / sp-x2.  dvs.h and
 * the four companion headers before this one stay what they are and DVS_VERSION stays 202: a pure addition.
 *
 * ---- The test ----------------------------------------------------------------------------------------------------------------
 * Test t is (x, y | Z) = (pairs[t], cond[t]); data, card, pairs, cond, max_cells, the (z, x, y) table — cell
 * (key * r_x + level_x) * r_y + level_y, key the mixed-radix configuration of Z, lowest variable id fastest — and the refusals
 * (three NaNs, bit 4 of status, used = 0) are those of dvs_ci_tests (dvs.h).  out[t][0], the observed statistic, and the classic
 * df (r_x - 1)(r_y - 1) q are byte for byte what dvs_ci_tests writes with test_type DVS_CI_MI for the *-mi types and DVS_CI_X2
 * for the *-x2 types: the same counts, the same per-configuration sums, the same reduction.
 * Notation: c = a cell count, n_xz / n_yz / n_z the row, column and whole sums of configuration z (a "row" is an x-level).
 *
 * ---- How permutation b draws its table -----------------------------------------------------------------------------------------
 * Permutation b in [0, n_perm) of test t draws, for every configuration z with n_z > 0 in ascending order, one random table
 * with that configuration's row and column sums, by drawing without replacement: the column pool starts as n_yz and m = n_z.
 * For x-level i ascending with n_xz > 0, except the last such level, which takes what remains of the pool: n_xz times, draw
 * u uniform on [0, m), find the column k whose cumulative pool count first exceeds u (pool[0] + .. + pool[k] > u), increment
 * cell[i][k], decrement pool[k], decrement m.  A configuration with a single occupied row draws nothing.
 * The draw.  All arithmetic is on u32 unless said.  fmix32 is MurmurHash3's finaliser:
 *     fmix32(v): v ^= v >> 16; v *= 0x85EBCA6B; v ^= v >> 13; v *= 0xC2B2AE35; v ^= v >> 16.
 *     key_t = fmix32(fmix32(seed_lo ^ (801 * 0x632BE5AB)) ^ seed_hi ^ ((test_offset + t) * 0x9E3779B1))
 *             with seed_lo / seed_hi the low and high halves of seed (site 800 of the library's counter-based generator)
 *     key_b = fmix32(key_t ^ (b * 0x9E3779B1))
 *     h_0   = fmix32(key_b ^ (j * 0x9E3779B1))        j = 0, 1, ..: the ordinal of the draw within the permutation, counted
 *                                                      over all configurations in the order above
 *     h_a   = fmix32(h_0 ^ (a * 0x632BE5AB))          attempt a = 1, 2, ..
 *     attempt a is accepted unless (u32)(h_a * m) < (2^32 - m) mod m, the products taken in u64; the first accepted attempt
 *     gives u = (h_a * m) >> 32.
 * This is multiply-shift with rejection (Lemire 2019): every u in [0, m) is hit by exactly floor(2^32 / m) accepted values of
 * h, so u is exactly uniform given a uniform h; a -> h_0 ^ (a * odd) runs over all 2^32 words, so the loop ends.  A draw is a
 * pure function of (seed, test_offset + t, b, j, a) and nothing else: not of slices, not of how a batch is cut into calls.
 *
 * ---- The statistic compared ----------------------------------------------------------------------------------------------------
 * The margins are fixed under permutation, so only the part of the statistic that varies is compared, in fp64:
 *     *-mi   V = sum_z sum_i sum_k klnk(c),                    klnk(c) = c * log(c) (one multiplication, rounded), 0 for c <= 1
 *     *-x2   V = sum_z n_z * (sum_i (sum_k c * c / n_yz) / n_xz), the k-sum over columns with n_yz > 0, the i-sum over rows
 *            with n_xz > 0; every operation rounded by itself (no fused multiply-add)
 * the sums taken z ascending, then i, then k, each into one accumulator from 0.  V_obs is the same function of the observed
 * table.  G^2 = 2 (V - C) with C = sum_z (sum_k klnk(n_yz) + sum_i klnk(n_xz) - klnk(n_z)) (one accumulator per z: k ascending,
 * then i ascending, then the subtraction; the z terms added in ascending order), and X^2 = V - S_counted, S_counted = sum_z n_z.
 * Permutation b exceeds when V_b >= V_obs * (1 - 2^-32).  The slack is derived, not tuned: V is a sum of at most 36 864
 * non-negative terms, each the result of at most four roundings (relative error below 4 * 2^-53 = 2^-51, whichever of the
 * LDS table or log produced klnk: both evaluate the same expression); a sum of N non-negative terms carries a relative
 * error below N * 2^-53 in any order; together below 2^-51 + 36 864 * 2^-53 < 2^-37.8 for each of V_b and V_obs, below 2^-36
 * for their quotient.  Two tables whose statistics are mathematically equal — mirrored tables, the observed table drawn again
 * — therefore always count as exceeding, as a tie should; the price is that a V_b within 2^-32 below V_obs counts too.
 *
 * ---- Results -------------------------------------------------------------------------------------------------------------------
 * out f64 [n_tests][3] = (observed statistic, df, p-value), used i32 [n_tests] = permutations that counted.
 *     DVS_CI_MC_*    p = (number of exceeding b in [0, n_perm)) / n_perm, df classic, used = n_perm.
 *     DVS_CI_SMC_*   E = floor(alpha * n_perm) + 1 (fp64 product).  Walk b ascending; at the first b where the running count
 *                    of exceeding permutations reaches E: p = E / n_perm, used = b + 1.  Never: p = count / n_perm, used =
 *                    n_perm.  df classic.
 *     DVS_CI_SP_*    df = max(0, mean over b of the permuted statistic), written to out[t][1]; the permuted statistic is
 *                    2 (V_b - C) for sp-mi and V_b - S_counted for sp-x2; the mean is (sum over the 256-permutation blocks,
 *                    ascending, of the block sums) / n_perm, a block sum being the tree x[i] += x[i + s], s = 128, 64, .., 1
 *                    over its permutations in order (absent ones +0.0).  p = Q(df / 2, statistic / 2), the regularised upper
 *                    incomplete gamma function as dvs_ci_tests evaluates it; 1 when df = 0.  used = n_perm.
 * p = count / n_perm (not (count + 1) / (n_perm + 1)) follows bnlearn's convention as recalled; parity with an R run is not
 * pinned — neither the convention nor, of course, the random stream.
 *
 * ---- The launch and its workspace ----------------------------------------------------------------------------------------------
 * blocks = ceil(n_perm / 256).  slices in [1, blocks] cuts a test's blocks into contiguous ranges, slice s owning blocks
 * [s * blocks / slices, (s + 1) * blocks / slices); one 256-thread workgroup per (test, slice), thread = permutation within
 * the block.  For DVS_CI_SMC_* a workgroup stops its slice once its own running count reaches E.  A second kernel walks each
 * test's blocks in ascending order and forms the results; it never reads a block that an early stop left unwritten.
 * workspace, caller-owned, dvs_ci_perm_workspace_bytes(n_tests, n_perm) bytes (0: an argument is out of range), three arrays
 * each starting at a multiple of 256 bytes:
 *     counts i32 [n_tests][blocks]      exceeding permutations of the block; counts[t][0] = -1 marks a refused test
 *     sums   f64 [n_tests][blocks]      the block sum of the permuted statistic (written for every type)
 *     masks  u64 [n_tests][blocks][4]   bit l of word w: permutation 256 * block + 64 * w + l exceeds
 * All cross-workgroup communication is these integers and fp64 values added in a fixed order; there are no floating-point
 * atomics.  Two calls give equal bytes in out and used, as does any slices and any cut of a batch into calls that keeps
 * test_offset + t of every test.
 *
 * Checked before anything is enqueued, in this order: n_tests and n_samples > 0 (2), n_vars in [1, 48] (3), perm_type (12),
 * n_perm in [1, 2^20] (13), alpha in (0, 1) for DVS_CI_SMC_* only (13), slices in [1, blocks] (13), max_cells in [1, 36864]
 * (13), n_tests * blocks < 2^31 (2), null pointers (10), workspace_bytes < dvs_ci_perm_workspace_bytes (14 with that size),
 * out_bytes < n_tests * 24 (14 with that size). */
#ifndef DVS_PERMTEST_H
#define DVS_PERMTEST_H

#include "dvs.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    DVS_CI_MC_MI = 0,
    DVS_CI_MC_X2 = 1,
    DVS_CI_SMC_MI = 2,
    DVS_CI_SMC_X2 = 3,
    DVS_CI_SP_MI = 4,
    DVS_CI_SP_X2 = 5
} dvs_ci_perm_type;

size_t dvs_ci_perm_workspace_bytes(int32_t n_tests, int32_t n_perm);

int dvs_ci_perm_tests(int32_t n_tests, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                      const int32_t* pairs, const uint64_t* cond, int32_t perm_type, int32_t n_perm, double alpha, uint64_t seed,
                      uint32_t test_offset, int32_t slices, int32_t max_cells, void* workspace, size_t workspace_bytes, double* out,
                      size_t out_bytes, int32_t* used, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
