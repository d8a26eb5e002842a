"""ctypes binding of libdvs_hip.so (C ABI: include/dvs.h).

The product has exactly one compute path: the HIP library.  ``load()`` raises if it is missing — there is
no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import (POINTER, Structure, c_char, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32,
                    c_uint64, c_void_p)

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libdvs_hip.so"

D_MODEL, HEADS, LAYERS, LATENT, FC_HIDDEN, EMB = 64, 8, 3, 32, 32, 32
MAX_TOKENS = 48           # 16 on the one-tile path (a wavefront owns a DAG); up to 48 on the tiled wide path
TILE_TOKENS = 16
DECODE_STATE_BYTES = 440
CLIP_SCRATCH_FLOATS = 4096  # DVS_CLIP_SCRATCH_FLOATS
RECORD_BYTES = 96         # one-tile path; record_bytes(lib, shape) gives the size that applies
LOSS_FLOATS = 5           # DVS_LOSS_FLOATS: total, recon, kld, non-finite flag, invalid-features flag
ABI_VERSION = 202         # DVS_VERSION of include/dvs.h this binding was written against
GP_ACQ_MAX_INDUCING = 1023  # DVS_GP_ACQ_MAX_INDUCING
STRUCT_HASH_INVALID = 0x7FFFFFFFFFFFFFFF  # DVS_STRUCT_HASH_INVALID
GEN_LABELS_CHOICE, GEN_ACCEPT_ISOLATES, GEN_ACCEPT_NO_CONNECTIVITY, GEN_GROUP_SHIFT = 1, 2, 4, 8   # DVS_GEN_* flags
CI_TYPES = {"mi": 0, "x2": 1, "mi-adf": 2, "x2-adf": 3}   # dvs_ci_type, by bnlearn's name
CI_MAX_CELLS = 36864      # the dense (z, x, y) table of dvs_ci_tests that fits LDS
FIT_METHODS = {"mle": 0, "bayes": 1}   # dvs_fit_method, by bnlearn's name
FIT_MAX_CELLS = 36864     # the dense (configuration, level) table of dvs_bn_fit that fits LDS
# bits of the BN entry points' status word (device int32, zeroed by the caller), as include/dvs.h defines them
STATUS_CYCLE = 1              # bit 0 (dvs_bn_sample, dvs_bn_lw): the structure has a cycle
STATUS_REFUSED = 16           # bit 4: a family, test, row or query was refused (NaN in its cells alone); worded per call site
STATUS_LABELS = 32            # bit 5 (dvs_bic_parent_masks): a DAG's labels are not a permutation of 0..n_vars-1
STATUS_NOT_PROBABILITY = 64   # bit 6 (dvs_bn_sample, dvs_bn_lw): a table row is not a probability vector
LW_STATUS_ZERO_WEIGHT = 128   # dvs_bn_lw status bit 7: a query whose weights sum to zero (information, not an error)
SCORE_TYPES = {"loglik": 0, "aic": 1, "bic": 2, "bde": 3, "bds": 4, "k2": 5, "bdj": 6}   # dvs_score_type, by bnlearn's name


class DvsShape(Structure):
    _fields_ = [("batch", c_int32), ("n_tokens", c_int32), ("n_classes", c_int32), ("training", c_int32),
                ("dropout", c_float), ("beta", c_float), ("eps_scale", c_float), ("dag_offset", c_uint32),
                ("seed", c_uint64)]


class DvsParamEntry(Structure):
    _fields_ = [("name", c_char * 64), ("offset", c_int64), ("rows", c_int32), ("cols", c_int32)]


def bind(lib: ctypes.CDLL) -> ctypes.CDLL:
    """Declare argument/return types of every entry point of include/dvs.h on a loaded library."""
    P = POINTER
    lib.dvs_version.restype = c_int
    lib.dvs_last_error.restype = c_char_p
    lib.dvs_device_cus.restype = c_int
    lib.dvs_param_count.restype = c_int64
    lib.dvs_param_count.argtypes = [P(DvsShape)]
    lib.dvs_param_table.restype = c_int
    lib.dvs_param_table.argtypes = [P(DvsShape), P(DvsParamEntry), c_int]
    lib.dvs_workspace_bytes.restype = c_size_t
    lib.dvs_workspace_bytes.argtypes = [P(DvsShape)]
    lib.dvs_record_bytes.restype = c_size_t
    lib.dvs_record_bytes.argtypes = [P(DvsShape)]
    lib.dvs_pack_features.restype = c_int
    # (shape, label 1-hot, position 1-hot, adjacency, target masks, records, records_bytes, status, stream)
    lib.dvs_pack_features.argtypes = [P(DvsShape), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p,
                                      c_void_p]
    lib.dvs_build_records.restype = c_int
    # (shape, labels, preds, records, records_bytes, status, stream)
    lib.dvs_build_records.argtypes = [P(DvsShape), c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.dvs_loss_forward.restype = c_int
    # (shape, records, records_bytes, params, n_params, workspace, workspace_bytes, eps, status, losses, mu, logvar, stream)
    lib.dvs_loss_forward.argtypes = [P(DvsShape), c_void_p, c_size_t, c_void_p, c_int64, c_void_p, c_size_t, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.dvs_loss_forward_notify.restype = c_int
    # (... as dvs_loss_forward ..., logvar, host_tail (pinned, 8 words), host_seq, stream)
    lib.dvs_loss_forward_notify.argtypes = [P(DvsShape), c_void_p, c_size_t, c_void_p, c_int64, c_void_p, c_size_t, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_uint32, c_void_p]
    lib.dvs_loss_backward.restype = c_int
    # (shape, records, records_bytes, params, n_params, workspace, workspace_bytes, gcoef, grads, stream)
    lib.dvs_loss_backward.argtypes = [P(DvsShape), c_void_p, c_size_t, c_void_p, c_int64, c_void_p, c_size_t, c_void_p,
                                      c_void_p, c_void_p]
    lib.dvs_loss_backward_sq.restype = c_int
    # (shape, records, records_bytes, params, n_params, workspace, workspace_bytes, gcoef, grads, clip_scratch, stream)
    lib.dvs_loss_backward_sq.argtypes = [P(DvsShape), c_void_p, c_size_t, c_void_p, c_int64, c_void_p, c_size_t, c_void_p,
                                         c_void_p, c_void_p, c_void_p]
    lib.dvs_loss_forward_defer.restype = c_int
    # (shape, records, records_bytes, params, n_params, workspace, workspace_bytes, eps, mu, logvar, stream)
    lib.dvs_loss_forward_defer.argtypes = [P(DvsShape), c_void_p, c_size_t, c_void_p, c_int64, c_void_p, c_size_t, c_void_p,
                                           c_void_p, c_void_p, c_void_p]
    lib.dvs_loss_backward_emit.restype = c_int
    # (... as dvs_loss_backward_sq ..., clip_scratch, status, losses, host_tail (pinned), host_seq, stream)
    lib.dvs_loss_backward_emit.argtypes = [P(DvsShape), c_void_p, c_size_t, c_void_p, c_int64, c_void_p, c_size_t, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_uint32, c_void_p]
    lib.dvs_encode.restype = c_int
    # (shape, records, records_bytes, params, n_params, workspace, workspace_bytes, mu, logvar, stream)
    lib.dvs_encode.argtypes = [P(DvsShape), c_void_p, c_size_t, c_void_p, c_int64, c_void_p, c_size_t, c_void_p, c_void_p,
                               c_void_p]
    lib.dvs_decode.restype = c_int
    # (shape, params, n_params, workspace, workspace_bytes, records, records_bytes, z, uniforms, state, state_bytes, stream)
    lib.dvs_decode.argtypes = [P(DvsShape), c_void_p, c_int64, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p,
                               c_void_p, c_size_t, c_void_p]
    lib.dvs_match_decoded.restype = c_int
    # (batch, n_vars, card, repeats, preds_are_u64, labels, preds, states, state_bytes, budget, flags, stream)
    lib.dvs_match_decoded.argtypes = [c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_size_t,
                                      c_int32, c_void_p, c_void_p]
    lib.dvs_decoded_structures.restype = c_int
    # (batch, n_vars, preds_are_u64, states, state_bytes, hash_mask, flags, labels, preds, keys, keys_bytes, hashes, stream)
    lib.dvs_decoded_structures.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_size_t, c_uint64, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.dvs_structset_filter.restype = c_int
    # (batch, n_vars, sorted_hashes, order, keys, keys_bytes, flags, seen_count, seen_hashes, seen_keys, seen_keys_bytes,
    #  out, stream)
    lib.dvs_structset_filter.argtypes = [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_int32,
                                         c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.dvs_generate_dags.restype = c_int
    # (batch, n_vars, card, preds_are_u64, num_edges, seed, dag_offset, try_limit, flags, labels, preds, preds_bytes, attempts,
    #  stream)
    lib.dvs_generate_dags.argtypes = [c_int32, c_int32, c_int32, c_int32, c_void_p, c_uint64, c_int64, c_int32, c_int32,
                                      c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.dvs_generate_edge_counts.restype = c_int
    # (batch, n_entries, edge_counts, cum_weights, seed, dag_offset, num_edges, stream)
    lib.dvs_generate_edge_counts.argtypes = [c_int32, c_int32, c_void_p, c_void_p, c_uint64, c_int64, c_void_p, c_void_p]
    lib.dvs_debug_launch.restype = c_int
    lib.dvs_debug_launch.argtypes = [c_size_t, c_void_p]
    lib.dvs_bic_scores.restype = c_int
    lib.dvs_bic_scores.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p]
    lib.dvs_bn_scores.restype = c_int
    lib.dvs_bn_scores.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, ctypes.c_double, c_void_p,
                                  c_void_p, c_void_p, c_void_p]
    lib.dvs_bn_toggle_scores.restype = c_int
    # (batch, n_vars, n_samples, data, card, parents, score_type, score_arg, worklist (nullable), local, local_bytes, toggles,
    #  toggles_bytes, status, stream)
    lib.dvs_bn_toggle_scores.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, ctypes.c_double,
                                         c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.dvs_hc_step.restype = c_int
    # (batch, n_vars, parents, local, toggles, toggles_bytes, max_parents, min_delta, forbidden (nullable), step_cap, worklist,
    #  steps, converged, flags, trace (nullable), trace_bytes, active, stream)
    lib.dvs_hc_step.argtypes = [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_int32, ctypes.c_double, c_void_p,
                                c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.dvs_tabu_step.restype = c_int
    # (... as dvs_hc_step up to active ..., tabu_len, ring, ring_bytes, visited, max_stall, stall, best_score, best_parents,
    #  best_bytes, stream)
    lib.dvs_tabu_step.argtypes = lib.dvs_hc_step.argtypes[:-1] + [c_int32, c_void_p, c_size_t, c_void_p, c_int32, c_void_p,
                                                                  c_void_p, c_void_p, c_size_t, c_void_p]
    lib.dvs_hc_perturb.restype = c_int
    # (batch, n_vars, parents, local, toggles, toggles_bytes, max_parents, forbidden (nullable), worklist, flags, seed,
    #  draw_index, stream)
    lib.dvs_hc_perturb.argtypes = [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_int32, c_void_p, c_void_p,
                                   c_void_p, c_uint64, c_uint32, c_void_p]
    lib.dvs_cpdag.restype = c_int
    # (batch, n_vars, parents, pdag, pdag_bytes, flags, stream)
    lib.dvs_cpdag.argtypes = [c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.dvs_pdag_compare.restype = c_int
    # (batch, n_vars, a, b, b_rows, counts, counts_bytes, stream)
    lib.dvs_pdag_compare.argtypes = [c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_size_t, c_void_p]
    lib.dvs_ci_tests.restype = c_int
    # (n_tests, n_vars, n_samples, data, card, pairs, cond, test_type, max_cells, out, out_bytes, status, stream)
    lib.dvs_ci_tests.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                 c_void_p, c_size_t, c_void_p, c_void_p]
    lib.dvs_pc_expand.restype = c_int
    # (n_pairs, n_vars, level, adj, pair_xy, offsets, n_tests, pairs, cond, tests_bytes, stream)
    lib.dvs_pc_expand.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                  c_size_t, c_void_p]
    lib.dvs_pc_reduce.restype = c_int
    # (n_pairs, n_vars, pair_xy, offsets, n_tests, cond, out, alpha, adj, adj_next, sepset, sepset_bytes, result,
    #  result_bytes, refused, stream)
    lib.dvs_pc_reduce.argtypes = [c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, ctypes.c_double,
                                  c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.dvs_pc_orient.restype = c_int
    # (batch, n_vars, skeleton, sepsets, sepsets_bytes, pdag, pdag_bytes, conflicts, flags, stream)
    lib.dvs_pc_orient.argtypes = [c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p,
                                  c_void_p]
    lib.dvs_bn_fit.restype = c_int
    # (batch, n_vars, n_samples, data, card, parents, method, iss, unobserved, offsets, cpt, cpt_bytes, status, stream)
    lib.dvs_bn_fit.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, ctypes.c_double, c_int32,
                               c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.dvs_bn_sample_workspace_bytes.restype = c_size_t
    lib.dvs_bn_sample_workspace_bytes.argtypes = [c_int64, c_int32]
    lib.dvs_bn_sample.restype = c_int
    # (n_vars, n_rows, card, parents, offsets, cpt, n_cells, seed, row_offset, workspace, workspace_bytes, data_out, status,
    #  stream)
    lib.dvs_bn_sample.argtypes = [c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_uint64, c_int64,
                                  c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]
    lib.dvs_bn_loglik.restype = c_int
    # (batch, n_vars, n_rows, data, card, parents, offsets, cpt, per_row (nullable), out, workspace, workspace_bytes, status,
    #  stream)
    lib.dvs_bn_loglik.argtypes = [c_int32, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.dvs_bn_lw_workspace_bytes.restype = c_size_t
    lib.dvs_bn_lw_workspace_bytes.argtypes = [c_int64, c_int32, c_int64, c_int64, c_uint64]
    lib.dvs_bn_lw.restype = c_int
    # (n_vars, n_queries, n_particles, card, parents, offsets, cpt, n_cells, evidence, observed, event (nullable), targets, seed,
    #  query_offset, workspace, workspace_bytes, sums, marginals (nullable), particles (nullable), particle_weights (nullable),
    #  status, stream)
    lib.dvs_bn_lw.argtypes = [c_int32, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                              c_void_p, c_uint64, c_uint64, c_int64, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p]
    lib.dvs_bn_blanket_posterior.restype = c_int
    # (batch, n_vars, n_rows, data, card, parents, offsets, cpt, cpt_bytes, target, use_children, posterior (nullable), pred,
    #  status, stream)
    lib.dvs_bn_blanket_posterior.argtypes = [c_int32, c_int32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_size_t, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.dvs_exact_workspace_bytes.restype = c_size_t
    lib.dvs_exact_workspace_bytes.argtypes = [c_int32, c_int32]
    lib.dvs_exact_search.restype = c_int
    # (batch, n_vars, table, table_bytes, max_parents, forbidden (nullable), workspace, workspace_bytes, parents, order, score,
    #  flags, stream)
    lib.dvs_exact_search.argtypes = [c_int32, c_int32, c_void_p, c_size_t, c_int32, c_void_p, c_void_p, c_size_t, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p]
    lib.dvs_arc_posterior_workspace_bytes.restype = c_size_t
    lib.dvs_arc_posterior_workspace_bytes.argtypes = [c_int32, c_int32]
    lib.dvs_arc_posterior.restype = c_int
    # (batch, n_vars, table, table_bytes, max_parents, forbidden (nullable), size_prior (nullable), workspace, workspace_bytes,
    #  prob, log_z, family (nullable), family_bytes, flags, stream)
    lib.dvs_arc_posterior.argtypes = [c_int32, c_int32, c_void_p, c_size_t, c_int32, c_void_p, c_void_p, c_void_p, c_size_t,
                                      c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.dvs_order_mcmc.restype = c_int
    # (chains, n_vars, n_families, steps, offsets, sets, sets_bytes, scores, scores_bytes, seed, chain_offset, step_offset,
    #  burn_in, thin, window, init, order, log_score, accepted, sums, sums_bytes, kept, best_score, best_parents,
    #  trace (nullable), trace_bytes, flags, stream)
    lib.dvs_order_mcmc.argtypes = [c_int32, c_int32, c_int64, c_int32, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t,
                                   c_uint64, c_int64, c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p,
                                   c_void_p]
    lib.dvs_order_mcmc_finish.restype = c_int
    # (chains, n_vars, sums, sums_bytes, kept, prob, stream)
    lib.dvs_order_mcmc_finish.argtypes = [c_int32, c_int32, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]
    lib.dvs_bn_scores_rows.restype = c_int
    # (... as dvs_bn_scores up to status ..., rows, set_size, n_sets, set_of (nullable), stream)
    lib.dvs_bn_scores_rows.argtypes = lib.dvs_bn_scores.argtypes[:-1] + [c_void_p, c_int32, c_int32, c_void_p, c_void_p]
    lib.dvs_bn_toggle_scores_rows.restype = c_int
    # (... as dvs_bn_toggle_scores up to status ..., rows, set_size, n_sets, set_of (nullable), stream)
    lib.dvs_bn_toggle_scores_rows.argtypes = lib.dvs_bn_toggle_scores.argtypes[:-1] + [c_void_p, c_int32, c_int32, c_void_p,
                                                                                      c_void_p]
    lib.dvs_bootstrap_rows.restype = c_int
    # (n_sets, set_size, n_samples, seed, set_offset, rows, stream)
    lib.dvs_bootstrap_rows.argtypes = [c_int32, c_int32, c_int32, c_uint64, c_int64, c_void_p, c_void_p]
    lib.dvs_arc_strength.restype = c_int
    # (batch, n_vars, pdag, counts, counts_bytes, stream)
    lib.dvs_arc_strength.argtypes = [c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.dvs_averaged_network.restype = c_int
    # (groups, n_vars, counts, n_networks, min_any, parents, parents_bytes, info, stream)
    lib.dvs_averaged_network.argtypes = [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.dvs_bic_parent_masks.restype = c_int
    lib.dvs_bic_parent_masks.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.dvs_gp_predict.restype = c_int
    lib.dvs_gp_predict.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, ctypes.c_double, ctypes.c_double,
                                   ctypes.c_double, c_void_p, c_void_p]
    lib.dvs_gp_kernel.restype = c_int
    lib.dvs_gp_kernel.argtypes = [c_int32, c_int32, c_int32, c_void_p, c_void_p, ctypes.c_double, ctypes.c_double, c_void_p,
                                  c_void_p]
    lib.dvs_gp_kernel_backward.restype = c_int
    lib.dvs_gp_kernel_backward.argtypes = [c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, ctypes.c_double,
                                           ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.dvs_gp_acquire.restype = c_int
    # (batch, n_inducing, dim, ld, x, inducing, weights [P | alpha], c0, outputscale, lengthscale, constant, best, xi,
    #  mean, var, ei, grad (nullable), stream)
    lib.dvs_gp_acquire.argtypes = [c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p] + [ctypes.c_double] * 6 + \
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.dvs_clip_adam.restype = c_int
    # (n, params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, max_norm, scratch, guard, stream)
    lib.dvs_clip_adam.argtypes = [c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float,
                                  c_int64, c_float, c_void_p, c_void_p, c_void_p]
    lib.dvs_clip_adam_from_partials.restype = c_int
    lib.dvs_clip_adam_from_partials.argtypes = lib.dvs_clip_adam.argtypes
    lib.dvs_profile_enable.restype = None
    lib.dvs_profile_enable.argtypes = [c_int]
    lib.dvs_profile_collect.restype = c_int
    lib.dvs_profile_collect.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_int]
    lib.dvs_debug_activation.restype = c_int
    lib.dvs_debug_activation.argtypes = [P(DvsShape), c_void_p, c_int, c_void_p, c_void_p]
    lib.dvs_debug_dag_losses.restype = c_int
    lib.dvs_debug_dag_losses.argtypes = [P(DvsShape), c_void_p, c_void_p, c_void_p]
    return lib


EXPORTS = ["dvs_version", "dvs_last_error", "dvs_device_cus", "dvs_param_count", "dvs_param_table",
           "dvs_workspace_bytes", "dvs_record_bytes", "dvs_pack_features", "dvs_build_records", "dvs_loss_forward", "dvs_loss_forward_notify", "dvs_loss_backward", "dvs_loss_backward_sq", "dvs_loss_forward_defer", "dvs_loss_backward_emit", "dvs_encode", "dvs_decode", "dvs_match_decoded", "dvs_decoded_structures", "dvs_structset_filter", "dvs_generate_dags", "dvs_generate_edge_counts", "dvs_bic_scores", "dvs_bn_scores", "dvs_bn_toggle_scores", "dvs_hc_step", "dvs_tabu_step", "dvs_hc_perturb", "dvs_cpdag", "dvs_pdag_compare", "dvs_ci_tests", "dvs_pc_expand", "dvs_pc_reduce", "dvs_pc_orient", "dvs_bn_fit", "dvs_bn_sample_workspace_bytes", "dvs_bn_sample", "dvs_bn_loglik", "dvs_bn_lw_workspace_bytes", "dvs_bn_lw", "dvs_bn_blanket_posterior", "dvs_exact_workspace_bytes", "dvs_exact_search", "dvs_arc_posterior_workspace_bytes", "dvs_arc_posterior", "dvs_order_mcmc", "dvs_order_mcmc_finish", "dvs_bn_scores_rows", "dvs_bn_toggle_scores_rows", "dvs_bootstrap_rows", "dvs_arc_strength", "dvs_averaged_network", "dvs_bic_parent_masks", "dvs_gp_predict", "dvs_gp_kernel", "dvs_gp_kernel_backward", "dvs_gp_acquire",
           "dvs_clip_adam", "dvs_clip_adam_from_partials", "dvs_debug_activation", "dvs_debug_dag_losses", "dvs_debug_launch", "dvs_profile_enable", "dvs_profile_collect"]


def profile_collect(lib):
    """{kernel name: (launches, total ms)} recorded since dvs_profile_enable(1)."""
    cap, stride = 64, 64
    names = ctypes.create_string_buffer(cap * stride)
    counts = (c_int * cap)()
    ms = (c_float * cap)()
    n = lib.dvs_profile_collect(names, stride, counts, ms, cap)
    out = {}
    for i in range(min(n, cap)):
        out[names.raw[i * stride:(i + 1) * stride].split(b"\0")[0].decode()] = (int(counts[i]), float(ms[i]))
    return out

_lib = None


def lib_path() -> str:
    return os.path.join(_HERE, LIB_NAME)


def load() -> ctypes.CDLL:
    """Load the in-tree HIP library (built by ``__graft_entry__.build()`` / ``make -C csrc``)."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(
                f"{LIB_NAME} not found at {path}: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"(hipcc --offload-arch=gfx950).  dags_vae_search_amd has no CPU fallback.")
        _lib = bind(ctypes.CDLL(path))
        if _lib.dvs_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_NAME}: unexpected ABI version {_lib.dvs_version()}")
    return _lib


def check(lib, code: int, what: str):
    if code != 0:
        msg = lib.dvs_last_error()
        raise RuntimeError(f"{what} failed with code {code}: {msg.decode() if msg else ''}")


# ---- the device-call layer: how every module of this package hands tensors, the stream and seeds to the library, and the
# refusals several entry points share.  A new module takes these from here instead of restating them.
def ptr(t, offset: int = 0):
    """a tensor's device address (plus ``offset`` bytes) as a pointer argument; None (a nullable argument left out) stays NULL"""
    return None if t is None else c_void_p(t.data_ptr() + offset)


def nbytes(t) -> int:
    return t.numel() * t.element_size()


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def seed64(seed) -> int:
    """any Python int as the c_uint64 seed argument: its low 64 bits"""
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def need_cuda(what, device):
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"dags_vae_search_amd: {what} runs on the GPU (got device {device}); this package has no CPU path")


def require_cuda(t, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"dags_vae_search_amd: {what} must live on the GPU (got device {t.device}); "
                           f"this package has no CPU path")


def workspace_bytes(lib, name: str, *args) -> int:
    """a ``*_bytes`` size query; 0 is its refusal, raised with the library's last error"""
    n = int(getattr(lib, name)(*args))
    if n == 0:
        check(lib, 1, name)
    return n


def level_counts(card):
    """n level counts as a list of ints"""
    card = [int(c) for c in card]
    if not 1 <= len(card) <= MAX_TOKENS or any(not 1 <= c <= 16 for c in card):
        raise ValueError("card must hold 1..48 level counts in 1..16")
    return card


def packed_rows(what, data, n):
    """``data``: an evaluator over n variables (bic.py) or packed int64 rows [S >= 1, ceil(n / 16)] -> the rows, contiguous"""
    if not torch.is_tensor(data) and hasattr(data, "packed"):
        if data.n_vars != n:
            raise ValueError(f"{what}: the evaluator has {data.n_vars} variables, the network {n}")
        data = data.packed
    if not torch.is_tensor(data) or data.dtype != torch.int64 or data.ndim != 2 or data.shape[1] != (n + 15) // 16 or data.shape[0] < 1:
        raise ValueError(f"{what}: data must be an evaluator or packed int64 rows [S >= 1, {(n + 15) // 16}]")
    need_cuda(what, data.device)
    return data.contiguous()


def parent_masks(what, name, t, n=None):
    """a batch of parent masks (or PDAG rows) on the device: int64 [B >= 1, n <= 48], contiguous"""
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: {name} must be a torch tensor of parent masks")
    need_cuda(what, t.device)
    if t.dtype != torch.int64 or t.ndim != 2 or t.shape[0] < 1 or not 1 <= t.shape[1] <= MAX_TOKENS or (n is not None and t.shape[1] != n):
        raise ValueError(f"{what}: {name} must be int64 [B >= 1, {n if n is not None else 'n <= 48'}] parent masks")
    return t.contiguous()


def forbidden_rows(forbidden, n, device):
    """``forbidden`` (None, a tensor, or anything numpy reads as n unsigned 64-bit rows) -> None or int64 [n] on the device"""
    if forbidden is None:
        return None
    if not torch.is_tensor(forbidden):
        forbidden = torch.as_tensor(np.asarray(forbidden).astype(np.uint64).view(np.int64))
    forb = forbidden.to(device=device, dtype=torch.int64).contiguous()
    if forb.shape != (n,):
        raise ValueError(f"forbidden must be [{n}] bit rows")
    return forb


def check_network_status(what, st: int):
    """the refusals dvs_bn_sample and dvs_bn_lw share: a cycle, a table row that is not a probability vector"""
    if st & STATUS_CYCLE:
        raise ValueError(f"{what}: the structure has a cycle")
    if st & STATUS_NOT_PROBABILITY:
        raise ValueError(f"{what}: a table row is not a probability vector (a NaN or negative cell, or a sum further than 1e-9 from 1)")


def make_shape(batch: int, n_tokens: int, n_classes: int, training: bool = False, dropout: float = 0.15,
               beta: float = 0.005, eps_scale: float = 0.01, dag_offset: int = 0, seed: int = 0) -> DvsShape:
    return DvsShape(int(batch), int(n_tokens), int(n_classes), 1 if training else 0, float(dropout), float(beta),
                    float(eps_scale), int(dag_offset) & 0xFFFFFFFF, seed64(seed))


def record_bytes(lib, shape: DvsShape) -> int:
    return workspace_bytes(lib, "dvs_record_bytes", ctypes.byref(shape))


def is_wide(n_tokens: int, n_classes: int) -> bool:
    """Shapes beyond one 16-token / 16-class tile take the workgroup-per-DAG kernels (csrc/dvs_wide.h)."""
    return n_tokens > TILE_TOKENS or n_classes > 16


def param_table(lib, shape: DvsShape):
    """[(name, offset, shape tuple)] of the 108 state-dict tensors inside the flat buffer, and its length."""
    entries = (DvsParamEntry * 128)()
    n = lib.dvs_param_table(ctypes.byref(shape), entries, 128)
    if n <= 0:
        check(lib, 1, "dvs_param_table")
    table = []
    for e in entries[:n]:
        shp = (e.rows, e.cols) if e.cols else (e.rows,)
        table.append((e.name.decode(), int(e.offset), shp))
    total = int(lib.dvs_param_count(ctypes.byref(shape)))
    return table, total
