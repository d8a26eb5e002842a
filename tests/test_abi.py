"""The C-ABI library loads on a CPU-only box and exports every symbol include/dvs.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

from dags_vae_search_amd import _lib as dl

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    txt = open(os.path.join(REPO, "include", "dvs.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dvs_[a-z_0-9]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    if not os.path.exists(dl.lib_path()):
        pytest.fail(f"{dl.lib_path()} is missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(dl.lib_path())
    names = header_functions()
    assert len(names) >= 14
    for n in names:
        assert hasattr(lib, n), n
    assert set(names) == set(dl.EXPORTS)          # the Python binding covers the whole header


def test_host_side_queries_without_a_gpu():
    lib = dl.load()
    assert lib.dvs_version() == 202 == dl.ABI_VERSION
    shape = dl.make_shape(4096, 15, 15)
    table, total = dl.param_table(lib, shape)
    assert len(table) == 108 and total % 4 == 0
    assert table[0][0] == "vertex_position_embed.W1" and table[-1][0] == "fc3.bias"
    assert all(off % 4 == 0 for _, off, _ in table)
    assert sum(int(__import__("numpy").prod(s)) for _, _, s in table) == 310160       # n=12 card=12
    assert lib.dvs_workspace_bytes(ctypes.byref(shape)) > 0
    assert dl.record_bytes(lib, shape) == 96
    alarm = dl.make_shape(16, 40, 40)                                                   # alarm size: wide path
    assert lib.dvs_param_count(ctypes.byref(alarm)) >= 470185                           # n=37 card=37
    table40, _ = dl.param_table(lib, alarm)
    assert sum(int(__import__("numpy").prod(s)) for _, _, s in table40) == 470185
    assert dl.record_bytes(lib, alarm) == 864
    bad = dl.make_shape(16, 49, 40)
    assert lib.dvs_param_count(ctypes.byref(bad)) < 0
    assert b"n_tokens" in lib.dvs_last_error()


def test_model_refuses_cpu_compute_and_keeps_state_dict_contract():
    import numpy as np
    import torch
    from dags_vae_search_amd import PaceVaeV3
    torch.manual_seed(9)
    m = PaceVaeV3(12, 12, 32, 8, 3, 64, 32, 32, 0.15)
    z = np.load(os.path.join(REPO, "tests", "golden", "golden_n12c12.npz"))
    sd = m.state_dict()
    # same module tree and init order as the reference => identical tensors under the same torch seed
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), z["param/" + k]), k
    assert m.max_num_vertices == 15 and m.vertex_label_cardinality == 15
    with pytest.raises(RuntimeError):
        m.encode_direct({})
    # parameters alias one flat buffer
    p = next(m.parameters())
    assert p.data_ptr() == m.flat_params.data_ptr()


def test_undersized_caller_buffers_are_rejected_before_anything_is_enqueued():
    """include/dvs.h, code 14: records_bytes / n_params / workspace_bytes / state_bytes below what the shape needs come
    back as an error (with the needed size in dvs_last_error) instead of a silent out-of-bounds device access.  The check
    runs before any HIP call, so it is testable on a CPU-only box with dummy non-null pointers."""
    lib = dl.load()
    shape = dl.make_shape(64, 15, 15)
    sb = ctypes.byref(shape)
    rec_need = 64 * dl.record_bytes(lib, shape)
    ws_need = lib.dvs_workspace_bytes(sb)
    n_params = lib.dvs_param_count(sb)
    dummy = ctypes.c_void_p(4096)           # never dereferenced: every call below fails validation first

    def last():
        return lib.dvs_last_error().decode()
    assert lib.dvs_pack_features(sb, dummy, dummy, dummy, dummy, dummy, rec_need - 1, dummy, None) == 14
    assert "records_bytes" in last() and str(rec_need) in last()
    assert lib.dvs_build_records(sb, dummy, dummy, dummy, rec_need - 1, dummy, None) == 14
    fwd = lambda rb, npar, wb: lib.dvs_loss_forward(sb, dummy, rb, dummy, npar, dummy, wb, None, None, dummy, None, None,
                                                    None)
    assert fwd(rec_need - 1, n_params, ws_need) == 14 and "records_bytes" in last()
    assert fwd(rec_need, n_params - 1, ws_need) == 14 and "n_params" in last()
    assert fwd(rec_need, n_params, ws_need - 4) == 14 and "workspace_bytes" in last() and str(ws_need) in last()
    assert lib.dvs_loss_backward(sb, dummy, rec_need, dummy, n_params, dummy, ws_need - 4, dummy, dummy, None) == 14
    assert lib.dvs_loss_backward(sb, dummy, rec_need, dummy, n_params - 1, dummy, ws_need, dummy, dummy, None) == 14
    assert lib.dvs_encode(sb, dummy, rec_need, dummy, n_params, dummy, ws_need - 4, dummy, dummy, None) == 14
    assert lib.dvs_decode(sb, dummy, n_params, dummy, ws_need, dummy, rec_need, dummy, None, dummy,
                          64 * dl.DECODE_STATE_BYTES - 1, None) == 14
    assert "state_bytes" in last()
    assert lib.dvs_decode(sb, dummy, n_params, dummy, ws_need - 4, dummy, rec_need, dummy, None, dummy,
                          64 * dl.DECODE_STATE_BYTES, None) == 14
    # a bigger batch against buffers sized for a smaller one: the classic mistake this argument exists for
    big = dl.make_shape(128, 15, 15)
    assert lib.dvs_loss_forward(ctypes.byref(big), dummy, rec_need, dummy, n_params, dummy, ws_need, None, None, dummy, None,
                                None, None) == 14
    # null pointers are still code 10 and bad shapes 1..5
    assert lib.dvs_loss_forward(sb, None, rec_need, dummy, n_params, dummy, ws_need, None, None, dummy, None, None, None) == 10


def _search_validation_cases():
    """(entry point, arguments, return code, text dvs_last_error must contain) for the search-side entry points: per entry
    point one size out of range, one null pointer, every *_bytes argument one byte short (the message ends in the size
    that was needed), and cases where two checks fail at once: the earlier check of the entry point decides."""
    D = ctypes.c_void_p(4096)               # never dereferenced: every case fails validation first
    nan = float("nan")
    SB = dl.DECODE_STATE_BYTES
    BIC, K2 = dl.SCORE_TYPES["bic"], dl.SCORE_TYPES["k2"]
    cases = []

    def entry(fn, base):
        def case(code, text, **at):         # at: {"i<index>": value} replaces base[index]
            args = list(base)
            for k, v in at.items():
                args[int(k[1:])] = v
            cases.append((fn, args, code, text))
        return case

    # (batch, n_vars, card, repeats, preds_are_u64, labels, preds, states, state_bytes, budget, flags, stream)
    c = entry("dvs_match_decoded", [8, 12, 12, 3, 0, D, D, D, 24 * SB, 100, D, None])
    c(3, "dvs_match_decoded: n_vars must be in [1, 45]", i1=46)
    c(2, "dvs_match_decoded: batch * repeats must be <= 2^30", i0=1 << 20, i3=1 << 11)
    c(12, "dvs_match_decoded: 16-bit predecessor rows hold at most 16 vertices", i1=17, i2=17)
    c(10, "dvs_match_decoded: null pointer", i5=None)
    c(14, f"dvs_match_decoded: state_bytes < batch * repeats * DVS_DECODE_STATE_BYTES = {24 * SB}", i8=24 * SB - 1)
    c(2, "dvs_match_decoded: batch and repeats must be > 0", i0=0, i1=46)          # batch before n_vars
    c(3, "dvs_match_decoded: card must be in [1, 45]", i2=46, i10=None)            # range before null
    c(12, "dvs_match_decoded: budget must be >= 1", i9=0, i7=None)                 # budget before null
    c(10, "dvs_match_decoded: null pointer", i10=None, i8=0)                       # null before state_bytes

    # (batch, n_vars, preds_are_u64, states, state_bytes, hash_mask, flags, labels, preds, keys, keys_bytes, hashes, stream)
    c = entry("dvs_decoded_structures", [8, 12, 0, D, 8 * SB, 2 ** 63 - 1, D, D, D, D, 768, D, None])
    c(3, "dvs_decoded_structures: n_vars must be in [1, 45]", i1=0)
    c(2, "dvs_decoded_structures: batch must be <= 2^30", i0=(1 << 30) + 1)
    c(10, "dvs_decoded_structures: null pointer", i11=None)
    c(14, f"dvs_decoded_structures: state_bytes < batch * DVS_DECODE_STATE_BYTES = {8 * SB}", i4=8 * SB - 1)
    c(14, "dvs_decoded_structures: keys_bytes < batch * n_vars * 8 = 768", i10=767)
    c(12, "dvs_decoded_structures: 16-bit predecessor rows", i1=17, i3=None)       # row width before null
    c(14, "dvs_decoded_structures: state_bytes <", i4=0, i10=0)                    # state_bytes before keys_bytes

    # (batch, n_vars, sorted_hashes, order, keys, keys_bytes, flags, seen_count, seen_hashes, seen_keys, seen_keys_bytes,
    #  out, stream)
    c = entry("dvs_structset_filter", [8, 12, D, D, D, 768, D, 5, D, D, 480, D, None])
    c(3, "dvs_structset_filter: n_vars must be in [1, 45]", i1=46)
    c(2, "dvs_structset_filter: batch and seen_count must be >= 0", i7=-1)
    c(10, "dvs_structset_filter: null pointer", i11=None)
    c(10, "dvs_structset_filter: null pointer (seen set)", i8=None)
    c(14, "dvs_structset_filter: keys_bytes < batch * n_vars * 8 = 768", i5=767)
    c(14, "dvs_structset_filter: seen_keys_bytes < seen_count * n_vars * 8 = 480", i10=479)
    c(10, "dvs_structset_filter: null pointer", i2=None, i5=0)                     # null before keys_bytes
    c(14, "dvs_structset_filter: keys_bytes <", i5=0, i10=0)                       # keys_bytes before seen_keys_bytes

    # (batch, n_vars, card, preds_are_u64, num_edges, seed, dag_offset, try_limit, flags, labels, preds, preds_bytes,
    #  attempts, stream)
    c = entry("dvs_generate_dags", [8, 12, 12, 0, D, 7, 0, 20, 0, D, D, 192, D, None])
    c(3, "dvs_generate_dags: n_vars must be in [2, 45]", i1=1)
    c(12, "dvs_generate_dags: unknown bits in flags", i8=8)
    c(12, "dvs_generate_dags: labels without replacement ('sample') need card >= n_vars", i2=11)
    c(12, "dvs_generate_dags: predecessor rows are u16 for n_vars <= 13 and u64 above", i3=1)
    c(12, "dvs_generate_dags: dag_offset must be >= 0", i6=-1)
    c(10, "dvs_generate_dags: null pointer", i12=None)
    c(14, "dvs_generate_dags: preds_bytes < batch * n_vars * row bytes = 192", i11=191)
    c(14, "dvs_generate_dags: preds_bytes < batch * n_vars * row bytes = 1280", i1=20, i2=20, i3=1, i11=1279)
    c(12, "dvs_generate_dags: try_limit must be in [1, 4096]", i7=0, i4=None)      # try_limit before null
    c(10, "dvs_generate_dags: null pointer", i9=None, i11=0)                       # null before preds_bytes

    # (batch, n_entries, edge_counts, cum_weights, seed, dag_offset, num_edges, stream)
    c = entry("dvs_generate_edge_counts", [8, 4, D, D, 7, 0, D, None])
    c(2, "dvs_generate_edge_counts: batch must be in [1, 2^30]", i0=0)
    c(12, "dvs_generate_edge_counts: n_entries must be in [1, 1024]", i1=1025)
    c(10, "dvs_generate_edge_counts: null pointer", i6=None)
    c(12, "dvs_generate_edge_counts: dag_offset must be >= 0", i5=-1, i2=None)     # dag_offset before null

    # (batch, n_vars, n_samples, data, card, parents, scratch, out, status, stream)
    c = entry("dvs_bic_scores", [8, 12, 100, D, D, D, D, D, D, None])
    c(3, "dvs_bic_scores: n_vars must be in [1, 48]", i1=49)
    c(2, "dvs_bic_scores: batch and n_samples must be > 0", i2=0)
    c(10, "dvs_bic_scores: null pointer", i6=None)
    c(3, "dvs_bic_scores: n_vars must be in [1, 48]", i1=49, i3=None)              # range before null

    # (batch, n_vars, n_samples, data, card, parents, score_type, score_arg, scratch, out, status, stream)
    c = entry("dvs_bn_scores", [8, 12, 100, D, D, D, BIC, nan, D, D, D, None])
    c(3, "dvs_bn_scores: n_vars must be in [1, 48]", i1=49)
    c(10, "dvs_bn_scores: null pointer", i10=None)
    c(12, "dvs_bn_scores: score_type is not a dvs_score_type", i6=7)
    c(13, "dvs_bn_scores: loglik, k2 and bdj take no argument (score_arg must be NaN)", i6=K2, i7=1.0)
    c(13, "dvs_bn_scores: k must be finite and >= 0", i7=-1.0)
    c(13, "dvs_bn_scores: iss must be finite and > 0", i6=dl.SCORE_TYPES["bde"], i7=0.0)
    c(10, "dvs_bn_scores: null pointer", i3=None, i6=7)                            # null before score_type

    # (batch, n_vars, n_samples, data, card, parents, score_type, score_arg, worklist (nullable), local, local_bytes, toggles,
    #  toggles_bytes, status, stream)
    c = entry("dvs_bn_toggle_scores", [8, 12, 100, D, D, D, BIC, nan, None, D, 768, D, 9216, D, None])
    c(3, "dvs_bn_toggle_scores: n_vars must be in [1, 48]", i1=49)
    c(2, "dvs_bn_toggle_scores: batch * n_vars^2 must be < 2^31", i0=1 << 20, i1=48)
    c(10, "dvs_bn_toggle_scores: null pointer", i11=None)
    c(14, "dvs_bn_toggle_scores: local_bytes < batch * n_vars * 8 = 768", i10=767)
    c(14, "dvs_bn_toggle_scores: toggles_bytes < batch * n_vars^2 * 8 = 9216", i12=9215)
    c(2, "dvs_bn_toggle_scores: batch and n_samples must be > 0", i0=0, i1=49)     # batch before n_vars
    c(3, "dvs_bn_toggle_scores: n_vars must be in [1, 48]", i1=49, i9=None)        # range before null
    c(12, "dvs_bn_toggle_scores: score_type is not a dvs_score_type", i6=-1, i10=0)     # score type before local_bytes
    c(14, "dvs_bn_toggle_scores: local_bytes <", i10=0, i12=0)                     # local_bytes before toggles_bytes

    # (batch, n_vars, parents, local, toggles, toggles_bytes, max_parents, min_delta, forbidden (nullable), step_cap, worklist,
    #  steps, converged, flags, trace (nullable), trace_bytes, active, stream)
    hc = [8, 12, D, D, D, 9216, 0, 0.0, None, 10, D, D, D, D, D, 1280, D, None]
    c = entry("dvs_hc_step", hc)
    c(2, "dvs_hc_step: batch must be > 0", i0=0)
    c(3, "dvs_hc_step: n_vars must be in [1, 48]", i1=49)
    c(2, "dvs_hc_step: batch * n_vars^2 must be < 2^31", i0=1 << 20, i1=48)
    c(10, "dvs_hc_step: null pointer", i16=None)
    c(13, "dvs_hc_step: min_delta must not be NaN", i7=nan)
    c(13, "dvs_hc_step: step_cap must be >= 1", i9=0)
    c(14, "dvs_hc_step: toggles_bytes < batch * n_vars^2 * 8 = 9216", i5=9215)
    c(14, "dvs_hc_step: trace_bytes < batch * step_cap * 16 = 1280", i15=1279)
    c(3, "dvs_hc_step: n_vars must be in [1, 48]", i1=49, i2=None)                 # range before null
    c(10, "dvs_hc_step: null pointer", i12=None, i9=0)                             # null before step_cap
    c(13, "dvs_hc_step: step_cap must be >= 1", i9=0, i5=0)                        # step_cap before toggles_bytes
    c(14, "dvs_hc_step: toggles_bytes <", i5=0, i15=0)                             # toggles_bytes before trace_bytes

    # (... as dvs_hc_step up to active ..., tabu_len, ring, ring_bytes, visited, max_stall, stall, best_score, best_parents,
    #  best_bytes, stream)
    c = entry("dvs_tabu_step", hc[:-1] + [5, D, 3840, D, 4, D, D, D, 768, None])
    c(3, "dvs_tabu_step: n_vars must be in [1, 48]", i1=49)
    c(2, "dvs_tabu_step: batch * n_vars^2 must be < 2^31", i0=1 << 20, i1=48)
    c(10, "dvs_tabu_step: null pointer", i18=None)
    c(10, "dvs_tabu_step: null pointer", i24=None)
    c(13, "dvs_tabu_step: min_delta must not be NaN", i7=nan)
    c(13, "dvs_tabu_step: tabu_len must be >= 1", i17=0)
    c(13, "dvs_tabu_step: max_stall must be >= 1", i21=0)
    c(14, "dvs_tabu_step: toggles_bytes < batch * n_vars^2 * 8 = 9216", i5=9215)
    c(14, "dvs_tabu_step: trace_bytes < batch * step_cap * 16 = 1280", i15=1279)
    c(14, "dvs_tabu_step: ring_bytes < batch * tabu_len * n_vars * 8 = 3840", i19=3839)
    c(14, "dvs_tabu_step: best_bytes < batch * n_vars * 8 = 768", i25=767)
    c(3, "dvs_tabu_step: n_vars must be in [1, 48]", i1=49, i20=None)              # range before null
    c(13, "dvs_tabu_step: step_cap must be >= 1", i9=0, i17=0)                     # step_cap before tabu_len
    c(13, "dvs_tabu_step: tabu_len must be >= 1", i17=0, i21=0)                    # tabu_len before max_stall
    c(14, "dvs_tabu_step: trace_bytes <", i15=0, i19=0)                            # trace_bytes before ring_bytes
    c(14, "dvs_tabu_step: ring_bytes <", i19=0, i25=0)                             # ring_bytes before best_bytes

    # (batch, n_vars, parents, local, toggles, toggles_bytes, max_parents, forbidden (nullable), worklist, flags, seed,
    #  draw_index, stream)
    c = entry("dvs_hc_perturb", [8, 12, D, D, D, 9216, 0, None, D, D, 7, 0, None])
    c(2, "dvs_hc_perturb: batch must be > 0", i0=-1)
    c(3, "dvs_hc_perturb: n_vars must be in [1, 48]", i1=49)
    c(2, "dvs_hc_perturb: batch * n_vars^2 must be < 2^31", i0=1 << 20, i1=48)
    c(10, "dvs_hc_perturb: null pointer", i9=None)
    c(14, "dvs_hc_perturb: toggles_bytes < batch * n_vars^2 * 8 = 9216", i5=9215)
    c(3, "dvs_hc_perturb: n_vars must be in [1, 48]", i1=0, i3=None)               # range before null
    c(10, "dvs_hc_perturb: null pointer", i8=None, i5=0)                           # null before toggles_bytes

    # (batch, n_vars, preds_are_u64, labels, preds, parents, status, stream)
    c = entry("dvs_bic_parent_masks", [8, 12, 0, D, D, D, D, None])
    c(3, "dvs_bic_parent_masks: n_vars must be in [1, 48]", i1=49)
    c(10, "dvs_bic_parent_masks: null pointer", i5=None)
    c(12, "dvs_bic_parent_masks: 16-bit predecessor rows hold at most 16 vertices", i1=17, i3=None)   # row width before null

    # (batch, n_inducing, dim, x, inducing, alpha, outputscale, lengthscale, constant, out, stream)
    c = entry("dvs_gp_predict", [8, 50, 32, D, D, D, 1.0, 1.0, 0.0, D, None])
    c(2, "dvs_gp_predict: sizes must be > 0", i1=0)
    c(10, "dvs_gp_predict: null pointer", i9=None)
    c(5, "dvs_gp_predict: lengthscale must be > 0", i7=0.0, i3=None)               # lengthscale before null

    # (na, nb, dim, xa, xb, outputscale, lengthscale, K, stream)
    c = entry("dvs_gp_kernel", [8, 50, 32, D, D, 1.0, 1.0, D, None])
    c(2, "dvs_gp_kernel: sizes must be > 0 and dim <= 32", i2=33)
    c(10, "dvs_gp_kernel: null pointer", i7=None)
    c(5, "dvs_gp_kernel: lengthscale and outputscale must be > 0", i5=0.0, i3=None)     # outputscale before null

    # (na, nb, dim, symmetric, xa, xb, outputscale, lengthscale, G, dxa, row_sums, stream)
    c = entry("dvs_gp_kernel_backward", [8, 50, 32, 0, D, D, 1.0, 1.0, D, D, D, None])
    c(2, "dvs_gp_kernel_backward: sizes must be > 0 and dim <= 32", i0=0)
    c(5, "dvs_gp_kernel_backward: lengthscale and outputscale must be > 0", i7=nan)
    c(10, "dvs_gp_kernel_backward: null pointer", i10=None)
    c(12, "dvs_gp_kernel_backward: symmetric needs na == nb", i3=1)
    c(10, "dvs_gp_kernel_backward: null pointer", i3=1, i8=None)                   # null before symmetric

    # (batch, n_inducing, dim, ld, x, inducing, weights, c0, outputscale, lengthscale, constant, best, xi, mean, var, ei,
    #  grad (nullable), stream)
    c = entry("dvs_gp_acquire", [8, 50, 32, 51, D, D, D, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, D, D, D, None, None])
    c(2, "dvs_gp_acquire: sizes must be > 0 and dim <= 32", i2=0)
    c(2, "dvs_gp_acquire: n_inducing must be <= 1023", i1=1024, i3=1025)
    c(12, "dvs_gp_acquire: ld must be >= n_inducing + 1 (P | alpha)", i3=50)
    c(12, "dvs_gp_acquire: c0 must be >= 0", i7=-1.0)
    c(10, "dvs_gp_acquire: null pointer", i15=None)
    c(5, "dvs_gp_acquire: lengthscale and outputscale must be > 0", i9=0.0, i1=1024)    # scales before n_inducing
    c(12, "dvs_gp_acquire: ld must be >= n_inducing + 1", i3=50, i4=None)          # ld before null
    return cases


def test_search_entry_points_validate_in_a_fixed_order_before_anything_is_enqueued():
    """The 16 search-side entry points (include/dvs.h, from dvs_match_decoded to dvs_gp_acquire): return code and
    dvs_last_error text of every kind of refusal, and which check decides when two fail.  Like the test above, no case
    reaches a HIP call, so dummy non-null pointers do."""
    lib = dl.load()
    cases = _search_validation_cases()
    assert len({fn for fn, *_ in cases}) == 16
    assert lib.dvs_structset_filter(0, 12, None, None, None, 0, None, 0, None, None, 0, None, None) == 0   # an empty batch
    for fn, args, code, text in cases:
        got = getattr(lib, fn)(*args)
        msg = lib.dvs_last_error().decode()
        assert (got, text in msg, msg.startswith(fn + ":")) == (code, True, True), (fn, args, got, msg)
