"""The C-ABI library loads on a CPU-only box and exports every symbol include/dvs.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

from dags_vae_search_amd import _lib as dl
from tests.abi_cases import call, call_rc, entry, run

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


def test_binding_is_derived_from_the_header_with_the_types_the_hand_written_table_had():
    """dl.SIGNATURES (what bind() declares) on the real header: restype and argtypes of the entry points that cover every kind
    of type the header uses, written out as the hand-written table had them."""
    from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p
    P, S = c_void_p, POINTER(dl.DvsShape)
    expected = {
        "dvs_version": (c_int, []),
        "dvs_last_error": (c_char_p, []),
        "dvs_param_table": (c_int, [S, POINTER(dl.DvsParamEntry), c_int]),
        "dvs_profile_enable": (None, [c_int]),
        "dvs_profile_collect": (c_int, [P, c_int, P, P, c_int]),
        "dvs_loss_forward_notify": (c_int, [S, P, c_size_t, P, c_int64, P, c_size_t, P, P, P, P, P, P, c_uint32, P]),
        "dvs_clip_adam": (c_int, [c_int64, P, P, P, P, c_float, c_float, c_float, c_float, c_int64, c_float, P, P, P]),
        "dvs_bn_lw": (c_int, [c_int32, c_int64, c_int64, P, P, P, P, c_int64, P, P, P, c_uint64, c_uint64, c_int64, P, c_size_t,
                              P, P, P, P, P, P]),
        "dvs_order_mcmc": (c_int, [c_int32, c_int32, c_int64, c_int32, P, P, c_size_t, P, c_size_t, c_uint64, c_int64, c_int64,
                                   c_int64, c_int32, c_int32, c_int32, P, P, P, P, c_size_t, P, P, P, P, c_size_t, P, P]),
    }
    for fn, (restype, argtypes) in expected.items():
        got_restype, args = dl.SIGNATURES[fn]
        assert (got_restype, [t for _, t in args]) == (restype, argtypes), fn
    assert [name for name, _ in dl.SIGNATURES["dvs_profile_collect"][1]] == ["names", "name_stride", "counts", "total_ms", "cap"]
    assert dl.EXPORTS == list(dl.SIGNATURES) and len(dl.EXPORTS) == 64
    assert (dl.ABI_VERSION, dl.RECORD_BYTES, dl.DECODE_STATE_BYTES, dl.LOSS_FLOATS) == (202, 96, 440, 5)
    assert dl.STRUCT_HASH_INVALID == 2 ** 63 - 1 and dl.CI_TYPES["mi-adf"] == 2 and dl.FIT_METHODS == {"mle": 0, "bayes": 1}


def test_header_parser_on_small_headers():
    from ctypes import c_double, c_int, c_int32, c_size_t, c_uint64, c_void_p
    sigs, consts = dl.parse_header("""
        /* a comment with a call in it: dvs_fake(int a, (char*) b); and more ) ( */
        #define DVS_BIG 0x7fffffffffffffffull   // dvs_other_fake(
        #define DVS_SMALL 12
        typedef enum dvs_kind { DVS_KIND_A = 0, DVS_KIND_B = 3 } dvs_kind;
        typedef struct dvs_pair { int32_t a; int32_t b; } dvs_pair;
        size_t dvs_three_lines(int32_t batch,   /* the first */
                               const uint64_t* rows, double scale,
                               uint64_t seed);
        void dvs_nothing(void);
        int dvs_shaped(const dvs_shape* s, void* stream);
    """)
    assert consts == {"DVS_BIG": 2 ** 63 - 1, "DVS_SMALL": 12, "DVS_KIND_A": 0, "DVS_KIND_B": 3}
    assert list(sigs) == ["dvs_three_lines", "dvs_nothing", "dvs_shaped"]
    assert sigs["dvs_three_lines"] == (c_size_t, [("batch", c_int32), ("rows", c_void_p), ("scale", c_double), ("seed", c_uint64)])
    assert sigs["dvs_nothing"] == (None, [])
    assert sigs["dvs_shaped"] == (c_int, [("s", ctypes.POINTER(dl.DvsShape)), ("stream", c_void_p)])
    for bad, named in (("int dvs_short_arg(int32_t n, short s);", "dvs_short_arg"), ("int dvs_by_value(dvs_shape s);", "dvs_by_value"),
                       ("long dvs_long_return(int n);", "dvs_long_return"), ("int dvs_unnamed(int32_t);", "dvs_unnamed"),
                       ("static int dvs_counter = 0;", "dvs_counter")):
        with pytest.raises(ValueError, match=named):
            dl.parse_header(bad)


def test_a_missing_header_is_an_error_that_gives_the_path(monkeypatch, tmp_path):
    monkeypatch.setattr(dl, "HEADER", str(tmp_path / "include" / "dvs.h"))
    with pytest.raises(RuntimeError, match=re.escape(str(tmp_path / "include" / "dvs.h"))):
        dl._read_header()


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

    c = entry("dvs_match_decoded", cases, batch=8, n_vars=12, card=12, repeats=3, preds_are_u64=0, labels=D, preds=D,
              states=D, state_bytes=24 * SB, budget=100, flags=D, stream=None)
    c(3, "n_vars must be in [1, 45]", n_vars=46)
    c(2, "batch * repeats must be <= 2^30", batch=1 << 20, repeats=1 << 11)
    c(12, "16-bit predecessor rows hold at most 16 vertices", n_vars=17, card=17)
    c(10, "null pointer", labels=None)
    c(14, f"state_bytes < batch * repeats * DVS_DECODE_STATE_BYTES = {24 * SB}", state_bytes=24 * SB - 1)
    c(2, "batch and repeats must be > 0", batch=0, n_vars=46)                          # batch before n_vars
    c(3, "card must be in [1, 45]", card=46, flags=None)                               # range before null
    c(12, "budget must be >= 1", budget=0, states=None)                                # budget before null
    c(10, "null pointer", flags=None, state_bytes=0)                                   # null before state_bytes

    c = entry("dvs_decoded_structures", cases, batch=8, n_vars=12, preds_are_u64=0, states=D, state_bytes=8 * SB,
              hash_mask=2 ** 63 - 1, flags=D, labels=D, preds=D, keys=D, keys_bytes=768, hashes=D, stream=None)
    c(3, "n_vars must be in [1, 45]", n_vars=0)
    c(2, "batch must be <= 2^30", batch=(1 << 30) + 1)
    c(10, "null pointer", hashes=None)
    c(14, f"state_bytes < batch * DVS_DECODE_STATE_BYTES = {8 * SB}", state_bytes=8 * SB - 1)
    c(14, "keys_bytes < batch * n_vars * 8 = 768", keys_bytes=767)
    c(12, "16-bit predecessor rows", n_vars=17, states=None)                           # row width before null
    c(14, "state_bytes <", state_bytes=0, keys_bytes=0)                                # state_bytes before keys_bytes

    c = entry("dvs_structset_filter", cases, batch=8, n_vars=12, sorted_hashes=D, order=D, keys=D, keys_bytes=768, flags=D,
              seen_count=5, seen_hashes=D, seen_keys=D, seen_keys_bytes=480, out=D, stream=None)
    c(3, "n_vars must be in [1, 45]", n_vars=46)
    c(2, "batch and seen_count must be >= 0", seen_count=-1)
    c(10, "null pointer", out=None)
    c(10, "null pointer (seen set)", seen_hashes=None)
    c(14, "keys_bytes < batch * n_vars * 8 = 768", keys_bytes=767)
    c(14, "seen_keys_bytes < seen_count * n_vars * 8 = 480", seen_keys_bytes=479)
    c(10, "null pointer", sorted_hashes=None, keys_bytes=0)                            # null before keys_bytes
    c(14, "keys_bytes <", keys_bytes=0, seen_keys_bytes=0)                             # keys_bytes before seen_keys_bytes

    c = entry("dvs_generate_dags", cases, batch=8, n_vars=12, card=12, preds_are_u64=0, num_edges=D, seed=7, dag_offset=0,
              try_limit=20, flags=0, labels=D, preds=D, preds_bytes=192, attempts=D, stream=None)
    c(3, "n_vars must be in [2, 45]", n_vars=1)
    c(12, "unknown bits in flags", flags=8)
    c(12, "labels without replacement ('sample') need card >= n_vars", card=11)
    c(12, "predecessor rows are u16 for n_vars <= 13 and u64 above", preds_are_u64=1)
    c(12, "dag_offset must be >= 0", dag_offset=-1)
    c(10, "null pointer", attempts=None)
    c(14, "preds_bytes < batch * n_vars * row bytes = 192", preds_bytes=191)
    c(14, "preds_bytes < batch * n_vars * row bytes = 1280", n_vars=20, card=20, preds_are_u64=1, preds_bytes=1279)
    c(12, "try_limit must be in [1, 4096]", try_limit=0, num_edges=None)               # try_limit before null
    c(10, "null pointer", labels=None, preds_bytes=0)                                  # null before preds_bytes

    c = entry("dvs_generate_edge_counts", cases, batch=8, n_entries=4, edge_counts=D, cum_weights=D, seed=7, dag_offset=0,
              num_edges=D, stream=None)
    c(2, "batch must be in [1, 2^30]", batch=0)
    c(12, "n_entries must be in [1, 1024]", n_entries=1025)
    c(10, "null pointer", num_edges=None)
    c(12, "dag_offset must be >= 0", dag_offset=-1, edge_counts=None)                  # dag_offset before null

    c = entry("dvs_bic_scores", cases, batch=8, n_vars=12, n_samples=100, data=D, card=D, parents=D, scratch=D, out=D,
              status=D, stream=None)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "batch and n_samples must be > 0", n_samples=0)
    c(10, "null pointer", scratch=None)
    c(3, "n_vars must be in [1, 48]", n_vars=49, data=None)                            # range before null

    c = entry("dvs_bn_scores", cases, batch=8, n_vars=12, n_samples=100, data=D, card=D, parents=D, score_type=BIC,
              score_arg=nan, scratch=D, out=D, status=D, stream=None)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(10, "null pointer", status=None)
    c(12, "score_type is not a dvs_score_type", score_type=7)
    c(13, "loglik, k2 and bdj take no argument (score_arg must be NaN)", score_type=K2, score_arg=1.0)
    c(13, "k must be finite and >= 0", score_arg=-1.0)
    c(13, "iss must be finite and > 0", score_type=dl.SCORE_TYPES["bde"], score_arg=0.0)
    c(10, "null pointer", data=None, score_type=7)                                     # null before score_type

    c = entry("dvs_bn_toggle_scores", cases, batch=8, n_vars=12, n_samples=100, data=D, card=D, parents=D, score_type=BIC,
              score_arg=nan, worklist=None, local=D, local_bytes=768, toggles=D, toggles_bytes=9216, status=D, stream=None)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "batch * n_vars^2 must be < 2^31", batch=1 << 20, n_vars=48)
    c(10, "null pointer", toggles=None)
    c(14, "local_bytes < batch * n_vars * 8 = 768", local_bytes=767)
    c(14, "toggles_bytes < batch * n_vars^2 * 8 = 9216", toggles_bytes=9215)
    c(2, "batch and n_samples must be > 0", batch=0, n_vars=49)                        # batch before n_vars
    c(3, "n_vars must be in [1, 48]", n_vars=49, local=None)                           # range before null
    c(12, "score_type is not a dvs_score_type", score_type=-1, local_bytes=0)          # score type before local_bytes
    c(14, "local_bytes <", local_bytes=0, toggles_bytes=0)                             # local_bytes before toggles_bytes

    # (batch, n_vars, parents, local, toggles, toggles_bytes, max_parents, min_delta, forbidden (nullable), step_cap, worklist,
    #  steps, converged, flags, trace (nullable), trace_bytes, active, stream)
    hc = dict(batch=8, n_vars=12, parents=D, local=D, toggles=D, toggles_bytes=9216, max_parents=0, min_delta=0.0,
              forbidden=None, step_cap=10, worklist=D, steps=D, converged=D, flags=D, trace=D, trace_bytes=1280, active=D)
    c = entry("dvs_hc_step", cases, **hc, stream=None)
    c(2, "batch must be > 0", batch=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "batch * n_vars^2 must be < 2^31", batch=1 << 20, n_vars=48)
    c(10, "null pointer", active=None)
    c(13, "min_delta must not be NaN", min_delta=nan)
    c(13, "step_cap must be >= 1", step_cap=0)
    c(14, "toggles_bytes < batch * n_vars^2 * 8 = 9216", toggles_bytes=9215)
    c(14, "trace_bytes < batch * step_cap * 16 = 1280", trace_bytes=1279)
    c(3, "n_vars must be in [1, 48]", n_vars=49, parents=None)                         # range before null
    c(10, "null pointer", converged=None, step_cap=0)                                  # null before step_cap
    c(13, "step_cap must be >= 1", step_cap=0, toggles_bytes=0)                        # step_cap before toggles_bytes
    c(14, "toggles_bytes <", toggles_bytes=0, trace_bytes=0)                           # toggles_bytes before trace_bytes

    c = entry("dvs_tabu_step", cases, **hc, tabu_len=5, ring=D, ring_bytes=3840, visited=D, max_stall=4, stall=D,
              best_score=D, best_parents=D, best_bytes=768, stream=None)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "batch * n_vars^2 must be < 2^31", batch=1 << 20, n_vars=48)
    c(10, "null pointer", ring=None)
    c(10, "null pointer", best_parents=None)
    c(13, "min_delta must not be NaN", min_delta=nan)
    c(13, "tabu_len must be >= 1", tabu_len=0)
    c(13, "max_stall must be >= 1", max_stall=0)
    c(14, "toggles_bytes < batch * n_vars^2 * 8 = 9216", toggles_bytes=9215)
    c(14, "trace_bytes < batch * step_cap * 16 = 1280", trace_bytes=1279)
    c(14, "ring_bytes < batch * tabu_len * n_vars * 8 = 3840", ring_bytes=3839)
    c(14, "best_bytes < batch * n_vars * 8 = 768", best_bytes=767)
    c(3, "n_vars must be in [1, 48]", n_vars=49, visited=None)                         # range before null
    c(13, "step_cap must be >= 1", step_cap=0, tabu_len=0)                             # step_cap before tabu_len
    c(13, "tabu_len must be >= 1", tabu_len=0, max_stall=0)                            # tabu_len before max_stall
    c(14, "trace_bytes <", trace_bytes=0, ring_bytes=0)                                # trace_bytes before ring_bytes
    c(14, "ring_bytes <", ring_bytes=0, best_bytes=0)                                  # ring_bytes before best_bytes

    c = entry("dvs_hc_perturb", cases, batch=8, n_vars=12, parents=D, local=D, toggles=D, toggles_bytes=9216, max_parents=0,
              forbidden=None, worklist=D, flags=D, seed=7, draw_index=0, stream=None)
    c(2, "batch must be > 0", batch=-1)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "batch * n_vars^2 must be < 2^31", batch=1 << 20, n_vars=48)
    c(10, "null pointer", flags=None)
    c(14, "toggles_bytes < batch * n_vars^2 * 8 = 9216", toggles_bytes=9215)
    c(3, "n_vars must be in [1, 48]", n_vars=0, local=None)                            # range before null
    c(10, "null pointer", worklist=None, toggles_bytes=0)                              # null before toggles_bytes

    c = entry("dvs_bic_parent_masks", cases, batch=8, n_vars=12, preds_are_u64=0, labels=D, preds=D, parents=D, status=D,
              stream=None)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(10, "null pointer", parents=None)
    c(12, "16-bit predecessor rows hold at most 16 vertices", n_vars=17, labels=None)  # row width before null

    c = entry("dvs_gp_predict", cases, batch=8, n_inducing=50, dim=32, x=D, inducing=D, alpha=D, outputscale=1.0,
              lengthscale=1.0, constant=0.0, out=D, stream=None)
    c(2, "sizes must be > 0", n_inducing=0)
    c(10, "null pointer", out=None)
    c(5, "lengthscale must be > 0", lengthscale=0.0, x=None)                           # lengthscale before null

    c = entry("dvs_gp_kernel", cases, na=8, nb=50, dim=32, xa=D, xb=D, outputscale=1.0, lengthscale=1.0, K=D, stream=None)
    c(2, "sizes must be > 0 and dim <= 32", dim=33)
    c(10, "null pointer", K=None)
    c(5, "lengthscale and outputscale must be > 0", outputscale=0.0, xa=None)          # outputscale before null

    c = entry("dvs_gp_kernel_backward", cases, na=8, nb=50, dim=32, symmetric=0, xa=D, xb=D, outputscale=1.0,
              lengthscale=1.0, G=D, dxa=D, row_sums=D, stream=None)
    c(2, "sizes must be > 0 and dim <= 32", na=0)
    c(5, "lengthscale and outputscale must be > 0", lengthscale=nan)
    c(10, "null pointer", row_sums=None)
    c(12, "symmetric needs na == nb", symmetric=1)
    c(10, "null pointer", symmetric=1, G=None)                                         # null before symmetric

    c = entry("dvs_gp_acquire", cases, batch=8, n_inducing=50, dim=32, ld=51, x=D, inducing=D, weights=D, c0=0.0,
              outputscale=1.0, lengthscale=1.0, constant=0.0, best=0.0, xi=0.0, mean=D, var=D, ei=D, grad=None, stream=None)
    c(2, "sizes must be > 0 and dim <= 32", dim=0)
    c(2, "n_inducing must be <= 1023", n_inducing=1024, ld=1025)
    c(12, "ld must be >= n_inducing + 1 (P | alpha)", ld=50)
    c(12, "c0 must be >= 0", c0=-1.0)
    c(10, "null pointer", ei=None)
    c(5, "lengthscale and outputscale must be > 0", lengthscale=0.0, n_inducing=1024)  # scales before n_inducing
    c(12, "ld must be >= n_inducing + 1", ld=50, x=None)                               # ld before null
    return cases


def test_search_entry_points_validate_in_a_fixed_order_before_anything_is_enqueued():
    """The 16 search-side entry points (include/dvs.h, from dvs_match_decoded to dvs_gp_acquire): return code and
    dvs_last_error text of every kind of refusal, and which check decides when two fail.  Like the test above, no case
    reaches a HIP call, so dummy non-null pointers do."""
    lib = dl.load()
    cases = _search_validation_cases()
    assert len({fn for fn, *_ in cases}) == 16
    assert lib.dvs_structset_filter(0, 12, None, None, None, 0, None, 0, None, None, 0, None, None) == 0   # an empty batch
    run(lib, cases)


# ---- tests/abi_cases.py: call / call_rc against a recording stand-in library (no device, no emulator build)
FN = "dvs_tabu_step"
NAMES = [name for name, _ in dl.SIGNATURES[FN][1]]
POINTERS = [name for name, ctype in dl.SIGNATURES[FN][1] if ctype is ctypes.c_void_p and name != "stream"]


class Backend:
    """its own recording library: every dvs_* call returns `rc`; a handle is ("h", k), at address 0x1000 + k"""
    stream = ctypes.c_void_p(0x5000)

    def __init__(self, rc=0):
        self.lib, self.rc, self.calls = self, rc, []

    def __getattr__(self, fn):
        return lambda *args: self.calls.append((fn, args)) or self.rc

    def dvs_last_error(self):
        return b"dvs_tabu_step: ring_bytes < 768"

    def ptr(self, h):
        assert h[0] == "h"
        return ctypes.c_void_p(0x1000 + h[1])


def full_args():
    """every argument of FN but the stream: the k-th a handle if it is a pointer, else the scalar 100 + k"""
    return {name: ("h", k) if name in POINTERS else 100 + k for k, name in enumerate(NAMES) if name != "stream"}


def test_arguments_go_in_the_order_of_the_header():
    assert len(NAMES) > 20
    be, raw = Backend(), ctypes.c_void_p(4096)
    args = {**full_args(), "forbidden": None, "ring": raw}
    assert call(be, FN, **dict(reversed(args.items()))) is None              # the order they are named in does not matter
    (fn, got), = be.calls
    assert fn == FN and len(got) == len(NAMES)
    for k, (name, value) in enumerate(zip(NAMES, got)):
        if name in ("stream", "forbidden", "ring"):                          # from the backend; NULL; a c_void_p as it is
            assert value is {"stream": be.stream, "forbidden": None, "ring": raw}[name]
        elif name in POINTERS:
            assert isinstance(value, ctypes.c_void_p) and value.value == 0x1000 + k, name      # a handle goes through be.ptr
        else:
            assert value == 100 + k, name
    shape = ctypes.byref(dl.make_shape(2, 8, 4))                             # a struct pointer and a given stream are kept
    call(be, "dvs_decode", s=shape, params=("h", 1), n_params=7, workspace=("h", 2), workspace_bytes=64, records=("h", 3),
         records_bytes=192, z=("h", 4), uniforms=None, state_out=("h", 5), state_bytes=880, stream=raw)
    assert be.calls[1][1][0] is shape and be.calls[1][1][1].value == 0x1001 and be.calls[1][1][-1] is raw


@pytest.mark.parametrize("change,listed", [({"ring_bytes": None}, "missing ['ring_bytes'], unknown []"),
                                           ({"ring_size": 1}, "missing [], unknown ['ring_size']")])
def test_a_missing_or_unknown_name_is_a_type_error(change, listed):
    be = Backend()
    args = {k: v for k, v in {**full_args(), **change}.items() if v is not None}
    for fn in (lambda: call(be, FN, **args), lambda: call_rc(be, FN, **args), lambda: entry(FN, [], stream=None, **args)):
        with pytest.raises(TypeError, match=FN) as e:                        # entry() shares the check
            fn()
        assert listed in str(e.value)
    assert be.calls == []


def test_a_refusal_fails_call_with_the_message_and_is_returned_by_call_rc():
    be = Backend(rc=14)
    with pytest.raises(AssertionError, match="dvs_tabu_step: ring_bytes < 768"):
        call(be, FN, **full_args())
    assert call_rc(be, FN, **full_args()) == 14 and len(be.calls) == 2
