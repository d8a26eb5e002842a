"""The evaluator surface is stated once (dags_vae_search_amd/evaluator.py): structure and host-side checks."""
import numpy as np
import pytest
import torch

from dags_vae_search_amd import _lib as dl
from dags_vae_search_amd import evaluator as ev
from dags_vae_search_amd.bic import AvailableCaseEvaluator, BNLearnWrapper, RowSetEvaluator
from dags_vae_search_amd.gaussian import GaussianEvaluator, GaussianRowSetEvaluator
from dags_vae_search_amd.mixed import MixedEvaluator

KINDS = {BNLearnWrapper: "discrete", RowSetEvaluator: "discrete", AvailableCaseEvaluator: "discrete",
         GaussianEvaluator: "continuous", GaussianRowSetEvaluator: "continuous", MixedEvaluator: "mixed"}
SHARED = ("score_masks", "toggle_scores", "launch_scores", "compact_parent_masks", "_compact_parent_masks")


def raises(exc, text, fn, *args, **kwargs):
    with pytest.raises(exc) as e:
        fn(*args, **kwargs)
    assert str(e.value) == text


@pytest.mark.parametrize("cls", list(KINDS), ids=lambda c: c.__name__)
def test_the_shared_methods_live_in_the_base_class_only(cls):
    assert issubclass(cls, ev.Evaluator) and cls.data_kind == KINDS[cls]
    for name in SHARED:
        assert name in vars(ev.Evaluator)
        for klass in cls.__mro__[:cls.__mro__.index(ev.Evaluator)]:
            assert name not in vars(klass), (klass.__name__, name)
    for hook in ("_launch_scores", "_launch_toggles", "_refusal"):
        assert callable(getattr(cls, hook))


class Stub:
    pass


def stub(kind):
    s = Stub()
    s.data_kind = kind
    return s


def test_data_kind_refusals_keep_their_messages():
    for s in (Stub(), stub("discrete")):
        dl.need_unmixed("bn_fit", s)
        dl.need_discrete("bn_fit", s)
    dl.need_unmixed("bn_fit", stub("continuous"))
    mixed = ("bn_fit: the evaluator holds mixed data (factors and real columns) and mixed data is not built for bn_fit: "
             "hill_climb, tabu_search, score_masks and cg_fit are")
    raises(ValueError, mixed, dl.need_unmixed, "bn_fit", stub("mixed"))
    raises(ValueError, mixed, dl.need_discrete, "bn_fit", stub("mixed"))
    raises(ValueError, "bn_fit: the evaluator holds real-valued data and bn_fit reads discrete levels: its Gaussian counterpart "
                       "is not built", dl.need_discrete, "bn_fit", stub("continuous"))
    raises(ValueError, "mmpc: the evaluator holds real-valued data and mmpc reads discrete levels (its tests on real-valued data "
                       "are test=\"cor\", \"zf\" and \"mi-g\"): its Gaussian counterpart is not built",
           dl.need_discrete, "mmpc", stub("continuous"))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_row_sets_checks_run_on_cpu_tensors(dtype):
    S = 5
    rows = torch.tensor([[0, 4, 4], [1, 1, 0]], dtype=dtype)
    sets = ev.RowSets(rows, None, S, "cpu")
    assert sets.rows.dtype == torch.int32 and sets.rows.tolist() == rows.tolist() and sets.rows.is_contiguous()
    assert (sets.n_sets, sets.set_size, sets.set_of) == (2, 3, None)
    assert sets.of(1) == (2, None) and sets.of(2) == (2, None)
    raises(ValueError, "3 structures but 2 row sets: pass set_of", sets.of, 3)
    named = ev.RowSets(rows, torch.tensor([1, 0, 1], dtype=dtype), S, "cpu")
    assert named.set_of.dtype == torch.int32 and named.of(3)[1].tolist() == [1, 0, 1]
    raises(ValueError, "2 structures but set_of names 3", named.of, 2)
    shape = "rows must be an integer tensor [n_sets >= 1, set_size >= 1]"
    raises(ValueError, shape, ev.RowSets, torch.tensor([0], dtype=dtype), None, S, "cpu")
    raises(ValueError, shape, ev.RowSets, torch.zeros(1, 1), None, S, "cpu")
    raises(ValueError, shape, ev.RowSets, [[0]], None, S, "cpu")
    raises(ValueError, "rows must lie in [0, 5)", ev.RowSets, torch.tensor([[S]], dtype=dtype), None, S, "cpu")
    raises(ValueError, "rows must lie in [0, 5)", ev.RowSets, torch.tensor([[-1]], dtype=dtype), None, S, "cpu")
    raises(ValueError, "set_of must be an integer tensor [B]", ev.RowSets, rows, torch.zeros(1, 1, dtype=dtype), S, "cpu")
    raises(ValueError, "set_of must be an integer tensor [B]", ev.RowSets, rows, torch.zeros(1), S, "cpu")
    raises(ValueError, "set_of must lie in [0, 2)", ev.RowSets, rows, torch.tensor([2], dtype=dtype), S, "cpu")


def test_score_argument_validators():
    takers = ("aic", "bic")
    for k in (None, 0.0, 2.5):
        ev.check_k(k, "bic", takers)
    ev.check_k(None, "bde", takers)
    for bad in (float("nan"), -1.0, float("inf")):
        raises(ValueError, f"k must be finite and >= 0 (got {bad!r})", ev.check_k, bad, "aic", takers)
    raises(ValueError, "k is the argument of aic / bic, not of 'bde'", ev.check_k, 1.0, "bde", takers)
    raises(ValueError, "k is the argument of pnal, not of 'nal'", ev.check_k, 1.0, "nal", ("pnal",))
    ev.check_positive("iss", None, "k2", ("bde", "bds"))
    ev.check_positive("iss", 1.5, "bds", ("bde", "bds"))
    ev.check_positive("iss_mu", 1.5)
    for bad in (float("nan"), -1.0, 0.0):
        raises(ValueError, f"iss must be finite and > 0 (got {bad!r})", ev.check_positive, "iss", bad, "bde", ("bde", "bds"))
        raises(ValueError, f"iss_mu must be finite and > 0 (got {bad!r})", ev.check_positive, "iss_mu", bad)
    raises(ValueError, "iss is the argument of bde / bds, not of 'bic'", ev.check_positive, "iss", 1.0, "bic", ("bde", "bds"))
    assert np.isnan(ev.score_arg(None)) and ev.score_arg(3) == 3.0 and isinstance(ev.score_arg(3), float)


def test_constructors_refuse_an_unknown_metric_before_the_device():
    levels, real = np.zeros((4, 3), np.int64), np.zeros((4, 3))
    raises(NotImplementedError, "built scores: aic, bde, bdj, bds, bic, k2, loglik (got 'nope')", BNLearnWrapper, "x", "nope", data=levels)
    raises(NotImplementedError, "built Gaussian scores: aic-g, bge, bic-g, loglik-g (got 'nope')", GaussianEvaluator, "x", "nope", data=real)
    raises(NotImplementedError, "built mixed-data scores: aic-cg, bic-cg, loglik-cg (got 'nope')", MixedEvaluator, "x", "nope",
           data=real, discrete=[2, 0, 0])
    raises(NotImplementedError, "available-case scores: nal, pnal (got 'nope')", AvailableCaseEvaluator, None, None, "nope")
    # the arguments are judged on the host too
    raises(ValueError, "k is the argument of aic / bic, not of 'k2'", BNLearnWrapper, "x", "k2", data=levels, k=1.0)
    raises(ValueError, "k is the argument of aic-g / bic-g, not of 'bge'", GaussianEvaluator, "x", "bge", data=real, k=1.0)
    raises(ValueError, "iss_w must be finite and > n_vars + 1 = 4 (got 4.0)", GaussianEvaluator, "x", "bge", data=real, iss_w=4.0)
    raises(ValueError, "k is the argument of aic-cg / bic-cg, not of 'loglik-cg'", MixedEvaluator, "x", "loglik-cg", data=real,
           discrete=[2, 0, 0], k=1.0)


def test_pack_levels_nibble_layout():
    codes = np.array([[(r + v) % 16 for v in range(17)] for r in range(3)], np.uint8)
    want = np.zeros((3, 2), np.uint64)
    for r in range(3):
        word0 = 0
        for v in range(16):
            word0 |= int(codes[r, v]) << (4 * v)
        want[r] = word0, int(codes[r, 16])                  # variable 16: the low nibble of word 1
    got = ev.pack_levels(codes, range(17), 17)
    assert got.dtype == np.int64 and got.shape == (3, 2) and got.view(np.uint64).tolist() == want.tolist()
    assert want[0, 0] == 0xFEDCBA9876543210 and want[2].tolist() == [0x10FEDCBA98765432, 2]
    # some columns of a wider data set: the other nibbles stay zero
    some = ev.pack_levels(codes[:, [1, 16]], [1, 16], 17)
    assert some.view(np.uint64).tolist() == [[int(codes[r, 1]) << 4, int(codes[r, 16])] for r in range(3)]
