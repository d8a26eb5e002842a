"""The device-call layer of ``_lib.py``, as far as it can be checked without a device: the wording of
the device check, the seed mask, the ``forbidden`` conversion and the refusals of the shared validators."""
import numpy as np
import pytest
import torch

from dags_vae_search_amd import _lib as dl


def test_need_cuda_message():
    with pytest.raises(RuntimeError) as e:
        dl.need_cuda("hill_climb", torch.device("cpu"))
    assert str(e.value) == "dags_vae_search_amd: hill_climb runs on the GPU (got device cpu); this package has no CPU path"
    with pytest.raises(RuntimeError, match=r"bn_fit runs on the GPU \(got device cpu\); this package has no CPU path"):
        dl.need_cuda("bn_fit", "cpu")
    dl.need_cuda("anything", "cuda:0")               # names a device, touches none
    with pytest.raises(RuntimeError) as e:
        dl.require_cuda(torch.zeros(1), "states")
    assert str(e.value) == "dags_vae_search_amd: states must live on the GPU (got device cpu); this package has no CPU path"


def test_seed64_keeps_the_low_64_bits():
    assert dl.seed64(7) == 7
    assert dl.seed64(-1) == 0xFFFFFFFFFFFFFFFF
    assert dl.seed64(-(1 << 63)) == 1 << 63
    assert dl.seed64((1 << 64) + 5) == 5
    assert dl.seed64((0xABCD << 64) | 0x0123456789ABCDEF) == 0x0123456789ABCDEF
    assert dl.make_shape(1, 8, 8, seed=-2).seed == 0xFFFFFFFFFFFFFFFE


def test_ptr_and_nbytes():
    t = torch.zeros(4, 3, dtype=torch.float64)
    assert dl.ptr(None) is None
    assert dl.ptr(t).value == t.data_ptr()
    assert dl.ptr(t, 16).value == t.data_ptr() + 16
    assert dl.nbytes(t) == 96


def test_forbidden_rows_keep_bit_63():
    rows = np.array([1 << 63, (1 << 63) | 5, 0], np.uint64)
    forb = dl.forbidden_rows(rows, 3, "cpu")
    assert forb.dtype == torch.int64 and forb.shape == (3,) and forb.is_contiguous()
    assert forb.tolist() == [-(1 << 63), -(1 << 63) + 5, 0]            # the same 64 bits, read as signed
    assert dl.forbidden_rows([1 << 63, 2, 4], 3, "cpu").tolist() == [-(1 << 63), 2, 4]     # Python ints go the same way
    given = torch.tensor([3, 0, -1], dtype=torch.int64)
    assert dl.forbidden_rows(given, 3, "cpu").tolist() == [3, 0, -1]
    assert dl.forbidden_rows(None, 3, "cpu") is None
    with pytest.raises(ValueError, match=r"forbidden must be \[4\] bit rows"):
        dl.forbidden_rows(rows, 4, "cpu")
    with pytest.raises(ValueError, match=r"forbidden must be \[3\] bit rows"):
        dl.forbidden_rows(torch.zeros(1, 3, dtype=torch.int64), 3, "cpu")


def test_level_counts_refusals():
    assert dl.level_counts(np.array([2, 16, 1], np.uint8)) == [2, 16, 1]
    assert dl.level_counts([3] * 48) == [3] * 48
    for bad in ([], [2] * 49, [2, 0], [2, 17], [-1]):
        with pytest.raises(ValueError, match=r"card must hold 1\.\.48 level counts in 1\.\.16"):
            dl.level_counts(bad)


class _Evaluator:
    def __init__(self, n_vars, packed):
        self.n_vars, self.packed = n_vars, packed


def test_packed_rows_refusals():
    what = "log_likelihood"
    shape_msg = r"log_likelihood: data must be an evaluator or packed int64 rows \[S >= 1, 2\]"
    for bad in (torch.zeros(5, 2, dtype=torch.int32), torch.zeros(5, 1, dtype=torch.int64), torch.zeros(0, 2, dtype=torch.int64),
                torch.zeros(10, dtype=torch.int64), np.zeros((5, 2), np.int64), None):
        with pytest.raises(ValueError, match=shape_msg):
            dl.packed_rows(what, bad, 17)                        # 17 variables take two words a row
    with pytest.raises(ValueError, match="log_likelihood: the evaluator has 8 variables, the network 17"):
        dl.packed_rows(what, _Evaluator(8, torch.zeros(5, 1, dtype=torch.int64)), 17)
    with pytest.raises(ValueError, match=shape_msg):             # an evaluator's rows pass the same check
        dl.packed_rows(what, _Evaluator(17, torch.zeros(5, 1, dtype=torch.int64)), 17)
    # well-formed rows get as far as the device check: there is no CPU path behind it
    for good in (torch.zeros(5, 2, dtype=torch.int64), _Evaluator(17, torch.zeros(5, 2, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match=r"log_likelihood runs on the GPU \(got device cpu\); this package has no CPU path"):
            dl.packed_rows(what, good, 17)


def test_parent_masks_refusals():
    with pytest.raises(TypeError, match="cpdag: parents must be a torch tensor of parent masks"):
        dl.parent_masks("cpdag", "parents", [[0, 1]])
    with pytest.raises(RuntimeError, match=r"cpdag runs on the GPU \(got device cpu\); this package has no CPU path"):
        dl.parent_masks("cpdag", "parents", torch.zeros(2, 3, dtype=torch.int64))


def test_network_status_messages():
    dl.check_network_status("sample", 0)
    dl.check_network_status("sample", dl.STATUS_REFUSED | dl.LW_STATUS_ZERO_WEIGHT)      # not this function's bits
    with pytest.raises(ValueError, match="cpquery: the structure has a cycle"):
        dl.check_network_status("cpquery", dl.STATUS_CYCLE | dl.STATUS_NOT_PROBABILITY)   # the cycle is named first
    with pytest.raises(ValueError, match="sample: a table row is not a probability vector"):
        dl.check_network_status("sample", dl.STATUS_NOT_PROBABILITY)
    assert (dl.STATUS_CYCLE, dl.STATUS_REFUSED, dl.STATUS_LABELS, dl.STATUS_NOT_PROBABILITY, dl.LW_STATUS_ZERO_WEIGHT) == \
        (1 << 0, 1 << 4, 1 << 5, 1 << 6, 1 << 7)
