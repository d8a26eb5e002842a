"""dvs_bn_scores at the C boundary on a CPU-only box: the export is in the header, in the library and in the binding, the
header's enum is the one the binding and the test corpus use, and every bad argument comes back with its code before any
HIP call (dummy non-null pointers are never dereferenced)."""
import ctypes
import os
import re

import pytest

from dags_vae_search_amd import _lib as dl
from tests import bn_score_corpus as bn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_export_is_in_the_header_the_library_and_the_binding():
    if not os.path.exists(dl.lib_path()):
        pytest.fail(f"{dl.lib_path()} is missing: run __graft_entry__.build()")
    txt = open(os.path.join(REPO, "include", "dvs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+dvs_bn_scores\s*\(", code)
    assert hasattr(ctypes.CDLL(dl.lib_path()), "dvs_bn_scores")
    assert "dvs_bn_scores" in dl.EXPORTS and "dvs_bic_scores" in dl.EXPORTS
    enum = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"DVS_SCORE_([A-Z0-9]+)\s*=\s*(\d+)", code)}
    assert enum == bn.TYPE_CODE == dl.SCORE_TYPES
    assert dl.load().dvs_version() == 202                       # a pure addition: the version number stays


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    """Unknown type: 12; iss <= 0 or not finite, k < 0 or not finite, a number for a type without an argument: 13; the
    shape and null-pointer codes of dvs_bic_scores."""
    bn.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))


def test_wrapper_refuses_unbuilt_types_and_misplaced_arguments():
    """Argument checks of BNLearnWrapper that need no device: they run before the data is touched."""
    from dags_vae_search_amd import BNLearnWrapper
    for name in ("ebic", "mbde", "bdla", "fnml", "qnml", "pred-loglik", "custom-score"):
        with pytest.raises(NotImplementedError) as e:
            BNLearnWrapper("asia", name, data=None)
        assert all(built in str(e.value) for built in dl.SCORE_TYPES)
    for name, kw in (("bic", {"iss": 10}), ("aic", {"iss": 1}), ("k2", {"iss": 1}), ("loglik", {"k": 1}), ("bde", {"k": 2}),
                     ("bds", {"k": 2}), ("bdj", {"k": 1}), ("bde", {"iss": 0}), ("bde", {"iss": float("nan")}),
                     ("aic", {"k": -1})):
        with pytest.raises(ValueError):
            BNLearnWrapper("asia", name, data=None, **kw)
