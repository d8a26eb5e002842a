"""ctypes binding of libdvs_hip.so (C ABI: include/dvs.h).

The product has exactly one compute path: the HIP library.  ``load()`` raises if it is missing — there is
no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import (POINTER, Structure, c_char, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32,
                    c_uint64, c_void_p)

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libdvs_hip.so"
HEADER = os.path.join(os.path.dirname(_HERE), "include", "dvs.h")
EXT_HEADER = os.path.join(os.path.dirname(_HERE), "include", "dvs_eliminate.h")   # the companion header: dvs_bn_eliminate
INC_HEADER = os.path.join(os.path.dirname(_HERE), "include", "dvs_incomplete.h")  # the second: expected counts, fit_counts, impute
AVAIL_HEADER = os.path.join(os.path.dirname(_HERE), "include", "dvs_available.h")  # the third: available-case scoring (nal / pnal)
LOCAL_HEADER = os.path.join(os.path.dirname(_HERE), "include", "dvs_local.h")      # the fourth: grouped CI tests, the MMPC round
PERM_HEADER = os.path.join(os.path.dirname(_HERE), "include", "dvs_permtest.h")    # the fifth: Monte Carlo permutation CI tests
GAUSS_HEADER = os.path.join(os.path.dirname(_HERE), "include", "dvs_gaussian.h")   # the sixth: Gaussian networks on real-valued data
GCI_HEADER = os.path.join(os.path.dirname(_HERE), "include", "dvs_gaussian_ci.h")  # the seventh: CI tests on real-valued data
GPAR_HEADER = os.path.join(os.path.dirname(_HERE), "include", "dvs_gaussian_params.h")  # the eighth: a fitted Gaussian network
MIXED_HEADER = os.path.join(os.path.dirname(_HERE), "include", "dvs_mixed.h")       # the ninth: conditional Gaussian networks on mixed data
MPAR_HEADER = os.path.join(os.path.dirname(_HERE), "include", "dvs_mixed_params.h")  # the tenth: a fitted conditional Gaussian network
GINC_HEADER = os.path.join(os.path.dirname(_HERE), "include", "dvs_gaussian_incomplete.h")  # the eleventh: a normal conditioned on partial evidence


class DvsShape(Structure):
    _fields_ = [("batch", c_int32), ("n_tokens", c_int32), ("n_classes", c_int32), ("training", c_int32),
                ("dropout", c_float), ("beta", c_float), ("eps_scale", c_float), ("dag_offset", c_uint32),
                ("seed", c_uint64)]


class DvsParamEntry(Structure):
    _fields_ = [("name", c_char * 64), ("offset", c_int64), ("rows", c_int32), ("cols", c_int32)]


# ---- include/dvs.h is the one statement of the C ABI: the binding and the mirrored constants are read from it
_SCALARS = {"int": c_int, "int32_t": c_int32, "int64_t": c_int64, "uint32_t": c_uint32, "uint64_t": c_uint64,
            "size_t": c_size_t, "float": c_float, "double": c_double, "void": None}
_STRUCT_POINTERS = {"dvs_shape": POINTER(DvsShape), "dvs_param_entry": POINTER(DvsParamEntry)}
_INT = r"(0[xX][0-9a-fA-F]+|\d+)[uUlL]*"


def parse_header(text: str):
    """C header text -> (signatures, constants).  signatures: {name: (restype, [(arg_name, ctype), ...])} in header order;
    constants: the integer ``#define DVS_*`` values and the enum members.  A statement that is not a typedef block or a
    prototype over the types above raises ValueError naming it: nothing is guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text.replace("\\\n", " "), flags=re.S)
    constants = {name: int(value, 0) for name, value in
                 re.findall(rf"^[ \t]*#[ \t]*define[ \t]+(DVS_\w+)[ \t]+{_INT}[ \t]*$", text, flags=re.M)}
    for body in re.findall(r"\benum\b[^{;]*\{([^}]*)\}", text):
        for member in filter(None, (m.strip() for m in body.split(","))):
            m = re.fullmatch(rf"(\w+)\s*=\s*{_INT}", member)
            if not m:
                raise ValueError(f"include/dvs.h: enum member without a plain integer value: {member!r}")
            constants[m.group(1)] = int(m.group(2), 0)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'\btypedef\b[^;{]*\{[^}]*\}[^;]*;|extern\s+"C"\s*\{|\}', "", text)
    signatures = {}
    for stmt in filter(None, (" ".join(st.split()) for st in text.split(";"))):
        m = re.fullmatch(r"(const char ?\*|\w+) ?(\w+) ?\((.*)\)", stmt)
        if not m:
            raise ValueError(f"include/dvs.h: not a prototype: {stmt!r}")
        ret, name, params = m.groups()
        if ret != "const char*" and ret not in _SCALARS:
            raise ValueError(f"include/dvs.h: {name}: unknown return type {ret!r}")
        args = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            pm = re.fullmatch(r"(?:const )?(\w+) ?(\*?) ?(\w+)", param.strip())
            if not pm or (not pm.group(2) and _SCALARS.get(pm.group(1)) is None):
                raise ValueError(f"include/dvs.h: {name}: unknown parameter type in {param.strip()!r}")
            base, pointer, arg = pm.groups()
            args.append((arg, _STRUCT_POINTERS.get(base, c_void_p) if pointer else _SCALARS[base]))
        signatures[name] = (c_char_p if ret == "const char*" else _SCALARS[ret], args)
    return signatures, constants


def _read_header(path=None):
    """parse_header of include/dvs.h, or of the companion header at ``path``; a missing file is an error that gives its path"""
    path = HEADER if path is None else path
    if not os.path.exists(path):
        raise RuntimeError(f"include/{os.path.basename(path)} not found at {path}: the binding of {LIB_NAME} is read from it")
    with open(path) as f:
        return parse_header(f.read())


SIGNATURES, _H = _read_header()
EXPORTS = list(SIGNATURES)
# include/dvs_eliminate.h declares what was added beside the 64 entry points of include/dvs.h; SIGNATURES and EXPORTS stay those
EXT_SIGNATURES, _X = _read_header(EXT_HEADER)
# include/dvs_incomplete.h, the second companion: learning from incomplete data; EXT_SIGNATURES stays the one entry it has
INC_SIGNATURES, _ = _read_header(INC_HEADER)
# include/dvs_available.h, the third: the available-case scorer and its toggle pass; the three tables above stay what they are
AVAIL_SIGNATURES, _ = _read_header(AVAIL_HEADER)
# include/dvs_local.h, the fourth: dvs_ci_tests_group and dvs_mmpc_update; the four tables above stay what they are
LOCAL_SIGNATURES, _ = _read_header(LOCAL_HEADER)
# include/dvs_permtest.h, the fifth: dvs_ci_perm_tests and its workspace size; the five tables above stay what they are
PERM_SIGNATURES, _P = _read_header(PERM_HEADER)
# include/dvs_gaussian.h, the sixth: moments, Gaussian scores, their toggle pass and the fit; the six tables above stay what they are
GAUSS_SIGNATURES, _G = _read_header(GAUSS_HEADER)
# include/dvs_gaussian_ci.h, the seventh: dvs_gbn_ci_tests and dvs_gbn_ci_tests_group; the seven tables above stay what they are
GCI_SIGNATURES, _GC = _read_header(GCI_HEADER)
# include/dvs_gaussian_params.h, the eighth: joint, quantiles, sample, loglik, predict; the eight tables above stay what they are
GPAR_SIGNATURES, _GP = _read_header(GPAR_HEADER)
# include/dvs_mixed.h, the ninth: partition, ragged moments, the cg scores, their toggle pass and the fit; the nine tables above stay what they are
MIXED_SIGNATURES, _M = _read_header(MIXED_HEADER)
# include/dvs_mixed_params.h, the tenth: sample, loglik and predict on a fitted CG network; the ten tables above stay what they are
MPAR_SIGNATURES, _MP = _read_header(MPAR_HEADER)
# include/dvs_gaussian_incomplete.h, the eleventh: dvs_gbn_condition and its workspace size; the eleven tables above stay what they are
GINC_SIGNATURES, _ = _read_header(GINC_HEADER)


def signature(fn: str):
    """(restype, [(argument name, ctype), ...]) of an entry point of include/dvs.h or of the companion header"""
    if fn in SIGNATURES:
        return SIGNATURES[fn]
    if fn in EXT_SIGNATURES:
        return EXT_SIGNATURES[fn]
    if fn in INC_SIGNATURES:
        return INC_SIGNATURES[fn]
    if fn in AVAIL_SIGNATURES:
        return AVAIL_SIGNATURES[fn]
    if fn in LOCAL_SIGNATURES:
        return LOCAL_SIGNATURES[fn]
    if fn in PERM_SIGNATURES:
        return PERM_SIGNATURES[fn]
    if fn in GAUSS_SIGNATURES:
        return GAUSS_SIGNATURES[fn]
    if fn in GCI_SIGNATURES:
        return GCI_SIGNATURES[fn]
    if fn in GPAR_SIGNATURES:
        return GPAR_SIGNATURES[fn]
    if fn in MIXED_SIGNATURES:
        return MIXED_SIGNATURES[fn]
    if fn in MPAR_SIGNATURES:
        return MPAR_SIGNATURES[fn]
    if fn in GINC_SIGNATURES:
        return GINC_SIGNATURES[fn]
    raise KeyError(f"{fn} is declared in none of include/dvs.h, include/dvs_eliminate.h, include/dvs_incomplete.h, "
                   f"include/dvs_available.h, include/dvs_local.h, include/dvs_permtest.h, include/dvs_gaussian.h, "
                   f"include/dvs_gaussian_ci.h and include/dvs_gaussian_params.h, nor in include/dvs_mixed.h or "
                   f"include/dvs_mixed_params.h, nor in include/dvs_gaussian_incomplete.h")

D_MODEL, HEADS, LAYERS, LATENT, FC_HIDDEN, EMB = 64, 8, 3, 32, 32, 32
MAX_TOKENS = 48           # 16 on the one-tile path (a wavefront owns a DAG); up to 48 on the tiled wide path
TILE_TOKENS = 16
DECODE_STATE_BYTES = _H["DVS_DECODE_STATE_BYTES"]
CLIP_SCRATCH_FLOATS = _H["DVS_CLIP_SCRATCH_FLOATS"]
RECORD_BYTES = _H["DVS_RECORD_BYTES"]   # one-tile path; record_bytes(lib, shape) gives the size that applies
LOSS_FLOATS = _H["DVS_LOSS_FLOATS"]     # total, recon, kld, non-finite flag, invalid-features flag
ABI_VERSION = _H["DVS_VERSION"]
GP_ACQ_MAX_INDUCING = _H["DVS_GP_ACQ_MAX_INDUCING"]
STRUCT_HASH_INVALID = _H["DVS_STRUCT_HASH_INVALID"]
GEN_LABELS_CHOICE, GEN_ACCEPT_ISOLATES, GEN_ACCEPT_NO_CONNECTIVITY, GEN_GROUP_SHIFT = (
    _H["DVS_GEN_" + k] for k in ("LABELS_CHOICE", "ACCEPT_ISOLATES", "ACCEPT_NO_CONNECTIVITY", "GROUP_SHIFT"))


def _by_bnlearn_name(prefix, keys):
    """{bnlearn's name: the value of the header's enum member}, e.g. "mi-adf" -> DVS_CI_MI_ADF"""
    return {k: _H[prefix + k.upper().replace("-", "_")] for k in keys}


CI_TYPES = _by_bnlearn_name("DVS_CI_", ("mi", "x2", "mi-adf", "x2-adf"))   # dvs_ci_type
CI_MAX_CELLS = 36864      # the dense (z, x, y) table of dvs_ci_tests that fits LDS
CI_PERM_TYPES = {k: _P["DVS_CI_" + k.upper().replace("-", "_")]      # dvs_ci_perm_type (include/dvs_permtest.h)
                 for k in ("mc-mi", "mc-x2", "smc-mi", "smc-x2", "sp-mi", "sp-x2")}
GSCORE_TYPES = {k: _G["DVS_GSCORE_" + k.upper()[:-2] if k.endswith("-g") else "DVS_GSCORE_" + k.upper()]     # dvs_gscore_type
                for k in ("loglik-g", "aic-g", "bic-g", "bge")}
GBN_CHUNK, GBN_MAX_PARENTS = _G["DVS_GBN_CHUNK"], _G["DVS_GBN_MAX_PARENTS"]      # include/dvs_gaussian.h
GCI_TYPES = {k: _GC["DVS_GCI_" + k.upper().replace("-", "_")] for k in ("cor", "zf", "mi-g")}      # dvs_gci_type
GCI_MAX_COND = _GC["DVS_GCI_MAX_COND"]     # the largest conditioning set of a Gaussian CI test (include/dvs_gaussian_ci.h)
GBN_PREDICT_MODES = {"parents": _GP["DVS_GBN_PREDICT_PARENTS"], "exact": _GP["DVS_GBN_PREDICT_EXACT"]}      # include/dvs_gaussian_params.h
CGSCORE_TYPES = {k: _M["DVS_CGSCORE_" + k.upper()[:-3]] for k in ("loglik-cg", "aic-cg", "bic-cg")}      # dvs_cgscore_type (include/dvs_mixed.h)
CG_MAX_CONFIGS = _M["DVS_CG_MAX_CONFIGS"]      # the configurations of the discrete parents of one continuous family
CGBN_PREDICT_MODES = {"parents": _MP["DVS_CGBN_PREDICT_PARENTS"], "exact": _MP["DVS_CGBN_PREDICT_EXACT"],
                      "class": _MP["DVS_CGBN_PREDICT_CLASS"]}      # include/dvs_mixed_params.h
STATUS_EMPTY_CONFIG = 128     # dvs_cgbn_* status bit 7: a row met an empty configuration (NaN in its cell; information)


def gbn_stride(n: int) -> int:
    """DVS_GBN_STRIDE(n): the doubles of one set's moments (m, mean [n], C [n][n])"""
    return 1 + n + n * n


FIT_METHODS = _by_bnlearn_name("DVS_FIT_", ("mle", "bayes"))   # dvs_fit_method
FIT_MAX_CELLS = 36864     # the dense (configuration, level) table of dvs_bn_fit that fits LDS
# bits of the BN entry points' status word (device int32, zeroed by the caller), as include/dvs.h defines them
STATUS_CYCLE = 1              # bit 0 (dvs_bn_sample, dvs_bn_lw): the structure has a cycle
STATUS_REFUSED = 16           # bit 4: a family, test, row or query was refused (NaN in its cells alone); worded per call site
STATUS_LABELS = 32            # bit 5 (dvs_bic_parent_masks): a DAG's labels are not a permutation of 0..n_vars-1
STATUS_NOT_PROBABILITY = 64   # bit 6 (dvs_bn_sample, dvs_bn_lw): a table row is not a probability vector
LW_STATUS_ZERO_WEIGHT = 128   # dvs_bn_lw status bit 7: a query whose weights sum to zero (information, not an error)
STATUS_NO_ROWS = 128          # dvs_bn_scores_avail status bit 7: a family that no row observes whole (-inf; information as well)
SCORE_TYPES = _by_bnlearn_name("DVS_SCORE_", ("loglik", "aic", "bic", "bde", "bds", "k2", "bdj"))   # dvs_score_type
# dvs_bn_eliminate (include/dvs_eliminate.h): the arena and table cap in fp64 cells, the plan words' tag and limits
ELIM_MAX_CELLS, ELIM_MAX_WORDS, ELIM_MAX_SCOPE, ELIM_MAX_INPUTS, ELIM_TAG = (
    _X["DVS_BN_ELIM_" + k] for k in ("MAX_CELLS", "MAX_WORDS", "MAX_SCOPE", "MAX_INPUTS", "TAG"))


def bind(lib: ctypes.CDLL) -> ctypes.CDLL:
    """Declare argument/return types of every entry point of include/dvs.h and of its companion headers on a loaded library."""
    for name, (restype, args) in (*SIGNATURES.items(), *EXT_SIGNATURES.items(), *INC_SIGNATURES.items(), *AVAIL_SIGNATURES.items(),
                                  *LOCAL_SIGNATURES.items(), *PERM_SIGNATURES.items(), *GAUSS_SIGNATURES.items(),
                                  *GCI_SIGNATURES.items(), *GPAR_SIGNATURES.items(), *MIXED_SIGNATURES.items(),
                                  *MPAR_SIGNATURES.items(), *GINC_SIGNATURES.items()):
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = [ctype for _, ctype in args]
    return lib


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


GCI_ENTRY_POINTS = ("ci_tests", "ci_test", "pc_stable", "mmpc", "ci_tests_group", "rsmax2", "mmhc")


def data_kind(evaluator) -> str:
    """"discrete", "continuous" or "mixed" (``Evaluator.data_kind``, evaluator.py); what does not say holds discrete data"""
    return getattr(evaluator, "data_kind", "discrete")


def need_unmixed(what, evaluator):
    """the entry points that are not built on mixed data refuse a MixedEvaluator (mixed.py)"""
    if data_kind(evaluator) == "mixed":
        raise ValueError(f"{what}: the evaluator holds mixed data (factors and real columns) and mixed data is not built for "
                         f"{what}: hill_climb, tabu_search, score_masks and cg_fit are")


def need_discrete(what, evaluator):
    """the entry points that read ``packed`` / ``card`` refuse an evaluator over real-valued data (gaussian.py)"""
    need_unmixed(what, evaluator)
    if data_kind(evaluator) == "continuous":
        gci = " (its tests on real-valued data are test=\"cor\", \"zf\" and \"mi-g\")" if what in GCI_ENTRY_POINTS else ""
        raise ValueError(f"{what}: the evaluator holds real-valued data and {what} reads discrete levels{gci}: its Gaussian "
                         f"counterpart is not built")


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
        need_unmixed(what, data)
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
