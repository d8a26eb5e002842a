"""The C ABI by argument name (the names of include/dvs.h, through dl.SIGNATURES): call / call_rc, which the corpus drivers
go through, and the refusal tables.

A table is a list of (entry point, arguments, return code, text dvs_last_error must contain).  Every case fails a check that
runs before anything is enqueued, so a CPU-only box and dummy non-null pointers do."""
import ctypes

from dags_vae_search_amd import _lib as dl


def _signature(fn, given, optional=()):
    """[(name, ctype)] of ``fn`` in header order; TypeError unless ``given`` names exactly those (``optional`` may be absent)."""
    sig = dl.SIGNATURES[fn][1]
    missing, unknown = {n for n, _ in sig} - set(given) - set(optional), set(given) - {n for n, _ in sig}
    if missing or unknown:
        raise TypeError(f"{fn}: arguments go by the names of include/dvs.h: missing {sorted(missing)}, unknown {sorted(unknown)}")
    return sig


def call_rc(be, fn, **args):
    """``fn`` on the library of ``be`` (a backend of tests/scoring_corpus.py), every argument named -> its return code.  A void*
    argument is a handle of ``be.put`` (passed as ``be.ptr(h)``), None (NULL) or a c_void_p (as it is); ``stream`` defaults to
    ``be.stream``; everything else, sizes included, goes as the caller states it."""
    ptr = lambda v: v if v is None or isinstance(v, ctypes.c_void_p) else be.ptr(v)
    return getattr(be.lib, fn)(*[ptr(args.get(n, be.stream)) if ctype is ctypes.c_void_p else args[n]
                                 for n, ctype in _signature(fn, args, optional=("stream",))])


def call(be, fn, **args):
    """call_rc that must succeed"""
    assert call_rc(be, fn, **args) == 0, be.lib.dvs_last_error()


def at(be, h, offset):
    """the address ``offset`` bytes into the buffer of handle ``h``, as an argument of call"""
    return ctypes.c_void_p(be.ptr(h).value + offset)


def entry(fn, into, **base):
    """``base`` names every argument of ``fn`` with a value that passes all checks.  Returns case(code, text, **overrides):
    it appends to ``into`` the call with the overridden arguments, which must return ``code`` and leave a message that
    starts with ``fn + ": "`` and contains ``text``."""
    names = [name for name, _ in _signature(fn, base)]

    def case(code, text, **overrides):
        _signature(fn, overrides, optional=names)
        args = {**base, **overrides}
        into.append((fn, [args[name] for name in names], code, f"{fn}: {text}"))
    return case


def run(lib, cases):
    for fn, args, code, text in cases:
        got = getattr(lib, fn)(*args)
        msg = lib.dvs_last_error().decode()
        assert (got, text in msg, msg.startswith(fn + ":")) == (code, True, True), (fn, args, got, msg)
