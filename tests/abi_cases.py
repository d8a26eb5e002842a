"""Refusal tables of the C ABI, keyed by argument name (the names of include/dvs.h, through dl.SIGNATURES).

A table is a list of (entry point, arguments, return code, text dvs_last_error must contain).  Every case fails a check that
runs before anything is enqueued, so a CPU-only box and dummy non-null pointers do."""
from dags_vae_search_amd import _lib as dl


def entry(fn, into, **base):
    """``base`` names every argument of ``fn`` with a value that passes all checks.  Returns case(code, text, **overrides):
    it appends to ``into`` the call with the overridden arguments, which must return ``code`` and leave a message that
    starts with ``fn + ": "`` and contains ``text``."""
    names = [name for name, _ in dl.SIGNATURES[fn][1]]
    if set(base) != set(names):
        raise TypeError(f"{fn}: base must name every argument: missing {sorted(set(names) - set(base))}, "
                        f"unknown {sorted(set(base) - set(names))}")

    def case(code, text, **overrides):
        if not set(overrides) <= set(names):
            raise TypeError(f"{fn}: unknown argument {sorted(set(overrides) - set(names))}")
        args = {**base, **overrides}
        into.append((fn, [args[name] for name in names], code, f"{fn}: {text}"))
    return case


def run(lib, cases):
    for fn, args, code, text in cases:
        got = getattr(lib, fn)(*args)
        msg = lib.dvs_last_error().decode()
        assert (got, text in msg, msg.startswith(fn + ":")) == (code, True, True), (fn, args, got, msg)
