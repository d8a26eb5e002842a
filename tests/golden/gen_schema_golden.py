"""Record tests/golden/encoder_schema.json from the REFERENCE's own encoder_dag_train_schema (src/encoders/utils.py:18-57).

    python tests/golden/gen_schema_golden.py <path of the reference checkout>

The function itself needs numpy only, but its module imports dask, igraph, pyarrow, tqdm and the toolkit at the top; whichever
of them is absent gets an inert placeholder module before the import (as gen_golden.py does for igraph), so that the values
written here are computed by the reference's code, unmodified.  The fixture is data: the argument triples and the
(edge count, batches) pairs they give.
"""
import importlib
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(12, 0.4, 20), (8, 0.6, 20), (37, 0.2, 20), (45, 0.4, 7), (5, 1.0, 3)]


class _Placeholder(types.ModuleType):
    """A module whose every attribute is an inert class (enough for annotations and base-class lists at import time)."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def import_reference_utils(ref):
    sys.path.insert(0, ref)
    for _ in range(32):
        try:
            return importlib.import_module("src.encoders.utils")
        except ModuleNotFoundError as e:
            if e.name is None or e.name.startswith("src"):
                raise
            sys.modules[e.name] = _Placeholder(e.name)
    raise RuntimeError("too many absent packages")


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["DVS_REFERENCE_DIR"]
    utils = import_reference_utils(ref)
    out = [{"num_vertices": n, "density_limit": d, "steps_limit": s,
            "schema": [[int(m), int(k)] for m, k in utils.encoder_dag_train_schema(n, d, s)]} for n, d, s in CASES]
    with open(os.path.join(HERE, "encoder_schema.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {len(out)} schemas")


if __name__ == "__main__":
    main()
