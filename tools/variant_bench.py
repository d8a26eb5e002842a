#!/usr/bin/env python3
"""A/B helper for kernel experiments: run bench.py against alternative builds of the library (libdvs_<name>.so next to the
shipped one, e.g. built with extra -D flags) in the same gpurun call.  The package itself only ever loads libdvs_hip.so;
this tool swaps the name before the first load, per child process.
    python tools/variant_bench.py hip stag32 stag96
A variant whose PYTHON side differs as well (another revision's entry points) is a whole checkout with its own built
libdvs_hip.so: `label=DIR` runs DIR/bench.py from DIR.
    python tools/variant_bench.py base=../parent_checkout hip base=../parent_checkout hip --batch 1024
Every child runs under its own time limit; the first one that fails ends the run (nothing more is started on the device)."""
import json
import os
import subprocess
import sys

CHILD = r'''
import sys, runpy
sys.path.insert(0, ".")
from dags_vae_search_amd import _lib as dl
dl.LIB_NAME = "libdvs_%s.so"
sys.argv = ["bench.py", "--steps", "100", "--warmup", "20", "--no-cpu-baseline", "--full"] + %r
runpy.run_path("bench.py", run_name="__main__")
'''
CHILD_SECONDS = 240
extra = []
names = []
for a in sys.argv[1:]:                   # library names first, then bench.py's own arguments from the first "--..." on
    (extra if extra or a.startswith("--") else names).append(a)
for name in names:
    label, _, tree = name.partition("=")
    try:
        out = subprocess.run([sys.executable, "-c", CHILD % ("hip" if tree else label, extra)], capture_output=True, text=True,
                             cwd=tree or None, timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired:
        print(label, f"no result within {CHILD_SECONDS} s: stopping", flush=True)
        sys.exit(124)
    try:
        d = json.loads(out.stdout.strip().splitlines()[-1])
        print(label, round(d["ms_per_step"], 4), "gpu_kernel_ms", round(d["roofline"]["whole_step"]["gpu_kernel_ms_per_step"], 4),
              {k: v for i, (k, v) in enumerate(d["kernels"].items()) if i < 9 or k.startswith("k_loss")}, flush=True)
        if os.environ.get("VARIANT_BENCH_JSON"):     # keep the whole result lines too, one per child
            with open(os.environ["VARIANT_BENCH_JSON"], "a") as f:
                f.write(json.dumps({"variant": label, **d}) + "\n")
    except Exception:
        print(label, "failed", out.stderr[-800:], flush=True)
        sys.exit(out.returncode or 1)
