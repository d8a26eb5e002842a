#!/usr/bin/env python3
"""Bitwise A/B of the host launch layer on the emulator: the check that a refactor of csrc/dvs_api.hip hands every launch
the arguments it had.  No GPU needed.  Builds the emulator library (tests/emu/build.py) from a git revision and from the
working tree, drives both through tests/emu/harness.py on the golden fixtures, and compares as raw bytes the losses, mu,
logvar, the flat gradient, the decode states and records, and the whole workspace after every call.  The emulator runs
workgroups in lock-step, so equal launches with equal arguments give equal bytes.

The revision is run twice: workspace bytes that differ between its own two runs are not reproducible and are left out of
the comparison (their count is printed per call); outputs are never left out.  DVS_SPLIT_STACK=1 and DVS_LATENT_KERNELS=1
are read once per process, so each group of cases runs in a child process of its own.  One line per call on stdout;
exit status 1 if anything differs.
usage: tools/emu_host_ab.py <rev>"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# group -> (environment of the child, cases); a case: (kind, fixture, batch, waves per workgroup, training, dropout)
# batch < 0: the last graphs of the fixture.  "n12k20": the n12c12 graphs under a label cardinality of 20 (N = 15, C = 23:
# wide by class count only); the class-sized parameters the fixture cannot supply are drawn from a fixed seed.
STEP = [("step", "n12c12", 6, 4, False, 0.0), ("step", "n12c12", 6, 8, False, 0.0),
        ("step", "n12c12", 6, 4, True, 0.15), ("step", "n12c12", 6, 8, True, 0.15),
        ("step", "asia_rand", 4, 8, True, 0.15),
        ("step", "n29c7", -3, 8, False, 0.0), ("step", "n29c7", -3, 8, True, 0.15),
        ("step", "n12k20", 4, 8, False, 0.0), ("step", "n12k20", 4, 8, True, 0.15)]
GROUPS = {
    "default": ({}, STEP + [("encode", "n12c12", 6, 4, False, 0.0), ("encode", "n12c12", 6, 8, False, 0.0),
                            ("encode", "n29c7", -3, 8, False, 0.0), ("encode", "n12k20", 4, 8, False, 0.0),
                            ("decode", "asia", 4, 4, False, 0.0), ("decode", "asia", 4, 8, False, 0.0),
                            ("decode", "n29c7", 2, 8, False, 0.0)]),
    "split_stack": ({"DVS_SPLIT_STACK": "1"}, STEP),
    "latent_kernels": ({"DVS_LATENT_KERNELS": "1"}, STEP),
}


def fixture(name):
    from oracle import features as ofeat
    from oracle.pace_oracle import PaceConfig
    from tests.helpers import load_golden
    cfg, params, graphs, z = load_golden("n12c12" if name == "n12k20" else name)
    params = {k: v.numpy() for k, v in params.items()}
    if name == "n12k20":
        cfg = PaceConfig(n=12, card=20)
        rng = np.random.default_rng(20)
        params["vertex_label_embed.0.weight"] = (0.1 * rng.standard_normal((32, cfg.C))).astype(np.float32)
        params["add_node.2.weight"] = (0.1 * rng.standard_normal((cfg.C, 32))).astype(np.float32)
        params["add_node.2.bias"] = (0.1 * rng.standard_normal(cfg.C)).astype(np.float32)
    return cfg, params, graphs, z, ofeat


def run_case(case, out):
    from dags_vae_search_amd import _lib as dl
    from tests.emu.harness import EmuModel, emu, ptr
    kind, name, B, nw, training, dropout = case
    os.environ["DVS_WAVES_PER_WG"] = str(nw)
    cfg, params, graphs, z, ofeat = fixture(name)
    graphs = graphs[:B] if B > 0 else graphs[B:]
    B = len(graphs)
    tag = "%s_%s_b%d_w%d_%s" % (kind, name, B, nw, "train%g" % dropout if training else "eval")
    m = EmuModel(cfg, params, B, training=training, dropout=dropout, seed=1234, dag_offset=7)
    sref = ctypes.byref(m.shape)

    def dump(what, a):
        np.ascontiguousarray(a).tofile(os.path.join(out, tag + "." + what))
    if kind == "decode":
        lib = emu()
        state = np.zeros(B * dl.DECODE_STATE_BYTES, np.uint8)
        zz = np.ascontiguousarray(z["eval/mu"][:B])
        U = np.random.default_rng(5).random((B, cfg.N, cfg.N)).astype(np.float32)
        dl.check(lib, lib.dvs_decode(sref, ptr(m.flat), m.flat.size, ptr(m.ws), m.ws.nbytes, ptr(m.records), m.records.nbytes,
                                     ptr(zz), ptr(U), ptr(state), state.nbytes, None), "decode")
        dump("out.states", state)
        dump("out.records", m.records)
        dump("ws.decode", m.ws)
        return
    assert m.pack(ofeat.dense_features(graphs, cfg.card)) == 0
    if kind == "encode":
        lib = emu()
        mu = np.zeros((B, 32), np.float32)
        lv = np.zeros((B, 32), np.float32)
        dl.check(lib, lib.dvs_encode(sref, ptr(m.records), m.records.nbytes, ptr(m.flat), m.flat.size, ptr(m.ws), m.ws.nbytes,
                                     ptr(mu), ptr(lv), None), "encode")
        dump("out.mu", mu)
        dump("out.logvar", lv)
        dump("ws.encode", m.ws)
        return
    losses, mu, lv = m.forward()
    dump("out.losses", losses)
    dump("out.mu", mu)
    dump("out.logvar", lv)
    dump("ws.forward", m.ws)
    _, flat = m.backward(1.0, 0.005)
    dump("out.grads", flat)
    dump("ws.backward", m.ws)


def child(lib, group, out):
    from dags_vae_search_amd import _lib as dl
    from tests.emu import harness
    harness._emu = dl.bind(ctypes.CDLL(lib))       # this library, not the working tree's own build
    for case in GROUPS[group][1]:
        run_case(case, out)


def build_emu(tree):
    return subprocess.check_output([sys.executable, os.path.join(tree, "tests", "emu", "build.py")], cwd=tree,
                                   text=True).strip().splitlines()[-1]


def main(rev):
    status = 0
    with tempfile.TemporaryDirectory(prefix="dvs_emu_ab_") as tmp:
        old = os.path.join(tmp, "old")
        subprocess.check_call(["git", "-C", ROOT, "worktree", "prune"])
        subprocess.check_call(["git", "-C", ROOT, "worktree", "add", "-f", "--detach", old, rev], stdout=subprocess.DEVNULL)
        try:
            lib_old = build_emu(old)
            libs = {"a1": lib_old, "a2": lib_old, "b": build_emu(ROOT)}
            for group, (env, _) in GROUPS.items():
                procs = []
                for run, lib in libs.items():
                    os.makedirs(os.path.join(tmp, group, run))
                    procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", lib, group,
                                                   os.path.join(tmp, group, run)], env={**os.environ, **env}, cwd=ROOT))
                if any(p.wait() != 0 for p in procs):
                    print("%s: a run failed" % group)
                    return 1
                for f in sorted(os.listdir(os.path.join(tmp, group, "b"))):
                    a1, a2, b = (np.fromfile(os.path.join(tmp, group, run, f), np.uint8) for run in ("a1", "a2", "b"))
                    same = a1.size == b.size
                    keep = np.ones(a1.size, bool) if f.split(".")[-2] == "out" or not same else a1 == a2
                    same = same and bool((a1[keep] == b[keep]).all())
                    left_out = int((~keep).sum())
                    print("%-14s %-52s %9d bytes  %s%s" % (group, f, b.size, "identical" if same else "DIFFERS",
                                                          "  (%d bytes not reproducible on %s, left out)" % (left_out, rev)
                                                          if left_out else ""))
                    status |= 0 if same else 1
        finally:
            subprocess.call(["git", "-C", ROOT, "worktree", "remove", "--force", old])
    return status


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--child":
        child(*sys.argv[2:])
    elif len(sys.argv) == 2:
        sys.exit(main(sys.argv[1]))
    else:
        sys.exit(__doc__)
