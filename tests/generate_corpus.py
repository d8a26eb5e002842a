"""TEST INFRASTRUCTURE: a float-free numpy restatement of the device graph generator (csrc/dvs_generate.h)
from oracle.rng's site_key / draw, and the seeded cases the emulator and GPU tests share.

The restatement is the specification: for DAG b, slot t = v (v - 1) / 2 + u is the edge u -> v (u < v), walked v outer and u
inner; attempt a takes slot t iff (draw(key_e, a * 1024 + t) * (P - t)) >> 32 < m - chosen; the result is the first accepted
attempt in attempt order; labels are drawn once from key_l.  Everything is integer arithmetic on uint64, vectorised over
the batch, so a reference for thousands of DAGs costs milliseconds.
"""
import functools

import numpy as np

from oracle import rng

SITE_EDGES, SITE_LABELS = 300, 301
CHOICE, ACCEPT_ISOLATES, ACCEPT_NO_CONNECTIVITY = 1, 2, 4
GROUP_SHIFT = 8                      # flags bits 8..11: lanes per DAG (tuning only; never changes the output)
U1 = np.uint64(1)


def _connected(rows, want):
    """rows: uint64 [B, n] predecessor bit rows; want: uint64 [B] vertex sets.  True where `want` is one weak component."""
    n = rows.shape[1]
    R = want & (~want + U1)
    while True:
        before = R.copy()
        for v in list(range(1, n)) + list(range(n - 1, 0, -1)):
            bit = U1 << np.uint64(v)
            inside = (R & bit) != 0
            R = np.where(inside, R | rows[:, v], np.where((rows[:, v] & R) != 0, R | bit, R))
        if np.array_equal(R, before):
            return R == want


def attempt_rows(key_e, a, n, m):
    """Selection sampling of attempt `a` for every DAG: uint64 [B, n] rows and the set of vertices of degree >= 1."""
    B = key_e.shape[0]
    P = n * (n - 1) // 2
    rows = np.zeros((B, n), np.uint64)
    touched = np.zeros(B, np.uint64)
    chosen = np.zeros(B, np.int64)
    t = 0
    for v in range(1, n):
        for u in range(v):
            h = rng.draw(key_e, np.uint64(a * 1024 + t))
            take = ((h * np.uint64(P - t)) >> np.uint64(32)).astype(np.int64) < (m - chosen)
            rows[:, v] |= np.where(take, U1 << np.uint64(u), np.uint64(0))
            chosen += take
            t += 1
        touched |= np.where(rows[:, v] != 0, rows[:, v] | (U1 << np.uint64(v)), np.uint64(0))
    return rows, touched


def draw_labels(key_l, n, card, choice):
    B = key_l.shape[0]
    labels = np.zeros((B, n), np.uint8)
    unused = np.ones((B, card), bool)
    for v in range(n):
        h = rng.draw(key_l, np.uint64(v))
        if choice:
            labels[:, v] = ((h * np.uint64(card)) >> np.uint64(32)).astype(np.uint8)
            continue
        r = ((h * np.uint64(card - v)) >> np.uint64(32)).astype(np.int64)
        rank = np.cumsum(unused, axis=1) - 1                  # rank of every still unused value, lowest first
        pick = np.argmax(unused & (rank == r[:, None]), axis=1)
        labels[:, v] = pick
        unused[np.arange(B), pick] = False
    return labels


def generate(n, card, num_edges, B=None, *, seed, dag_offset=0, try_limit=100, flags=0):
    """(labels u8 [B, n], preds u16 / u64 [B, n], attempts i32 [B]) exactly as dvs_generate_dags writes them."""
    m = np.asarray(num_edges, np.int64)
    if m.ndim == 0:
        m = np.full(B, int(m), np.int64)
    B = m.shape[0]
    P = n * (n - 1) // 2
    dag = np.arange(B, dtype=np.uint64) + np.uint64(dag_offset)
    key_e = rng.site_key(seed, SITE_EDGES, dag)
    key_l = rng.site_key(seed, SITE_LABELS, dag)
    valid = (m >= n - 1) & (m <= P)
    attempts = np.where(valid, 0, -1).astype(np.int32)
    preds = np.zeros((B, n), np.uint64)
    open_ = valid.copy()
    full = np.uint64((1 << n) - 1)
    for a in range(try_limit):
        idx = np.nonzero(open_)[0]
        if idx.size == 0:
            break
        rows, touched = attempt_rows(key_e[idx], a, n, m[idx])
        if flags & ACCEPT_NO_CONNECTIVITY:
            ok = np.ones(idx.size, bool)
        else:
            ok = _connected(rows, touched if flags & ACCEPT_ISOLATES else np.full(idx.size, full))
        won = idx[ok]
        preds[won] = rows[ok]
        attempts[won] = a + 1
        open_[won] = False
    labels = draw_labels(key_l, n, card, bool(flags & CHOICE))
    labels[attempts <= 0] = 0
    return labels, preds.astype(np.uint64 if n > 13 else np.uint16), attempts


def popcount(x):
    x = np.asarray(x).astype(np.uint64)
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8)).reshape(x.shape + (64,)).sum(-1)


def edge_sets(preds):
    """Per DAG the frozenset of (u, v) edges."""
    out = []
    for rows in np.asarray(preds).astype(np.uint64):
        out.append(frozenset((u, v) for v, r in enumerate(rows) for u in range(v) if (int(r) >> u) & 1))
    return out


# ---- the cases the emulator and the GPU share: (name, n, card, num_edges (int or array), B, seed, try_limit, flags) ----------
def _cycle(B, lo, hi, first):
    return (lo + (np.arange(B) + first - lo) % (hi - lo + 1)).astype(np.int32)


CASES = {
    "n4_m3": dict(n=4, card=4, num_edges=3, B=77, seed=7, try_limit=100, flags=0),
    "n5_m5": dict(n=5, card=5, num_edges=5, B=77, seed=11, try_limit=100, flags=0),
    "n8_m7_try2": dict(n=8, card=8, num_edges=7, B=256, seed=5, try_limit=2, flags=0),
    # per-DAG m cycling through 11 .. 26.  The cycle starts at 16: with seed 3 that phase has, in the restatement, DAGs that
    # need more than 64 attempts (so a 64-lane group goes into a second round) and one that fails; starting at 11 the
    # largest count is exactly 64 and no group boundary is crossed.
    "n12_mixed": dict(n=12, card=12, num_edges=_cycle(1000, 11, 26, 16), B=1000, seed=3, try_limit=100, flags=0),
    "n13_m20": dict(n=13, card=13, num_edges=20, B=130, seed=13, try_limit=100, flags=0),
    "n14_m20": dict(n=14, card=14, num_edges=20, B=130, seed=14, try_limit=100, flags=0),
    "n45_m90": dict(n=45, card=45, num_edges=90, B=64, seed=3, try_limit=100, flags=0),
    "n45_m198": dict(n=45, card=45, num_edges=198, B=64, seed=3, try_limit=100, flags=0),
    "n8_choice_card1": dict(n=8, card=1, num_edges=10, B=70, seed=21, try_limit=100, flags=CHOICE),
    "n8_choice_card45": dict(n=8, card=45, num_edges=10, B=70, seed=22, try_limit=100, flags=CHOICE),
    "n8_isolates": dict(n=8, card=8, num_edges=7, B=70, seed=23, try_limit=100, flags=ACCEPT_ISOLATES),
    "n8_no_connectivity": dict(n=8, card=8, num_edges=7, B=70, seed=24, try_limit=100, flags=ACCEPT_NO_CONNECTIVITY),
    # m = n - 2 and m = P + 1 are refused per DAG (attempts == -1) next to the two extremes that are not
    "n8_m_out_of_range": dict(n=8, card=8, num_edges=np.tile(np.asarray([6, 7, 28, 29], np.int32), 18), B=72, seed=25,
                              try_limit=100, flags=0),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's (labels, preds, attempts) of a case; computed once, shared, read-only."""
    c = CASES[name]
    out = generate(c["n"], c["card"], c["num_edges"], c["B"], seed=c["seed"], try_limit=c["try_limit"], flags=c["flags"])
    for a in out:
        a.setflags(write=False)
    return out


def edge_counts(case):
    m = np.asarray(case["num_edges"], np.int32)
    return np.ascontiguousarray(np.full(case["B"], int(m), np.int32) if m.ndim == 0 else m)


def run_abi(lib, ptr, n, card, num_edges, *, seed, dag_offset=0, try_limit=100, flags=0, to_device=None, to_host=None):
    """Call dvs_generate_dags on numpy buffers (emulator) or, with to_device / to_host, on device tensors."""
    from dags_vae_search_amd import _lib as dl
    B = len(num_edges)
    wide = n > 13
    labels = np.full((B, n), 0xAB, np.uint8)
    preds = np.full((B, n), 0xABAB, np.uint64 if wide else np.uint16)
    attempts = np.full(B, -7, np.int32)
    bufs = [np.ascontiguousarray(num_edges, np.int32), labels, preds, attempts]
    dev = [to_device(b) for b in bufs] if to_device else bufs
    code = lib.dvs_generate_dags(B, n, card, 1 if wide else 0, ptr(dev[0]), seed, dag_offset, try_limit, flags, ptr(dev[1]),
                                 ptr(dev[2]), preds.nbytes, ptr(dev[3]), None)
    dl.check(lib, code, "dvs_generate_dags")
    if to_host:
        return to_host(dev[1], labels.dtype), to_host(dev[2], preds.dtype), to_host(dev[3], attempts.dtype)
    return labels, preds, attempts


# ---- checks shared by tests/test_emu_generate.py and tests/test_gpu_generate.py -----------------------------------------------
# `run(n, card, num_edges, seed=, dag_offset=, try_limit=, flags=)` goes through the C ABI and returns numpy arrays.
def assert_equal_bits(got, want, what):
    for name, g, w in zip(("labels", "preds", "attempts"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        bad = np.nonzero((g != w).reshape(len(w), -1).any(1))[0]
        assert bad.size == 0, f"{what}: {name} differ in {bad.size} of {len(w)} DAGs, first {bad[:5].tolist()}"


def check_case(run, name, group=0):
    c = CASES[name]
    got = run(c["n"], c["card"], edge_counts(c), seed=c["seed"], try_limit=c["try_limit"], flags=c["flags"] | group << GROUP_SHIFT)
    assert_equal_bits(got, reference(name), f"{name} (group {group})")


def check_sharding(run):
    c = CASES["n12_mixed"]
    m = edge_counts(c)[:200]
    whole = run(12, 12, m, seed=9, try_limit=100, flags=0)
    head = run(12, 12, m[:120], seed=9, try_limit=100, flags=0)
    tail = run(12, 12, m[120:], seed=9, dag_offset=120, try_limit=100, flags=0)
    assert_equal_bits(tuple(np.concatenate([h, t]) for h, t in zip(head, tail)), whole, "120 + 80 at dag_offset 120")
    assert_equal_bits(whole, generate(12, 12, m, seed=9), "B = 200")
    # a large offset: the global DAG index is what is hashed
    far = run(12, 12, m[:70], seed=9, dag_offset=(1 << 31) + 5, try_limit=100, flags=0)
    assert_equal_bits(far, generate(12, 12, m[:70], seed=9, dag_offset=(1 << 31) + 5), "dag_offset 2^31 + 5")


def check_determinism(run):
    m = np.full(130, 14, np.int32)
    a = run(10, 10, m, seed=77, try_limit=100, flags=0)
    b = run(10, 10, m, seed=77, try_limit=100, flags=0)
    assert_equal_bits(b, a, "second call")
    c = run(10, 10, m, seed=78, try_limit=100, flags=0)
    assert (c[1] != a[1]).any() and (c[0] != a[0]).any()
    # the high half of the seed counts too
    d = run(10, 10, m, seed=77 + (1 << 32), try_limit=100, flags=0)
    assert (d[1] != a[1]).any()
    assert_equal_bits(d, generate(10, 10, m, seed=77 + (1 << 32)), "seed with high bits")


def check_refusals(lib, ptr, alloc):
    """alloc(nbytes) -> something ptr() takes, valid device memory of that size for this library."""
    def call(n=8, card=None, wide=None, try_limit=100, flags=0, B=16, preds_bytes=None, dag_offset=0):
        card = n if card is None else card
        wide = (n > 13) if wide is None else wide
        need = B * n * (8 if wide else 2)
        bufs = [alloc(B * 4), alloc(B * n), alloc(max(need, 8)), alloc(B * 4)]
        code = lib.dvs_generate_dags(B, n, card, 1 if wide else 0, ptr(bufs[0]), 1, dag_offset, try_limit, flags, ptr(bufs[1]),
                                     ptr(bufs[2]), need if preds_bytes is None else preds_bytes, ptr(bufs[3]), None)
        return code, lib.dvs_last_error().decode()
    assert lib.dvs_version() == 202
    code, msg = call(n=12, B=10, preds_bytes=10 * 12 * 2 - 1)
    assert code == 14 and "240" in msg, (code, msg)
    code, msg = call(n=14, B=10, preds_bytes=10 * 14 * 8 - 8)
    assert code == 14 and "1120" in msg, (code, msg)
    code, msg = call(n=8, card=7)
    assert code != 0 and "card >= n_vars" in msg, (code, msg)
    assert call(n=8, card=7, flags=CHOICE)[0] == 0              # with replacement any card will do
    for n, wide in ((13, True), (14, False)):
        code, msg = call(n=n, card=n, wide=wide)
        assert code != 0 and "preds_are_u64" in msg, (code, msg)
    for t in (0, 4097, -1):
        code, msg = call(try_limit=t)
        assert code != 0 and "try_limit" in msg, (code, msg)
    assert call(try_limit=1)[0] == 0 and call(try_limit=4096)[0] == 0
    for n in (1, 46):
        code, msg = call(n=n, card=45, flags=CHOICE, wide=n > 13)
        assert code != 0 and "n_vars" in msg, (code, msg)
    for card in (0, 46):
        code, msg = call(card=card, flags=CHOICE)
        assert code != 0 and "card" in msg, (code, msg)
    for flags in (8, 16, 8 << GROUP_SHIFT, 1 << 12):
        code, msg = call(flags=flags)
        assert code != 0 and "flags" in msg, (code, msg)
    assert call(dag_offset=-1)[0] != 0
