"""CPU: the search-candidate kernels (csrc/dvs_structs.h) on the host emulator against the host stage they replace.
dvs_decoded_structures: flags / row codec / structure key of hand-made decoded rows against is_search_valid,
encode_graphs, BNLearnWrapper._parent_masks, dvs_bic_parent_masks and structure_key.  dvs_structset_filter: against
search.new_structures over successive batches, with production hashes and with 16 hash values."""
import ctypes

import numpy as np
import pytest
import torch

from dags_vae_search_amd import _lib as dl
from dags_vae_search_amd.search import hash_keys, structure_key
from tests import recon_corpus as rc
from tests import structs_corpus as sc
from tests.emu.harness import emu, ptr


def run_structures(raw, n, hash_mask=sc.ALL_ONES):
    lib = emu()
    B = raw.shape[0]
    wide = n > 13
    flags = np.full(B, 0xFF, np.uint8)
    labels = np.full((B, n), 0xFF, np.uint8)
    preds = np.full((B, n), 0xFFFF, np.uint64 if wide else np.uint16)
    keys = np.full((B, n), 0xFFFF, np.uint64)
    hashes = np.zeros(B, np.uint64)
    raw = np.ascontiguousarray(raw)
    dl.check(lib, lib.dvs_decoded_structures(B, n, 1 if wide else 0, ptr(raw), raw.nbytes, hash_mask, ptr(flags), ptr(labels),
                                             ptr(preds), ptr(keys), keys.nbytes, ptr(hashes), None), "dvs_decoded_structures")
    return flags, labels, preds, keys, hashes


class EmuSet:
    """StructureSet's bookkeeping with numpy arrays, around the emulator's dvs_structset_filter."""

    def __init__(self, n):
        self.n = n
        self.hashes = np.zeros(0, np.uint64)
        self.keys = np.zeros((0, n), np.uint64)

    def verdicts(self, keys, hashes, flags):
        lib = emu()
        B = len(hashes)
        order = np.argsort(hashes, kind="stable").astype(np.int64)
        sorted_hashes = np.ascontiguousarray(hashes[order])
        out = np.full(B, 0xFF, np.uint8)
        S = len(self.hashes)
        dl.check(lib, lib.dvs_structset_filter(B, self.n, ptr(sorted_hashes), ptr(order), ptr(keys), keys.nbytes, ptr(flags), S,
                                               ptr(self.hashes) if S else None, ptr(self.keys) if S else None,
                                               self.keys.nbytes, ptr(out), None), "dvs_structset_filter")
        return out

    def filter(self, keys, hashes, flags):
        out = self.verdicts(keys, hashes, flags)
        new = out == 1
        h = np.concatenate([self.hashes, hashes[new]])
        order = np.argsort(h, kind="stable")
        self.hashes = np.ascontiguousarray(h[order])
        self.keys = np.ascontiguousarray(np.concatenate([self.keys, keys[new]])[order])
        return out


@pytest.mark.parametrize("n", sc.SHAPES)
def test_flags_codec_and_key_equal_the_host_stage(n):
    raw, kinds, base_of = sc.corpus(n)
    flags, labels, preds, keys, hashes = run_structures(raw, n)
    graphs, valid = sc.check_rows(raw, n, flags, labels, preds, keys)
    kinds = np.asarray(kinds)
    # which kinds are valid, and why the others are not
    for kind, want in (("base", 1), ("reordered", 1), ("edge", 1), ("swap", 1), ("extra", 1), ("short", 2), ("low", 4),
                       ("high", 4), ("repeat", 8)):
        assert (flags[kinds == kind] == want).all(), (kind, flags[kinds == kind])
    # dvs_bic_parent_masks on the codec gives the same key (zeros on the invalid rows of both)
    lib = emu()
    masks = np.full((len(raw), n), 0xFFFF, np.uint64)
    status = np.zeros(1, np.int32)
    dl.check(lib, lib.dvs_bic_parent_masks(len(raw), n, 1 if n > 13 else 0, ptr(labels), ptr(preds), ptr(masks), ptr(status),
                                           None), "dvs_bic_parent_masks")
    assert np.array_equal(masks[valid], keys[valid])
    # the same structure grown in another vertex order: equal key; one edge changed / two labels swapped: another key
    P = sc.PER_KIND
    row = {kind: np.nonzero(kinds == kind)[0] for kind in sc.KINDS}
    for b in range(P):
        base = keys[row["base"][b]]
        assert np.array_equal(keys[row["reordered"][b]], base) and hashes[row["reordered"][b]] == hashes[row["base"][b]]
        assert np.array_equal(keys[row["extra"][b]], base)              # PACE-vertex and closing-vertex edges do not count
        assert not np.array_equal(keys[row["edge"][b]], base)
        assert not np.array_equal(keys[row["swap"][b]], base)
    # hashes: the kernel's value is hash_keys of the key; invalid rows sort last; the mask applies
    want = hash_keys(torch.from_numpy(keys.view(np.int64))).numpy().view(np.uint64)
    assert np.array_equal(hashes[valid], want[valid])
    assert (hashes[~valid] == sc.HASH_INVALID).all() and (hashes[valid] < sc.HASH_INVALID).all()
    small = run_structures(raw, n, 0xF)
    assert (small[4][valid] <= 0xF).all() and (small[4][~valid] == sc.HASH_INVALID).all()
    assert np.array_equal(small[4][valid], hash_keys(torch.from_numpy(keys.view(np.int64)), 0xF).numpy().view(np.uint64)[valid])
    for a, b in zip(small[:4], (flags, labels, preds, keys)):
        assert a.tobytes() == b.tobytes()
    assert len(set(hashes[valid].tolist())) == len({structure_key(graphs[i]) for i in np.nonzero(valid)[0]})


@pytest.mark.parametrize("n", sc.SHAPES)
def test_key_equality_is_structure_key_equality(n):
    raw, _, _ = sc.corpus(n)
    rng = np.random.default_rng(n)
    # 200 rows: the corpus' valid rows plus further renumbered / changed copies, so that equal pairs are frequent
    graphs, valid = sc.host_view(raw, n)
    pool = [graphs[i] for i in np.nonzero(valid)[0]]
    extra = []
    while len(pool) + len(extra) < 200:
        g = pool[int(rng.integers(0, len(pool)))]
        extra.append(rc.topo_permuted(rng, g) if rng.random() < 0.6 else rc.one_edge_changed(rng, g))
    raw = np.concatenate([raw[valid], rc.states_of(extra, n)])[:200]
    flags, _, _, keys, _ = run_structures(raw, n)
    graphs, valid = sc.host_view(raw, n)
    assert valid.all() and (flags == 1).all() and len(graphs) == 200
    sk = [structure_key(g) for g in graphs]
    same_key = (keys[:, None, :] == keys[None, :, :]).all(2)
    same_sk = np.asarray([[a == b for b in sk] for a in sk])
    assert np.array_equal(same_key, same_sk)
    assert same_sk.sum() > 200                       # equal pairs beyond the diagonal occur


@pytest.mark.parametrize("n", [4, 8, 13, 14, 45])
def test_filter_equals_new_structures_over_successive_batches(n):
    raw, _, _ = sc.corpus(n)
    rng = np.random.default_rng(100 + n)
    graphs_all, valid = sc.host_view(raw, n)
    # the initial set: a third of the base structures
    first = rng.choice(sc.PER_KIND, sc.PER_KIND // 3, replace=False)
    seen = {structure_key(graphs_all[i]) for i in first}
    results = {}
    for mask in (sc.ALL_ONES, 0xF):
        host_seen = set(seen)
        sset = EmuSet(n)
        f, _, _, k, h = run_structures(raw[first], n, mask)
        assert (sset.filter(k, h, f) == 1).all() and len(sset.hashes) == len(first)
        outs = []
        brng = np.random.default_rng(7 * n)
        for batch in range(4):
            rows = brng.integers(0, len(raw), 150)            # with repeats: duplicates inside a batch and across batches
            f, _, _, k, h = run_structures(raw[rows], n, mask)
            out = sset.filter(k, h, f)
            again = EmuSet(n)
            want = sc.host_new_mask([graphs_all[i] for i in rows], n, host_seen)
            assert np.array_equal(out == 1, want), (batch, np.nonzero((out == 1) != want)[0][:8])
            assert ((out == 0) == ~valid[rows]).all()
            assert len(sset.hashes) == len(host_seen)
            assert (np.diff(sset.hashes.astype(np.float64)) >= 0).all()
            # the set is unchanged by a verdict-only call; rows just inserted are now reported as seen
            after = sset.verdicts(k, h, f)
            assert ((after == 2) == valid[rows]).all()
            assert again.verdicts(k, h, f).tobytes() == again.verdicts(k, h, f).tobytes()      # two calls: equal bytes
            outs.append(out)
        results[mask] = np.concatenate(outs)
        assert (results[mask] == 1).any() and (results[mask] == 2).any() and (results[mask] == 4).any()
    assert results[sc.ALL_ONES].tobytes() == results[0xF].tobytes()


def test_filter_many_copies_empty_set_and_empty_batch():
    n = 8
    rng = np.random.default_rng(3)
    g = sc.permutation_dag(rng, n)
    raw = rc.states_of([g] * 4096, n)
    for mask in (sc.ALL_ONES, 0xF):
        f, _, _, k, h = run_structures(raw, n, mask)
        sset = EmuSet(n)                                 # empty set: null set pointers
        out = sset.verdicts(k, h, f)
        assert out[0] == 1 and (out[1:] == 4).all()
        assert sset.verdicts(k, h, f).tobytes() == out.tobytes()
        sset.filter(k, h, f)
        assert len(sset.hashes) == 1 and (sset.verdicts(k, h, f) == 2).all()
    # an invalid row whose (zero) key equals a valid empty graph's is never a match
    empty = sc.LabeledGraph(list(range(n)), [])
    raw = rc.states_of([empty, empty, empty], n, nv=[5, n + 3, n + 3])
    f, _, _, k, h = run_structures(raw, n)
    h[:] = 0                                             # forced collision with the invalid row
    assert list(EmuSet(n).verdicts(k, h, f)) == [0, 1, 4]
    # empty batch: accepted, nothing to do
    lib = emu()
    assert lib.dvs_structset_filter(0, n, None, None, None, 0, None, 0, None, None, 0, None, None) == 0


def test_abi_argument_checks_without_a_gpu():
    lib = dl.load()
    d = ctypes.c_void_p(16)                 # dummy pointers: every check runs before anything is enqueued
    B, n = 64, 12
    sb, kb = B * dl.DECODE_STATE_BYTES, B * n * 8
    ds = lambda batch=B, nv=n, wide=0, states=d, state_bytes=sb, flags=d, keys=d, keys_bytes=kb, hashes=d: \
        lib.dvs_decoded_structures(batch, nv, wide, states, state_bytes, sc.ALL_ONES, flags, d, d, keys, keys_bytes, hashes, None)
    assert ds(states=None) == 10 and ds(flags=None) == 10 and ds(keys=None) == 10 and ds(hashes=None) == 10
    assert ds(batch=0) == 2 and ds(nv=0) == 3 and ds(nv=46, wide=1) == 3 and ds(nv=17) == 12
    assert ds(state_bytes=sb - 1) == 14 and str(sb).encode() in lib.dvs_last_error()
    assert ds(keys_bytes=kb - 1) == 14 and str(kb).encode() in lib.dvs_last_error()
    S = 10
    skb = S * n * 8
    sf = lambda batch=B, nv=n, hashes=d, order=d, keys=d, keys_bytes=kb, flags=d, seen=S, sh=d, sk=d, seen_bytes=skb, out=d: \
        lib.dvs_structset_filter(batch, nv, hashes, order, keys, keys_bytes, flags, seen, sh, sk, seen_bytes, out, None)
    assert sf(hashes=None) == 10 and sf(order=None) == 10 and sf(keys=None) == 10 and sf(flags=None) == 10
    assert sf(out=None) == 10 and sf(sh=None) == 10 and sf(sk=None) == 10
    assert sf(batch=-1) == 2 and sf(seen=-1) == 2 and sf(nv=0) == 3 and sf(nv=46) == 3
    assert sf(keys_bytes=kb - 1) == 14 and str(kb).encode() in lib.dvs_last_error()
    assert sf(seen_bytes=skb - 1) == 14 and str(skb).encode() in lib.dvs_last_error()
    assert sf(batch=0) == 0
