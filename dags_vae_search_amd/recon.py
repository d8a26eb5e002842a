"""Reconstruction evaluation on the device (the reference's batch_test / model_test, experiments/03_synthetic_12/
main.py:200-283 and experiments/01_bn_asia/main.py:195-266).

``model_test`` (train.py) decodes on the device but judges every decoded graph on the host: one graph object per row and a
``graph_equals`` call per pair, which goes through networkx VF2 when labels repeat (milliseconds per pair).  Here the
decoded rows stay on the device as ``dvs_decode_state`` records and ``dvs_match_decoded`` (csrc/dvs_match.h) judges all of
them in one launch: validity, isomorphism ignoring labels (the "structure recon accuracy" of 01_bn_asia) and
label-preserving isomorphism, exactly.  Rows whose search exceeds the node budget come back as undecided and only those are
judged on the host.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _lib as dl
from ._lib import nbytes, ptr, require_cuda, stream
from .features import _as_labels_edges
from .records import CompactBatch, encode_graphs

DEFAULT_BUDGET = 8192        # search nodes per pair and search (symmetric graphs need ~n when colour refinement is stable)
MAX_CHUNK_ROWS = 65536       # decoded rows per decode_states / match launch
FLAG_VALID, FLAG_STRUCT, FLAG_LABELLED, FLAG_UNDECIDED = 1, 2, 4, 8


def match_decoded(targets: CompactBatch, states: torch.Tensor, repeats: int, card: int,
                  budget: int = DEFAULT_BUDGET) -> torch.Tensor:
    """Flags (device uint8 [B * repeats]) of decoded rows ``states`` (device uint8 [B * repeats, DECODE_STATE_BYTES], row k
    decoded from target k // repeats): bit 0 ``LabeledDag.is_valid_graph``, bit 1 ``graph_equals(attributes_match=False)``,
    bit 2 ``graph_equals``, bit 3 undecided (bits 1-2 unspecified).  ``card``: the toolkit's label cardinality."""
    require_cuda(states, "states")
    lib = dl.load()
    dev = states.device
    B, n = targets.labels.shape
    rows = B * int(repeats)
    if states.dtype != torch.uint8 or tuple(states.shape) != (rows, dl.DECODE_STATE_BYTES):
        raise AssertionError(f"Expected states uint8 [{rows}, {dl.DECODE_STATE_BYTES}], got {states.dtype} {tuple(states.shape)}")
    wide = n > 13
    labels = targets.labels.to(dev, torch.uint8).contiguous()
    preds = targets.preds.to(dev).contiguous().to(torch.int64 if wide else torch.int16)
    states = states.contiguous()
    flags = torch.empty(rows, dtype=torch.uint8, device=dev)
    dl.check(lib, lib.dvs_match_decoded(B, n, int(card), int(repeats), 1 if wide else 0, ptr(labels), ptr(preds),
                                        ptr(states), nbytes(states), int(budget), ptr(flags), stream()),
             "dvs_match_decoded")
    return flags


def judge_on_host(raw, targets: Sequence, toolkit, n_tokens: int):
    """Flags bits 1-2 of decoded rows judged by ``toolkit.graph_equals``: the fallback for rows ``match_decoded`` left
    undecided.  raw: numpy uint8 [rows, DECODE_STATE_BYTES]; targets: one target graph per row."""
    from .pace import graphs_from_states
    out = []
    for target, g in zip(targets, graphs_from_states(raw, n_tokens)):
        s = toolkit.graph_equals(target, g, attributes_match=False)
        out.append(FLAG_STRUCT * int(s) | FLAG_LABELLED * int(s and toolkit.graph_equals(target, g)))
    return out


def topological_targets(graphs: Sequence, n: int) -> CompactBatch:
    """Row codec of the target graphs; a graph whose edges do not all go from a lower to a higher vertex id is re-indexed
    into a topological order first (isomorphism does not depend on the numbering; ``encode_graphs`` needs u < v)."""
    out = []
    for g in graphs:
        labels, edges = _as_labels_edges(g)
        if all(u < v for u, v in edges):
            out.append((list(labels), list(edges)))
            continue
        indeg = [0] * len(labels)
        succ = [[] for _ in labels]
        for u, v in edges:
            succ[u].append(v)
            indeg[v] += 1
        order = [v for v in range(len(labels)) if indeg[v] == 0]
        for u in order:
            for v in succ[u]:
                indeg[v] -= 1
                if indeg[v] == 0:
                    order.append(v)
        if len(order) != len(labels):
            raise ValueError("evaluate_reconstruction: a target graph is not a DAG")
        pos = {v: i for i, v in enumerate(order)}
        out.append(([labels[v] for v in order], [(pos[u], pos[v]) for u, v in edges]))
    return encode_graphs(out, n)


def evaluate_reconstruction(model, dataset, toolkit, batch_size: int = 32, encode_times: int = 10, decode_times: int = 10,
                            shuffle: bool = True, seed: Optional[int] = None, log=None, budget: int = DEFAULT_BUDGET):
    """``model_test`` with the judging on the device: the same loop, DataLoader, per-batch loss and denominators; the
    encode_times x decode_times decodes of each graph's posterior mean are ONE ``decode_states`` call per batch (chunks of at
    most 65 536 rows) judged by ``match_decoded``; the counts are summed on the device.  Returns model_test's keys plus
    "structure_accuracy" (isomorphic ignoring labels, 01_bn_asia's "structure recon accuracy") and "undecided" (rows the
    device search left to the host's ``graph_equals``).  Same rates as model_test in distribution, not draw for draw: the
    decodes of a batch take one seed step instead of encode_times x decode_times."""
    from torch.utils.data import DataLoader
    model.eval()
    if seed is not None:
        torch.manual_seed(seed)
        model.seed(seed)
    n = model.max_num_vertices - 3
    if toolkit.num_vertices != n:
        raise ValueError(f"toolkit has {toolkit.num_vertices} vertices, the model decodes {n}")
    # decoded labels are < the model's cardinality <= 45, so a wider toolkit range judges exactly as 45 does
    card = min(int(toolkit.label_cardinality), 45)
    R = encode_times * decode_times
    per_chunk = max(1, MAX_CHUNK_ROWS // R)
    loader = DataLoader(dataset=dataset, batch_size=batch_size, collate_fn=lambda data: [g for g in data], shuffle=shuffle)
    total_nll, n_graphs = 0.0, 0
    counts = [0, 0, 0, 0]            # valid, labelled, structure, undecided
    for i, batch in enumerate(loader):
        mu, _ = model.encode(batch)
        _, nll, _ = model.loss(batch)
        targets = topological_targets(batch, n)
        sums = torch.zeros(4, dtype=torch.int64, device=mu.device)
        chunks = []
        for s in range(0, len(batch), per_chunk):
            z = mu[s:s + per_chunk].repeat_interleave(R, dim=0)
            states = model.decode_states(z)
            flags = match_decoded(targets[s:s + per_chunk], states, R, card, budget)
            f = flags.to(torch.int64)
            und = (f >> 3) & 1
            sums += torch.stack([(f & 1).sum(), ((f >> 2) & 1 & (1 - und)).sum(), ((f >> 1) & 1 & (1 - und)).sum(),
                                 und.sum()])
            chunks.append((s, und, states))
        v, lab, st, un = sums.tolist()        # the batch's one host synchronisation (with the loss above)
        for s, und, states in chunks if un else ():    # the device search ran out of budget: judge those rows on the host
            idx = torch.nonzero(und).flatten()
            raw = states[idx].cpu().numpy()
            for f in judge_on_host(raw, [batch[s + k // R] for k in idx.tolist()], toolkit, model.max_num_vertices):
                st += (f >> 1) & 1
                lab += (f >> 2) & 1
        counts[0] += v
        counts[1] += lab
        counts[2] += st
        counts[3] += un
        total_nll += float(nll.detach())
        n_graphs += len(batch)
        if log is not None:
            decodes = n_graphs * R
            log(f"batch {i}: AVG recon loss: {total_nll / n_graphs}, valid ratio: {counts[0] / decodes:.4f}, "
                f"recon accuracy: {counts[1] / decodes:.4f}, structure recon accuracy: {counts[2] / decodes:.4f}")
    decodes = max(n_graphs * R, 1)
    return {"recon_loss": total_nll / max(n_graphs, 1), "valid_ratio": counts[0] / decodes,
            "recon_accuracy": counts[1] / decodes, "graphs": n_graphs, "structure_accuracy": counts[2] / decodes,
            "undecided": counts[3]}
