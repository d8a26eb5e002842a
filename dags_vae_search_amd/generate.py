"""Training graphs generated on the device (csrc/dvs_generate.h).

The reference builds its encoder data sets one igraph object at a time: ``LabeledDag.generate_random_graph_erdos_renyi``
(src/toolkit/labeled.py:281-333) under ``generate_encoder_graphs_batch`` / ``create_encoder_dataset`` with the curriculum of
``encoder_dag_train_schema`` (src/encoders/utils.py:18-57, 96-202).  Here one kernel launch writes a whole batch of
Erdos-Renyi DAGs straight into the compact row codec (``CompactBatch``: what ``dvs_build_records`` and ``train_batch`` take),
so fresh graphs per step — or the whole curriculum data set — never pass through the host.  The draws are counter-based
(seed, global DAG index): a stream sharded over ranks by ``dag_offset`` is the unsharded stream.

Vertices come out in generation order, which is topological (``synthetic_dags`` does the same).  The reference stores
igraph's topological re-sort of an isomorphic copy: the same distribution over labelled graphs up to isomorphism, another
representative.
"""
from __future__ import annotations

import logging
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib as dl
from ._lib import nbytes, ptr, require_cuda, stream
from .records import CompactBatch, CompactDagDataset

logger = logging.getLogger(__name__)

LABEL_METHODS = ("sample", "choice")


def encoder_dag_train_schema(num_vertices: int, density_limit: float, steps_limit: int) -> List[Tuple[int, int]]:
    """[(edge count, batches)]: the curriculum of src/encoders/utils.py:18-57 — ``steps_limit`` edge counts from a tree
    (n - 1) up to ``density_limit`` of the n (n - 1) / 2 pairs, entry i repeated (i + 1)^2 times."""
    if num_vertices < 1:
        raise ValueError("num_vertices must be at least 1.")
    if not (0 < density_limit <= 1):
        raise ValueError("density_limit must be between 0 (exclusive) and 1 (inclusive).")
    if steps_limit < 1:
        raise ValueError("steps_limit must be at least 1.")
    min_edges = num_vertices - 1
    max_edges = (num_vertices * (num_vertices - 1)) // 2
    max_edges_density = int(max_edges * density_limit)
    if max_edges_density < min_edges:
        raise ValueError("max_edges_density cannot be less than min_edges. Check num_vertices and density_limit.")
    unique_edges = sorted(set(map(int, np.linspace(min_edges, max_edges_density, steps_limit))))
    return [(edge_count, (i + 1) ** 2) for i, edge_count in enumerate(unique_edges)]


def _flags(label_random_method: str, accept_isolates: bool, accept_no_connectivity: bool) -> int:
    if label_random_method not in LABEL_METHODS:
        raise ValueError("`label_random_method` must be one of ['sample', 'choice']")
    return (dl.GEN_LABELS_CHOICE if label_random_method == "choice" else 0) | \
        (dl.GEN_ACCEPT_ISOLATES if accept_isolates else 0) | (dl.GEN_ACCEPT_NO_CONNECTIVITY if accept_no_connectivity else 0)


def _device(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"dags_vae_search_amd: graphs are generated on the GPU (got device {dev}); "
                           f"this package has no CPU path")
    return dev


def generate_dags(n: int, card: int, num_edges: Union[int, torch.Tensor], count: Optional[int] = None, *, seed: int,
                  dag_offset: int = 0, label_random_method: str = "sample", accept_isolates: bool = False,
                  accept_no_connectivity: bool = False, try_limit: int = 100, device="cuda"):
    """``count`` Erdos-Renyi DAGs of ``n`` vertices as ``(CompactBatch, attempts)``, both on the device.

    ``num_edges``: one edge count for all (then ``count`` is required), or a device int32 tensor with one per DAG.
    ``attempts`` (int32 [count]): the 1-based attempt that was accepted, 0 where none of ``try_limit`` was (the reference
    raises there), -1 where the DAG's edge count is outside [n - 1, n (n - 1) / 2]; those DAGs' rows are zero.
    DAG b depends on (seed, dag_offset + b) only."""
    flags = _flags(label_random_method, accept_isolates, accept_no_connectivity)
    if torch.is_tensor(num_edges):
        require_cuda(num_edges, "num_edges")
        dev = num_edges.device
        m = num_edges.to(torch.int32).contiguous().reshape(-1)
        if count is not None and int(count) != m.numel():
            raise ValueError(f"count = {count} does not match the {m.numel()} edge counts")
    else:
        assert num_edges >= n - 1, \
            f"Expected at least {n - 1} edges (connectivity condition), but got {num_edges}"
        dev = _device(device)
        if count is None:
            raise ValueError("generate_dags: count is required with one edge count for all DAGs")
        m = torch.full((int(count),), int(num_edges), dtype=torch.int32, device=dev)
    lib = dl.load()
    B = m.numel()
    wide = n > 13
    with torch.cuda.device(dev):
        labels = torch.empty((B, n), dtype=torch.uint8, device=dev)
        preds = torch.empty((B, n), dtype=torch.int64 if wide else torch.int16, device=dev)
        attempts = torch.empty(B, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_generate_dags(B, int(n), int(card), 1 if wide else 0, ptr(m), dl.seed64(seed),
                                            int(dag_offset), int(try_limit), flags, ptr(labels), ptr(preds), nbytes(preds),
                                            ptr(attempts), stream()), "dvs_generate_dags")
    return CompactBatch(labels, preds), attempts


def draw_edge_counts(schema, count: int, *, seed: int, dag_offset: int = 0, device="cuda") -> torch.Tensor:
    """Device int32 [count]: per DAG one edge count of ``schema`` ([(edge count, weight)]), drawn with the weights from
    (seed, dag_offset + b): the mixture a shuffled curriculum data set has."""
    dev = _device(device)
    lib = dl.load()
    table = torch.tensor([[m for m, _ in schema], np.cumsum([w for _, w in schema]).tolist()], dtype=torch.int32).to(dev)
    out = torch.empty(int(count), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        dl.check(lib, lib.dvs_generate_edge_counts(int(count), len(schema), ptr(table[0]), ptr(table[1]),
                                                   dl.seed64(seed), int(dag_offset), ptr(out), stream()),
                 "dvs_generate_edge_counts")
    return out


def create_encoder_dataset(n: int, card: int, batch_size: int, steps_limit: int, density_limit: float = 0.6, *, seed: int,
                           label_random_method: str = "sample", accept_isolates: bool = False,
                           accept_no_connectivity: bool = False, try_limit: int = 100, device="cuda") -> CompactDagDataset:
    """The reference's ``create_encoder_dataset`` as a device-resident ``CompactDagDataset``: for schema entry i,
    (i + 1)^2 batches of ``batch_size`` graphs with that edge count — one launch per entry, one host synchronisation at the
    end.  DAGs for which no attempt was accepted are dropped with a warning (the reference's short batch); their number is
    the data set's ``dropped``."""
    schema = encoder_dag_train_schema(n, density_limit, steps_limit)
    logger.info("Train schema (num edges, batches count): %s", schema)
    parts, tries, offset = [], [], 0
    for m, batches in schema:
        batch, attempts = generate_dags(n, card, m, batches * batch_size, seed=seed, dag_offset=offset,
                                        label_random_method=label_random_method, accept_isolates=accept_isolates,
                                        accept_no_connectivity=accept_no_connectivity, try_limit=try_limit, device=device)
        parts.append(batch)
        tries.append(attempts)
        offset += batches * batch_size
    keep = torch.cat(tries) > 0
    data = CompactBatch(torch.cat([p.labels for p in parts])[keep], torch.cat([p.preds for p in parts])[keep])
    dropped = offset - len(data)
    if dropped:
        logger.warning("Requested %d graphs, but only %d were generated within %d attempts each.", offset, len(data), try_limit)
    dataset = CompactDagDataset.from_compact(data, n)
    dataset.dropped = dropped
    return dataset


class DagStream:
    """An endless iterator of fresh ``CompactBatch``es for ``train_batch``: every DAG's edge count is drawn on the device
    with the curriculum's (i + 1)^2 weights, then the DAG itself, both from (seed, global DAG index).  The stream keeps a
    running ``dag_offset``, so it does not repeat (the index wraps at 2^32 DAGs), and with ``shard = (rank, world)`` step k
    yields DAGs [(k world + rank) batch_size, (k world + rank + 1) batch_size) of the unsharded stream of batch size
    ``world * batch_size``.  DAGs that found no accepted attempt are kept out: such a batch is shorter (``last_attempts``
    holds the step's attempt counts; checking them costs the stream's only host synchronisation, ``check=False`` skips it
    and leaves the zero rows in)."""

    def __init__(self, n: int, card: int, batch_size: int, seed: int, *, density_limit: float = 0.4, steps_limit: int = 20,
                 label_random_method: str = "sample", accept_isolates: bool = False, accept_no_connectivity: bool = False,
                 try_limit: int = 100, shard: Tuple[int, int] = (0, 1), dag_offset: int = 0, check: bool = True,
                 device="cuda"):
        self.n, self.card, self.batch_size, self.seed = int(n), int(card), int(batch_size), int(seed)
        self.schema = encoder_dag_train_schema(n, density_limit, steps_limit)
        self.kw = dict(label_random_method=label_random_method, accept_isolates=accept_isolates,
                       accept_no_connectivity=accept_no_connectivity, try_limit=try_limit)
        _flags(label_random_method, accept_isolates, accept_no_connectivity)
        self.rank, self.world = int(shard[0]), int(shard[1])
        if not 0 <= self.rank < self.world:
            raise ValueError(f"shard = {shard}: rank must be in [0, world)")
        self.dag_offset = int(dag_offset)
        self.check = check
        self.device = _device(device)
        self.last_attempts = None

    def __iter__(self):
        return self

    def __next__(self) -> CompactBatch:
        offset = self.dag_offset + self.rank * self.batch_size
        self.dag_offset += self.world * self.batch_size
        m = draw_edge_counts(self.schema, self.batch_size, seed=self.seed, dag_offset=offset, device=self.device)
        batch, attempts = generate_dags(self.n, self.card, m, seed=self.seed, dag_offset=offset, **self.kw)
        self.last_attempts = attempts
        if self.check:
            keep = attempts > 0
            if not bool(keep.all()):
                batch = batch[keep]
        return batch
