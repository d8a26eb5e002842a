"""ORACLE (test infrastructure, never shipped): CPU restatement of ``PaceVaeV3.decode`` (reference
src/encoders/pace.py:1666-1749) with its helpers ``prepare_features_v2`` (1480-1611), ``generate_mask`` (1307-1343),
``compute_graph_positions`` (1245-1248) and ``from_pace_graph_to_labeled_graph`` (1290-1305), igraph-free.

PARITY UNPINNED against a *run* of the reference: its decode needs a real igraph (absent in the build container) and
draws from numpy's / torch's global generators (``np.random.choice`` 1712, ``torch.rand_like`` 1728), which no other
implementation can reproduce.  What pins this file: the decoder stack it calls is the pinned one of pace_oracle.py;
the feature building for the grown graph follows the same mask/position functions as oracle/features.py (pinned by
the 254-row known answer); and the reference's published reconstruction accuracy of the shipped asia checkpoint
(experiments/01_bn_asia/main.py:560: valid 1.000, exact 0.935) is reproduced statistically in tests.  Randomness is
INJECTED: ``uniforms[b, idx, 0]`` replaces the uniform behind ``np.random.choice`` at step ``idx`` (inverse CDF,
``cdf.searchsorted(u, side='right')`` — numpy's own algorithm), ``uniforms[b, idx, 1 + vi]`` replaces
``random_score[b]`` for edge candidate ``vi``.

Quirks kept on purpose (each is what the reference does):
  * the grown graph never gets the start->input edge 0->1 (decode adds edges only from vertices vi+1 >= 1);
  * at the last step the vertex is labelled ``output`` but is hooked to the loose ends only if the SAMPLED type was
    ``output`` (1738-1743); otherwise its in-edges are sampled like any other vertex;
  * a graph that samples ``output`` early stops growing; the reference then fails in
    from_pace_graph_to_labeled_graph (IndexError on the missing vertices) — here such graphs are returned as ``None``
    by ``to_labeled`` and the caller decides;
  * padding tokens of a short graph: label ``output``, position max+1, attend each other only (1540-1583).

Trace form.  ``decode_trace`` is the one copy of the loop: it runs in a chosen dtype (parameters, ``z`` and the feature
tensors are cast; ``po._embed`` / ``po._decoder`` follow their inputs) and asks a callback for each step's uniforms after
showing it the node-type probabilities and edge scores of that step, so the uniforms can depend on the thresholds of the
run itself.  ``decode`` is that loop with fixed uniforms in float32 — what the graph-for-graph tests compare with.  In
FLOAT64 it is the reference of tests/decode_corpus.py: ``tight_uniforms`` places every uniform a chosen distance tau from
the float64 threshold on a side drawn in advance, so that an implementation whose probability is off by more than tau
takes another decision and grows another graph; ``MarginTrace`` measures the same distances for uniforms that cannot be
steered (the library's own counter-based draws, oracle/rng.py: ``decode_uniforms``).
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import features as ofeat
from . import pace_oracle as po

LABEL_INPUT, LABEL_OUTPUT, LABEL_START = 0, 1, 2


class GrownGraph:
    """A PACE graph under construction: labels per vertex and directed edges (u -> v)."""

    def __init__(self):
        self.labels: List[int] = [LABEL_START, LABEL_INPUT]
        self.edges: List[Tuple[int, int]] = []
        self.finished = False

    @property
    def nv(self) -> int:
        return len(self.labels)

    def positions(self) -> List[int]:
        return ofeat.topological_order_fifo(self.nv, self.edges)     # positions[v] = order[v] (pace.py:1286 quirk)

    def out_degree_zero(self) -> List[int]:
        has_out = {u for u, _ in self.edges}
        return [v for v in range(self.nv) if v not in has_out]


def features_v2(graphs: Sequence[GrownGraph], N: int, C: int, heads: int = 8):
    """prepare_features_v2 (pace.py:1480-1611) for partially grown graphs, as torch tensors."""
    B = len(graphs)
    lab = np.zeros((B, N, C), np.float32)
    pos = np.zeros((B, N, N), np.float32)
    adj = np.zeros((B, N, N), np.float32)
    tmask = np.ones((B, N, N), bool)
    for b, g in enumerate(graphs):
        nv = g.nv
        p = g.positions()
        labels = list(g.labels) + [LABEL_OUTPUT] * (N - nv)
        poss = list(p) + [max(p) + 1] * (N - nv)
        lab[b, np.arange(N), labels] = 1.0
        pos[b, np.arange(N), poss] = 1.0
        a = np.zeros((nv, nv), np.float32)
        for u, v in g.edges:
            a[u, v] = 1.0
        adj[b, :nv, :nv] = a
        reach = ofeat.reachability(a)                    # reach[a][b]: a reaches b or a == b
        tmask[b, :nv, :nv] = ~reach
        tmask[b, nv:, nv:] = False
    tmask = np.transpose(tmask, (0, 2, 1))               # .transpose(1, 2) at pace.py:1606
    tm = np.repeat(tmask[:, None], heads, axis=1).reshape(B * heads, N, N)
    return torch.from_numpy(lab), torch.from_numpy(pos), torch.from_numpy(adj), torch.from_numpy(tm)


def _cast(P, z, dtype):
    return {k: v.to(dtype) for k, v in P.items()}, torch.as_tensor(z).to(dtype)


def decode_memory(P, cfg: po.PaceConfig, z: torch.Tensor) -> torch.Tensor:
    """memory = fc3(z) (pace.py:1675), sequence-first [N, B, d]; follows the dtype of P and z."""
    return F.linear(z, P["fc3.weight"], P["fc3.bias"]).reshape(-1, cfg.N, cfg.d_model).transpose(0, 1)


def step_probabilities(P, cfg: po.PaceConfig, memory: torch.Tensor, graphs: Sequence[GrownGraph], idx: int):
    """What step ``idx`` samples from, for the partial graphs as they stand (pace.py:1690-1717), in the dtype of P:
    node-type probabilities [B, C] and edge scores [B, idx - 1] (candidate vi = vertex vi + 1 -> new vertex)."""
    dtype = memory.dtype
    lab, pos, adj, tm = features_v2(graphs, cfg.N, cfg.C, cfg.heads)
    x = po._embed(P, cfg, lab.to(dtype), pos.to(dtype), adj.to(dtype), False)
    out = po._decoder(P, cfg, x.transpose(0, 1), memory, tm, False).transpose(0, 1)
    hid = out[:, idx - 1, :]
    t1 = torch.relu(F.linear(hid, P["add_node.0.weight"], P["add_node.0.bias"]))
    probs = torch.softmax(F.linear(t1, P["add_node.2.weight"], P["add_node.2.bias"]), 1).numpy()
    pair = torch.cat([torch.stack([hid] * (idx - 1), 1), out[:, :idx - 1, :]], -1)
    e = torch.relu(F.linear(pair, P["add_edge.0.weight"], P["add_edge.0.bias"]))
    score = torch.sigmoid(F.linear(e, P["add_edge.2.weight"], P["add_edge.2.bias"])).numpy()[:, :, 0]
    return probs, score


def node_cdf(p: np.ndarray) -> np.ndarray:
    """np.random.choice's thresholds for one probability vector: cumsum / total in float64 (type c iff
    cdf[c-1] <= u < cdf[c])."""
    cdf = np.asarray(p).astype(np.float64).cumsum()
    return cdf / cdf[-1]


def decode_trace(P, cfg: po.PaceConfig, z: torch.Tensor, draw, dtype=torch.float32) -> List[GrownGraph]:
    """The one copy of the generation loop (pace.py:1666-1749), run in ``dtype``.  At every step
    ``draw(idx, graphs, probs, score)`` sees the graphs as they stand and what the step samples from (numpy, in
    ``dtype``) and returns that step's uniforms [B, N] (``[:, 0]`` node type, ``[:, 1 + vi]`` edge candidate vi), so the
    uniforms may depend on the thresholds of this very run."""
    N, C = cfg.N, cfg.C
    B = z.shape[0]
    with torch.no_grad():
        P, z = _cast(P, z, dtype)
        memory = decode_memory(P, cfg, z)
        graphs = [GrownGraph() for _ in range(B)]
        for idx in range(2, N):
            probs, score = step_probabilities(P, cfg, memory, graphs, idx)
            u = draw(idx, graphs, probs, score)
            new_types = [int(min(node_cdf(probs[b]).searchsorted(float(u[b, 0]), side="right"), C - 1)) for b in range(B)]
            for b, g in enumerate(graphs):
                if not g.finished:
                    g.labels.append(new_types[b] if idx < N - 1 else LABEL_OUTPUT)
            for vi in range(idx - 2, -1, -1):
                for b, g in enumerate(graphs):
                    if g.finished:
                        continue
                    last = g.nv - 1
                    if new_types[b] == LABEL_OUTPUT:
                        for v in g.out_degree_zero():
                            if v != last:
                                g.edges.append((v, last))
                        g.finished = True
                        continue
                    if float(u[b, 1 + vi]) < float(score[b, vi]):
                        g.edges.append((vi + 1, last))
    return graphs


def decode(P, cfg: po.PaceConfig, z: torch.Tensor, uniforms: np.ndarray, dtype=torch.float32) -> List[GrownGraph]:
    """pace.py:1666-1749 with injected uniforms [B, N, N]; returns the grown PACE graphs."""
    return decode_trace(P, cfg, z, lambda idx, graphs, probs, score: uniforms[:, idx], dtype)


class MarginTrace:
    """``draw`` callback for FIXED uniforms [B, N, N] that also records, per row, the smallest distance of a draw that
    decided something from the threshold it was compared with (node type: the nearest inner cdf edge; edge candidate:
    its score): ``margin[b]``.  A row whose margin exceeds the error of another implementation's probabilities must come
    out of that implementation graph for graph."""

    def __init__(self, uniforms: np.ndarray):
        self.U = uniforms
        self.margin = np.full(uniforms.shape[0], np.inf)

    def __call__(self, idx, graphs, probs, score):
        C = probs.shape[1]
        for b, g in enumerate(graphs):
            if g.finished:
                continue
            cdf = node_cdf(probs[b])
            u0 = float(self.U[b, idx, 0])
            m = float(np.abs(cdf[:-1] - u0).min()) if C > 1 else np.inf
            if int(min(cdf.searchsorted(u0, side="right"), C - 1)) != LABEL_OUTPUT:
                m = min(m, float(np.abs(self.U[b, idx, 1:idx].astype(np.float64) - score[b, :idx - 1]).min()))
            self.margin[b] = min(self.margin[b], m)
        return self.U[:, idx]


def _f32_away(x: float, direction: float) -> np.float32:
    """x as float32, then one float32 step further in ``direction`` (+1 up, -1 down)."""
    return np.nextafter(np.float32(x), np.float32(np.inf if direction > 0 else -np.inf))


class TightDraws:
    """``draw`` callback that puts every uniform a distance ``tau`` from the threshold this run computes, on a side fixed
    in advance by the seeded generator ``rng`` — see ``tight_uniforms``.  Keeps what it saw: ``U`` (float32 [B, N, N]),
    ``forced``, ``decisions``, and per step ``probs[idx]`` / ``score[idx]`` / ``alive[idx]`` of the run that called it."""

    def __init__(self, rng, tau: float, B: int, N: int, floor_tau: Optional[float] = None):
        self.tau = float(tau)
        # sides and target classes must not depend on the tau of one rung of a ladder: forcing and class eligibility are
        # judged at floor_tau (the largest tau of the ladder) when it is given
        self.floor_tau = self.tau if floor_tau is None else float(floor_tau)
        assert self.tau <= self.floor_tau
        self.N = N
        self.U = np.zeros((B, N, N), np.float32)
        self.R = rng.random((B, N, N + 3))                    # every seeded choice, drawn up front in a fixed order
        self.early = {b: 2 + int(self.R[b, 0, N] * (N - 3)) for b in range(B) if b % 4 == 3 and N >= 5}
        self.early.update({b: 2 for b in range(B) if b % 4 == 3 and N < 5})
        self.forced = self.decisions = 0
        self.probs, self.score, self.alive = {}, {}, {}

    def _edge(self, s: float, r: float, tau: float):
        want_edge = r < 0.5
        forced = False
        lo, hi = _f32_away(s - self.floor_tau, -1), _f32_away(s + self.floor_tau, +1)
        if want_edge and not lo >= 0.0:
            want_edge, forced = False, True
        elif not want_edge and not hi < 1.0:
            want_edge, forced = True, True
        u = _f32_away(s - tau, -1) if want_edge else _f32_away(s + tau, +1)
        assert 0.0 <= u < 1.0 and (u < s) == want_edge
        return u, forced

    def _node(self, b: int, idx: int, p: np.ndarray, tau: float):
        C, last = len(p), idx == self.N - 1
        cdf = node_cdf(p)
        eligible = [c for c in range(C) if p[c] >= 4.0 * self.floor_tau]
        if last:
            want_out = b % 2 == 0
        else:
            want_out = b in self.early and idx >= self.early[b]
        wanted = [c for c in eligible if (c == LABEL_OUTPUT) == want_out]
        forced = not wanted
        if forced:
            wanted = eligible
        r_class, r_end = self.R[b, idx, self.N + 1], self.R[b, idx, self.N + 2]
        c = wanted[int(r_class * len(wanted))]
        lo = cdf[c - 1] if c > 0 else 0.0
        u = _f32_away(lo + tau, +1) if r_end < 0.5 else _f32_away(cdf[c] - tau, -1)
        assert lo <= u < cdf[c] and 0.0 <= u < 1.0
        return u, c, forced

    def _fill(self, idx, tau, U, count):
        probs, score = self.probs[idx], self.score[idx]
        for b, alive in enumerate(self.alive[idx]):
            if not alive:
                continue
            u, c, forced = self._node(b, idx, probs[b], tau)
            U[b, idx, 0] = u
            self.forced += forced * count
            self.decisions += count
            if c == LABEL_OUTPUT:
                continue                                     # the loose ends are hooked; no edge is drawn
            for vi in range(idx - 1):
                u, forced = self._edge(float(score[b, vi]), self.R[b, idx, 1 + vi], tau)
                U[b, idx, 1 + vi] = u
                self.forced += forced * count
                self.decisions += count

    def __call__(self, idx, graphs, probs, score):
        self.probs[idx], self.score[idx] = np.array(probs), np.array(score)
        self.alive[idx] = [not g.finished for g in graphs]
        self._fill(idx, self.tau, self.U, 1)
        return self.U[:, idx]

    def with_last_step_at(self, tau: float) -> np.ndarray:
        """The uniforms of this run with the LAST step's draws at distance ``tau`` instead (same sides, same target
        classes, so the same reference graphs: nothing feeds back from the last step)."""
        assert float(tau) <= self.floor_tau
        U = self.U.copy()
        self._fill(self.N - 1, float(tau), U, 0)
        return U


def tight_uniforms(P, cfg: po.PaceConfig, z: torch.Tensor, rng, tau: float, floor_tau: Optional[float] = None,
                   observe=None):
    """Threshold-bracketing draws: run the FLOAT64 trace and put every uniform ``tau`` away from the threshold the
    reference computes there, so that another implementation whose probability is off by more than ``tau`` towards the
    uniform takes the other decision and grows another graph.

      edge candidate, score s   side from ``rng``; u = s - tau gives the edge, u = s + tau none; u is cast to float32 and
                                moved one nextafter further away from s; where that leaves [0, 1) the other side is taken
                                and the decision counts as forced.
      node type                 target class from the classes with p_c >= 4 tau, an end from ``rng``: u = cdf[c-1] + tau or
                                cdf[c] - tau, rounded to float32 into the interval.
      row roles, by row index   b % 4 != 3: never ``output`` before the last step (grows to full size);
                                b % 4 == 3: ``output`` from a seeded step in 2 .. N-2 on (early finish, loose ends hooked);
                                last step: even rows ``output``, odd rows another class (both arms of the last-vertex
                                quirk).  Where no class of the wanted kind has p_c >= 4 tau any eligible class is taken
                                and the decision counts as forced.

    ``floor_tau`` (>= tau) is the distance at which forcing and eligibility are judged, so that the sides of a ladder of
    taus are the same (``TightDraws.with_last_step_at`` redraws the last step, from which nothing feeds back, at another
    rung).  ``observe(idx, graphs, probs, score)`` is called before each step's draws.  Returns (uniforms float32 [B, N, N], reference graphs, forced
    count, the TightDraws with the reference's own probabilities per step)."""
    B = z.shape[0]
    td = TightDraws(rng, tau, B, cfg.N, floor_tau)

    def draw(idx, graphs, probs, score):
        if observe is not None:
            observe(idx, graphs, probs, score)
        return td(idx, graphs, probs, score)

    graphs = decode_trace(P, cfg, z, draw, torch.float64)
    return td.U, graphs, td.forced, td


def to_labeled(g: GrownGraph, N: int) -> Optional[Tuple[List[int], List[Tuple[int, int]]]]:
    """from_pace_graph_to_labeled_graph (pace.py:1290-1305): user vertex k = PACE vertex k + 2, label - 3; the edges
    INTO PACE vertex 2 are skipped (``vertex_id == graph_label_start`` compares a vertex id with a label, 1298).
    None where the reference raises (graph shorter than N vertices)."""
    if g.nv < N:
        return None
    labels = [g.labels[v] - 3 for v in range(2, N - 1)]
    es = set(g.edges)
    edges = []
    for v in range(2, N - 1):
        if v == LABEL_START:
            continue
        for u in range(2, v + 2):
            if (u, v) in es:
                edges.append((u - 2, v - 2))
    return labels, edges
