"""The unitig pipeline straight from the score columns: ``assemble_contigs`` without the full graph object.

``assemble_contigs`` builds the string graph of the raw reads as a networkx graph (every scored pair with a positive
score becomes three dicts), reduces a copy of it and walks what is left.  Almost every edge is removed again, so here
the full graph is never made:

  Inputs: the raw reads R[0 .. N); d[0 .. n), the distinct reads in first-occurrence order; ids[j], the distinct read
  of R[j]; first[x], the first raw position of x; prev[j], the previous raw position holding ids[j], or -1; and
  (score, end)(x, y), the reference's overlap score (match 10, mismatch -1, no gaps).
  1. String graph (``_string_graph``, ``combinations(reads, 2)`` order).  Nodes are d in order.  The successor list of
     x is produced by j = first[x] + 1 .. N - 1 ascending: position j yields ids[j] iff prev[j] <= first[x] and
     score(x, ids[j]) > 0.  A self-loop (x, x) appears when x has a second copy.  The edge carries weight = score and
     end_position = end.
  2. Reduction.  ``transitive_reduction2``'s rule on that CSR; the kept edges in CSR order, added tail-major in node
     order, are the reduced graph with ``DiGraph.copy()``'s predecessor order.
  3. Walk (``find_unitigs``).  From every node not yet on a path, in node order, the path goes on while its last node
     has one kept out-edge and one kept in-edge and that edge's head is on no earlier path.  A head that is on the path
     itself is the cycle of non-branching nodes on which the reference never returns: ``ValueError``.
  4. Spelling.  The path's first read plus read[v][end_position:] for every further node v.

``ovl_unitigs_host`` (one host thread) and ``ovl_unitigs`` / ``ovl_unitigs_candidates`` (the GPU) compute that from the
columns; ``reduced_string_graph`` returns the kept edge columns, ``assemble_contigs_direct`` the contigs.  On the
resident route the distinct reads are uploaded, the k = 0 candidate list is enumerated and scored on the device, and
only ids, 16 bytes per node and the outputs cross the link.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from ._lib import OvlError


class ReducedStringGraph:
    """The reduced string graph of a raw read list as columns: ``nodes`` (the distinct reads in first-occurrence
    order), the kept edges ``tail``, ``head`` (node indices), ``weight``, ``end_position`` (int32, CSR order),
    ``n_edges`` (the string graph's edges before the reduction), ``n_kept`` and ``cycle_node`` (-1, or the node at
    which ``find_unitigs``' walk comes back to its own path)."""

    def __init__(self, nodes: List[str], res: dict):
        self.nodes = nodes
        self.tail, self.head = res["tail"], res["head"]
        self.weight, self.end_position = res["weight"], res["end_position"]
        self.n_edges, self.n_kept, self.cycle_node = res["n_edges"], res["n_kept"], res["cycle_node"]

    def to_digraph(self):
        """``transitive_reduction2(_string_graph(reads))`` as a networkx DiGraph: the same nodes, successor order,
        predecessor order and attributes; only the kept edges' dicts are built."""
        import networkx as nx
        G = nx.DiGraph()
        G.add_nodes_from(self.nodes)
        nodes = self.nodes
        G.add_edges_from((nodes[t], nodes[h], {"weight": w, "end_position": e})
                         for t, h, w, e in zip(self.tail.tolist(), self.head.tolist(), self.weight.tolist(),
                                               self.end_position.tolist()))
        return G


def _check_text(reads) -> None:
    try:
        "".join(reads).encode("latin-1")
    except UnicodeEncodeError:
        raise OvlError(-4, "the contigs are spelled from the reads' bytes: characters above 255 are not supported")


def _columns(distinct, ids, engine, scorer, enc):
    """(score, end, self_score, self_end) over the distinct reads: every ordered pair in ovl_candidates(k = 0) order
    and, for the reads with a second copy, the self pair (None, None without one)."""
    from . import overlapGraphs as og
    n = len(distinct)
    x = np.repeat(np.arange(n, dtype=np.int32), max(n - 1, 0))
    y = np.tile(np.arange(max(n - 1, 0), dtype=np.int32), n)
    y = y + (y >= x)
    rep = np.flatnonzero(np.bincount(ids, minlength=n) >= 2).astype(np.int32)
    sc, en = og._score(distinct, np.concatenate([x, rep]), np.concatenate([y.astype(np.int32), rep]), engine, scorer,
                       enc)
    P = x.shape[0]
    if rep.shape[0] == 0:
        return sc[:P], en[:P], None, None
    self_sc, self_en = np.zeros(n, np.int32), np.zeros(n, np.int32)
    self_sc[rep], self_en[rep] = sc[P:], en[P:]
    return sc[:P], en[:P], self_sc, self_en


def _run(reads, engine, scorer, device, timing):
    """(distinct reads, the result dict of the form that ran)."""
    from . import overlapGraphs as og
    from .candidates import dedup_reads
    from .engine import default_engine, encode_reads, unitigs_host, use_device
    st = og._Stages(timing)
    reads = list(reads)
    distinct, _ = dedup_reads(reads)
    _check_text(distinct)
    index = {r: i for i, r in enumerate(distinct)}
    ids = np.fromiter((index[r] for r in reads), dtype=np.int32, count=len(reads))
    st("dedup")
    enc = encode_reads(distinct)
    st("encode")
    if not distinct:
        return distinct, unitigs_host(enc, ids, np.zeros(0, np.int32), np.zeros(0, np.int32))
    on_device = use_device(device, len(distinct), og.UNITIGS_DEVICE_MIN_WORK, engine)
    if on_device and scorer is None:
        eng = engine or default_engine()
        eng.set_reads(distinct, enc)
        st("set_reads")
        eng.enumerate_candidates(0)
        st("enumerate")
        res = eng.unitigs_candidates(enc, ids)
    else:
        cols = _columns(distinct, ids, engine, scorer, enc)
        st("score")
        res = (engine or default_engine()).unitigs(enc, ids, *cols) if on_device else unitigs_host(enc, ids, *cols)
    st("unitigs")
    return distinct, res


def reduced_string_graph(reads: Sequence[str], engine=None, scorer=None, device: Optional[bool] = None,
                         timing: Optional[dict] = None) -> ReducedStringGraph:
    """The reduced string graph of ``reads`` -- ``transitive_reduction2(_string_graph(reads))`` -- as the kept edge
    columns and the node list, without the full graph (``.to_digraph()`` builds the networkx graph of the kept edges).
    ``engine``, ``scorer``, ``device`` and ``timing`` as in ``assemble_contigs_direct``."""
    distinct, res = _run(reads, engine, scorer, device, timing)
    return ReducedStringGraph(distinct, res)


def assemble_contigs_direct(reads: Sequence[str], engine=None, scorer=None, device: Optional[bool] = None,
                            timing: Optional[dict] = None) -> List[str]:
    """The contigs of ``assemble_contigs(reads)`` in the same order, from the score columns (this module's rule).
    Raises ``find_unitigs``' ``ValueError`` on a cycle of non-branching nodes.

    ``device=None`` takes the resident route (reads, k = 0 candidate list, scores, graph and node facts on the GPU)
    from ``overlapGraphs.UNITIGS_DEVICE_MIN_WORK`` distinct reads when a GPU is visible, else the host form
    (ovl_unitigs_host) over columns scored by the engine; True / False force the choice.  With ``scorer`` the columns come from it (and the
    device form, when forced, is ovl_unitigs over the uploaded columns).  ``timing`` receives the stage times in
    seconds."""
    distinct, res = _run(reads, engine, scorer, device, timing)
    if res["cycle_node"] >= 0:
        node = distinct[res["cycle_node"]]
        raise ValueError(f"find_unitigs: the path from {node!r} comes back to {node!r}, a cycle of "
                         "non-branching nodes on which the reference's walk never ends")
    text = res["bases"].tobytes().decode("latin-1")
    off = res["c_off"].tolist()
    return [text[off[k]:off[k + 1]] for k in range(res["n_contigs"])]
