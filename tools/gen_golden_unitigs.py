"""Generate tests/golden/unitigs.json from the reference's own unitig pipeline.

Runs only where the reference checkout exists (oracle/gen_golden.REF):

    python tools/gen_golden_unitigs.py

Executes overlapGraphs.transitive_reduction2 (overlapGraphs.py:354-367), overlapGraphs.find_unitigs (:370-402) and
overlapGraphs.assemble_contigs (:405-412) with stdout swallowed (the reference prints a line per removed edge and
per step), as tools/gen_golden_string.py executes the string pipeline: numba.njit replaced by the identity,
overlapGraphs.overlap_alignment patched to the int64-scoring call and memoised per (read_a, read_b).  Only inputs
and outputs are written.

The reference's find_unitigs never returns when its walk comes back to a node of the current path (a cycle of
nodes with in- and out-degree 1).  Before calling it the generator walks the reduced graph itself, bounded, and
skips -- and reports -- a read set on which it would not terminate; no fixture is written for that case.

  graphs: hand-built and random digraphs without weights -> the reduced graph's edges (in G.edges order) and
          predecessor lists
  reads:  read sets -> the reduced string graph (nodes are the distinct reads), find_unitigs' output and
          assemble_contigs' contigs
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import random
import sys
import time

import networkx as nx
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from gen_golden import GOLDEN, REF, import_reference, mutate  # noqa: E402


def quiet(fn, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kw)


def graph_case(og, name, n_nodes, edges, note=""):
    """edges: [u, v] in insertion order over nodes 0 .. n_nodes-1 (inserted in that order)."""
    G = nx.DiGraph()
    G.add_nodes_from(f"n{i}" for i in range(n_nodes))
    for u, v in edges:
        G.add_edge(f"n{u}", f"n{v}")
    before = list(G.edges(data=True))
    R = quiet(og.transitive_reduction2, G)
    assert list(G.edges(data=True)) == before and R is not G
    idx = {f"n{i}": i for i in range(n_nodes)}
    return {"name": name, "note": note, "n_nodes": n_nodes, "edges": [list(e) for e in edges],
            "nodes": [idx[n] for n in R.nodes()],
            "reduced_edges": [[idx[u], idx[v]] for u, v in R.edges()],
            "pred": [[idx[p] for p in R.pred[n]] for n in R.nodes()],
            "input_pred": [[idx[p] for p in G.pred[n]] for n in G.nodes()]}


def random_graph(rng, n, density, self_loops):
    edges = [[u, v] for u in range(n) for v in range(n) if (u != v or self_loops) and rng.random() < density]
    rng.shuffle(edges)  # insertion order differs from tail-major order: the copy's predecessor order differs
    return edges


def hand_graphs(og):
    rng = random.Random(20261020)
    out = [
        graph_case(og, "self_loop_first", 3, [[0, 0], [0, 1], [0, 2]], "v is its own first successor: (v, w) is a "
                   "path, every later successor goes"),
        graph_case(og, "self_loop_last", 3, [[0, 1], [0, 2], [0, 0]], "the self-loop stands last: 1 reaches nothing, "
                   "(0, 2) stays; (0, 0) stays too"),
        graph_case(og, "self_loop_last_reached", 3, [[0, 1], [1, 0], [0, 0]], "1 reaches 0: the self-loop goes"),
        graph_case(og, "two_cycle", 2, [[0, 1], [1, 0]]),
        graph_case(og, "two_cycle_with_exit", 3, [[0, 1], [1, 0], [0, 2], [1, 2]]),
        graph_case(og, "diamond", 4, [[0, 1], [0, 2], [1, 3], [2, 3]], "no successor of 0 reaches the other"),
        graph_case(og, "diamond_with_chord", 4, [[0, 1], [0, 2], [1, 3], [2, 3], [0, 3]]),
        graph_case(og, "chain_shortcut_after", 4, [[0, 1], [1, 2], [2, 3], [0, 3]], "(0, 3) stands after (0, 1), "
                   "and 1 reaches 3: removed"),
        graph_case(og, "chain_shortcut_before", 4, [[0, 3], [0, 1], [1, 2], [2, 3]], "(0, 3) stands first: kept, "
                   "although 1 reaches 3"),
        graph_case(og, "later_reaches_earlier", 3, [[0, 1], [0, 2], [2, 1]], "only the earlier of a pair can remove"),
        graph_case(og, "earlier_reaches_later", 3, [[0, 2], [0, 1], [2, 1]]),
        graph_case(og, "long_path", 6, [[0, 1], [0, 5], [1, 2], [2, 3], [3, 4], [4, 5]], "a path of four edges"),
        graph_case(og, "sinks_and_isolated", 6, [[0, 1], [0, 2], [1, 2], [4, 0]], "nodes 2, 3, 5 have no out-edges"),
        graph_case(og, "shuffled_insertion", 4, [[3, 0], [2, 0], [0, 1], [3, 1], [1, 0], [2, 3], [3, 2]],
                   "predecessor order of the copy differs from the input's"),
        graph_case(og, "no_edges", 3, []),
        graph_case(og, "single_node", 1, []),
        graph_case(og, "single_node_loop", 1, [[0, 0]]),
        graph_case(og, "complete_3_loops", 3, [[u, v] for u in range(3) for v in range(3)]),
    ]
    for i in range(24):
        n = rng.randint(2, 9)
        density = rng.choice([0.15, 0.3, 0.6, 1.0])
        out.append(graph_case(og, f"random_{i}", n, random_graph(rng, n, density, i % 3 == 0)))
    return out


def walk_terminates(R):
    """find_unitigs' walk over R, bounded: False when it would come back to a node of its current path."""
    visited = set()
    for node in R.nodes():
        if node in visited:
            continue
        path = [node]
        while R.out_degree(path[-1]) == 1 and R.in_degree(path[-1]) == 1:
            nxt = next(iter(R.successors(path[-1])))
            if nxt in visited:
                break
            if nxt in path:
                return False
            path.append(nxt)
        visited.update(path)
    return True


def reads_case(og, name, reads):
    t0 = time.time()
    G = quiet(og.construct_string_graph, reads)
    R = quiet(og.transitive_reduction2, G)
    if not walk_terminates(R):
        print(f"{name}: SKIPPED -- the reference's find_unitigs does not terminate on this read set")
        return None
    unitigs = quiet(og.find_unitigs, R)
    contigs = quiet(og.assemble_contigs, reads)
    distinct = list(dict.fromkeys(reads))
    idx = {r: i for i, r in enumerate(distinct)}
    rec = {"fn": "construct_string_graph", "name": name, "reads": list(reads), "distinct": distinct,
           "graph_edges": G.number_of_edges(),
           "nodes": [idx[n] for n in R.nodes()],
           "edges": [[idx[u], idx[v], int(d["weight"]), int(d["end_position"])] for u, v, d in R.edges(data=True)],
           "pred": [[idx[p] for p in R.pred[n]] for n in R.nodes()],
           "unitigs": list(unitigs), "contigs": list(contigs),
           "cyclic": not nx.is_directed_acyclic_graph(G)}
    print(f"{name}: {len(reads)} reads, {G.number_of_edges()} -> {R.number_of_edges()} edges, "
          f"{len(contigs)} contigs, cyclic={rec['cyclic']}, {time.time() - t0:.1f}s")
    return rec


def main():
    aligners, og, gefr = import_reference()
    memo = {}

    def overlap_alignment(s, t):
        if (s, t) not in memo:
            memo[(s, t)] = aligners.overlap_alignment(s, t, match_score=np.int64(10), mismatch=np.int64(-1),
                                                      indel=np.int64(-(2 ** 31)))
        return memo[(s, t)]

    og.overlap_alignment = overlap_alignment
    genome = gefr.read_genome_from_fasta(os.path.join(REF, "sequence.fasta"))
    with open(os.path.join(GOLDEN, "graphs.json"), "r", encoding="utf-8") as fh:
        known = {g["name"]: g for g in json.load(fh)["graphs"]}
    small = known["small_k0"]["reads"]          # 30-base reads with copies, "ACG", "ACGTA" and a tail read
    small_err = known["small_err_k4"]["reads"]
    string_small = known["string_small"]["reads"]

    graphs = hand_graphs(og)
    print(f"graphs: {len(graphs)}")

    def phix(seed, n_reads, length, p, dups):
        random.seed(seed)
        rng = random.Random(seed)
        start = rng.randint(0, len(genome) - 4 * length - 1)
        region = genome[start:start + 4 * length]   # a short stretch: the reads overlap one another
        reads = gefr.generate_error_free_reads(region, length, n_reads - dups)
        if p:
            reads = [mutate(rng, r, p) for r in reads]
        reads += [reads[rng.randrange(len(reads))] for _ in range(dups)]
        rng.shuffle(reads)
        return reads

    cases = [
        ("string_small", string_small),
        ("small_all", small),
        ("small_err", small_err),
        ("ten_reads", [genome[2000 + 7 * i:2030 + 7 * i] for i in range(10)]),
        ("ten_reads_reversed", [genome[2000 + 7 * i:2030 + 7 * i] for i in reversed(range(10))]),
        ("one_read_twice", [genome[100:140], genome[100:140]]),
        ("phix_40x40_p0", phix(1, 40, 40, 0.0, 4)),
        ("phix_60x60_p01", phix(2, 60, 60, 0.01, 5)),
        ("phix_80x50_p0", phix(3, 80, 50, 0.0, 8)),
        ("phix_40x40_p0_nodup", list(dict.fromkeys(phix(5, 40, 40, 0.0, 0)))),
    ]
    sets = [rec for rec in (reads_case(og, name, reads) for name, reads in cases) if rec is not None]
    meta = {"generator": "tools/gen_golden_unitigs.py",
            "reference": "roiteichman/Genome-Assembly-Using-Overlap-Graphs",
            "numba": "absent: njit replaced by identity; overlap_alignment called with np.int64 scoring (10, -1, -2^31)",
            "graphs": "nodes n0 .. n{n_nodes-1} inserted in order, edges [u, v] in insertion order; reduced_edges in "
                      "G.edges order; pred / input_pred per node in node order",
            "reads": "the reduced graph of construct_string_graph as oracle/gen_golden.graph_case records that "
                     "builder (nodes are distinct-read indices), find_unitigs' strings over it and the contigs of "
                     "assemble_contigs in order; cyclic: the unreduced graph has a cycle (duplicate reads)"}
    with open(os.path.join(GOLDEN, "unitigs.json"), "w") as fh:
        json.dump({"meta": meta, "graphs": graphs, "reads": sets}, fh)


if __name__ == "__main__":
    main()
