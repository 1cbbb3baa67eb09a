"""Generate tests/golden/string_graph.json from the reference's own string-graph pipeline.

Runs only where the reference checkout exists (oracle/gen_golden.REF):

    python tools/gen_golden_string.py

Executes overlapGraphs.transitive_reduction (overlapGraphs.py:235-303) and overlapGraphs.assemble_contigs_string
(:306-329) with stdout swallowed (the reference prints a line per two-hop step), as oracle/gen_golden.py executes
the graph builders: numba.njit replaced by the identity, and overlapGraphs.overlap_alignment patched to the
int64-scoring call of oracle/gen_golden.ref_call -- un-patched, CPython adds the Python int -2**31 to an np.int32
cell and every score comes out near 2^31.  The patched call is memoised per (read_a, read_b): the graph of a read
set is built twice (once for the reduced-graph record, once inside assemble_contigs_string).  Only inputs and
outputs are written.

  graphs: hand-built weighted digraphs -> the reduced graph's edges (in G.edges order) and predecessor lists
  reads:  read sets -> the reduced graph (oracle/gen_golden.graph_record) and assemble_contigs_string's contigs
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
from gen_golden import GOLDEN, REF, graph_record, import_reference, mutate  # noqa: E402


def quiet(fn, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kw)


def graph_case(og, name, n_nodes, edges, note=""):
    """edges: [u, v, weight] in insertion order over nodes 0 .. n_nodes-1 (inserted in that order)."""
    G = nx.DiGraph()
    G.add_nodes_from(f"n{i}" for i in range(n_nodes))
    for u, v, w in edges:
        G.add_edge(f"n{u}", f"n{v}", weight=w)
    before = list(G.edges(data=True))
    R = quiet(og.transitive_reduction, G)
    assert list(G.edges(data=True)) == before and R is not G
    idx = {f"n{i}": i for i in range(n_nodes)}
    return {"name": name, "note": note, "n_nodes": n_nodes, "edges": [list(e) for e in edges],
            "nodes": [idx[n] for n in R.nodes()],
            "reduced_edges": [[idx[u], idx[v], int(d["weight"])] for u, v, d in R.edges(data=True)],
            "pred": [[idx[p] for p in R.pred[n]] for n in R.nodes()],
            "input_pred": [[idx[p] for p in G.pred[n]] for n in G.nodes()]}


def random_graph(rng, n, density, lo, hi, self_loops):
    edges = [[u, v, rng.randint(lo, hi)] for u in range(n) for v in range(n)
             if (u != v or self_loops) and rng.random() < density]
    rng.shuffle(edges)  # insertion order differs from tail-major order: the copy's predecessor order differs
    return edges


def hand_graphs(og):
    rng = random.Random(20261019)
    out = [
        graph_case(og, "self_loop_nonneg", 3, [[0, 0, 0], [0, 1, 5], [1, 2, 3], [0, 2, 9]],
                   "w == v with weight >= 0 removes every out-edge of v"),
        graph_case(og, "self_loop_negative", 3, [[0, 0, -1], [0, 1, 5], [0, 2, 4], [1, 2, -3]],
                   "w == v with weight < 0 removes nothing by itself"),
        graph_case(og, "w_eq_x_loop_zero", 3, [[0, 1, 5], [1, 1, 0], [1, 2, 1]], "w == x: (1, 1) >= 0 removes (0, 1)"),
        graph_case(og, "w_eq_x_loop_negative", 3, [[0, 1, 5], [1, 1, -1], [1, 2, 1]], "w == x: (1, 1) < 0 keeps (0, 1)"),
        graph_case(og, "exact_tie", 3, [[0, 1, 2], [1, 2, 3], [0, 2, 5]], "sum == weight reduces"),
        graph_case(og, "one_short", 3, [[0, 1, 2], [1, 2, 2], [0, 2, 5]], "sum < weight keeps"),
        graph_case(og, "zero_and_negative", 4, [[0, 1, 0], [1, 2, -4], [0, 2, -4], [0, 3, -5], [2, 3, 0], [1, 3, -6]]),
        graph_case(og, "sinks_and_isolated", 6, [[0, 1, 4], [0, 2, 3], [1, 2, 1], [4, 0, 2]],
                   "nodes 2, 3, 5 have no out-edges"),
        graph_case(og, "shuffled_insertion", 4, [[3, 0, 7], [2, 0, 1], [0, 1, 2], [3, 1, 9], [1, 0, 5], [2, 3, 4],
                                                 [3, 2, 8]], "predecessor order of the copy differs from the input's"),
        graph_case(og, "two_cycle", 2, [[0, 1, 3], [1, 0, 3]]),
        graph_case(og, "no_edges", 3, []),
        graph_case(og, "single_node_loop", 1, [[0, 0, 2]]),
        graph_case(og, "eliminated_still_expanded", 4, [[0, 1, 1], [0, 2, 1], [0, 3, 9], [1, 2, 0], [2, 3, 8]],
                   "(0, 2) is eliminated through 1, and still eliminates (0, 3)"),
    ]
    for i in range(28):
        n = rng.randint(2, 9)
        density = rng.choice([0.3, 0.6, 1.0])
        lo, hi = rng.choice([(1, 12), (-3, 6), (0, 3), (-5, 0)])
        out.append(graph_case(og, f"random_{i}", n, random_graph(rng, n, density, lo, hi, i % 3 == 0)))
    return out


def reads_case(og, name, reads):
    t0 = time.time()
    G, copies = quiet(og.construct_overlap_graph_string, reads)
    R = quiet(og.transitive_reduction, G)
    contigs = quiet(og.assemble_contigs_string, reads)
    distinct = list(dict.fromkeys(reads))
    rec = graph_record(R, copies, {r: i for i, r in enumerate(distinct)})
    rec.update({"fn": "transitive_reduction", "name": name, "reads": list(reads), "distinct": distinct,
                "overlap_edges": G.number_of_edges(), "contigs": list(contigs)})
    print(f"{name}: {len(reads)} reads, {G.number_of_edges()} -> {R.number_of_edges()} edges, "
          f"{len(contigs)} contigs, {time.time() - t0:.1f}s")
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

    sets = [
        reads_case(og, "string_small", string_small),
        reads_case(og, "small_all", small),
        reads_case(og, "small_err", small_err),
        reads_case(og, "ten_reads", [genome[2000 + 7 * i:2030 + 7 * i] for i in range(10)]),
        reads_case(og, "one_read_twice", [genome[100:140], genome[100:140]]),
        reads_case(og, "phix_40x40_p0", phix(1, 40, 40, 0.0, 4)),
        reads_case(og, "phix_60x60_p01", phix(2, 60, 60, 0.01, 5)),
        reads_case(og, "phix_80x50_p0", phix(3, 80, 50, 0.0, 8)),
        reads_case(og, "phix_120x40_p01", phix(4, 120, 40, 0.01, 10)),
    ]
    meta = {"generator": "tools/gen_golden_string.py",
            "reference": "roiteichman/Genome-Assembly-Using-Overlap-Graphs",
            "numba": "absent: njit replaced by identity; overlap_alignment called with np.int64 scoring (10, -1, -2^31)",
            "graphs": "nodes n0 .. n{n_nodes-1} inserted in order, edges [u, v, weight] in insertion order; "
                      "reduced_edges in G.edges order; pred / input_pred per node in node order",
            "reads": "the reduced graph of construct_overlap_graph_string as oracle/gen_golden.graph_record, and "
                     "the contigs of assemble_contigs_string in order"}
    with open(os.path.join(GOLDEN, "string_graph.json"), "w") as fh:
        json.dump({"meta": meta, "graphs": graphs, "reads": sets}, fh)


if __name__ == "__main__":
    main()
