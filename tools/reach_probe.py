"""Time the reachability reduction on one GPU against the library's host form and write profiles/reach.json.

Workloads (fixed seeds):

  string2000   construct_string_graph's CSR for PhiX reads N = 2,000, l = 100, p = 0.01
  string400    the tests' 400 PhiX reads of 60 bases; for its first 150 reads also the literal loop, once:
               itertools.combinations over graph.successors(v) with nx.has_path, what the stage costs as the
               reference runs it
  digraph16k   a random digraph of 16,384 nodes at 3 edges per node (partial reachability, a 32 MB matrix)
  sweep        string graphs of the first m of the 400 reads, m = 8 .. 400: the crossover
  sweep2000    the same over the first m of string2000's reads, m = 500 .. 1,700, where the 400 reads hold none
  pipeline     assemble_contigs' stages at N = 2,000, timed one by one

Per workload: one warm-up, then ``--reps`` timed repetitions of the device call (wall clock around
OverlapEngine.reach_reduce, upload and download included) and of the host form (ovl_reach_reduce_host, one thread)
on the same arrays; medians and spreads (max - min); the launches' own time from the HIP events around them
(engine.set_timing) over the same number of calls; the closure's word-ORs (one per set bit of a row's pivot word and
word of the row, summed over the pivot blocks: the update launches' work, replayed with torch tensors) per second
of that time.  The two masks must be equal.  A host run that takes longer than ``--host-budget`` seconds is
repeated three times instead of ``--reps`` (recorded as "host_reps").  The crossover is the smallest node count of
the two sweeps together from which the device call's median stays below the host form's ("crossover_nodes",
recomputed from the sections in the file whenever a sweep runs).

    python tools/reach_probe.py [--workload all|string2000|string400|digraph16k|sweep|sweep2000|pipeline] [--out profiles/reach.json]

Sections already in the output file are kept, so the workloads can be run one at a time.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from itertools import combinations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genome-assembly-using-overlap-graphs_amd"))


def summary(ts):
    return {"median_s": statistics.median(ts), "spread_s": max(ts) - min(ts), "all_s": ts}


def word_ors(off, heads):
    """Word-ORs of the device closure's update launches: for every pivot block K and every row i, the popcount of
    R[i]'s word K as it stands when block K is processed, times the words per row.  Replayed with torch tensors
    (on the GPU when there is one) from the same adjacency rows."""
    import numpy as np
    import torch
    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    n = off.shape[0] - 1
    words = (n + 63) // 64
    rows = np.zeros((n, words), np.uint64)
    tails = np.repeat(np.arange(n), np.diff(off))
    np.bitwise_or.at(rows, (tails, heads >> 6), np.uint64(1) << (heads & 63).astype(np.uint64))
    R = torch.from_numpy(rows.view(np.int64)).to(dev)
    total = 0
    for K in range(words):
        lo, hi = 64 * K, min(64 * K + 64, n)
        P = R[lo:hi].clone()
        for k in range(hi - lo):  # the pivot rows' closure inside the block, row-OR Warshall
            has = ((P[:, K] >> k) & 1).bool()
            P = torch.where(has[:, None], P | P[k], P)
        c = R[:, K].clone()
        total += int(np.unpackbits(c.cpu().numpy().view(np.uint8)).sum()) * words
        for k in range(hi - lo):
            R = torch.where(((c >> k) & 1).bool()[:, None], R | P[k], R)
    return total


def measure(engine, off, heads, reps, host_budget, count_ors=True):
    import numpy as np
    from ovlgraph.engine import reach_reduce_host

    t0 = time.perf_counter()
    want = reach_reduce_host(off, heads)  # warm-up, and the mask the device must reproduce
    first_host = time.perf_counter() - t0
    got = engine.reach_reduce(off, heads)
    assert np.array_equal(got, want), "device and host masks differ"
    info = engine.last_reach()
    host_reps = reps if first_host <= host_budget else 3
    t_dev, t_host, t_kernel = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter(); engine.reach_reduce(off, heads); t_dev.append(time.perf_counter() - t0)
    for _ in range(host_reps):
        t0 = time.perf_counter(); reach_reduce_host(off, heads); t_host.append(time.perf_counter() - t0)
    engine.set_timing(True)
    for _ in range(reps):
        engine.reach_reduce(off, heads)
        t_kernel.append(engine.last_timing()["kernel_ms"] * 1e-3)
    engine.set_timing(False)
    k = statistics.median(t_kernel)
    dev, host = summary(t_dev), summary(t_host)
    n, m = int(off.shape[0] - 1), int(heads.shape[0])
    ors = word_ors(off, heads) if count_ors else None
    return {
        "nodes": n, "edges": m, "reduced": int(want.sum()), "work": n * m,
        "words_per_row": info["words_per_row"], "pivot_blocks": info["pivot_blocks"],
        "window_bits": info["window_bits"], "launches": 2 * info["pivot_blocks"] + 2,
        "matrix_bytes": n * info["words_per_row"] * 8,
        "device_call": dev, "host": host, "host_reps": host_reps, "kernels": summary(t_kernel),
        "host_over_device_call": host["median_s"] / dev["median_s"],
        "closure_word_ors": ors,
        "kernels_word_ors_per_s": ors / k if ors and k > 0 else None,
        "host_word_ors_per_s": ors / host["median_s"] if ors and host["median_s"] > 0 else None,
    }


def literal_loop(G):
    """The reference's stage as it runs it: one nx.has_path search per ordered pair of successors."""
    import networkx as nx
    removed = set()
    calls = 0
    for v in G.nodes():
        for u, w in combinations(G.successors(v), 2):
            calls += 1
            if nx.has_path(G, u, w):
                removed.add((v, w))
    return removed, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reach.json"))
    ap.add_argument("--workload", default="all",
                    choices=("all", "string2000", "string400", "digraph16k", "sweep", "sweep2000", "pipeline"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-budget", type=float, default=15.0)
    args = ap.parse_args()

    import numpy as np
    from ovlgraph import OverlapEngine
    from ovlgraph import overlapGraphs as og
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads

    out = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            out = json.load(fh)
    out["reps"] = args.reps
    genome = read_genome_from_fasta()
    engine = OverlapEngine(0)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    def string_csr(reads):
        G = og._string_graph(reads, engine, None)
        return (G,) + og._csr_heads(list(G), G._adj)

    reads400 = list(dict.fromkeys(simulate_reads(genome, 60, 440, 0.01, seed=5)))[:400]

    if args.workload in ("all", "string2000"):
        _, off, heads = string_csr(simulate_reads(genome, 100, 2000, 0.01, seed=1))
        out["string2000"] = dict(measure(engine, off, heads, args.reps, args.host_budget), N=2000, l=100, p=0.01)
        print(json.dumps({"string2000": out["string2000"]}), flush=True)
        save()
    if args.workload in ("all", "string400"):
        _, off, heads = string_csr(reads400)
        rec = dict(measure(engine, off, heads, args.reps, args.host_budget), N=400, l=60, p=0.01)
        G, off, heads = string_csr(reads400[:150])
        from ovlgraph.engine import reach_reduce_host
        t0 = time.perf_counter()
        removed, calls = literal_loop(G)
        t_literal = time.perf_counter() - t0
        mask = reach_reduce_host(off, heads)
        nodes = list(G)
        tails = np.repeat(np.arange(len(nodes)), np.diff(off))
        assert {(nodes[t], nodes[h]) for t, h in zip(tails[mask == 1], heads[mask == 1])} == removed
        t0 = time.perf_counter(); reach_reduce_host(off, heads); t_host = time.perf_counter() - t0
        t0 = time.perf_counter(); engine.reach_reduce(off, heads); t_dev = time.perf_counter() - t0
        rec["literal_150"] = {"nodes": len(nodes), "edges": int(heads.shape[0]), "has_path_calls": calls,
                              "literal_s": t_literal, "host_s": t_host, "device_call_s": t_dev}
        out["string400"] = rec
        print(json.dumps({"string400": rec}), flush=True)
        save()
    if args.workload in ("all", "digraph16k"):
        rng = np.random.default_rng(16384)
        n = 16384
        heads = rng.integers(0, n, size=3 * n, dtype=np.int64).astype(np.int32)
        off = np.arange(0, 3 * n + 1, 3, dtype=np.int64)
        out["digraph16k"] = dict(measure(engine, off, heads, args.reps, args.host_budget), edges_per_node=3)
        print(json.dumps({"digraph16k": out["digraph16k"]}), flush=True)
        save()
    def sweep(name, reads, sizes):
        rows = []
        for m in sizes:
            _, off, heads = string_csr(reads[:m])
            r = measure(engine, off, heads, args.reps, args.host_budget, count_ors=False)
            rows.append(dict(r, reads=m))
            print(json.dumps({"reads": m, "nodes": r["nodes"], "device_call_s": r["device_call"]["median_s"],
                              "host_s": r["host"]["median_s"], "kernels_s": r["kernels"]["median_s"]}), flush=True)
        out[name] = rows
        out.pop("crossover_work", None)
        both = sorted(out.get("sweep", []) + out.get("sweep2000", []), key=lambda r: r["nodes"])
        cross = None
        for i, r in enumerate(both):
            if all(x["device_call"]["median_s"] < x["host"]["median_s"] for x in both[i:]):
                cross = r["nodes"]
                break
        out["crossover_nodes"] = cross
        print(json.dumps({"crossover_nodes": cross}), flush=True)
        save()

    if args.workload in ("all", "sweep"):
        sweep("sweep", reads400, (8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 400))
    if args.workload in ("all", "sweep2000"):
        sweep("sweep2000", simulate_reads(genome, 100, 2000, 0.01, seed=1), (500, 600, 700, 850, 1000, 1300, 1700))
    if args.workload in ("all", "pipeline"):
        reads = simulate_reads(genome, 100, 2000, 0.01, seed=1)
        t0 = time.perf_counter()
        G = og._string_graph(reads, engine, None)
        t1 = time.perf_counter()
        nodes = list(G)
        off, heads = og._csr_heads(nodes, G._adj)
        t2 = time.perf_counter()
        mask = engine.reach_reduce(off, heads)
        t3 = time.perf_counter()
        R = og.transitive_reduction2(G, engine=engine, device=True)
        t4 = time.perf_counter()
        try:
            contigs = og.find_unitigs(R)
        except ValueError as e:  # a cycle of non-branching nodes: the reference never returns on it
            contigs = None
            note = str(e)
        t5 = time.perf_counter()
        out["pipeline2000"] = {
            "reads": len(reads), "nodes": len(nodes), "edges": int(heads.shape[0]), "reduced": int(mask.sum()),
            "string_graph_s": t1 - t0, "csr_s": t2 - t1, "reach_reduce_device_call_s": t3 - t2,
            "transitive_reduction2_s": t4 - t3, "find_unitigs_s": t5 - t4,
            "contigs": len(contigs) if contigs is not None else None,
            "find_unitigs_error": None if contigs is not None else note}
        print(json.dumps({"pipeline2000": out["pipeline2000"]}), flush=True)
        save()
    engine.close()


if __name__ == "__main__":
    main()
