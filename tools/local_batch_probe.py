"""Time calculate_measures' alignment step two ways on one GPU and write profiles/local_batch.json:

(a) the per-contig loop over aligners.align_read_or_contig_to_reference (one launch per contig),
(b) one aligners.align_to_reference_batch call (one wavefront per contig in one launch),

on two workloads: the contigs the project's own assemble_contigs_using_overlap_graphs makes from PhiX reads
(N = 10,000, l = 100, p = 0.01, k = 5, fixed seed), and a synthetic batch of 4,096 items of 100 bases against
the whole genome.  One warm-up, then five timed repetitions each in alternating order; median and spread
(max - min) of both; the two result lists must be equal.  The batch kernel's own time comes from the HIP events
around it (engine.set_timing), and the cells per second from that.

    python tools/local_batch_probe.py [--out profiles/local_batch.json] [--reads 10000] [--items 4096]
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genome-assembly-using-overlap-graphs_amd"))


def time_both(aligners, engine, items, genome, read_length, reps):
    def loop():
        return [aligners.align_read_or_contig_to_reference(it, genome, read_length, engine=engine) for it in items]

    def batch():
        return aligners.align_to_reference_batch(items, genome, read_length, engine=engine)

    ra, rb = loop(), batch()  # warm-up, and the equality the comparison rests on
    assert ra == rb, "the batched call and the per-item loop disagree"
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); loop(); ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); batch(); tb.append(time.perf_counter() - t0)
    engine.set_timing(True)
    batch()
    kernel_ms = engine.last_timing()["kernel_ms"]
    stats = engine.last_local_batch()
    engine.set_timing(False)
    G = len(genome)
    cells = sum(len(it) * (len(it) if 0 < len(it) < read_length else G) for it in items)

    def summary(ts):
        return {"median_s": statistics.median(ts), "spread_s": max(ts) - min(ts), "all_s": ts}

    a, b = summary(ta), summary(tb)
    return {
        "items": len(items), "cells": cells, "loop": a, "batch": b,
        "ratio_loop_over_batch": a["median_s"] / b["median_s"],
        "accepted": a["median_s"] - b["median_s"] > a["spread_s"] + b["spread_s"],
        "batch_kernel_ms": kernel_ms,
        "batch_kernel_cells_per_s": cells / (kernel_ms * 1e-3) if kernel_ms > 0 else None,
        "routing": stats,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_batch.json"))
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--items", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261019)
    args = ap.parse_args()

    import numpy as np
    from ovlgraph import OverlapEngine, aligners
    from ovlgraph.overlapGraphs import assemble_contigs_using_overlap_graphs
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads

    genome = read_genome_from_fasta()
    engine = OverlapEngine(0)
    out = {"genome_length": len(genome), "seed": args.seed, "reps": args.reps}

    reads = simulate_reads(genome, 100, args.reads, 0.01, seed=args.seed)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        contigs = assemble_contigs_using_overlap_graphs(reads, 5, engine=engine)
    out["assembly"] = {
        "N": args.reads, "l": 100, "p": 0.01, "k": 5, "assemble_s": time.perf_counter() - t0,
        "contigs": len(contigs),
        "length_histogram": dict(sorted(Counter((len(c) // 100) * 100 for c in contigs).items())),
        "longest": max((len(c) for c in contigs), default=0),
    }
    print(json.dumps(out["assembly"]), flush=True)
    out["contigs"] = time_both(aligners, engine, contigs, genome, 100, args.reps)
    print(json.dumps(out["contigs"]), flush=True)

    rng = np.random.Generator(np.random.PCG64(args.seed))
    items = []
    for st in rng.integers(0, len(genome) - 100, size=args.items).tolist():  # exactly 100 bases, 1 % substituted
        item = list(genome[st:st + 100])
        for pos in np.nonzero(rng.random(100) <= 0.01)[0].tolist():
            item[pos] = "ACGT"[("ACGT".index(item[pos]) + int(rng.integers(1, 4))) % 4]
        items.append("".join(item))
    out["synthetic"] = time_both(aligners, engine, items, genome, 100, args.reps)
    print(json.dumps(out["synthetic"]), flush=True)
    engine.close()

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
