"""Time the unitig pipeline from the score columns on one GPU against assemble_contigs and write
profiles/unitigs_direct.json.

Workloads (fixed seeds):

  reads400     the tests' 400 distinct PhiX reads of 60 bases
  reads2000    PhiX reads N = 2,000, l = 100, p = 0.01 (DESIGN.md 4.12's workload)
  sweep        the first r of reads2000's reads, r = 8 .. 2,000: the routing crossover

Per workload, after one warm-up of each route, ``--reps`` repetitions (wall clock, medians and spreads max - min) of

  direct       assemble_contigs_direct(reads, engine, device=True), the resident route: the whole call, its Python
               stages (dedup, encode, set_reads, enumerate, unitigs) and, from a second set of repetitions with timing
               on, the device stages of ovl_unitigs_candidates (scoring, edge build, closure plus marking, node facts)
               with the call's own clock; the host walk alone (ovl_unitigs_walk_host over the kept edges)
  host_route   assemble_contigs_direct(..., device=False): the columns scored by the engine, then ovl_unitigs_host
  host_form    ovl_unitigs_host alone on one thread, over columns made beforehand
  graph_route  assemble_contigs(reads, engine): the string graph as a networkx object, transitive_reduction2,
               find_unitigs

The routes must return the same contigs (or raise the same ValueError).  The sweep times direct against host_route; the
crossover is the smallest r from which direct's median stays below host_route's ("crossover_reads").

    python tools/unitigs_probe.py [--workload all|reads400|reads2000|sweep] [--out profiles/unitigs_direct.json]

Sections already in the output file are kept, so the workloads can be run one at a time.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genome-assembly-using-overlap-graphs_amd"))


def summary(ts):
    return {"median_s": statistics.median(ts), "spread_s": max(ts) - min(ts), "all_s": ts}


def outcome(fn):
    try:
        return fn()
    except ValueError as e:
        return str(e)


def timed(fn, reps):
    outcome(fn)  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        outcome(fn)
        ts.append(time.perf_counter() - t0)
    return ts


def measure_direct(engine, reads, reps):
    """The resident route: whole call, Python stages, device stages."""
    from ovlgraph.unitigs import assemble_contigs_direct
    rec = {"call": summary(timed(lambda: assemble_contigs_direct(reads, engine, device=True), reps))}
    stages, device = {}, {}
    engine.set_timing(True)
    try:
        for _ in range(reps):
            st = {}
            outcome(lambda: assemble_contigs_direct(reads, engine, device=True, timing=st))
            for k, v in st.items():
                stages.setdefault(k, []).append(v)
            last = dict(engine.last_unitigs(), **engine.last_timing())
            for k in ("score_ms", "build_ms", "reduce_ms", "facts_ms", "kernel_ms", "call_ms"):
                device.setdefault(k, []).append(last[k] * 1e-3)
    finally:
        engine.set_timing(False)
    rec["python_stages"] = {k: summary(v) for k, v in stages.items()}
    rec["device_stages"] = {k[:-3] + "_s": summary(v) for k, v in device.items()}
    rec["counts"] = {k: last[k] for k in ("edges", "kept", "paths", "words_per_row")}
    return rec


def measure_walk(engine, reads, reps):
    """find_unitigs' walk in native code over the kept edges, alone."""
    import numpy as np
    from ovlgraph.engine import unitigs_walk_host
    from ovlgraph.unitigs import reduced_string_graph
    red = reduced_string_graph(reads, engine, device=True)
    off = np.zeros(len(red.nodes) + 1, np.int64)
    np.cumsum(np.bincount(red.tail, minlength=len(red.nodes)), out=off[1:])
    return summary(timed(lambda: unitigs_walk_host(off, red.head), reps))


def measure_host_form(engine, reads, reps):
    import numpy as np
    from ovlgraph.candidates import dedup_reads
    from ovlgraph.engine import encode_reads, unitigs_host
    from ovlgraph.unitigs import _columns
    distinct, _ = dedup_reads(reads)
    index = {r: i for i, r in enumerate(distinct)}
    ids = np.fromiter((index[r] for r in reads), dtype=np.int32, count=len(reads))
    enc = encode_reads(distinct)
    cols = [None if c is None else np.array(c) for c in _columns(distinct, ids, engine, None, enc)]
    return summary(timed(lambda: unitigs_host(enc, ids, *cols), reps))


def workload(engine, reads, reps, graph_reps):
    from ovlgraph import overlapGraphs as og
    from ovlgraph.unitigs import assemble_contigs_direct
    want = outcome(lambda: og.assemble_contigs(reads, engine))
    for device in (True, False):
        assert outcome(lambda: assemble_contigs_direct(reads, engine, device=device)) == want, "the routes differ"
    rec = {"reads": len(reads), "distinct": len(set(reads)),
           "contigs": len(want) if isinstance(want, list) else None,
           "find_unitigs_error": None if isinstance(want, list) else want}
    rec["direct"] = measure_direct(engine, reads, reps)
    rec["direct"]["walk_alone"] = measure_walk(engine, reads, reps)
    rec["host_route"] = summary(timed(lambda: assemble_contigs_direct(reads, engine, device=False), reps))
    rec["host_form"] = measure_host_form(engine, reads, reps)
    rec["graph_route"] = summary(timed(lambda: og.assemble_contigs(reads, engine), graph_reps))
    d, g = rec["direct"]["call"], rec["graph_route"]
    rec["graph_over_direct"] = g["median_s"] / d["median_s"]
    rec["ahead_by_more_than_both_spreads"] = g["median_s"] - d["median_s"] > g["spread_s"] + d["spread_s"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unitigs_direct.json"))
    ap.add_argument("--workload", default="all", choices=("all", "reads400", "reads2000", "sweep"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    from ovlgraph import OverlapEngine
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads
    from ovlgraph.unitigs import assemble_contigs_direct

    out = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            out = json.load(fh)
    out["reps"] = args.reps
    genome = read_genome_from_fasta()
    reads400 = list(dict.fromkeys(simulate_reads(genome, 60, 440, 0.01, seed=5)))[:400]
    reads2000 = simulate_reads(genome, 100, 2000, 0.01, seed=1)
    engine = OverlapEngine(0)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    if args.workload in ("all", "reads400"):
        out["reads400"] = dict(workload(engine, reads400, args.reps, args.reps), N=400, l=60, p=0.01)
        print(json.dumps({"reads400": out["reads400"]}), flush=True)
        save()
    if args.workload in ("all", "reads2000"):
        out["reads2000"] = dict(workload(engine, reads2000, args.reps, args.reps), N=2000, l=100, p=0.01)
        print(json.dumps({"reads2000": out["reads2000"]}), flush=True)
        save()
    if args.workload in ("all", "sweep"):
        rows = []
        for r in (8, 16, 32, 64, 96, 128, 192, 256, 384, 512, 768, 1000, 1400, 2000):
            reads = reads2000[:r]
            dev = summary(timed(lambda: assemble_contigs_direct(reads, engine, device=True), args.reps))
            host = summary(timed(lambda: assemble_contigs_direct(reads, engine, device=False), args.reps))
            rows.append({"reads": r, "distinct": len(set(reads)), "direct": dev, "host_route": host})
            print(json.dumps({"reads": r, "direct_s": dev["median_s"], "host_route_s": host["median_s"]}), flush=True)
        out["sweep"] = rows
        cross = None
        for i, row in enumerate(rows):
            if all(x["direct"]["median_s"] < x["host_route"]["median_s"] for x in rows[i:]):
                cross = row["distinct"]
                break
        out["crossover_reads"] = cross
        print(json.dumps({"crossover_reads": cross}), flush=True)
        save()
    engine.close()


if __name__ == "__main__":
    main()
