"""Time placed consensus on one GPU and write profiles/consensus_placed.json.

Workloads: PhiX, l = 100, p = 0.01, seed 0, k = 12 seed candidates, at N = 10,000 and N = 50,000 reads, laid out by
``assemble_contigs_best_successor`` on the GPU; the distinct reads vote at the layout's placement with their copy
counts (slack 8, one round).  One warm-up, then ``--reps`` timed repetitions of each measurement; median and spread
(max - min):

  placed       the whole OverlapEngine.consensus_placed call (encoding, uploads, kernels, results)
  kernels      the band kernel and the vote kernel, from the HIP events around them (set_timing,
               last_consensus_placed)
  polish       baseline 1: consensus.polish_contigs(contigs, reads, 100), one round, placement by read_best included
  consensus    baseline 2: OverlapEngine.consensus with place = the layout's contig and read_length = 0 (every read
               against its whole contig)
               ``ahead_of_*``: the placed call's median is below the baseline's by more than the two spreads together
  pipeline     assemble_contigs_best_successor end to end with polish=0 and with polish=1
  sweep        (first workload) consensus_placed_host against engine.consensus_placed on the first r distinct reads, r
               growing; cells = sum over the reads of read length x (2 * slack + 1).  "crossover_cells" is the first
               point from which the device call's median stays below the host form's by more than the two spreads;
               it sets consensus.CONSENSUS_PLACED_DEVICE_MIN_CELLS.  The box's CPU is recorded with it.
  quality      the longest contig's ungapped mismatches against the genome (placed by an exact 30-base anchor), before
               and after polishing

    python tools/consensus_placed_probe.py [--out profiles/consensus_placed.json] [--reads 10000 50000]
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

SWEEP = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096)
SLACK = 8


def summary(ts):
    return {"median_s": statistics.median(ts), "spread_s": max(ts) - min(ts), "all_s": ts}


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return summary(ts)


def ahead(fast, slow):
    return slow["median_s"] - fast["median_s"] > slow["spread_s"] + fast["spread_s"]


def cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def mismatches_against(genome, contig):
    for a in range(0, len(contig) - 30, 30):
        at = genome.find(contig[a:a + 30])
        if at >= 0:
            shift = at - a
            lo, hi = max(0, -shift), min(len(contig), len(genome) - shift)
            return sum(contig[i] != genome[i + shift] for i in range(lo, hi))
    return None


def brief(d):
    return {k: ([v["median_s"], v["spread_s"]] if isinstance(v, dict) and "median_s" in v else v)
            for k, v in d.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus_placed.json"))
    ap.add_argument("--reads", type=int, nargs="+", default=[10000, 50000])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    from ovlgraph import OverlapEngine
    from ovlgraph import consensus as cs
    from ovlgraph.engine import consensus_placed_host
    from ovlgraph.layout import assemble_contigs_best_successor
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads

    genome = read_genome_from_fasta()
    engine = OverlapEngine(0)
    L = 100
    out = {"genome_length": len(genome), "seed": 0, "reps": args.reps, "cpu": cpu_model(), "slack": SLACK,
           "workloads": []}
    for n_reads in args.reads:
        reads = simulate_reads(genome, L, n_reads, 0.01, seed=0)
        lay = {}
        contigs = assemble_contigs_best_successor(reads, k=12, engine=engine, layout_out=lay)
        distinct, contig, offset = lay["reads"], lay["contig"], lay["offset"]
        from ovlgraph.candidates import dedup_reads
        copies = dedup_reads(reads)[1]
        total = sum(len(c) for c in contigs)
        w = {"N": n_reads, "l": L, "p": 0.01, "k": 12, "distinct_reads": len(distinct), "contigs": len(contigs),
             "bases": total, "longest_contig": max(len(c) for c in contigs),
             "band_cells": sum(len(r) for r in distinct) * (2 * SLACK + 1),
             "whole_contig_cells": int(sum(len(r) * len(contigs[c]) for r, c in zip(distinct, contig.tolist())))}
        print(json.dumps(w), flush=True)

        def placed():
            return engine.consensus_placed(distinct, contigs, contig, offset, SLACK, copies, 1)

        got = placed()
        host = consensus_placed_host(distinct, contigs, contig, offset, SLACK, copies, 1)
        assert all(np.array_equal(got[k], host[k]) for k in host), "device and host form disagree"
        w["placed"] = timed(placed, args.reps)
        engine.set_timing(True)
        placed()
        parts = {"band": [], "vote": []}
        for _ in range(args.reps):
            placed()
            last = engine.last_consensus_placed()
            for k in parts:
                parts[k].append(last[k + "_ms"] * 1e-3)
        engine.set_timing(False)
        w["kernels"] = {k: summary(v) for k, v in parts.items()}
        w["counters"] = {k: last[k] for k in ("voted_reads", "windowless_reads", "ops", "launches", "rounds")}
        w["host"] = timed(lambda: consensus_placed_host(distinct, contigs, contig, offset, SLACK, copies, 1), args.reps)
        print(json.dumps(brief({"placed": w["placed"], "band": w["kernels"]["band"], "vote": w["kernels"]["vote"],
                                "host": w["host"], "counters": w["counters"]})), flush=True)

        w["polish"] = timed(lambda: cs.polish_contigs(contigs, reads, L, engine=engine, device=True), args.reps)
        w["consensus"] = timed(lambda: engine.consensus(distinct, contigs, contig, 0), args.reps)
        w["ahead_of_polish"] = ahead(w["placed"], w["polish"])
        w["ahead_of_consensus"] = ahead(w["placed"], w["consensus"])
        print(json.dumps(brief({k: w[k] for k in ("polish", "consensus", "ahead_of_polish", "ahead_of_consensus")})),
              flush=True)

        w["pipeline"] = {
            "polish_0": timed(lambda: assemble_contigs_best_successor(reads, k=12, engine=engine), args.reps),
            "polish_1": timed(lambda: assemble_contigs_best_successor(reads, k=12, engine=engine, polish=1),
                              args.reps)}
        stages = {}
        polished = assemble_contigs_best_successor(reads, k=12, engine=engine, polish=1, timing=stages)
        w["pipeline"]["stages_s"] = stages
        k = max(range(len(contigs)), key=lambda i: len(contigs[i]))
        w["quality"] = {"longest_contig_mismatches_before": mismatches_against(genome, contigs[k]),
                        "longest_contig_mismatches_after": mismatches_against(genome, polished[k]),
                        "bases_changed": got["total_changed"]}
        print(json.dumps(brief(dict(w["pipeline"], **w["quality"]))), flush=True)

        if not out["workloads"]:
            sweep, cross = [], None
            for r in SWEEP + (len(distinct),):
                if r > len(distinct):
                    continue
                rs, cs_, os_, ws = distinct[:r], contig[:r], offset[:r], copies[:r]
                h = timed(lambda: consensus_placed_host(rs, contigs, cs_, os_, SLACK, ws, 1), args.reps)
                d = timed(lambda: engine.consensus_placed(rs, contigs, cs_, os_, SLACK, ws, 1), args.reps)
                point = {"reads": r, "cells": sum(len(x) for x in rs) * (2 * SLACK + 1), "host": h, "device": d}
                sweep.append(point)
                print(json.dumps(brief(point)), flush=True)
            for i, p in enumerate(sweep):
                if all(ahead(q["device"], q["host"]) for q in sweep[i:]):
                    cross = p["cells"]
                    break
            w["sweep"] = sweep
            w["crossover_cells"] = cross
            print(json.dumps({"crossover_cells": cross}), flush=True)
        out["workloads"].append(w)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
