"""Time consensus polishing on one GPU and write profiles/consensus.json.

Workload: the profiles/local_batch.json assembly (PhiX, N = 10,000 reads of l = 100, p = 0.01, k = 5, fixed seed),
its reads placed on its contigs by ``read_best`` (first best).  One warm-up, then ``--reps`` timed repetitions of each
measurement; median and spread (max - min):

  kernels      the alignment launches (with their uploads), the pileup kernel and the vote kernel of ovl_consensus,
               from the HIP events around them (engine.set_timing, last_consensus)
  consensus    the whole OverlapEngine.consensus call (encoding, uploads, kernels, results)
  polish       consensus.polish_contigs(device=True), one round, end to end, placement included
  host         engine.consensus_host on the same placement
  baseline     what the code before ovl_consensus could do with the same placement: one
               engine.local_align_batch(traceback=True) with the contigs concatenated and one window per read, then
               a numpy pileup of the returned ops on the host.  Its counts are checked against the device call's.
               ``accepted``: the consensus call's median is below the baseline's by more than the two spreads.
  sweep        consensus_host against engine.consensus on the first r reads (all contigs), r growing: the
               crossover ("crossover_cells", cells = sum over placed reads of read length x window length) is the
               first point from which the device call's median stays below the host form's by more than the two
               spreads; it sets consensus.CONSENSUS_DEVICE_MIN_CELLS.  The box's CPU is recorded with it.
  quality      calculate_measures' two mismatch rates, and the contigs' summed alignment scores against the genome,
               before and after one round of polish_contigs

    python tools/consensus_probe.py [--out profiles/consensus.json] [--reads 10000]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genome-assembly-using-overlap-graphs_amd"))

SWEEP = (1, 2, 4, 8, 16, 32, 64, 128, 256, 1024)


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


def cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def windows(reads, contigs, place, read_length):
    """(lo, length) of every read's window in the concatenated contigs (aligners.py:187-195); (0, 0) unplaced."""
    starts, lo = [], 0
    for c in contigs:
        starts.append(lo)
        lo += len(c)
    wins = []
    for r, p in zip(reads, place):
        if p < 0:
            wins.append((0, 0))
            continue
        m, n = len(contigs[p]), len(r)
        w = n if 0 < n < read_length and n < m else m
        wins.append((starts[p] + m - w, w))
    return wins


def numpy_pileup(np, reads, wins, res, total):
    """The counts of DESIGN.md §4.14 from local_align_batch's (score, end_i, end_j, ., ., walks) on the host."""
    score, ei, ej, _, _, walks = res
    n = np.array([len(w) for w in walks], dtype=np.int64)
    ops = np.concatenate(walks) if len(walks) else np.zeros(0, dtype=np.int8)
    seg = np.repeat(np.arange(len(walks)), n)
    start = np.cumsum(n) - n
    col, row = (ops == 1) | (ops == 3), (ops == 1) | (ops == 2)
    c0 = np.concatenate(([0], np.cumsum(col)))
    r0 = np.concatenate(([0], np.cumsum(row)))
    wj = ej.astype(np.int64)[seg] - (c0[:-1] - np.repeat(c0[start], n))
    wi = ei.astype(np.int64)[seg] - (r0[:-1] - np.repeat(r0[start], n))
    q = np.frombuffer("".join(reads).encode("latin-1"), dtype=np.uint8)
    q_off = np.cumsum([0] + [len(r) for r in reads])[:-1]
    lut = np.full(256, -1, dtype=np.int64)
    for k, ch in enumerate(b"ACGT"):
        lut[ch] = k
    ch = np.where(ops == 3, 4, np.where(ops == 2, 5, lut[q[np.minimum(q_off[seg] + wi - 1, len(q) - 1)]]))
    lo = np.array([w[0] for w in wins], dtype=np.int64)
    idx = (lo[seg] + wj - 1) * 6 + ch
    return np.bincount(idx[ch >= 0], minlength=total * 6).reshape(total, 6).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus.json"))
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261019)
    args = ap.parse_args()

    import numpy as np
    from ovlgraph import OverlapEngine
    from ovlgraph import consensus as cs
    from ovlgraph import performanceMeasures as pm
    from ovlgraph.engine import consensus_host
    from ovlgraph.overlapGraphs import assemble_contigs_using_overlap_graphs
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads

    genome = read_genome_from_fasta()
    engine = OverlapEngine(0)
    L = 100
    reads = simulate_reads(genome, L, args.reads, 0.01, seed=args.seed)
    with contextlib.redirect_stdout(io.StringIO()):
        contigs = assemble_contigs_using_overlap_graphs(reads, 5, engine=engine)
    place = engine.read_best(reads, contigs, L)["first_best"]
    wins = windows(reads, contigs, place.tolist(), L)
    cells = sum(len(r) * w[1] for r, w in zip(reads, wins))
    total = sum(len(c) for c in contigs)
    out = {"genome_length": len(genome), "seed": args.seed, "reps": args.reps, "cpu": cpu_model(),
           "workload": {"N": args.reads, "l": L, "p": 0.01, "k": 5, "reads": len(reads), "contigs": len(contigs),
                        "bases": total, "cells": cells, "longest_contig": max((len(c) for c in contigs), default=0)}}
    print(json.dumps(out["workload"]), flush=True)

    def device():
        return engine.consensus(reads, contigs, place, L)

    call = timed(device, args.reps)
    engine.set_timing(True)
    device()
    parts = {"align": [], "pileup": [], "vote": []}
    for _ in range(args.reps):
        device()
        last = engine.last_consensus()
        for k in parts:
            parts[k].append(last[k + "_ms"] * 1e-3)
    engine.set_timing(False)
    out["kernels"] = {k: summary(v) for k, v in parts.items()}
    out["routing"] = {k: last[k] for k in ("batch_reads", "single_reads", "ops", "launches")}
    out["consensus"] = call
    print(json.dumps({"kernels": {k: v["median_s"] for k, v in out["kernels"].items()}, "routing": out["routing"],
                      "consensus": call}), flush=True)
    out["polish"] = timed(lambda: cs.polish_contigs(contigs, reads, L, engine=engine, device=True), args.reps)
    print(json.dumps({"polish": out["polish"]}), flush=True)

    # the baseline: the batched alignment with its ops back over the link, then a numpy pileup
    ref = "".join(contigs)

    def baseline():
        res = engine.local_align_batch(reads, ref, wins, traceback=True)
        return numpy_pileup(np, reads, wins, res, total)

    want = device()
    assert np.array_equal(baseline(), want["counts"]), "baseline and consensus disagree"
    base = timed(baseline, args.reps)
    t0 = time.perf_counter()
    res = engine.local_align_batch(reads, ref, wins, traceback=True)
    t1 = time.perf_counter()
    numpy_pileup(np, reads, wins, res, total)
    t2 = time.perf_counter()
    out["baseline"] = dict(base, align_batch_s=t1 - t0, numpy_pileup_s=t2 - t1)
    out["ratio_baseline_over_consensus"] = base["median_s"] / call["median_s"]
    out["accepted"] = base["median_s"] - call["median_s"] > base["spread_s"] + call["spread_s"]
    print(json.dumps({"baseline": out["baseline"], "ratio": out["ratio_baseline_over_consensus"],
                      "accepted": out["accepted"]}), flush=True)

    # the host form on the whole workload: one repetition less often, it is the slow one
    h = consensus_host(reads, contigs, place, L)
    assert all(np.array_equal(h[k], want[k]) for k in h), "host form and device call disagree"
    out["host"] = timed(lambda: consensus_host(reads, contigs, place, L), args.reps)
    print(json.dumps({"host": out["host"]}), flush=True)

    # host form against device call on growing subsets of the reads
    sweep, cross = [], None
    for r in SWEEP:
        if r > len(reads):
            break
        rs, ps = reads[:r], place[:r]
        host = timed(lambda: consensus_host(rs, contigs, ps, L), args.reps)
        dev = timed(lambda: engine.consensus(rs, contigs, ps, L), args.reps)
        point = {"reads": r, "cells": sum(len(x) * w[1] for x, w in zip(rs, wins)), "host": host, "device": dev}
        sweep.append(point)
        print(json.dumps({k: (v if not isinstance(v, dict) else [v["median_s"], v["spread_s"]])
                          for k, v in point.items()}), flush=True)
    for i, p in enumerate(sweep):
        if all(q["host"]["median_s"] - q["device"]["median_s"] > q["host"]["spread_s"] + q["device"]["spread_s"]
               for q in sweep[i:]):
            cross = p["cells"]
            break
    out["sweep"] = sweep
    out["crossover_cells"] = cross
    print(json.dumps({"crossover_cells": cross}), flush=True)

    # quality: the two mismatch rates before and after one round
    polished, pile = cs.polish_contigs(contigs, reads, L, engine=engine, device=True)
    quality = {"n_changed": pile.n_changed, "n_other": pile.n_other}
    for name, cset in (("before", contigs), ("after", polished)):
        with contextlib.redirect_stdout(io.StringIO()):
            m, details = pm.calculate_measures(cset, reads, len(reads), L, 0.01, 5, genome, "probe", 1,
                                               engine=engine)
        quality[name] = {k: m[k] for k in ("Number of Contigs", "Genome Coverage", "N50",
                                           "Mismatch Rate Aligned Regions", "Mismatch Rate Genome Level")}
        # the rates saturate when every genome position lies under some contig with an error; the contigs' summed
        # alignment scores against the genome move with every corrected base
        quality[name]["Alignment Score Sum"] = int(sum(d["Alignment Score"] for d in details.values()))
    out["quality"] = quality
    print(json.dumps({"quality": quality}), flush=True)
    engine.close()

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
