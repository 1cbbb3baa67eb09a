"""Time the read-depth coverage on one GPU and write profiles/read_depth.json.

Workload: the profiles/local_batch.json assembly (PhiX, N = 10,000 reads of l = 100, p = 0.01, k = 5, fixed seed),
its reads against its contigs.  One warm-up, then ``--reps`` timed repetitions of each measurement; median and
spread (max - min):

  score_pass   the lane kernel's launches and their folds, from the HIP events around them (engine.set_timing),
               and the cells per second from that
  read_best    the whole OverlapEngine.read_best call (encoding, upload, score pass, start-position pass, results)
  read_depth   performanceMeasures.read_depth(device=True) end to end (read_best, the draws, the accumulation)
  baseline     the same pairs the way the code before ovl_read_best could do them: one
               engine.local_align_batch(traceback=False) over (read, contig) items, the contigs concatenated into
               one reference and each item's window one contig.  It runs on a strided subset of ``--baseline-reads``
               reads (the item records, the copies of the read per contig and eight int32 per item back make the
               whole workload's 2.6 * 10^7 items too large for it) and is SCALED by the pair count to the workload.
  sweep        read_best_host against engine.read_best on the first r reads and c contigs, r x c growing: the
               crossover ("crossover_cells") is the smallest cell count from which the device call's median stays
               below the host form's; it sets performanceMeasures.READ_DEPTH_DEVICE_MIN_CELLS.  The box's CPU is
               recorded with it.

    python tools/read_depth_probe.py [--out profiles/read_depth.json] [--reads 10000] [--baseline-reads 40]
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

SWEEP = ((1, 4), (2, 8), (4, 8), (8, 16), (16, 32), (32, 64), (64, 128))


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


def pair_cells(reads, contigs, read_length):
    """DP cells of every (read, contig): the read's length times the window it is aligned to."""
    total = 0
    sum_m = sum(len(c) for c in contigs)
    for r in reads:
        n = len(r)
        if 0 < n < read_length:
            total += n * sum(min(n, len(c)) for c in contigs)
        else:
            total += n * sum_m
    return total


def cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_depth.json"))
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--baseline-reads", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261019)
    args = ap.parse_args()

    import numpy as np
    from ovlgraph import OverlapEngine
    from ovlgraph import performanceMeasures as pm
    from ovlgraph.engine import read_best_host
    from ovlgraph.overlapGraphs import assemble_contigs_using_overlap_graphs
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads

    genome = read_genome_from_fasta()
    engine = OverlapEngine(0)
    L = 100
    reads = simulate_reads(genome, L, args.reads, 0.01, seed=args.seed)
    with contextlib.redirect_stdout(io.StringIO()):
        contigs = assemble_contigs_using_overlap_graphs(reads, 5, engine=engine)
    R, C = len(reads), len(contigs)
    cells = pair_cells(reads, contigs, L)
    out = {"genome_length": len(genome), "seed": args.seed, "reps": args.reps, "cpu": cpu_model(),
           "workload": {"N": args.reads, "l": L, "p": 0.01, "k": 5, "reads": R, "contigs": C, "pairs": R * C,
                        "cells": cells, "longest_contig": max((len(c) for c in contigs), default=0)}}
    print(json.dumps(out["workload"]), flush=True)

    # the whole call, and the score pass inside it
    call = timed(lambda: engine.read_best(reads, contigs, L), args.reps)
    engine.set_timing(True)
    engine.read_best(reads, contigs, L)
    kernel = []
    for _ in range(args.reps):
        engine.read_best(reads, contigs, L)
        kernel.append(engine.last_timing()["kernel_ms"] * 1e-3)
    engine.set_timing(False)
    routing = engine.last_read_best()
    k = summary(kernel)
    out["score_pass"] = dict(k, cells_per_s=cells / k["median_s"] if k["median_s"] > 0 else None, routing=routing)
    out["read_best"] = call
    print(json.dumps({"score_pass": out["score_pass"], "read_best": call}), flush=True)
    out["read_depth"] = timed(
        lambda: pm.read_depth(contigs, reads, L, engine=engine, device=True, rng=np.random.RandomState(1)), args.reps)
    print(json.dumps({"read_depth": out["read_depth"]}), flush=True)

    # the baseline on a strided subset, scaled by the pair count
    S = max(1, min(args.baseline_reads, R))
    sub = reads[:: max(1, R // S)][:S]
    ref = "".join(contigs)
    starts, lo = [], 0
    for c in contigs:
        starts.append(lo)
        lo += len(c)
    queries = [r for r in sub for _ in contigs]
    wins = []  # aligners.py:187-195: a read shorter than read_length takes the contig's tail
    for r in sub:
        for st, c in zip(starts, contigs):
            w = min(len(r), len(c)) if 0 < len(r) < L else len(c)
            wins.append((st + len(c) - w, w))

    def baseline():
        return engine.local_align_batch(queries, ref, wins, traceback=False)

    want = engine.read_best(sub, contigs, L, scores=True)["scores"]
    assert np.array_equal(baseline()[0].reshape(len(sub), C), want), "baseline and read_best disagree"
    base = timed(baseline, args.reps)
    engine.set_timing(True)
    baseline()
    base_kernel_s = engine.last_timing()["kernel_ms"] * 1e-3
    engine.set_timing(False)
    scale = (R * C) / (len(sub) * C)
    out["baseline"] = dict(base, reads=len(sub), pairs=len(sub) * C, kernel_s=base_kernel_s, scale=scale,
                           scaled_median_s=base["median_s"] * scale, scaled_spread_s=base["spread_s"] * scale,
                           scaled_kernel_s=base_kernel_s * scale,
                           kernel_cells_per_s=pair_cells(sub, contigs, L) / base_kernel_s if base_kernel_s else None,
                           note="measured on the subset; the scaled_* figures are multiplied by pairs / subset pairs")
    out["ratio_scaled_baseline_over_read_best"] = out["baseline"]["scaled_median_s"] / call["median_s"]
    out["accepted"] = (out["baseline"]["scaled_median_s"] - call["median_s"]
                       > out["baseline"]["scaled_spread_s"] + call["spread_s"])
    print(json.dumps({"baseline": out["baseline"], "ratio": out["ratio_scaled_baseline_over_read_best"],
                      "accepted": out["accepted"]}), flush=True)

    # host form against device call on growing subsets
    sweep, cross = [], None
    for r, c in SWEEP:
        rs, cs = reads[:r], contigs[:c]
        if len(rs) < r or len(cs) < c:
            break
        a, b = read_best_host(rs, cs, L, scores=True), engine.read_best(rs, cs, L, scores=True)
        assert all(np.array_equal(a[key], b[key]) for key in a), "host form and device call disagree"
        host = timed(lambda: read_best_host(rs, cs, L), args.reps)
        dev = timed(lambda: engine.read_best(rs, cs, L), args.reps)
        point = {"reads": r, "contigs": c, "cells": pair_cells(rs, cs, L), "host": host, "device": dev}
        sweep.append(point)
        print(json.dumps({key: (v if not isinstance(v, dict) else v["median_s"]) for key, v in point.items()}),
              flush=True)
    for i, p in enumerate(sweep):
        if all(q["device"]["median_s"] < q["host"]["median_s"] for q in sweep[i:]):
            cross = p["cells"]
            break
    out["sweep"] = sweep
    out["crossover_cells"] = cross
    print(json.dumps({"crossover_cells": cross}), flush=True)
    engine.close()

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
