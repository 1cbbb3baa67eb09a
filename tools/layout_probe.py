"""Time the best-successor layout on one GPU and write profiles/layout.json.

Workloads: PhiX, reads of l = 100 at p = 0.01 (fixed seed), k = 12 seed candidates, at N = 10,000 and N = 50,000
(``--reads``).  One warm-up, then ``--reps`` timed repetitions of each measurement; median and spread (max - min).
Per workload:

  kernels      the parts of ovl_layout_candidates from the HIP events around them (engine.set_timing, last_layout):
               the scoring launches, the link kernel, the forest kernels (doubling, cycle check, heads, scan, placement,
               path marks; one host synchronisation lies inside) and the spelling -- with the link kernel reducing runs
               of equal a inside the wavefront ("runs") and issuing one atomic per eligible pair ("plain",
               OVL_LAYOUT_LINK), the two forms' repetitions alternating
  call         the whole OverlapEngine.layout_candidates call (outputs back on the host, contigs not yet decoded), both
               forms
  end_to_end   assemble_contigs_best_successor(reads, k) from the reads to the contigs, with the read set already
               resident from the call before (ovl_set_reads recognises it and skips the upload), and "cold": another
               read set made resident before every call, outside its time, so that the call uploads its reads
  reference    assemble_contigs_using_overlap_graphs(k, seeds="any") on the same box (``--assemble-reps``; 0 leaves it
               unmeasured)
  host_route   with the list and its scores already on the host: ovl_layout_host and ovl_layout (upload included),
               twice the repetitions
  contigs      count, longest and N50 of both layouts; the best-successor layout's links, cycles, on-path reads

and a sweep over small inputs, the first r reads of the first workload, their host list scored once: ovl_layout_host
against ovl_layout on the same columns.  ``crossover_pairs`` is the first point, of the sweep and the workloads' host
routes together, from which the device form's median stays below the host form's by more than the two spreads (null:
it never did) -- layout.LAYOUT_DEVICE_MIN_PAIRS.

    python tools/layout_probe.py [--out profiles/layout.json] [--reads 10000 50000]
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

SWEEP = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 8400, 8600, 8800)
PARTS = ("score_ms", "link_ms", "forest_ms", "spell_ms")


def summary(ts):
    # (one repetition has no spread: null, not 0)
    return {"median_s": statistics.median(ts), "spread_s": max(ts) - min(ts) if len(ts) > 1 else None, "all_s": ts}


def timed(fn, reps, before=None):
    """One warm-up, then ``reps`` timed calls of ``fn``; ``before`` runs ahead of each call, outside its time."""
    if before:
        before()
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return summary(ts)


def brief(v):
    return [v["median_s"], v["spread_s"]]


def cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def n50(contigs):
    lens = sorted((len(c) for c in contigs), reverse=True)
    half, run = sum(lens) / 2.0, 0
    for x in lens:
        run += x
        if run >= half:
            return x
    return 0


def contig_figures(contigs):
    return {"contigs": len(contigs), "longest_contig": max((len(c) for c in contigs), default=0), "n50": n50(contigs)}


def engine_with(form):
    """An engine whose link kernel takes the form ``form`` (the knob is read when the context is made)."""
    from ovlgraph import OverlapEngine
    saved = os.environ.get("OVL_LAYOUT_LINK")
    os.environ["OVL_LAYOUT_LINK"] = form
    try:
        return OverlapEngine(0)
    finally:
        if saved is None:
            os.environ.pop("OVL_LAYOUT_LINK", None)
        else:
            os.environ["OVL_LAYOUT_LINK"] = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layout.json"))
    ap.add_argument("--reads", type=int, nargs="+", default=[10000, 50000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--assemble-reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    from ovlgraph.candidates import dedup_reads
    from ovlgraph.engine import layout_host
    from ovlgraph.layout import assemble_contigs_best_successor
    from ovlgraph.overlapGraphs import assemble_contigs_using_overlap_graphs, candidates_and_scores
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads

    genome = read_genome_from_fasta()
    engines = {form: engine_with(form) for form in ("runs", "plain")}
    eng = engines["runs"]
    k = args.k
    out = {"genome_length": len(genome), "seed": args.seed, "reps": args.reps, "k": k, "cpu": cpu_model(),
           "workloads": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    def same(x, y):
        return all(np.array_equal(x[key], y[key]) for key in ("succ", "link", "contig", "offset", "on_path", "bases"))

    def small_inputs():
        reads = simulate_reads(genome, 100, args.reads[0], 0.01, seed=args.seed)
        distinct = dedup_reads(reads)[0]
        sweep = []
        for r in SWEEP:
            if r > len(distinct):
                break
            sub = distinct[:r]
            a, b, sc, en = (np.array(x) for x in candidates_and_scores(sub, k, eng, None, "host", None, "any"))
            assert same(eng.layout(sub, a, b, sc, en), layout_host(sub, a, b, sc, en))
            point = {"reads": r, "pairs": int(a.shape[0]),
                     "host": timed(lambda: layout_host(sub, a, b, sc, en), args.reps),
                     "device": timed(lambda: eng.layout(sub, a, b, sc, en), args.reps)}
            sweep.append(point)
            print(json.dumps({key: (v if not isinstance(v, dict) else brief(v)) for key, v in point.items()}),
                  flush=True)
        out["sweep"] = sweep
        save()

    def crossover():
        # over the sweep and the whole workloads' host routes, by pairs
        points = sorted(out.get("sweep", []) + [dict(w["host_route"], pairs=w["pairs"]) for w in out["workloads"]],
                        key=lambda q: q["pairs"])
        cross = None
        for i, p in enumerate(points):
            if all(q["host"]["median_s"] - q["device"]["median_s"] > q["host"]["spread_s"] + q["device"]["spread_s"]
                   for q in points[i:]):
                cross = p["pairs"]
                break
        out["crossover_pairs"] = cross
        print(json.dumps({"crossover_pairs": cross}), flush=True)
        save()

    for n_reads in args.reads:
        reads = simulate_reads(genome, 100, n_reads, 0.01, seed=args.seed)
        distinct = dedup_reads(reads)[0]
        w = {"N": n_reads, "l": 100, "p": 0.01, "k": k, "distinct": len(distinct)}
        for e in engines.values():
            e.set_reads(distinct)
            w["pairs"] = e.enumerate_seed_candidates(k)
        calls = {form: [] for form in engines}
        parts = {form: {p: [] for p in PARTS} for form in engines}
        results = {}
        for timing in (False, True):
            for form, e in engines.items():
                e.set_timing(timing)
                results[form] = e.layout_candidates()  # warm-up
            for _ in range(args.reps):
                for form, e in engines.items():
                    t0 = time.perf_counter()
                    res = e.layout_candidates()
                    t1 = time.perf_counter()
                    if timing:
                        for p in PARTS:
                            parts[form][p].append(res[p] * 1e-3)
                    else:
                        calls[form].append(t1 - t0)
        for e in engines.values():
            e.set_timing(False)
        assert same(results["runs"], results["plain"])
        w["call"] = {form: summary(ts) for form, ts in calls.items()}
        w["kernels"] = {form: {p[:-3]: summary(ts) for p, ts in parts[form].items()} for form in engines}
        w["layout"] = {key: int(results["runs"][key]) for key in ("links", "cycles", "levels", "on_path_reads",
                                                                   "n_contigs")}
        print(json.dumps({"N": n_reads, "pairs": w["pairs"], "layout": w["layout"],
                          "call": {f: brief(v) for f, v in w["call"].items()},
                          "kernels": {f: {p: brief(v) for p, v in d.items()} for f, d in w["kernels"].items()}}),
              flush=True)

        # the host route: the list and its scores on the host, then either form
        a, b = eng.candidates_copy(w["pairs"])
        sc, en = eng.score_candidates()
        assert same(layout_host(distinct, a, b, sc, en), results["runs"])
        w["host_route"] = {"host": timed(lambda: layout_host(distinct, a, b, sc, en), 2 * args.reps),
                           "device": timed(lambda: eng.layout(distinct, a, b, sc, en), 2 * args.reps),
                           "reps": 2 * args.reps}
        print(json.dumps({"host_route": {f: brief(w["host_route"][f]) for f in ("host", "device")}}), flush=True)

        contigs = assemble_contigs_best_successor(reads, k=k, engine=eng)
        # the same reads again are recognised as resident by ovl_set_reads, which then skips their upload; with another
        # read set made resident before every call (outside its time) the call uploads them
        w["end_to_end"] = timed(lambda: assemble_contigs_best_successor(reads, k=k, engine=eng), args.reps)
        w["end_to_end_cold"] = timed(lambda: assemble_contigs_best_successor(reads, k=k, engine=eng), args.reps,
                                     before=lambda: eng.set_reads(["ACGTACGTACGTACGT", "TTTTACGTACGTACGG"]))
        w["contigs"] = {"best_successor": contig_figures(contigs)}
        print(json.dumps({"end_to_end": brief(w["end_to_end"]), "end_to_end_cold": brief(w["end_to_end_cold"]),
                          "contigs": w["contigs"]}), flush=True)

        if args.assemble_reps > 0:
            def assemble():
                with contextlib.redirect_stdout(io.StringIO()):
                    return assemble_contigs_using_overlap_graphs(reads, engine=eng, k=k, seeds="any")

            t0 = time.perf_counter()
            ref = assemble()
            first = time.perf_counter() - t0
            w["reference"] = dict(timed(assemble, args.assemble_reps), first_s=first, reps=args.assemble_reps)
            w["contigs"]["reference"] = contig_figures(ref)
            w["ratio"] = w["reference"]["median_s"] / w["end_to_end"]["median_s"]
            w["ratio_cold"] = w["reference"]["median_s"] / w["end_to_end_cold"]["median_s"]
            print(json.dumps({"reference": brief(w["reference"]), "contigs": w["contigs"]["reference"],
                              "ratio": w["ratio"], "ratio_cold": w["ratio_cold"]}), flush=True)
        else:
            w["reference"] = "not measured"
        out["workloads"].append(w)
        save()
        if len(out["workloads"]) == 1:
            small_inputs()  # (before the larger workloads: what is measured so far is on disk)

    crossover()
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
