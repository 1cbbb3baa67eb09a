"""Time seed-candidate enumeration on one GPU and write profiles/seed_candidates.json.

Workloads: PhiX, reads of l = 100 at p = 0.01 (fixed seed), k = 12, at N = 10,000 and N = 50,000 (``--reads``).  One
warm-up, then ``--reps`` timed repetitions of each measurement; median and spread (max - min).  Per workload:

  kernels      the key kernel, the sort, the count kernel with the scan and the emit kernel of ovl_seed_candidates,
               from the HIP events around them (engine.set_timing, last_seed_timing), with the emit pass reading every
               offset's group from HBM ("keep") and searching it again ("search", OVL_SEED_GROUPS), the two forms'
               repetitions alternating
  call         the whole OverlapEngine.enumerate_seed_candidates call, both forms
  host         candidates.enumerate_seed_candidates (numpy) on the same reads; its list is checked against the device's
  score        OverlapEngine.score_candidates over the resident seed list
  assembly     assemble_contigs_using_overlap_graphs(seeds="any") end to end (``--assemble-reps`` repetitions; 0
               leaves it, and the contig figures, unmeasured), and the contig count, longest contig and N50 under both
               rules (k = 5 for the reference's)

and a sweep over small inputs, the first r reads of the first workload: the device call with its list copied to
the host against the numpy host form -- the only two steps in which the "device" and "host" routes of
candidates_and_scores differ.  ``crossover_reads`` is the first point from which the device route's median stays below
the host form's by more than the two spreads.

    python tools/seed_candidates_probe.py [--out profiles/seed_candidates.json] [--reads 10000 50000]
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

SWEEP = (8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096)
PARTS = ("keys_ms", "sort_ms", "count_ms", "emit_ms")


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
    """An engine whose emit pass takes the groups as ``form`` says (the knob is read when the context is made)."""
    from ovlgraph import OverlapEngine
    saved = os.environ.get("OVL_SEED_GROUPS")
    os.environ["OVL_SEED_GROUPS"] = form
    try:
        return OverlapEngine(0)
    finally:
        if saved is None:
            os.environ.pop("OVL_SEED_GROUPS", None)
        else:
            os.environ["OVL_SEED_GROUPS"] = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seed_candidates.json"))
    ap.add_argument("--reads", type=int, nargs="+", default=[10000, 50000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--assemble-reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    from ovlgraph.candidates import dedup_reads, enumerate_seed_candidates
    from ovlgraph.overlapGraphs import assemble_contigs_using_overlap_graphs
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads

    genome = read_genome_from_fasta()
    engines = {form: engine_with(form) for form in ("keep", "search")}
    k = args.k
    out = {"genome_length": len(genome), "seed": args.seed, "reps": args.reps, "k": k, "cpu": cpu_model(),
           "workloads": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    def small_inputs():
        # small inputs: where the two routes of candidates_and_scores differ
        reads = simulate_reads(genome, 100, args.reads[0], 0.01, seed=args.seed)
        distinct = dedup_reads(reads)[0]
        eng = engines["keep"]
        sweep, cross = [], None
        for r in SWEEP:
            if r > len(distinct):
                break
            sub = distinct[:r]
            eng.set_reads(sub)

            def device():
                return eng.candidates_copy(eng.enumerate_seed_candidates(k))

            point = {"reads": r, "pairs": eng.enumerate_seed_candidates(k),
                     "host": timed(lambda: enumerate_seed_candidates(sub, k), args.reps),
                     "device": timed(device, args.reps)}
            sweep.append(point)
            print(json.dumps({key: (v if not isinstance(v, dict) else [v["median_s"], v["spread_s"]])
                              for key, v in point.items()}), flush=True)
        for i, p in enumerate(sweep):
            if all(q["host"]["median_s"] - q["device"]["median_s"] > q["host"]["spread_s"] + q["device"]["spread_s"]
                   for q in sweep[i:]):
                cross = p["reads"]
                break
        out["sweep"] = sweep
        out["crossover_reads"] = cross
        print(json.dumps({"crossover_reads": cross}), flush=True)
        save()

    for n_reads in args.reads:
        reads = simulate_reads(genome, 100, n_reads, 0.01, seed=args.seed)
        distinct = dedup_reads(reads)[0]
        w = {"N": n_reads, "l": 100, "p": 0.01, "k": k, "distinct": len(distinct)}
        for eng in engines.values():
            eng.set_reads(distinct)
        # the whole call, and the kernels from their events, the two forms alternating
        calls = {form: [] for form in engines}
        parts = {form: {p: [] for p in PARTS} for form in engines}
        for timing in (False, True):
            for eng in engines.values():
                eng.set_timing(timing)
                eng.enumerate_seed_candidates(k)  # warm-up
            for _ in range(args.reps):
                for form, eng in engines.items():
                    t0 = time.perf_counter()
                    n_pairs = eng.enumerate_seed_candidates(k)
                    t1 = time.perf_counter()
                    if timing:
                        last = eng.last_seed_timing()
                        for p in PARTS:
                            parts[form][p].append(last[p] * 1e-3)
                    else:
                        calls[form].append(t1 - t0)
        for eng in engines.values():
            eng.set_timing(False)
        w["pairs"] = n_pairs
        w["call"] = {form: summary(ts) for form, ts in calls.items()}
        w["kernels"] = {form: {p[:-3]: summary(ts) for p, ts in parts[form].items()} for form in engines}
        w["kernels_sum"] = {form: sum(v["median_s"] for v in w["kernels"][form].values()) for form in engines}
        print(json.dumps({"N": n_reads, "pairs": n_pairs,
                          "call": {f: [v["median_s"], v["spread_s"]] for f, v in w["call"].items()},
                          "kernels": {f: {p: v["median_s"] for p, v in d.items()} for f, d in w["kernels"].items()}}),
              flush=True)

        eng = engines["keep"]
        host = enumerate_seed_candidates(distinct, k)
        for form, e in engines.items():
            a, b = e.candidates_copy(n_pairs)
            assert all(np.array_equal(x, y) for x, y in zip((a, b, e.seed_offsets()), host)), form
        w["host"] = timed(lambda: enumerate_seed_candidates(distinct, k), args.reps)
        w["score"] = timed(lambda: eng.score_candidates(), args.reps)
        print(json.dumps({"host": [w["host"]["median_s"], w["host"]["spread_s"]],
                          "score": [w["score"]["median_s"], w["score"]["spread_s"]]}), flush=True)

        if args.assemble_reps > 0:
            print(json.dumps({"assembling": n_reads}), flush=True)

            def assemble(**kw):
                with contextlib.redirect_stdout(io.StringIO()):
                    return assemble_contigs_using_overlap_graphs(reads, engine=eng, **kw)

            t0 = time.perf_counter()
            contigs = assemble(k=k, seeds="any")
            first = time.perf_counter() - t0
            # a repetition that takes minutes is measured once more, not five times
            reps = args.assemble_reps if first < 20.0 else 1
            w["assembly"] = dict(timed(lambda: assemble(k=k, seeds="any"), reps), first_s=first, reps=reps)
            w["contigs"] = {"any_k%d" % k: contig_figures(contigs),
                            "suffix_k5": contig_figures(assemble(k=5, seeds="suffix"))}
            print(json.dumps({"assembly": [w["assembly"]["median_s"], w["assembly"]["spread_s"]],
                              "contigs": w["contigs"]}), flush=True)
        else:
            w["assembly"] = w["contigs"] = "not measured"
        out["workloads"].append(w)
        save()
        if len(out["workloads"]) == 1:
            small_inputs()  # (before the larger workloads: what is measured so far is on disk)

    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
