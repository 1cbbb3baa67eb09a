"""Time k-mer spectrum read correction on one GPU and write profiles/spectrum.json.

Workloads: PhiX, reads of l = 100 (fixed seed), k = 12, the threshold by the rule: N = 10,000 and N = 50,000 at
p = 0.01 and N = 50,000 at p = 0.05.  One warm-up, then ``--reps`` timed repetitions of each measurement; median and
spread (max - min).  Per workload:

  kernels      the key pass, the sort, the count pass and the correction pass of ovl_correct_reads, from the HIP events
               around them (engine.set_timing, last_correct)
  vote         the correction pass with its solid work items counted by LDS atomics and by ballot
               (OVL_SPECTRUM_VOTE), the two forms' repetitions alternating
  call         the whole OverlapEngine.correct_reads and kmer_spectrum calls on encoded reads (upload and download in)
  host         engine.correct_reads_host on the same reads; its output is checked against the device's
  errors       substitution errors before and after against the p = 0 reads of the same seed, and the correct bases
               changed by mistake
  downstream   distinct reads, and the candidate pairs and contigs / longest / N50 of assemble_contigs_best_successor
               with and without the stage (``--no-assembly`` leaves them unmeasured)

and a sweep over small inputs, the first r reads of the first workload, r doubling from 8: the device call against the
host form.  ``crossover_reads`` is the first point from which the device's median stays below the host form's by more
than the two spreads; ``crossover_windows`` the same point in windows.

    python tools/spectrum_probe.py [--out profiles/spectrum.json]
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

WORKLOADS = ((10000, 0.01), (50000, 0.01), (50000, 0.05))
PARTS = ("keys_ms", "sort_ms", "count_ms", "correct_ms")


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


def short(v):
    return [round(v["median_s"] * 1e3, 4), round(v["spread_s"] * 1e3, 4)]


def engine_with(vote):
    """An engine whose correction pass counts as ``vote`` says (the knob is read when the context is made)."""
    from ovlgraph import OverlapEngine
    saved = os.environ.get("OVL_SPECTRUM_VOTE")
    os.environ["OVL_SPECTRUM_VOTE"] = vote
    try:
        return OverlapEngine(0)
    finally:
        if saved is None:
            os.environ.pop("OVL_SPECTRUM_VOTE", None)
        else:
            os.environ["OVL_SPECTRUM_VOTE"] = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-assembly", action="store_true")
    args = ap.parse_args()

    import numpy as np
    from ovlgraph import OverlapEngine
    from ovlgraph.candidates import dedup_reads
    from ovlgraph.engine import correct_reads_host, encode_reads
    from ovlgraph.layout import assemble_contigs_best_successor
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads

    genome = read_genome_from_fasta()
    eng = OverlapEngine(0)
    k = args.k
    out = {"genome_length": len(genome), "seed": args.seed, "reps": args.reps, "k": k, "l": 100, "cpu": cpu_model(),
           "workloads": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    def decode(enc, buf):
        text = buf.tobytes().decode("latin-1")
        off = enc[1].tolist()
        return [text[off[r]:off[r + 1]] for r in range(len(off) - 1)]

    def small_inputs():
        reads = simulate_reads(genome, 100, WORKLOADS[0][0], WORKLOADS[0][1], seed=args.seed)
        sweep, cross, r = [], None, 8
        while r <= len(reads):
            sub = reads[:r]
            enc = encode_reads(sub)
            point = {"reads": r, "windows": int(np.maximum(np.diff(enc[1]) - k + 1, 0).sum()),
                     "host": timed(lambda: correct_reads_host(sub, k, 0, enc), args.reps),
                     "device": timed(lambda: eng.correct_reads(sub, k, 0, enc), args.reps)}
            sweep.append(point)
            print(json.dumps({"reads": r, "windows": point["windows"], "host_ms": short(point["host"]),
                              "device_ms": short(point["device"])}), flush=True)
            r *= 2
        for i, p in enumerate(sweep):
            if all(q["host"]["median_s"] - q["device"]["median_s"] > q["host"]["spread_s"] + q["device"]["spread_s"]
                   for q in sweep[i:]):
                cross = p
                break
        out["sweep"] = sweep
        out["crossover_reads"] = cross["reads"] if cross else None
        out["crossover_windows"] = cross["windows"] if cross else None
        print(json.dumps({"crossover_reads": out["crossover_reads"], "crossover_windows": out["crossover_windows"]}),
              flush=True)
        save()

    for n_reads, p in WORKLOADS:
        reads = simulate_reads(genome, 100, n_reads, p, seed=args.seed)
        clean = simulate_reads(genome, 100, n_reads, 0.0, seed=args.seed)
        enc = encode_reads(reads)
        w = {"N": n_reads, "l": 100, "p": p, "k": k}
        dev = eng.correct_reads(reads, k, 0, enc)
        host = correct_reads_host(reads, k, 0, enc)
        assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1]) and dev[2] == host[2]
        w["stats"] = dev[2]
        corrected = decode(enc, dev[0])
        c, n, t = (np.frombuffer("".join(x).encode("latin-1"), dtype=np.uint8) for x in (corrected, reads, clean))
        w["errors"] = {"before": int((n != t).sum()), "after": int((c != t).sum()),
                       "correct_bases_changed": int(((c != n) & (n == t)).sum()), "changes": int((c != n).sum())}
        # the kernels from their events, then the whole calls with timing off
        parts = {q: [] for q in PARTS}
        eng.set_timing(True)
        eng.correct_reads(reads, k, 0, enc)
        for _ in range(args.reps):
            eng.correct_reads(reads, k, 0, enc)
            last = eng.last_correct()
            for q in PARTS:
                parts[q].append(last[q] * 1e-3)
        eng.set_timing(False)
        w["kernels"] = {q[:-3]: summary(ts) for q, ts in parts.items()}
        w["kernels_sum_s"] = sum(v["median_s"] for v in w["kernels"].values())
        votes = {vote: engine_with(vote) for vote in ("atomic", "ballot")}
        took = {vote: [] for vote in votes}
        for e in votes.values():
            e.set_timing(True)
            got = e.correct_reads(reads, k, 0, enc)  # warm-up
            assert np.array_equal(got[0], host[0]) and got[2] == host[2]
        for _ in range(args.reps):
            for vote, e in votes.items():
                e.correct_reads(reads, k, 0, enc)
                took[vote].append(e.last_correct()["correct_ms"] * 1e-3)
        for e in votes.values():
            e.close()
        w["vote"] = {vote: summary(ts) for vote, ts in took.items()}
        w["call"] = {"correct_reads": timed(lambda: eng.correct_reads(reads, k, 0, enc), args.reps),
                     "kmer_spectrum": timed(lambda: eng.kmer_spectrum(reads, k, enc), args.reps)}
        w["host"] = timed(lambda: correct_reads_host(reads, k, 0, enc), args.reps)
        print(json.dumps({"N": n_reads, "p": p, "stats": w["stats"], "errors": w["errors"],
                          "kernels_ms": {q: short(v) for q, v in w["kernels"].items()},
                          "vote_ms": {q: short(v) for q, v in w["vote"].items()},
                          "call_ms": {q: short(v) for q, v in w["call"].items()}, "host_ms": short(w["host"])}),
              flush=True)
        if not args.no_assembly:
            down = {}
            for name, rs in (("raw", reads), ("corrected", corrected)):
                lay = {}
                contigs = assemble_contigs_best_successor(rs, k=k, engine=eng, layout_out=lay)
                down[name] = {"distinct_reads": len(dedup_reads(rs)[0]), "candidate_pairs": eng.candidates_device()[2],
                              "contigs": len(contigs), "longest_contig": max((len(x) for x in contigs), default=0),
                              "n50": n50(contigs), "links": lay["links"]}
            w["downstream"] = down
            print(json.dumps({"downstream": down}), flush=True)
        else:
            w["downstream"] = "not measured"
        out["workloads"].append(w)
        save()
        if len(out["workloads"]) == 1:
            small_inputs()  # (before the larger workloads: what is measured so far is on disk)
    eng.close()


if __name__ == "__main__":
    main()
