"""Time transitive reduction on one GPU against the library's host loop and write profiles/transitive.json.

Workloads (each a CSR built by the project's own graph builders, fixed seeds):

  string2000   the string graph (all ordered pairs, score > 0) of PhiX reads N = 2,000, l = 100, p = 0.01
  kfiltered    the k-filtered graph of the bench's target point (N = 50,000, l = 100, k = 5), in copy space
  sweep        string graphs of the first m of the tests' 400 PhiX reads of 60 bases, m = 8 .. 400: the crossover

Per workload: one warm-up, then ``--reps`` timed repetitions of the device call (wall clock around
OverlapEngine.transitive_reduce, upload and download included) and of the host loop (ovl_transitive_reduce_host,
one thread) on the same arrays; medians and spreads (max - min); the kernel's own time from the HIP events around
it (engine.set_timing) over the same number of calls; two-hop steps per second of the kernel, and the LDS bytes
per second they stand for (one 4-byte row read per step), next to the chip's ds_read_b32 rate.  The two masks must
be equal.  A host run that takes longer than ``--host-budget`` seconds is repeated three times instead of
``--reps`` (recorded as "host_reps").  The crossover is the smallest step count of the sweep from which the
device call's median stays below the host loop's.

    python tools/transitive_probe.py [--workload all|string2000|kfiltered|sweep] [--out profiles/transitive.json]

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

LDS_READ_B32_BYTES_PER_S = 75e12  # every CU streaming ds_read_b32 (MI355X, ~2.4 GHz)


def summary(ts):
    return {"median_s": statistics.median(ts), "spread_s": max(ts) - min(ts), "all_s": ts}


def measure(engine, off, heads, weights, reps, host_budget):
    import numpy as np
    from ovlgraph.engine import transitive_reduce_host

    t0 = time.perf_counter()
    want = transitive_reduce_host(off, heads, weights)  # warm-up, and the mask the device must reproduce
    first_host = time.perf_counter() - t0
    got = engine.transitive_reduce(off, heads, weights)
    assert np.array_equal(got, want), "device and host masks differ"
    info = engine.last_transitive()
    host_reps = reps if first_host <= host_budget else 3
    t_dev, t_host, t_kernel = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter(); engine.transitive_reduce(off, heads, weights); t_dev.append(time.perf_counter() - t0)
    for _ in range(host_reps):
        t0 = time.perf_counter(); transitive_reduce_host(off, heads, weights); t_host.append(time.perf_counter() - t0)
    engine.set_timing(True)
    for _ in range(reps):
        engine.transitive_reduce(off, heads, weights)
        t_kernel.append(engine.last_timing()["kernel_ms"] * 1e-3)
    engine.set_timing(False)
    steps = info["two_hop_steps"]
    k = statistics.median(t_kernel)
    dev, host = summary(t_dev), summary(t_host)
    return {
        "nodes": int(off.shape[0] - 1), "edges": int(heads.shape[0]), "reduced": int(want.sum()),
        "two_hop_steps": steps, "window": info["window"], "passes": info["passes"],
        "device_call": dev, "host": host, "host_reps": host_reps, "kernel": summary(t_kernel),
        "host_over_device_call": host["median_s"] / dev["median_s"],
        "kernel_steps_per_s": steps / k if k > 0 else None,
        "kernel_lds_read_bytes_per_s": 4 * steps / k if k > 0 else None,
        "kernel_lds_share_of_read_b32_rate": 4 * steps / k / LDS_READ_B32_BYTES_PER_S if k > 0 else None,
        "host_steps_per_s": steps / host["median_s"] if host["median_s"] > 0 else None,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transitive.json"))
    ap.add_argument("--workload", default="all", choices=("all", "string2000", "kfiltered", "sweep"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-budget", type=float, default=15.0)
    args = ap.parse_args()

    from ovlgraph import OverlapEngine
    from ovlgraph import overlapGraphs as og
    from ovlgraph.reads import config_reads, read_genome_from_fasta, simulate_reads

    out = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            out = json.load(fh)
    out["reps"] = args.reps
    out["lds_read_b32_bytes_per_s"] = LDS_READ_B32_BYTES_PER_S
    genome = read_genome_from_fasta()
    engine = OverlapEngine(0)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    def csr_of(G):
        return G.__dict__["_ovl_edges"].csr()

    if args.workload in ("all", "string2000"):
        G, _ = og.construct_overlap_graph_string(simulate_reads(genome, 100, 2000, 0.01, seed=1), engine=engine)
        out["string2000"] = dict(measure(engine, *csr_of(G), args.reps, args.host_budget), N=2000, l=100, p=0.01)
        print(json.dumps({"string2000": out["string2000"]}), flush=True)
        save()
    if args.workload in ("all", "kfiltered"):
        G, _ = og.construct_overlap_graph_nx_k(config_reads("target", seed=0, genome=genome), k=5, engine=engine)
        out["kfiltered"] = dict(measure(engine, *csr_of(G), args.reps, args.host_budget), N=50000, l=100, p=0.01, k=5)
        print(json.dumps({"kfiltered": out["kfiltered"]}), flush=True)
        save()
    if args.workload in ("all", "sweep"):
        reads = list(dict.fromkeys(simulate_reads(genome, 60, 440, 0.01, seed=5)))[:400]
        rows = []
        for m in (8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 400):
            G, _ = og.construct_overlap_graph_string(reads[:m], engine=engine)
            r = measure(engine, *csr_of(G), args.reps, args.host_budget)
            rows.append(dict(r, reads=m))
            print(json.dumps({"reads": m, "steps": r["two_hop_steps"], "device_call_s": r["device_call"]["median_s"],
                              "host_s": r["host"]["median_s"], "kernel_s": r["kernel"]["median_s"]}), flush=True)
        cross = None
        for i, r in enumerate(rows):
            if all(x["device_call"]["median_s"] < x["host"]["median_s"] for x in rows[i:]):
                cross = r["two_hop_steps"]
                break
        out["sweep"] = rows
        out["crossover_steps"] = cross
        print(json.dumps({"crossover_steps": cross}), flush=True)
        save()
    engine.close()


if __name__ == "__main__":
    main()
