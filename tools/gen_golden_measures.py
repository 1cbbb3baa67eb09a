"""Generate tests/golden/measures.json from the reference's own performanceMeasures source.

Runs only where the reference checkout exists (oracle/gen_golden.REF):

    python tools/gen_golden_measures.py

Executes performanceMeasures.calculate_measures (performanceMeasures.py:190-252) as oracle/gen_golden.py executes
the aligners: numba.njit replaced by the identity (oracle/gen_golden.import_reference).  The reference's ``plots``
module needs matplotlib and writes files, so a stand-in that only records which hooks fired is put into
sys.modules before the import.  The scoring arguments are the reference's defaults (10, -1, -1) on a few hundred
bases: no int32 cell is anywhere near wrapping, so CPython computes what Numba does.  Only inputs and outputs are
written.
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import random
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from gen_golden import GOLDEN, REF, import_reference  # noqa: E402
from gen_golden_local import indel_mutate  # noqa: E402

FIRED = []


def stub_plots():
    mod = types.ModuleType("plots")
    for name in ("plot_genome_coverage", "plot_genome_depth", "plot_reconstructed_coverage"):
        setattr(mod, name, lambda *a, _n=name, **k: FIRED.append(_n))
    sys.modules["plots"] = mod


def main():
    _, _, gefr = import_reference()
    stub_plots()
    import performanceMeasures as pm  # noqa: E402  (the reference's, REF is on sys.path)

    genome_all = gefr.read_genome_from_fasta(os.path.join(REF, "sequence.fasta"))
    rng = random.Random(20261019)

    def window(length):
        st = rng.randint(0, len(genome_all) - length)
        return genome_all[st:st + length]

    def run(name, contigs, genome, reads_length, num_iteration, error_prob=0.0, k=5):
        del FIRED[:]
        num_reads = len(contigs)
        t0 = time.time()
        with contextlib.redirect_stdout(io.StringIO()):
            measures, details = pm.calculate_measures(list(contigs), list(contigs), num_reads, reads_length,
                                                      error_prob, k, genome, name, num_iteration)
        assert list(measures) == ["Number of Contigs", "Genome Coverage", "N50", "Mismatch Rate Aligned Regions",
                                  "Mismatch Rate Genome Level"]
        rec = {
            "name": name,
            "args": {"contigs": list(contigs), "num_reads": num_reads, "reads_length": reads_length,
                     "error_prob": error_prob, "k": k, "ref_genome": genome, "experiment_name": name,
                     "num_iteration": num_iteration},
            "details": [[c, str(d["Print"]), str(d["Alignment_reference"]), str(d["Alignment_query"]),
                         int(d["Alignment Score"]), int(d["Start Position"]), int(d["End Position"])]
                        for c, d in details.items()],
            "measures": {"Number of Contigs": int(measures["Number of Contigs"]),
                         "Genome Coverage": float(measures["Genome Coverage"]),
                         "N50": int(measures["N50"]),
                         "Mismatch Rate Aligned Regions": float(measures["Mismatch Rate Aligned Regions"]),
                         "Mismatch Rate Genome Level": float(measures["Mismatch Rate Genome Level"])},
            "plots_fired": list(FIRED),
        }
        print(f"{name}: {len(contigs)} contigs, {len(details)} distinct, {time.time() - t0:.1f}s, "
              f"{rec['measures']}, plots {rec['plots_fired']}")
        return rec

    cases = []

    # 1. full coverage without errors: exact overlapping slices from the first base to the last
    g = window(400)
    contigs = [g[st:st + 60] for st in range(0, len(g) - 60, 12)] + [g[-60:]]
    rng.shuffle(contigs)
    cases.append(run("full_coverage_exact", contigs[:30], g, 50, 1))

    # 2. substitutions and indels: the aligned strings carry gaps
    g = window(500)
    contigs = []
    for _ in range(30):
        n = rng.randint(60, 180)
        st = rng.randint(0, len(g) - n)
        contigs.append(indel_mutate(rng, g[st:st + n], 0.04, 0.06))
    cases.append(run("errors_with_indels", contigs, g, 50, 1, error_prob=0.05))

    # 3. contigs shorter than reads_length (aligned to the genome's tail only), a repeated contig, an empty one
    g = window(350)
    contigs = []
    for _ in range(10):  # short, from the tail
        n = rng.randint(5, 79)
        contigs.append(indel_mutate(rng, g[len(g) - n:], 0.05, 0.03))
    for _ in range(6):   # short, from elsewhere: the tail window misses most of them
        n = rng.randint(10, 79)
        st = rng.randint(0, len(g) - 200)
        contigs.append(g[st:st + n])
    for _ in range(10):  # full-length
        n = rng.randint(80, 200)
        st = rng.randint(0, len(g) - n)
        contigs.append(indel_mutate(rng, g[st:st + n], 0.02, 0.02))
    contigs += [contigs[3], contigs[20], contigs[20], ""]
    cases.append(run("short_and_repeated", contigs, g, 80, 1, error_prob=0.02))

    # 4. uncovered stretches of the genome, on a later iteration (coverage not uniform: plotted)
    g = window(450)
    contigs = []
    for _ in range(28):
        n = rng.randint(50, 90)
        st = rng.choice([rng.randint(0, 120), rng.randint(250, len(g) - n)])
        contigs.append(indel_mutate(rng, g[st:st + n], 0.01, 0.01))
    cases.append(run("uncovered_bases", contigs, g, 50, 2, error_prob=0.01))

    # 5. a later iteration with uniform coverage: the plot hooks stay silent
    g = window(300)
    cases.append(run("uniform_second_iteration", [g, g], g, 50, 2))
    assert cases[-1]["plots_fired"] == [] and cases[0]["plots_fired"]

    meta = {"generator": "tools/gen_golden_measures.py",
            "reference": "roiteichman/Genome-Assembly-Using-Overlap-Graphs",
            "numba": "absent: njit replaced by identity; default scoring (10, -1, -1), far from int32 wrapping",
            "plots": "stand-in module recording which hooks fired",
            "details": "[contig, Print, Alignment_reference, Alignment_query, Alignment Score, Start Position, "
                       "End Position] in the details dict's order"}
    with open(os.path.join(GOLDEN, "measures.json"), "w") as fh:
        json.dump({"meta": meta, "cases": cases}, fh)


if __name__ == "__main__":
    main()
