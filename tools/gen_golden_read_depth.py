"""Generate tests/golden/read_depth.json from the reference's own aligner source.

Runs only where the reference checkout exists (oracle/gen_golden.REF):

    python tools/gen_golden_read_depth.py

For every (read, contig) of one small input it records what the reference's
``align_read_or_contig_to_reference(read, contig, read_length, match, mismatch, indel)`` returns at indices 3 to 5
(score, start, end): the values that plots.py:115-135 (plot_reconstructed_coverage) selects on.  The aligner is
executed as oracle/gen_golden.py executes it: numba.njit replaced by the identity (import_reference).  The scoring
is the reference's default (10, -1, -1) on reads of about 40 bases, far from int32 wrapping, so CPython computes what
Numba does.  Only the inputs and those triples are written.
"""
from __future__ import annotations

import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from gen_golden import GOLDEN, REF, import_reference, mutate, rand_seq  # noqa: E402

READ_LENGTH = 40
SCORING = (10, -1, -1)


def main():
    aligners, _, gefr = import_reference()
    genome_all = gefr.read_genome_from_fasta(os.path.join(REF, "sequence.fasta"))
    rng = random.Random(20261020)
    st = rng.randint(0, len(genome_all) - 600)
    g = genome_all[st:st + 600]

    # pieces of the window that overlap (reads inside an overlap tie), one repeated, one of 25 bases, one empty
    contigs = [g[0:150], g[120:300], g[280:420], g[400:600], g[120:300], g[300:325], "", g[50:200]]
    # an alignment longer than twice its read: A + B against A + 60 x "T" + B opens one gap of 60 for 200 points
    a, b = rand_seq(rng, 20, "ACG"), rand_seq(rng, 20, "ACG")
    contigs.append(a + "T" * 60 + b)
    gap_contig = len(contigs) - 1

    reads = []
    for _ in range(110):  # full-length reads with a few substitutions
        p = rng.randint(0, len(g) - READ_LENGTH)
        reads.append(mutate(rng, g[p:p + READ_LENGTH], 0.02))
    for _ in range(20):   # error-free reads from the stretch three contigs share
        p = rng.randint(120, 150 - 15)
        reads.append(g[p:p + READ_LENGTH])
    for _ in range(18):   # shorter than read_length: aligned to each contig's tail only
        n = rng.randint(8, READ_LENGTH - 1)
        p = rng.choice([150 - n, 300 - n, 600 - n, rng.randint(0, len(g) - n)])
        reads.append(mutate(rng, g[p:p + n], 0.03))
    for _ in range(3):    # longer than read_length
        n = rng.randint(READ_LENGTH + 1, READ_LENGTH + 12)
        p = rng.randint(0, len(g) - n)
        reads.append(g[p:p + n])
    reads += ["", a + b, reads[5]]
    gap_read = len(reads) - 2
    assert len(reads) == 154

    t0 = time.time()
    m, x, d = SCORING
    triples = []
    for read in reads:
        row = []
        for contig in contigs:
            t = aligners.align_read_or_contig_to_reference(read, contig, READ_LENGTH, m, x, d)
            assert len(t) == 6
            row.append([int(t[3]), int(t[4]), int(t[5])])
        triples.append(row)
    print(f"{len(reads)} reads x {len(contigs)} contigs in {time.time() - t0:.1f}s")

    n_best = []
    for row in triples:
        best = max(t[0] for t in row)
        n_best.append(sum(1 for t in row if t[0] == best))
    hist = {k: n_best.count(k) for k in sorted(set(n_best))}
    print("reads by number of best contigs:", hist)
    assert sum(1 for k in n_best if k >= 2) >= 20 and any(k >= 3 for k in n_best)
    assert any(0 < len(r) < READ_LENGTH for r in reads) and "" in reads
    assert "" in contigs and len(set(contigs)) < len(contigs)
    gs, gst, gen = triples[gap_read][gap_contig]
    assert gs == 340 and gen - gst == 100 > 2 * len(reads[gap_read]), (gs, gst, gen)
    assert max(t[0] for t in triples[gap_read]) == 340  # and that contig is the read's best

    meta = {"generator": "tools/gen_golden_read_depth.py",
            "reference": "roiteichman/Genome-Assembly-Using-Overlap-Graphs",
            "numba": "absent: njit replaced by identity; default scoring (10, -1, -1), far from int32 wrapping",
            "triples": "triples[r][c] = align_read_or_contig_to_reference(reads[r], contigs[c], read_length, "
                       "match, mismatch, indel)[3:6] = [score, start, end]",
            "n_best_histogram": {str(k): v for k, v in hist.items()},
            "gap_read": gap_read, "gap_contig": gap_contig}
    with open(os.path.join(GOLDEN, "read_depth.json"), "w") as fh:
        json.dump({"meta": meta, "read_length": READ_LENGTH, "match": m, "mismatch": x, "indel": d,
                   "reads": reads, "contigs": contigs, "triples": triples}, fh, separators=(",", ":"))


if __name__ == "__main__":
    main()
