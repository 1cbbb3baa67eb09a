"""Generate tests/golden/consensus.json from the reference's own aligner source.

Runs only where the reference checkout exists (oracle/gen_golden.REF):

    python tools/gen_golden_consensus.py

For one small input (reads, contigs and a placement of the reads on the contigs) it records, for every placed read,
what the reference's ``align_read_or_contig_to_reference(read, contig, read_length, match, mismatch, indel)`` returns
at indices 1 to 5: the two aligned strings, the score, start and end.  The consensus pileup is a
function of exactly these; tests/test_consensus_cpu.py piles the strings up itself and compares.  The aligner is
executed as oracle/gen_golden.py executes it: numba.njit replaced by the identity (import_reference).  The scoring is
the reference's default (10, -1, -1) on short reads, far from int32 wrapping.  The placement is the first best
contig by the reference's scores (plots.py:126-131), then overridden for the reads that are there to exercise one
case each.  The file also stores the noisy reads of the planted-error test (``mutate`` draws, four seeds).  Only
inputs and recorded results are written.
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
    rng = random.Random(20261021)
    st = rng.randint(0, len(genome_all) - 600)
    g = genome_all[st:st + 600]
    m, x, d = SCORING

    a, b = rand_seq(rng, 20, "ACG"), rand_seq(rng, 20, "ACG")      # the gap case: A + B against A + 60 T + B
    a2, b2 = rand_seq(rng, 20, "ACG"), rand_seq(rng, 20, "ACG")    # the ins case: A + 30 T + B against A + B
    with_n = list(g[400:500])
    with_n[50] = "N"
    tie = list(rand_seq(rng, 40, "ACGT"))
    tie[10], tie[20] = "A", "G"
    tie = "".join(tie)
    contigs = [g[0:150], g[120:300], g[120:300], "", a + "T" * 60 + b, a2 + b2, g[300:325], "".join(with_n), tie]
    GAP, INS, SHORT, WITH_N, TIE, EMPTY = 4, 5, 6, 7, 8, 3

    reads, forced, note = [], {}, {}

    def add(read, place=None, what=None):
        reads.append(read)
        if place is not None:
            forced[len(reads) - 1] = place
        if what:
            note[what] = len(reads) - 1

    for _ in range(60):   # full-length reads with a few substitutions
        p = rng.randint(0, 300 - READ_LENGTH)
        add(mutate(rng, g[p:p + READ_LENGTH], 0.02))
    for _ in range(16):   # reads over the contig that holds an N
        p = rng.randint(400, 500 - READ_LENGTH)
        add(mutate(rng, g[p:p + READ_LENGTH], 0.02))
    for n in (8, 17, 25, 33, 39):   # shorter than read_length: aligned to the contig's tail only
        add(mutate(rng, g[150 - n:150], 0.03), 0)
        add(g[300 - n:300], 1)
    add(g[120:135] + g[140:150], 0, "tail_gap")       # a tail window whose alignment needs a gap or stops short
    add("CC" + g[302:325] + "ACGTA", SHORT, "negative_shift")   # 30 bases on a contig of 25: shift 25 - 30
    add("", 0, "empty_read")
    add(g[10:50], EMPTY, "empty_contig")
    add(g[20:60], -1, "unplaced")
    add(g[0:40], 1, "not_its_best")                   # from contig 0, placed on contig 1
    add("T" * READ_LENGTH, INS, "score_zero")         # contig 5 holds no T
    add(a + b, GAP, "gap_read")
    add(a2 + "T" * 30 + b2, INS, "ins_read")
    rn = list(g[430:470])
    rn[7] = "N"
    add("".join(rn), WITH_N, "n_in_read")
    for c10, c20 in (("A", "A"), ("A", "C"), ("C", "A"), ("C", "C")):   # two columns whose leading channels tie
        t = list(tie)
        t[10], t[20] = c10, c20
        add("".join(t), TIE)
    add(g[130:170], 2, "repeat_second_copy")          # the second copy of the repeated contig gets a vote too

    t0 = time.time()
    place = []
    for r, read in enumerate(reads):
        if r in forced:
            place.append(forced[r])
            continue
        best, first = None, -1
        for c, contig in enumerate(contigs):
            score = int(aligners.align_read_or_contig_to_reference(read, contig, READ_LENGTH, m, x, d)[3])
            if best is None or score > best:
                best, first = score, c
        place.append(first)
    records = []
    for r, read in enumerate(reads):
        if place[r] < 0:
            records.append(None)
            continue
        t = aligners.align_read_or_contig_to_reference(read, contigs[place[r]], READ_LENGTH, m, x, d)
        assert len(t) == 6
        records.append([str(t[1]), str(t[2]), int(t[3]), int(t[4]), int(t[5])])
    print(f"{len(reads)} reads placed and aligned in {time.time() - t0:.1f}s")

    rec = records[note["gap_read"]]
    assert rec[2] == 340 and rec[1].count("-") == 60 and rec[0].count("-") == 0, rec
    rec = records[note["ins_read"]]
    assert rec[2] == 370 and rec[0].count("-") == 30 and rec[1].count("-") == 0, rec
    assert records[note["score_zero"]][2] == 0 and records[note["empty_read"]][2] == 0
    assert records[note["empty_contig"]][2] == 0 and records[note["unplaced"]] is None
    rec = records[note["negative_shift"]]
    assert rec[2] > 0 and rec[3] < 0 <= rec[4], rec          # the reference's start is shifted below 0
    assert "N" in records[note["n_in_read"]][1] and len(set(place)) >= 8

    # the planted-error test's noisy reads: mutate() over one Random(seed) per seed (tests/test_consensus_cpu.py)
    rng950 = random.Random(950)
    g950 = "".join(rng950.choice("ACGT") for _ in range(600))
    noisy = {}
    for seed in (1, 2, 3, 4):
        nrng = random.Random(seed)
        noisy[str(seed)] = [mutate(nrng, g950[p:p + 40], 0.03) for p in range(0, 561, 2)]

    meta = {"generator": "tools/gen_golden_consensus.py",
            "reference": "roiteichman/Genome-Assembly-Using-Overlap-Graphs",
            "numba": "absent: njit replaced by identity; default scoring (10, -1, -1), far from int32 wrapping",
            "records": "records[r] = align_read_or_contig_to_reference(reads[r], contigs[place[r]], read_length, "
                       "match, mismatch, indel)[1:6] = [aligned_ref, aligned_query, score, start, end]; null when "
                       "place[r] is -1",
            "noisy": "noisy[seed] = [mutate(rng, g[p:p+40], 0.03) for p in range(0, 561, 2)], rng = Random(seed), "
                     "g = 600 draws of Random(950).choice('ACGT')",
            "cases": note}
    with open(os.path.join(GOLDEN, "consensus.json"), "w") as fh:
        json.dump({"meta": meta, "read_length": READ_LENGTH, "match": m, "mismatch": x, "indel": d,
                   "reads": reads, "contigs": contigs, "place": place, "records": records, "noisy": noisy},
                  fh, separators=(",", ":"))


if __name__ == "__main__":
    main()
