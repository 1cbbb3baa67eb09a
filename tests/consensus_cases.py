"""Shared by tests/test_consensus_cpu.py and tests/test_gpu_consensus.py: the consensus rule of DESIGN.md §4.14
restated over an aligner's two aligned strings, and the planted-error input."""
import random

import numpy as np

CHANNEL = {"A": 0, "C": 1, "G": 2, "T": 3}
GAP, INS = 4, 5


def window(L, m, read_length):
    """(lo, length, shift) of aligners.py:187-195: the contig columns a read of length L is aligned to and what
    the reference adds to window-relative positions."""
    if L >= read_length:
        return 0, m, 0
    wl = L if 0 < L < m else m
    return m - wl, wl, m - L


def restate(contigs, reads, place, read_length, records, min_depth):
    """The rule over ``records[r] = (aligned_ref, aligned_query, score, start, end)`` of read r against contig
    ``place[r]`` (None where place[r] is -1), with the reference's shifted start / end.  Returns the dict that
    ``consensus_host`` returns."""
    off = np.zeros(len(contigs) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in contigs], out=off[1:])
    total = int(off[-1])
    counts = np.zeros((total, 6), dtype=np.int32)
    aln = np.zeros((len(reads), 3), dtype=np.int32)
    n_other = 0
    for r, read in enumerate(reads):
        if place[r] < 0:
            continue
        a_ref, a_query, score, start, end = records[r]
        if score == 0:
            continue
        lo, _, shift = window(len(read), len(contigs[place[r]]), read_length)
        first, last = start - shift + lo, end - shift + lo  # the contig's own columns
        aln[r] = (score, first, last)
        col = first  # the next contig column the alignment consumes
        for t, q in zip(a_ref, a_query):
            if t == "-":      # up: a read base with no contig base votes at the column at its left
                counts[off[place[r]] + col - 1, INS] += 1
            elif q == "-":    # left: a contig base with no read base
                counts[off[place[r]] + col, GAP] += 1
                col += 1
            else:
                if q in CHANNEL:
                    counts[off[place[r]] + col, CHANNEL[q]] += 1
                else:
                    n_other += 1
                col += 1
        assert col == last, (r, col, last)
    text = "".join(contigs)
    called = []
    for b in range(total):
        v = counts[b, :4]
        if int(v.sum()) < min_depth:
            called.append(text[b])
            continue
        tied = [ch for ch in "ACGT" if v[CHANNEL[ch]] == v.max()]
        called.append(text[b] if text[b] in tied else tied[0])
    called = "".join(called)
    return {"counts": counts, "called": np.frombuffer(called.encode("latin-1"), dtype=np.uint8),
            "n_changed": sum(x != y for x, y in zip(called, text)), "n_other": n_other, "aln": aln}


def oracle_records(oracle_mod, contigs, reads, place, read_length, params):
    """``records`` for ``restate`` from the oracle's align_read_or_contig_to_reference."""
    return [None if p < 0 else oracle_mod.align_read_or_contig_to_reference(read, contigs[p], read_length, *params)[1:6]
            for read, p in zip(reads, place)]


def assert_same(got, want, what=""):
    for k in ("counts", "called", "aln"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (what, k, bad[:5].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
    assert got["n_changed"] == want["n_changed"] and got["n_other"] == want["n_other"], what


def planted():
    """The planted-error input: (g, true contigs, contigs with 6 + 3 + 0 substitutions, error-free reads)."""
    rng = random.Random(950)
    g = "".join(rng.choice("ACGT") for _ in range(600))
    step = dict(zip("ACGT", "CGTA"))

    def plant(s, positions):
        s = list(s)
        for p in positions:
            s[p] = step[s[p]]
        return "".join(s)

    truth = [g[0:300], g[300:600], g[100:160]]
    contigs = [plant(truth[0], (30, 77, 140, 141, 200, 260)), plant(truth[1], (20, 180, 280)), truth[2]]
    reads = [g[p:p + 40] for p in range(0, 561, 5)]
    return g, truth, contigs, reads
