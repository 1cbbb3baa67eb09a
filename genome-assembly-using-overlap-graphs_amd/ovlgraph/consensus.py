"""Consensus polishing: the third letter of overlap-layout-consensus.

A contig is a concatenation of read suffixes, so every substitution error of a read on the walk is copied into it,
while ten to thirty reads cover each of its bases.  ``pileup`` places every read on a contig (its first best one,
as ``read_depth`` finds it), aligns it there as ``align_read_or_contig_to_reference`` does and lets its walk vote per
contig base; ``polish_contigs`` replaces every base that enough reads outvote.  Only substitutions are applied: gap
and insertion votes are recorded and never change a base, so polished contigs keep their lengths.

The alignments, the pileup and the vote run in native code: ``ovl_consensus`` on the GPU (the batch alignment
kernel's walks stay in device memory, a pileup kernel and a vote kernel consume them there) or
``ovl_consensus_host`` on one host thread.
"""
from __future__ import annotations

import numpy as np

from ._lib import OvlError

# pileup(device=None) takes the GPU from this many DP cells, counted over the placed reads as read length x window
# length.  From tools/consensus_probe.py's sweep over the first r reads of the PhiX workload on all its contigs
# (profiles/consensus.json, five repetitions after a warm-up, median (max - min), host form on an EPYC 9575F):
# 46,100 cells (4 reads) 0.616 (0.021) ms on the host against the device call's 0.690 (0.012) ms; 122,200 cells
# (8 reads) 0.862 (0.036) against 0.728 (0.014) ms; 212,800 cells 1.16 against 0.73 ms; 1.39 * 10^7 cells (1,024
# reads) 44.0 against 0.89 ms; the whole workload, 1.30 * 10^8 cells, 402 against 2.7 ms.  The device call costs
# about 0.7 ms whatever it holds (the contigs' upload and 7.6 MB of counts back), the host form fills 3.2 * 10^8
# cells a second, so the crossover moves with the box's CPU.  The constant is the first point from which the device
# call won clear of the two spreads together.
CONSENSUS_DEVICE_MIN_CELLS = 122_200


class Pileup:
    """What ``pileup`` returns: ``counts`` (one (len(contig), 6) int32 view per contig position: A, C, G, T, gap,
    ins), ``called`` (one string per contig position), ``n_changed``, ``n_other`` (read bytes outside ACGT that met
    a contig base), ``place`` (int32 per read: the contig position it voted on, -1 for none), ``aln`` (reads x 3
    int32: score, first column and one past the last column of the alignment, in the contig's own coordinates) and
    ``rounds`` (set by ``polish_contigs``: the rounds it ran)."""

    def __init__(self, counts, called, n_changed, n_other, place, aln):
        self.counts = counts
        self.called = called
        self.n_changed = n_changed
        self.n_other = n_other
        self.place = place
        self.aln = aln
        self.rounds = 1


def _window_len(L: int, m: int, read_length: int) -> int:
    """The contig columns a read of length L is aligned to (aligners.py:187-195)."""
    return m if L >= read_length or L == 0 or L >= m else L


def _place(contigs, reads, read_length, scoring, engine, device):
    """first_best of read_best / read_best_host, chosen as ``read_depth`` chooses."""
    from .engine import default_engine, device_count, read_best_host
    from .performanceMeasures import READ_DEPTH_DEVICE_MIN_CELLS
    if device is None:
        cells = sum(len(r) for r in reads) * sum(len(c) for c in contigs)
        device = cells >= READ_DEPTH_DEVICE_MIN_CELLS and (engine is not None or device_count() > 0)
    if device:
        res = (engine or default_engine()).read_best(reads, contigs, read_length, *scoring)
    else:
        res = read_best_host(reads, contigs, read_length, *scoring)
    return res["first_best"]


def pileup(contigs, reads, read_length, place=None, depth=None, min_depth=3, match_score=10, mismatch=-1, indel=-1,
           engine=None, device=None):
    """Pile the reads up on the contigs and call every base (ovl_consensus / ovl_consensus_host).

    ``place`` gives each read's contig position (-1: the read does not vote).  Without it the placement is
    ``depth.chosen`` when a ``ReadDepth`` is given, else ``first_best`` of ``read_best`` (on the device or the host by
    ``read_depth``'s rule).  ``device=None`` takes the host form when no GPU is visible or the placed reads hold
    fewer than ``CONSENSUS_DEVICE_MIN_CELLS`` cells; True / False force the choice."""
    from .engine import consensus_host, default_engine, device_count
    contigs, reads = list(contigs), list(reads)
    scoring = (match_score, mismatch, indel)
    if place is None:
        place = depth.chosen if depth is not None else _place(contigs, reads, read_length, scoring, engine, device)
    place = np.ascontiguousarray(place, dtype=np.int32)
    if place.shape != (len(reads),):
        raise OvlError(-1, "place must hold one contig position (or -1) per read")
    if device is None:
        C = len(contigs)
        cells = sum(len(r) * _window_len(len(r), len(contigs[p]), read_length)
                    for r, p in zip(reads, place.tolist()) if 0 <= p < C)
        device = cells >= CONSENSUS_DEVICE_MIN_CELLS and (engine is not None or device_count() > 0)
    if device:
        res = (engine or default_engine()).consensus(reads, contigs, place, read_length, *scoring, min_depth)
    else:
        res = consensus_host(reads, contigs, place, read_length, *scoring, min_depth)
    off = np.zeros(len(contigs) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in contigs], out=off[1:])
    text = res["called"].tobytes().decode("latin-1")
    return Pileup([res["counts"][off[k]:off[k + 1]] for k in range(len(contigs))],
                  [text[off[k]:off[k + 1]] for k in range(len(contigs))],
                  res["n_changed"], res["n_other"], place, res["aln"])


def polish_contigs(contigs, reads, read_length, rounds=1, min_depth=3, match_score=10, mismatch=-1, indel=-1,
                   engine=None, device=None):
    """Polish the contigs by up to ``rounds`` rounds of ``pileup``: every round places the reads again on the
    contigs as they stand and replaces the bases the pileup calls differently; it stops early after a round that
    changed nothing.  Returns ``(polished, pileup)``: the contigs in their order and with their lengths (a repeated
    contig is polished per position) and the last round's ``Pileup``."""
    if rounds < 1:
        raise OvlError(-1, "polish_contigs needs rounds >= 1")
    polished = list(contigs)
    for done in range(1, int(rounds) + 1):
        pile = pileup(polished, reads, read_length, None, None, min_depth, match_score, mismatch, indel, engine,
                      device)
        pile.rounds = done
        polished = list(pile.called)
        if pile.n_changed == 0:
            break
    return polished, pile
