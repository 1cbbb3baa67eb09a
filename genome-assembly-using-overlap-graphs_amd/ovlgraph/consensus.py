"""Consensus polishing: the third letter of overlap-layout-consensus.

A contig is a concatenation of read suffixes, so every substitution error of a read on the walk is copied into it,
while ten to thirty reads cover each of its bases.  ``pileup`` places every read on a contig (its first best one,
as ``read_depth`` finds it), aligns it there as ``align_read_or_contig_to_reference`` does and lets its walk vote per
contig base; ``polish_contigs`` replaces every base that enough reads outvote.  Only substitutions are applied: gap
and insertion votes are recorded and never change a base, so polished contigs keep their lengths.

The alignments, the pileup and the vote run in native code: ``ovl_consensus`` on the GPU (the batch alignment
kernel's walks stay in device memory, a pileup kernel and a vote kernel consume them there) or
``ovl_consensus_host`` on one host thread.

``pileup_placed`` is the second entry: it takes the placement a layout already made (``contig[r]`` and ``offset[r]`` of
``ovl_layout``) instead of finding one, aligns every read only inside a band around the diagonal that placement names,
lets a distinct read vote with its copy count, and runs its rounds without leaving the device
(``ovl_consensus_placed`` / ``ovl_consensus_placed_host``).  The rule:

  A read r of length L > 0 with weight > 0, placed on contig c of length m, votes only if it passes every step.
  1. Window.  lo = max(0, offset - slack), hi = min(m, offset + L + slack).  If hi <= lo the read casts no vote.
     Otherwise t = contig[lo:hi), w = hi - lo, d = offset - lo.
  2. Band.  DP cell (i, j), 1 <= i <= L, 1 <= j <= w, is in the band iff |(j - i) - d| <= slack.  Row 0, column 0 and
     every cell outside the band hold value 0 and code 0.
  3. Fill.  dg, u, l from the three neighbours' values (an out-of-band neighbour counts as 0).  If dg >= u and dg >= l
     and dg >= 0: diag (code 1); else if u >= l and u >= 0: up (2); else if l >= 0: left (3); else the value is 0.  The
     code is stored only when the value is > 0.
  4. Best cell.  The first strict maximum over the in-band cells in row-major order; a best score below
     min_vote_score casts no vote and leaves ``aln`` at zeros.
  5. Walk.  From the best cell along the codes; it stops at code 0.
  6. Votes.  As in ``pileup``, on the contig's own columns; every +1 becomes +weight[r], ``n_other`` included.
     ``aln[r]`` is (score, lo + stop column, lo + best column).
  7. Call.  As in ``pileup``.
  8. Rounds.  Round k + 1 runs on the contigs as round k called them; the loop stops after a round that changed
     nothing, or after ``rounds`` rounds.

``pileup_placed_loop`` is that statement as literal loops; the native forms are pinned to it element for element.
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

# pileup_placed(device=None): the band kernel holds at most 31 diagonals in registers (ovl_consensus_placed) ...
CONSENSUS_PLACED_MAX_DEVICE_SLACK = 15
# ... and takes the GPU from this many band cells, counted as read length x (2 * slack + 1) over the reads: the
# crossover_cells of tools/consensus_placed_probe.py (profiles/consensus_placed.json; the first r distinct reads of the
# PhiX N = 10,000 workload, slack 8, five repetitions after a warm-up, median (max - min), host form on an EPYC 9575F).
# 1,700 cells (1 read) 0.047 (0.007) ms on the host against the device call's 0.402 (0.037) ms; 54,400 cells (32 reads)
# 0.184 (0.027) against 0.428 (0.048); 107,372 cells (64 reads) 0.387 (0.019) against 0.425 (0.010), the host still
# ahead; 214,795 cells (128 reads) 0.816 (0.013) against 0.433 (0.007); 1,722,287 cells 6.32 against 0.53; the whole
# workload, 15,115,380 cells, 55.5 against 1.11 ms.  From 214,795 cells on every point has the device call ahead by
# more than the two spreads together.  The device call costs about 0.4 ms whatever it holds; the host form fills
# 2.7 * 10^8 band cells a second.
CONSENSUS_PLACED_DEVICE_MIN_CELLS = 214_795


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
    from .engine import default_engine, read_best_host, use_device
    from .performanceMeasures import READ_DEPTH_DEVICE_MIN_CELLS
    if use_device(device, lambda: sum(len(r) for r in reads) * sum(len(c) for c in contigs),
                  READ_DEPTH_DEVICE_MIN_CELLS, engine):
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
    from .engine import consensus_host, default_engine, use_device
    contigs, reads = list(contigs), list(reads)
    scoring = (match_score, mismatch, indel)
    if place is None:
        place = depth.chosen if depth is not None else _place(contigs, reads, read_length, scoring, engine, device)
    place = np.ascontiguousarray(place, dtype=np.int32)
    if place.shape != (len(reads),):
        raise OvlError(-1, "place must hold one contig position (or -1) per read")

    def cells():
        return sum(len(r) * _window_len(len(r), len(contigs[p]), read_length)
                   for r, p in zip(reads, place.tolist()) if 0 <= p < len(contigs))
    if use_device(device, cells, CONSENSUS_DEVICE_MIN_CELLS, engine):
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


class _Placed(Pileup):
    """``Pileup`` of ``pileup_placed``: ``place`` is the layout's ``contig``; also ``offset`` (int32 per read),
    ``total_changed`` (bases that differ from the input contigs after the last round) and ``rounds`` (rounds run)."""


def _placed_pileup(res, contigs, contig, offset) -> Pileup:
    off = np.zeros(len(contigs) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in contigs], out=off[1:])
    text = res["called"].tobytes().decode("latin-1")
    pile = _Placed([res["counts"][off[k]:off[k + 1]] for k in range(len(contigs))],
                   [text[off[k]:off[k + 1]] for k in range(len(contigs))],
                   res["n_changed"], res["n_other"], contig, res["aln"])
    pile.offset = offset
    pile.total_changed = res["total_changed"]
    pile.rounds = res["rounds"]
    return pile


def pileup_placed(contigs, reads, contig, offset, slack=8, weights=None, rounds=1, min_depth=3, min_vote_score=1,
                  match_score=10, mismatch=-1, indel=-1, engine=None, device=None):
    """Pile the reads up on the contigs where a layout placed them and call every base, for up to ``rounds`` rounds
    (ovl_consensus_placed / ovl_consensus_placed_host; the rule: this module's docstring).

    ``contig`` and ``offset`` are the layout's placement (``contig[r]`` = -1: the read does not vote), ``weights`` the
    votes of each read (None: one each; the copy counts of ``dedup_reads`` for distinct reads).  Returns a ``Pileup``
    with ``place = contig``, plus ``offset``, ``total_changed`` and ``rounds``; ``called`` is the polished contigs.
    ``device=None`` takes the host form when no GPU is visible, when ``slack > 15`` or when the band cells, the sum of
    read length x (2 * slack + 1), are fewer than ``CONSENSUS_PLACED_DEVICE_MIN_CELLS``; True / False force the
    choice."""
    from .engine import consensus_placed_host, default_engine, use_device
    contigs, reads = list(contigs), list(reads)
    contig = np.ascontiguousarray(contig, dtype=np.int32)
    offset = np.ascontiguousarray(offset, dtype=np.int32)
    if contig.shape != (len(reads),) or offset.shape != (len(reads),):
        raise OvlError(-1, "contig and offset must hold one int32 per read")
    if device is None:
        device = slack <= CONSENSUS_PLACED_MAX_DEVICE_SLACK and use_device(
            None, lambda: sum(len(r) for r in reads) * (2 * slack + 1), CONSENSUS_PLACED_DEVICE_MIN_CELLS, engine)
    args = (reads, contigs, contig, offset, slack, weights, rounds, min_depth, min_vote_score, match_score, mismatch,
            indel)
    res = (engine or default_engine()).consensus_placed(*args) if device else consensus_placed_host(*args)
    return _placed_pileup(res, contigs, contig, offset)


def pileup_placed_loop(contigs, reads, contig, offset, slack=8, weights=None, rounds=1, min_depth=3, min_vote_score=1,
                       match_score=10, mismatch=-1, indel=-1):
    """The rule of this module's docstring as literal loops over dicts of cells (slow; what the native forms are
    checked against).  Returns what ``engine.consensus_placed_host`` returns: ``counts`` (bases x 6 int32), ``called``
    (uint8 over the concatenated contigs), ``n_changed``, ``n_other``, ``aln`` (reads x 3 int32), ``total_changed``
    and ``rounds``."""
    chan = {"A": 0, "C": 1, "G": 2, "T": 3}
    first = [list(c) for c in contigs]
    cur = [list(c) for c in contigs]
    start = [0]
    for c in contigs:
        start.append(start[-1] + len(c))
    done = 0
    while True:
        counts = [[0] * 6 for _ in range(start[-1])]
        aln = [[0, 0, 0] for _ in reads]
        n_other = 0
        for r, q in enumerate(reads):
            c, L = int(contig[r]), len(q)
            wt = 1 if weights is None else int(weights[r])
            if c < 0 or L == 0 or wt == 0:
                continue
            m, o = len(cur[c]), int(offset[r])
            # 1
            lo, hi = max(0, o - slack), min(m, o + L + slack)
            if hi <= lo:
                continue
            t, w, d = cur[c][lo:hi], hi - lo, o - lo
            # 2, 3, 4: a cell that is not in the dicts holds value 0 and code 0
            val, code = {}, {}
            best, bi, bj = 0, 0, 0
            for i in range(1, L + 1):
                for j in range(max(1, i + d - slack), min(w, i + d + slack) + 1):
                    dg = val.get((i - 1, j - 1), 0) + (match_score if q[i - 1] == t[j - 1] else mismatch)
                    u = val.get((i - 1, j), 0) + indel
                    l = val.get((i, j - 1), 0) + indel
                    v, op = 0, 0
                    if dg >= u and dg >= l and dg >= 0:
                        v, op = dg, 1
                    elif u >= l and u >= 0:
                        v, op = u, 2
                    elif l >= 0:
                        v, op = l, 3
                    if v > 0:
                        val[(i, j)], code[(i, j)] = v, op
                    if v > best:
                        best, bi, bj = v, i, j
            if best < min_vote_score:
                continue
            # 5, 6
            i, j = bi, bj
            while i > 0 and j > 0 and code.get((i, j), 0):
                op = code[(i, j)]
                col = counts[start[c] + lo + j - 1]
                if op == 1:
                    if q[i - 1] in chan:
                        col[chan[q[i - 1]]] += wt
                    else:
                        n_other += wt
                    i, j = i - 1, j - 1
                elif op == 2:
                    col[5] += wt
                    i -= 1
                else:
                    col[4] += wt
                    j -= 1
            aln[r] = [best, lo + j, lo + bj]
        # 7
        called, n_changed = [], 0
        for c, text in enumerate(cur):
            out = []
            for b, own in enumerate(text):
                v = counts[start[c] + b][:4]
                call = own
                if sum(v) >= min_depth:
                    top = max(v)
                    if not (own in chan and v[chan[own]] == top):
                        call = "ACGT"[v.index(top)]
                out.append(call)
                n_changed += call != own
            called.append(out)
        # 8
        cur = called
        done += 1
        if n_changed == 0 or done >= rounds:
            break
    flat = "".join("".join(c) for c in cur)
    total_changed = sum(a != b for x, y in zip(cur, first) for a, b in zip(x, y))
    return {"counts": np.asarray(counts, np.int32).reshape(start[-1], 6),
            "called": np.frombuffer(flat.encode("latin-1"), dtype=np.uint8), "n_changed": n_changed,
            "n_other": n_other, "aln": np.asarray(aln, np.int32).reshape(len(reads), 3),
            "total_changed": total_changed, "rounds": done}
