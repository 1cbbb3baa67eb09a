"""Best-successor layout: contigs straight from the score columns, without a graph object.

  Inputs: n reads with lengths len[r]; E pairs (a[p], b[p], score[p], end[p]) in list order; min_score and
  min_overlap.
  1. Eligible.  Pair p is eligible iff a[p] != b[p], score[p] >= min_score and min_overlap <= end[p] < len[b[p]].
     A link that adds no base is no link.
  2. Link.  link[a] is the eligible pair of a with the greatest score; ties go to the smallest p.
     succ[a] = b[link[a]].  A read without an eligible pair has link = succ = -1.
  3. Cycles.  succ is a functional graph.  Every cycle is cut at its pair with the least score; ties go to the
     greatest p.  The source of that pair gets link = succ = -1.  What remains is a forest of in-trees, each with
     one root (succ = -1).
  4. Span.  tail[root] = 0; otherwise tail[a] = tail[succ[a]] + len[succ[a]] - end[link[a]].
     span[a] = len[a] + tail[a] is the length of the contig spelled from a.
  5. Contigs.  One contig per root, in ascending root index.  Its head is the read of the tree with the greatest
     span; ties go to the smallest read index.  The contig is the head followed, along succ, by
     read[succ][end[link]:] (the reference's own concatenation, create_contig).  Its length is span[head].
  6. Placement.  Every read r gets contig[r], its tree's contig; offset[r] = span[head] - span[r], which for a read
     on the head's path is where its first base lies; and on_path[r].
  Everything is integer and independent of pair order, except the tie rules, which name p.

``layout_loop`` is that statement as literal loops; ``ovl_layout_host`` (one host thread) and ``ovl_layout`` /
``ovl_layout_candidates`` (the GPU) are pinned to it element for element.  ``layout`` picks between the host and the
device form; ``assemble_contigs_best_successor`` is the pipeline from reads to contigs, which on its resident route
(reads, candidate list, scores and layout all on the device) brings only the layout's outputs back.

The rule works on distinct reads: a read's copies do not multiply contigs.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from ._lib import OvlError

# layout(device=None) takes the GPU from this many pairs: the crossover_pairs of tools/layout_probe.py
# (profiles/layout.json; PhiX, k = 12 seed candidates, median (max - min) after a warm-up, host form on an EPYC 9575F;
# ovl_layout's time includes the upload of its 16 bytes per pair).  The sweep over the first r reads of the N = 10,000
# workload, five repetitions: 3,371 pairs 0.047 (0.006) ms on the host against 0.401 (0.027) ms; 53,457 pairs 0.192
# (0.036) against 0.516 (0.018); 211,222 pairs 0.533 (0.036) against 0.686 (0.034), the host still ahead; 833,018 pairs
# 1.786 (0.190) against 1.300 (0.038); 873,830 pairs 1.737 (0.044) against 1.239 (0.079); 915,310 pairs 1.728 (0.091)
# against 1.330 (0.038); 958,266 pairs 1.770 (0.037) against 1.275 (0.044).  The two whole workloads, ten repetitions:
# 992,836 pairs 1.714 (0.096) against 1.236 (0.042) ms; 15,630,431 pairs 24.00 (2.54) against 11.30 (1.32) ms.  From
# 833,018 pairs on, every point has the device form ahead by more than the two spreads together; no point between
# 211,222 and 833,018 pairs was measured, so the crossover lies somewhere in that gap and the constant is its upper end.
# The device form costs about 0.35 ms whatever it holds; the host form takes 1.5 to 2.5 ns per pair.  The resident
# route of assemble_contigs_best_successor does not go through the constant: its columns are on the device already.
LAYOUT_DEVICE_MIN_PAIRS = 833_018

_ARRAYS = ("succ", "link", "contig", "offset", "on_path")


def layout_loop(reads: Sequence[str], a, b, score, end, min_score: int = 1, min_overlap: int = 1) -> Dict[str, object]:
    """The rule of this module's docstring as literal loops (slow; what the native forms are checked against).
    Returns ``succ``, ``link``, ``contig``, ``offset`` (int32), ``on_path`` (uint8), ``contigs`` (list of str) and
    the counts ``links``, ``cycles``, ``on_path_reads``."""
    n = len(reads)
    length = [len(r) for r in reads]
    a, b, score, end = ([int(v) for v in x] for x in (a, b, score, end))
    # 1, 2
    link = [-1] * n
    for p in range(len(a)):
        if a[p] == b[p] or score[p] < min_score or not (min_overlap <= end[p] < length[b[p]]):
            continue
        if link[a[p]] < 0 or score[p] > score[link[a[p]]]:  # ties: the smallest p, which came first
            link[a[p]] = p
    succ = [b[link[r]] if link[r] >= 0 else -1 for r in range(n)]
    # 3
    cycles = 0
    for r in range(n):
        seen, x = {}, r  # (a dict keeps the walk's order)
        while x >= 0 and x not in seen:
            seen[x] = True
            x = succ[x]
        if x != r:  # r's walk ends at a root, or closes a cycle that r is not on
            continue
        cut = r
        for y in seen:  # the whole cycle: least score, then greatest p
            if (score[link[y]], -link[y]) < (score[link[cut]], -link[cut]):
                cut = y
        link[cut] = succ[cut] = -1
        cycles += 1
    # 4
    tail, root = [0] * n, list(range(n))
    for r in range(n):
        x = r
        while succ[x] >= 0:
            tail[r] += length[succ[x]] - end[link[x]]
            x = succ[x]
        root[r] = x
    span = [length[r] + tail[r] for r in range(n)]
    # 5
    roots = [r for r in range(n) if succ[r] < 0]
    head = {}
    for rt in roots:
        tree = [r for r in range(n) if root[r] == rt]
        head[rt] = min(tree, key=lambda r: (-span[r], r))
    contigs: List[str] = []
    on_path = [0] * n
    for rt in roots:
        x = head[rt]
        text = reads[x]
        on_path[x] = 1
        while succ[x] >= 0:
            text += reads[succ[x]][end[link[x]]:]
            x = succ[x]
            on_path[x] = 1
        assert len(text) == span[head[rt]]
        contigs.append(text)
    # 6
    rank = {rt: k for k, rt in enumerate(roots)}
    contig = [rank[root[r]] for r in range(n)]
    offset = [span[head[root[r]]] - span[r] for r in range(n)]
    return {"succ": np.asarray(succ, np.int32).reshape(n), "link": np.asarray(link, np.int32).reshape(n),
            "contig": np.asarray(contig, np.int32).reshape(n), "offset": np.asarray(offset, np.int32).reshape(n),
            "on_path": np.asarray(on_path, np.uint8).reshape(n), "contigs": contigs, "n_contigs": len(contigs),
            "links": sum(s >= 0 for s in succ), "cycles": cycles, "on_path_reads": sum(on_path)}


def _check_text(reads) -> None:
    try:
        "".join(reads).encode("latin-1")
    except UnicodeEncodeError:
        raise OvlError(-4, "layout spells contigs from the reads' bytes: characters above 255 are not supported")


def _with_contigs(res: Dict[str, object]) -> Dict[str, object]:
    """``contigs`` (list of str) from the native forms' ``bases`` and ``c_off``."""
    text = res["bases"].tobytes().decode("latin-1")
    off = res["c_off"].tolist()
    res["contigs"] = [text[off[k]:off[k + 1]] for k in range(res["n_contigs"])]
    return res


def layout(reads: Sequence[str], a, b, score, end, min_score: int = 1, min_overlap: int = 1, engine=None,
           device: Optional[bool] = None) -> Dict[str, object]:
    """The layout of the scored pairs (a, b, score, end) over ``reads`` (distinct reads): a dict of ``succ``,
    ``link``, ``contig``, ``offset`` (int32 per read), ``on_path`` (uint8 per read), ``contigs`` (list of str),
    ``bases`` / ``c_off`` / ``n_contigs`` (the same contigs as bytes) and the counts ``links``, ``cycles``,
    ``levels``, ``on_path_reads``.

    ``device=None`` takes the host form (ovl_layout_host) when no GPU is visible or the list holds fewer than
    ``LAYOUT_DEVICE_MIN_PAIRS`` pairs, else the device form (ovl_layout); True / False force the choice."""
    from .engine import default_engine, layout_host, use_device
    reads = list(reads)
    _check_text(reads)
    if use_device(device, lambda: len(a), LAYOUT_DEVICE_MIN_PAIRS, engine):
        return _with_contigs((engine or default_engine()).layout(reads, a, b, score, end, min_score, min_overlap))
    return _with_contigs(layout_host(reads, a, b, score, end, min_score, min_overlap))


def assemble_contigs_best_successor(reads: Sequence[str], k: int = 12, seeds: str = "any", min_score: int = 1,
                                    min_overlap: int = 1, min_contig_length: int = 0, engine=None, scorer=None,
                                    candidates: str = "auto", timing: Optional[dict] = None,
                                    layout_out: Optional[dict] = None, polish: int = 0, slack: int = 8,
                                    min_depth: int = 3) -> List[str]:
    """Contigs of ``reads`` by the best-successor layout of their candidate pairs (``seeds``: the candidate rule,
    ``overlapGraphs.SEED_MODES``), scored as the reference scores (match 10, mismatch -1, no gaps).

    The resident route: the distinct reads are uploaded, the candidate list is enumerated on the GPU, and
    ``ovl_layout_candidates`` scores it into device columns and lays it out there; neither the list nor the scores
    come back.  With a ``scorer``, with ``candidates="host"``, or under "auto" when the k-mer keys do not fit the
    device's (OVL_E_UNSUPPORTED): the host list, its scores (through ``scorer`` or the engine), then ``layout``.
    ``min_contig_length`` drops shorter contigs (the contigs that grow from a truncated read at the genome's end are
    about one read long).  ``layout_out`` receives the placement arrays, the counts and, under ``"reads"``, the
    distinct reads they index; ``timing`` the stage times in seconds.

    ``polish=R > 0`` polishes the contigs for up to R rounds of ``consensus.pileup_placed`` at the layout's own
    placement (band half-width ``slack``, a base called from ``min_depth`` votes), every distinct read voting with its
    copy count, before ``min_contig_length`` filters.  ``layout_out`` then also receives ``"copies"``, ``"polished"``
    (the contigs returned, unfiltered; ``"contigs"`` stays the layout's) and ``"pileup"``, and ``timing`` a
    ``"polish"`` stage.  With ``polish=0`` nothing of this happens."""
    from . import overlapGraphs as og
    from .candidates import dedup_reads
    from .engine import INDEL_DEFAULT, default_engine, encode_reads
    if candidates not in og.CANDIDATE_MODES:
        raise ValueError(f"candidates must be one of {og.CANDIDATE_MODES}")
    og._check_seeds(seeds, k)
    st = og._Stages(timing)
    if polish < 0:
        raise ValueError("polish must be >= 0")
    distinct, copies = dedup_reads(reads)
    _check_text(distinct)
    st("dedup")
    res = None
    if scorer is None and candidates != "host":
        eng = engine or default_engine()
        enc = encode_reads(distinct)
        st("encode")
        eng.set_reads(distinct, enc)
        st("set_reads")
        try:
            if seeds == "any":
                eng.enumerate_seed_candidates(k)
            else:
                eng.enumerate_candidates(k)
        except OvlError as e:
            if e.code != -4 or candidates == "device":
                raise
        else:
            st("enumerate")
            res = _with_contigs(eng.layout_candidates(10, -1, INDEL_DEFAULT, -1, min_score, min_overlap))
            st("layout")
    if res is None:
        a, b, sc, en = og.candidates_and_scores(distinct, k, engine, scorer, "host", None, seeds)
        st("candidates_and_scores")
        res = layout(distinct, a, b, sc, en, min_score, min_overlap, engine)
        st("layout")
    if layout_out is not None:
        layout_out.update({key: res[key] for key in _ARRAYS + ("links", "cycles", "levels", "on_path_reads")})
        layout_out["contigs"] = list(res["contigs"])
        layout_out["reads"] = distinct
    contigs = res["contigs"]
    if polish > 0:
        from .consensus import pileup_placed
        pile = pileup_placed(contigs, distinct, res["contig"], res["offset"], slack, copies, polish, min_depth,
                             engine=engine)
        contigs = list(pile.called)
        st("polish")
        if layout_out is not None:
            layout_out.update({"copies": copies, "polished": contigs, "pileup": pile})
    return [c for c in contigs if len(c) >= min_contig_length]
