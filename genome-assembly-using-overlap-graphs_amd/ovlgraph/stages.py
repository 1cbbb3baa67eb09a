"""The stages of libovl that have a host form beside the device form: one marshalling per stage.

Each ``_X_call(fn, head, ...)`` lays the arguments out as the C ABI takes them, makes the one foreign call and shapes
the result.  ``head`` holds the arguments before the stage's own: ``()`` for the host form (``ovl_X_host``, which
needs neither a context nor a GPU) and ``(ctx,)`` for the device form (``ovl_X``), whose error text is read from that
context.  The ``*_host`` functions here and the ``OverlapEngine`` methods of the same names are one call of it each.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import OvlError, _ptr, check, read_out


def encode_reads(reads: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """Concatenate reads into one byte buffer + int64 offsets.

    Bytes are symbols compared for equality only, so any injective
    character->byte map preserves the reference's ``s[i-1] == t[j-1]`` test
    (aligners.py:35).  Latin-1 covers every str whose characters are < 256;
    otherwise up to 256 distinct characters are renumbered.
    """
    n = len(reads)
    offs = np.zeros(n + 1, dtype=np.int64)
    if n:
        np.cumsum(np.fromiter((len(r) for r in reads), dtype=np.int64, count=n), out=offs[1:])
    joined = "".join(reads)
    try:
        buf = np.frombuffer(joined.encode("latin-1"), dtype=np.uint8)
    except UnicodeEncodeError:
        table: Dict[str, int] = {}
        for ch in joined:
            if ch not in table:
                if len(table) >= 256:
                    raise OvlError(-4, "more than 256 distinct symbols in the read set")
                table[ch] = len(table)
        buf = np.fromiter((table[ch] for ch in joined), dtype=np.uint8, count=len(joined))
    if buf.size == 0:
        buf = np.zeros(1, dtype=np.uint8)
    return np.ascontiguousarray(buf), offs


def _opt(a):
    """``_ptr`` of an optional array: None stays the ABI's null."""
    return None if a is None else _ptr(a)


def _ctx_of(head):
    return head[0] if head else None


# ---------------------------------------------------------------- the two graph reductions
def _csr_arrays(off, heads, weights=None):
    """A CSR graph as the contiguous (int64 off, int32 heads, int64 weights or None) the C ABI takes."""
    off = np.ascontiguousarray(off, dtype=np.int64)
    heads = np.ascontiguousarray(heads, dtype=np.int32)
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.int64)
    if off.ndim != 1 or off.shape[0] < 1 or heads.ndim != 1 or (weights is not None and heads.shape != weights.shape):
        raise OvlError(-1, "CSR graph: off needs n_nodes + 1 entries, heads "
                           f"{'and weights ' if weights is not None else ''}one entry per edge")
    if int(off[-1]) > heads.shape[0]:
        raise OvlError(-1, f"CSR graph: off[-1] = {int(off[-1])} exceeds the {heads.shape[0]} edges given")
    return off, heads, weights


def _transitive_call(fn, head, off, heads, weights) -> np.ndarray:
    """One call of ovl_transitive_reduce / ovl_transitive_reduce_host: the uint8 mask over the CSR edges."""
    off, heads, weights = _csr_arrays(off, heads, weights)
    reduced = np.zeros(max(heads.shape[0], 1), dtype=np.uint8)
    check(fn(*head, _ptr(off), _ptr(heads), _ptr(weights), off.shape[0] - 1, _ptr(reduced),
             ctypes.byref(ctypes.c_int64(0))), _ctx_of(head))
    return reduced[:heads.shape[0]]


def transitive_reduce_host(off, heads, weights) -> np.ndarray:
    """``OverlapEngine.transitive_reduce`` by the library's host loop (ovl_transitive_reduce_host): no context,
    no GPU."""
    return _transitive_call(_lib.load().ovl_transitive_reduce_host, (), off, heads, weights)


def _reach_call(fn, head, off, heads, closure: bool):
    """One call of ovl_reach_reduce / ovl_reach_reduce_host on a weightless CSR graph: the mask, and with
    ``closure`` the n x ceil(n / 64) uint64 matrix."""
    off, heads, _ = _csr_arrays(off, heads)
    n = off.shape[0] - 1
    reduced = np.zeros(max(heads.shape[0], 1), dtype=np.uint8)
    matrix = np.zeros((n, (n + 63) // 64), dtype=np.uint64) if closure else None
    check(fn(*head, _ptr(off), _ptr(heads), n, _ptr(reduced), ctypes.byref(ctypes.c_int64(0)), _opt(matrix)),
          _ctx_of(head))
    mask = reduced[:heads.shape[0]]
    return (mask, matrix) if closure else mask


def reach_reduce_host(off, heads, closure: bool = False):
    """``OverlapEngine.reach_reduce`` on one host thread (ovl_reach_reduce_host): no context, no GPU."""
    return _reach_call(_lib.load().ovl_reach_reduce_host, (), off, heads, closure)


# ---------------------------------------------------------------- read depth
def _read_best_call(fn, head, reads, contigs, read_length, match, mismatch, indel, scores) -> Dict[str, np.ndarray]:
    """One call of ovl_read_best / ovl_read_best_host: reads and contigs under one symbol map, five int32 arrays over
    the reads, the tie bits and (``scores``) the score matrix."""
    reads, contigs = list(reads), list(contigs)
    R, C = len(reads), len(contigs)
    buf, offs = encode_reads(reads + contigs)
    r_off = np.ascontiguousarray(offs[: R + 1])
    c_off = np.ascontiguousarray(offs[R:])
    outs = [np.zeros(max(R, 1), dtype=np.int32) for _ in range(5)]
    bits = np.zeros((max(R, 1), max((C + 31) // 32, 1)), dtype=np.uint32)
    sc = np.zeros((max(R, 1), max(C, 1)), dtype=np.int32) if scores else None
    check(fn(*head, _ptr(buf), _ptr(r_off), R, _ptr(buf), _ptr(c_off), C, int(read_length), int(match),
             int(mismatch), int(indel), *[_ptr(o) for o in outs], _ptr(bits), _opt(sc)), _ctx_of(head))
    res = dict(zip(("best_score", "first_best", "n_best", "start", "end"), (o[:R] for o in outs)))
    res["tie_bits"] = bits[:R, : (C + 31) // 32]
    if sc is not None:
        res["scores"] = sc[:R, :C]
    return res


def read_best_host(reads, contigs, read_length: int, match: int = 10, mismatch: int = -1, indel: int = -1,
                   scores: bool = False) -> Dict[str, np.ndarray]:
    """``OverlapEngine.read_best`` on one host thread (ovl_read_best_host): no context, no GPU."""
    return _read_best_call(_lib.load().ovl_read_best_host, (), reads, contigs, read_length, match, mismatch, indel,
                           scores)


# ---------------------------------------------------------------- consensus, free and placed
def _consensus_arrays(reads, contigs, place, counts: bool):
    """Reads, contigs and the placement as the C ABI of ovl_consensus takes them, with the arrays to receive the
    results: the counts (total bases x 6 int32, when asked for), the called bytes and three int32 per read."""
    reads, contigs = list(reads), list(contigs)
    R, C = len(reads), len(contigs)
    if not all(s.isascii() for s in reads + contigs):
        raise OvlError(-4, "consensus needs ASCII reads and contigs (the called bases are bytes)")
    buf, offs = encode_reads(reads + contigs)
    place = np.ascontiguousarray(place, dtype=np.int32)
    if place.shape != (R,):
        raise OvlError(-1, "place must hold one contig position (or -1) per read")
    total = int(offs[-1] - offs[R])
    cnt = np.zeros((max(total, 1), 6), dtype=np.int32) if counts else None
    called = np.zeros(max(total, 1), dtype=np.uint8)
    aln = np.zeros((max(R, 1), 3), dtype=np.int32)
    return R, C, buf, np.ascontiguousarray(offs[: R + 1]), np.ascontiguousarray(offs[R:]), place, total, cnt, called, aln


def _consensus_result(R, total, cnt, called, aln, n_changed, n_other) -> Dict[str, object]:
    res = {"called": called[:total], "n_changed": int(n_changed.value), "n_other": int(n_other.value),
           "aln": aln[:R]}
    if cnt is not None:
        res["counts"] = cnt[:total]
    return res


def _consensus_call(fn, head, reads, contigs, place, read_length, match, mismatch, indel, min_depth, counts):
    """One call of ovl_consensus / ovl_consensus_host."""
    R, C, buf, r_off, c_off, place, total, cnt, called, aln = _consensus_arrays(reads, contigs, place, counts)
    n_changed, n_other = ctypes.c_int64(0), ctypes.c_int64(0)
    check(fn(*head, _ptr(buf), _ptr(r_off), R, _ptr(buf), _ptr(c_off), C, _ptr(place), int(read_length), int(match),
             int(mismatch), int(indel), int(min_depth), _opt(cnt), _ptr(called), ctypes.byref(n_changed),
             ctypes.byref(n_other), _ptr(aln)), _ctx_of(head))
    return _consensus_result(R, total, cnt, called, aln, n_changed, n_other)


def consensus_host(reads, contigs, place, read_length: int, match: int = 10, mismatch: int = -1, indel: int = -1,
                   min_depth: int = 3, counts: bool = True) -> Dict[str, object]:
    """``OverlapEngine.consensus`` on one host thread (ovl_consensus_host): no context, no GPU."""
    return _consensus_call(_lib.load().ovl_consensus_host, (), reads, contigs, place, read_length, match, mismatch,
                           indel, min_depth, counts)


def _placed_call(fn, head, reads, contigs, contig, offset, slack, weights, rounds, min_depth, min_vote_score, match,
                 mismatch, indel, counts):
    """One call of ovl_consensus_placed / ovl_consensus_placed_host."""
    R, C, buf, r_off, c_off, contig, total, cnt, called, aln = _consensus_arrays(reads, contigs, contig, counts)
    offset = np.ascontiguousarray(offset, dtype=np.int32)
    if offset.shape != (R,):
        raise OvlError(-1, "offset must hold one int32 per read")
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.int32)
        if weights.shape != (R,):
            raise OvlError(-1, "weights must hold one int32 per read")
    n_changed, n_other, total_changed = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    rounds_done = ctypes.c_int32(0)
    check(fn(*head, _ptr(buf), _ptr(r_off), R, _opt(weights), _ptr(buf), _ptr(c_off), C, _ptr(contig), _ptr(offset),
             int(slack), int(match), int(mismatch), int(indel), int(min_vote_score), int(min_depth), int(rounds),
             _opt(cnt), _ptr(called), ctypes.byref(n_changed), ctypes.byref(n_other), ctypes.byref(total_changed),
             ctypes.byref(rounds_done), _ptr(aln)), _ctx_of(head))
    res = _consensus_result(R, total, cnt, called, aln, n_changed, n_other)
    res["total_changed"] = int(total_changed.value)
    res["rounds"] = int(rounds_done.value)
    return res


def consensus_placed_host(reads, contigs, contig, offset, slack: int = 8, weights=None, rounds: int = 1,
                          min_depth: int = 3, min_vote_score: int = 1, match: int = 10, mismatch: int = -1,
                          indel: int = -1, counts: bool = True) -> Dict[str, object]:
    """``OverlapEngine.consensus_placed`` on one host thread (ovl_consensus_placed_host): no context, no GPU, any
    slack."""
    return _placed_call(_lib.load().ovl_consensus_placed_host, (), reads, contigs, contig, offset, slack, weights,
                        rounds, min_depth, min_vote_score, match, mismatch, indel, counts)


# ---------------------------------------------------------------- layout
LAYOUT_COUNTS = ("links", "cycles", "levels", "on_path_reads")  # ovl_last_layout, in the ABI's order


def _layout_outputs(n: int, total: int):
    """The arrays that receive a layout: succ, link, contig, offset (int32 per read), on_path (uint8 per read), the
    contigs' bytes (at most the reads' bytes) and their offsets (n + 1 int64)."""
    outs = [np.zeros(max(n, 1), dtype=np.int32) for _ in range(4)]
    return outs, np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(total, 1), dtype=np.uint8), \
        np.zeros(n + 1, dtype=np.int64)


def _layout_result(n: int, outs, on_path, bases, c_off, n_contigs: int, stats) -> Dict[str, object]:
    res: Dict[str, object] = dict(zip(("succ", "link", "contig", "offset"), (o[:n] for o in outs)))
    res["on_path"] = on_path[:n]
    res["c_off"] = c_off[: n_contigs + 1]
    res["bases"] = bases[: int(c_off[n_contigs])]
    res["n_contigs"] = n_contigs
    res.update(stats)
    return res


def _layout_call(fn, head, last, reads, a, b, score, end, min_score, min_overlap, encoded) -> Dict[str, object]:
    """One call of ovl_layout / ovl_layout_host; ``last()`` reads the counts that go with the result."""
    buf, offs = encoded if encoded is not None else encode_reads(reads)
    n = offs.shape[0] - 1
    cols = [np.ascontiguousarray(x, dtype=np.int32) for x in (a, b, score, end)]
    if any(x.ndim != 1 or x.shape != cols[0].shape for x in cols):
        raise OvlError(-1, "layout: a, b, score and end must be 1-D arrays of equal length")
    outs, on_path, bases, c_off = _layout_outputs(n, int(offs[-1] - offs[0]))
    nc = ctypes.c_int32(0)
    check(fn(*head, _ptr(buf), _ptr(offs), n, *[_ptr(x) for x in cols], cols[0].shape[0], int(min_score),
             int(min_overlap), *[_ptr(o) for o in outs], _ptr(on_path), _ptr(bases), _ptr(c_off), ctypes.byref(nc)),
          _ctx_of(head))
    return _layout_result(n, outs, on_path, bases, c_off, nc.value, last())


def last_layout_host() -> Dict[str, int]:
    """{links, cycles, levels, on_path_reads} of this thread's last ``layout_host`` (ovl_last_layout without a
    context)."""
    return dict(zip(LAYOUT_COUNTS, read_out(_lib.load().ovl_last_layout, None)))


def layout_host(reads, a, b, score, end, min_score: int = 1, min_overlap: int = 1, encoded=None) -> Dict[str, object]:
    """``OverlapEngine.layout`` on one host thread (ovl_layout_host): no context, no GPU."""
    return _layout_call(_lib.load().ovl_layout_host, (), last_layout_host, reads, a, b, score, end, min_score,
                        min_overlap, encoded)


# ---------------------------------------------------------------- read correction
CORRECT_STATS = ("kmers", "distinct", "solid", "untrusted", "changed", "ties", "threshold", "windows")


def _spectrum_call(fn, head, buf, offs, k: int):
    """The two-call protocol of ovl_kmer_spectrum(_host): size the arrays, then fill them."""
    n = offs.shape[0] - 1
    nd = ctypes.c_int64(0)
    rc = fn(*head, _ptr(buf), _ptr(offs), n, int(k), None, None, 0, ctypes.byref(nd))
    if rc not in (0, -5):
        check(rc, _ctx_of(head))
    keys = np.zeros(max(nd.value, 1), dtype=np.uint64)
    counts = np.zeros(max(nd.value, 1), dtype=np.int32)
    if nd.value > 0:
        check(fn(*head, _ptr(buf), _ptr(offs), n, int(k), _ptr(keys), _ptr(counts), nd.value, ctypes.byref(nd)),
              _ctx_of(head))
    return keys[: nd.value], counts[: nd.value]


def _correct_call(fn, head, buf, offs, k: int, min_count: int):
    """ovl_correct_reads(_host): (the corrected bytes, the changed bases per read, the stats as a dict)."""
    n = offs.shape[0] - 1
    out = np.zeros(max(buf.shape[0], 1), dtype=np.uint8)
    changed = np.zeros(max(n, 1), dtype=np.int32)
    stats = np.zeros(8, dtype=np.int64)
    check(fn(*head, _ptr(buf), _ptr(offs), n, int(k), int(min_count), _ptr(out), _ptr(changed), _ptr(stats)),
          _ctx_of(head))
    return out[: int(offs[-1])], changed[:n], dict(zip(CORRECT_STATS, (int(v) for v in stats)))


def kmer_spectrum_host(reads, k: int, encoded=None):
    """``OverlapEngine.kmer_spectrum`` on one host thread (ovl_kmer_spectrum_host): no context, no GPU."""
    buf, offs = encoded if encoded is not None else encode_reads(reads)
    return _spectrum_call(_lib.load().ovl_kmer_spectrum_host, (), buf, offs, k)


def correct_reads_host(reads, k: int, min_count: int = 0, encoded=None):
    """``OverlapEngine.correct_reads`` on one host thread (ovl_correct_reads_host): no context, no GPU."""
    buf, offs = encoded if encoded is not None else encode_reads(reads)
    return _correct_call(_lib.load().ovl_correct_reads_host, (), buf, offs, k, min_count)


# ---------------------------------------------------------------- unitig pipeline from the score columns
UNITIGS_COUNTS = ("edges", "kept", "paths", "words_per_row")  # ovl_last_unitigs, in the ABI's order
UNITIGS_CYCLE = 1  # OVL_UNITIGS_CYCLE: the walk came back to its own path


def _unitigs_call(fn, head, last, encoded, ids, columns, scoring=None) -> Dict[str, object]:
    """One call of ovl_unitigs_host / ovl_unitigs (``columns``: score, end, self_score, self_end over the distinct
    reads ``encoded``) or ovl_unitigs_candidates (``columns`` None, ``scoring``: match, mismatch, indel, band; the
    reads and the k = 0 list are resident), then the kept edge columns by ovl_unitigs_edges_copy; ``last()`` reads
    the counts that go with the result.  ``cycle_node`` is -1, or the node at which the walk came back to its own
    path: the paths and contigs are then absent."""
    buf, offs = encoded
    n = offs.shape[0] - 1
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    if ids.ndim != 1:
        raise OvlError(-1, "unitigs: ids must be a 1-D array")
    path_off = np.zeros(n + 1, dtype=np.int64)
    path_nodes = np.zeros(max(n, 1), dtype=np.int32)
    bases = np.zeros(max(int(offs[-1] - offs[0]), 1), dtype=np.uint8)
    c_off = np.zeros(n + 1, dtype=np.int64)
    nc, cyc = ctypes.c_int32(0), ctypes.c_int32(-1)
    n_edges, n_kept = ctypes.c_int64(0), ctypes.c_int64(0)
    outs = (_ptr(path_off), _ptr(path_nodes), _ptr(bases), _ptr(c_off), ctypes.byref(nc), ctypes.byref(n_edges),
            ctypes.byref(n_kept), ctypes.byref(cyc))
    if columns is not None:
        cols = [None if x is None else np.ascontiguousarray(x, dtype=np.int32) for x in columns]
        if any(x.shape != (n * (n - 1),) for x in cols[:2]) or any(x is not None and x.shape != (n,) for x in cols[2:]):
            raise OvlError(-1, "unitigs: score and end hold n (n - 1) entries, the self columns n")
        rc = fn(*head, _ptr(buf), _ptr(offs), n, _ptr(ids), ids.shape[0], *[_opt(x) for x in cols], *outs)
    else:
        first = buf[int(offs[0]):]
        rc = fn(*head, _ptr(first) if first.shape[0] else _ptr(buf), _ptr(ids), ids.shape[0],
                *[int(v) for v in scoring], *outs)
    if rc != UNITIGS_CYCLE:
        check(rc, _ctx_of(head))
    kept = int(n_kept.value)
    edges = [np.zeros(max(kept, 1), dtype=np.int32) for _ in range(4)]
    check(_lib.load().ovl_unitigs_edges_copy(_ctx_of(head), *[_ptr(e) for e in edges]), _ctx_of(head))
    res: Dict[str, object] = dict(zip(("tail", "head", "weight", "end_position"), (e[:kept] for e in edges)))
    res.update(n_edges=int(n_edges.value), n_kept=kept, cycle_node=int(cyc.value) if rc == UNITIGS_CYCLE else -1)
    if rc != UNITIGS_CYCLE:
        k = nc.value
        res.update(n_contigs=k, path_off=path_off[: k + 1], path_nodes=path_nodes[:n], c_off=c_off[: k + 1],
                   bases=bases[: int(c_off[k])])
    res.update(last())
    return res


def last_unitigs_host() -> Dict[str, int]:
    """{edges, kept, paths, words_per_row} of this thread's last ``unitigs_host`` (ovl_last_unitigs without a
    context)."""
    return dict(zip(UNITIGS_COUNTS, read_out(_lib.load().ovl_last_unitigs, None)))


def unitigs_host(encoded, ids, score, end, self_score=None, self_end=None) -> Dict[str, object]:
    """``OverlapEngine.unitigs`` on one host thread (ovl_unitigs_host): no context, no GPU."""
    return _unitigs_call(_lib.load().ovl_unitigs_host, (), last_unitigs_host, encoded, ids,
                         (score, end, self_score, self_end))


def unitigs_walk_host(off, heads):
    """find_unitigs' walk over a CSR graph (ovl_unitigs_walk_host): ``(path_off, path_nodes, -1)``, or
    ``(None, None, node)`` when the walk from a node comes back to its own path at ``node``."""
    off, heads, _ = _csr_arrays(off, heads)
    n = off.shape[0] - 1
    path_off = np.zeros(n + 1, dtype=np.int64)
    path_nodes = np.zeros(max(n, 1), dtype=np.int32)
    n_paths, cyc = ctypes.c_int32(0), ctypes.c_int32(-1)
    rc = _lib.load().ovl_unitigs_walk_host(_ptr(off), _ptr(heads), n, _ptr(path_off), _ptr(path_nodes),
                                           ctypes.byref(n_paths), ctypes.byref(cyc))
    if rc == UNITIGS_CYCLE:
        return None, None, int(cyc.value)
    check(rc)
    return path_off[: n_paths.value + 1], path_nodes[:n], -1
