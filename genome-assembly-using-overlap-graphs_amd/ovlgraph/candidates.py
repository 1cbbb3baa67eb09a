"""k-mer candidate-pair enumeration (host side; stays in Python per BASELINE.json north_star).

Produces exactly the ordered pair list that ``construct_overlap_graph_nx_k``
feeds to ``overlap_alignment`` in the reference (overlapGraphs.py:17-52):

* reads are de-duplicated in first-occurrence order (``read_copies``,
  overlapGraphs.py:18-20);
* for ``k > 0`` a prefix index maps ``read[:k]`` (the whole read when it is
  shorter than ``k``) to the reads carrying it, in ``read_copies`` order
  (overlapGraphs.py:30-40);
* the outer loop walks ``read_copies`` in order; its lookup key is
  ``read[-k:]`` (whole read when shorter, overlapGraphs.py:44-47); the inner
  loop walks the indexed list in order, or every distinct read when ``k == 0``
  (overlapGraphs.py:49-50); identical reads are skipped (overlapGraphs.py:52).

Indices refer to positions in the de-duplicated read list.
``enumerate_candidates`` is the vectorised version used by the product path;
``enumerate_candidates_loop`` is a literal loop restatement kept as its checker.
"""
from __future__ import annotations

from collections import Counter
from typing import Dict, List, Sequence, Tuple

import numpy as np


def dedup_reads(reads: Sequence[str]) -> Tuple[List[str], List[int]]:
    """Distinct reads in first-occurrence order plus their copy counts (overlapGraphs.py:18-20).

    ``Counter`` counts in C and keeps first-insertion order, the order of the reference's
    ``read_copies[read] = read_copies.get(read, 0) + 1`` loop."""
    counts = Counter(reads)
    return list(counts.keys()), list(counts.values())


def _prefix_key(r: str, k: int) -> str:
    return r[:k] if len(r) >= k else r


def _suffix_key(r: str, k: int) -> str:
    return r[-k:] if len(r) >= k > 0 else r


def enumerate_candidates_loop(distinct: Sequence[str], k: int) -> Tuple[np.ndarray, np.ndarray]:
    """Literal restatement of overlapGraphs.py:30-52 (slow; used to check the vectorised path)."""
    if k < 0:
        raise AssertionError("k-mer length must be non-negative")
    index: Dict[str, List[int]] = {}
    if k > 0:
        for i, r in enumerate(distinct):
            index.setdefault(_prefix_key(r, k), []).append(i)
    all_idx = list(range(len(distinct)))
    a_out: List[int] = []
    b_out: List[int] = []
    for ia, ra in enumerate(distinct):
        cands = index.get(_suffix_key(ra, k), []) if k > 0 else all_idx
        for ib in cands:
            if ib != ia:  # distinct list => index inequality == string inequality
                a_out.append(ia)
                b_out.append(ib)
    return np.asarray(a_out, dtype=np.int32), np.asarray(b_out, dtype=np.int32)


def enumerate_candidates(distinct: Sequence[str], k: int) -> Tuple[np.ndarray, np.ndarray]:
    """Vectorised candidate enumeration with the reference's iteration order.

    Returns ``(a_idx, b_idx)`` int32 arrays; pair ``p`` means
    ``overlap_alignment(distinct[a_idx[p]], distinct[b_idx[p]])``.
    """
    if k < 0:
        raise AssertionError("k-mer length must be non-negative")
    D = len(distinct)
    if D == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    if k == 0:
        # every ordered pair (a, b) with a != b, a-major, b ascending
        a = np.repeat(np.arange(D, dtype=np.int64), D - 1)
        b = np.tile(np.arange(D - 1, dtype=np.int64), D)
        b = b + (b >= a)  # skip the diagonal while keeping b ascending
        return a.astype(np.int32), b.astype(np.int32)

    key_ids: Dict[str, int] = {}
    pre = np.empty(D, dtype=np.int64)
    for i, r in enumerate(distinct):
        pre[i] = key_ids.setdefault(_prefix_key(r, k), len(key_ids))
    n_keys = len(key_ids)
    suf = np.empty(D, dtype=np.int64)
    for i, r in enumerate(distinct):
        suf[i] = key_ids.get(_suffix_key(r, k), -1)

    order = np.argsort(pre, kind="stable")          # reads grouped by prefix key, index order kept
    sizes = np.bincount(pre, minlength=n_keys)
    starts = np.zeros(n_keys + 1, dtype=np.int64)
    np.cumsum(sizes, out=starts[1:])

    has = suf >= 0
    cnt = np.zeros(D, dtype=np.int64)
    cnt[has] = sizes[suf[has]]
    total = int(cnt.sum())
    if total == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    a = np.repeat(np.arange(D, dtype=np.int64), cnt)
    # position of each output inside its group: global position minus the group's first output
    first_out = np.zeros(D, dtype=np.int64)
    np.cumsum(cnt[:-1], out=first_out[1:])
    grp_start = np.zeros(D, dtype=np.int64)
    grp_start[has] = starts[suf[has]]
    pos = np.arange(total, dtype=np.int64) - np.repeat(first_out, cnt) + np.repeat(grp_start, cnt)
    b = order[pos]
    keep = a != b
    return a[keep].astype(np.int32), b[keep].astype(np.int32)


# ----------------------------------------------------------------------------- seed candidates
# The second candidate rule (include/ovl.h ovl_seed_candidates), stated once:
#
#   Reads are the distinct reads in read_copies order, and k >= 1.  The prefix key of read b is b[:k]; a read
#   shorter than k has no key and takes no part.  For each read a in order, for each offset o = 1, 2, ...,
#   len(a) - k ascending, for each read b != a in read order whose prefix key equals a[o:o+k]: emit (a, b, o),
#   unless (a, b) was already emitted at a smaller offset.
#
# Each b has one prefix key, so offsets of a with different k-mers have disjoint groups and offsets with equal
# k-mers the same group: "already emitted" is "a's k-mer at o also occurs at an offset o' with 1 <= o' < o".


def enumerate_seed_candidates_loop(distinct: Sequence[str], k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The literal loops of the seed rule (slow; the checker of ``enumerate_seed_candidates``)."""
    if k < 1:
        raise ValueError("seed candidates need a k-mer length of at least 1")
    index: Dict[str, List[int]] = {}
    for i, r in enumerate(distinct):
        if len(r) >= k:
            index.setdefault(r[:k], []).append(i)
    a_out: List[int] = []
    b_out: List[int] = []
    o_out: List[int] = []
    for ia, ra in enumerate(distinct):
        emitted = set()
        for o in range(1, len(ra) - k + 1):
            for ib in index.get(ra[o:o + k], []):
                if ib != ia and ib not in emitted:
                    emitted.add(ib)
                    a_out.append(ia)
                    b_out.append(ib)
                    o_out.append(o)
    return (np.asarray(a_out, dtype=np.int32), np.asarray(b_out, dtype=np.int32),
            np.asarray(o_out, dtype=np.int32))


def _kmer_ids(codes: np.ndarray, n_symbols: int, k: int) -> np.ndarray:
    """An integer per position p <= len(codes) - k of a code array, equal exactly where the k codes from p on are
    equal: the codes packed into one uint64 where k of them fit, else ranks of the k-code windows."""
    bits = max(1, int(n_symbols - 1).bit_length())
    n = codes.shape[0] - k + 1
    if k * bits <= 63:
        key = np.zeros(n, dtype=np.uint64)
        for q in range(k):
            key <<= np.uint64(bits)
            key |= codes[q:q + n].astype(np.uint64)
    else:
        win = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(codes.astype(np.uint32), k))
        key = win.view(np.dtype((np.void, 4 * k))).ravel()
    return np.unique(key, return_inverse=True)[1].reshape(-1).astype(np.int64)


def enumerate_seed_candidates(distinct: Sequence[str], k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The seed rule vectorised with numpy, the host form of ``OverlapEngine.enumerate_seed_candidates``.

    Returns ``(a_idx, b_idx, offset)`` int32 arrays in the rule's order: pair ``p`` means that
    ``distinct[a_idx[p]][offset[p]:offset[p] + k] == distinct[b_idx[p]][:k]`` at the smallest such offset >= 1.
    """
    if k < 1:
        raise ValueError("seed candidates need a k-mer length of at least 1")
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    D = len(distinct)
    lens = np.fromiter((len(r) for r in distinct), dtype=np.int64, count=D)
    total = int(lens.sum())
    if D == 0 or total < k:
        return empty
    start = np.zeros(D, dtype=np.int64)
    np.cumsum(lens[:-1], out=start[1:])
    points = np.frombuffer("".join(distinct).encode("utf-32-le"), dtype=np.uint32)
    symbols, codes = np.unique(points, return_inverse=True)
    ids = _kmer_ids(codes.reshape(-1), symbols.shape[0], k)
    n_ids = int(ids.max()) + 1

    # the prefix index: reads with a key grouped by it, read order kept inside a group
    has_key = np.flatnonzero(lens >= k)
    pre = ids[start[has_key]]
    members = has_key[np.argsort(pre, kind="stable")]
    sizes = np.bincount(pre, minlength=n_ids)
    first = np.zeros(n_ids + 1, dtype=np.int64)
    np.cumsum(sizes, out=first[1:])

    # the probes: every (a, o) with 1 <= o <= len(a) - k, a-major, o ascending
    n_off = np.maximum(lens - k, 0)
    n_probe = int(n_off.sum())
    if n_probe == 0:
        return empty
    pa = np.repeat(np.arange(D, dtype=np.int64), n_off)
    probe0 = np.zeros(D, dtype=np.int64)
    np.cumsum(n_off[:-1], out=probe0[1:])
    po = np.arange(n_probe, dtype=np.int64) - np.repeat(probe0, n_off) + 1
    pk = ids[start[pa] + po]
    # a probe whose k-mer occurred at an earlier offset of the same read emits nothing
    is_first = np.zeros(n_probe, dtype=bool)
    is_first[np.unique(pa * n_ids + pk, return_index=True)[1]] = True
    live = np.flatnonzero(is_first & (sizes[pk] > 0))
    if live.shape[0] == 0:
        return empty
    pa, po, pk = pa[live], po[live], pk[live]
    cnt = sizes[pk]
    n_out = int(cnt.sum())
    out0 = np.zeros(live.shape[0], dtype=np.int64)
    np.cumsum(cnt[:-1], out=out0[1:])
    a = np.repeat(pa, cnt)
    o = np.repeat(po, cnt)
    b = members[np.arange(n_out, dtype=np.int64) - np.repeat(out0, cnt) + np.repeat(first[pk], cnt)]
    keep = a != b
    return a[keep].astype(np.int32), b[keep].astype(np.int32), o[keep].astype(np.int32)
