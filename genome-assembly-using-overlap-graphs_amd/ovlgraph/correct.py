"""k-mer spectrum read correction: the reads corrected against their own k-mer spectrum, before anything is scored.

  Codes, keys and windows.  Codes are A = 0, C = 1, G = 2, T = 3, taken from the bytes ACGT; any other byte has no
  code.  k is in [1, 31].  The key of a window r[o:o+k] whose bytes all have codes is
  sum_j code(r[o+j]) << 2(k-1-j), a uint64 below 2^62, so key order is the k-mers' order as byte strings.  A window
  that holds a byte without a code has no key, and so has every window of a read shorter than k.
  Spectrum.  The distinct keys over all windows of all reads (reads counted as given, duplicates included) in
  ascending order, each with its number of occurrences as an int32.
  Threshold.  h[c] = the number of distinct keys with count c.  solid_threshold is the smallest c >= 1 with
  c >= max count or h[c+1] >= h[c] (the first valley of the histogram).  A key is solid when its count is >=
  min_count; a window without a key is never solid.
  Correction, one round.  Every decision reads the original reads only, so reads and positions are independent of
  each other and of the order in which they are handled.  For a read r of length L >= k and a position i the
  covering windows are the offsets o in [max(0, i-k+1), min(i, L-k)].  Position i is trusted when at least one
  covering window is solid, and stays.  An untrusted position whose byte has no code stays.  Otherwise, for each of
  the three other bases x, s(x) is the number of covering windows that are solid after r[i] alone is replaced by x;
  if the largest s(x) is >= 1 and strictly greater than the other two, r[i] becomes that x; on a tie, or when all
  are 0, r[i] stays.  Reads shorter than k are returned as they are.  Lengths never change.

``kmer_spectrum_loop`` and ``correct_reads_loop`` are that statement as literal loops; ``ovl_kmer_spectrum_host`` /
``ovl_correct_reads_host`` (one host thread) and ``ovl_kmer_spectrum`` / ``ovl_correct_reads`` (the GPU) are pinned to
them element for element.  ``kmer_spectrum`` and ``correct_reads`` pick between the forms.  The stage composes in front
of the assembly functions: ``assemble_contigs_best_successor(correct_reads(reads, 12)[0], k=12)``.

One strand only, substitutions only, no quality scores.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

from ._lib import OvlError

FORMS = ("auto", "device", "host", "loop")
STATS = ("kmers", "distinct", "solid", "untrusted", "changed", "ties", "threshold", "windows")
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_BASE = "ACGT"

# form="auto" takes the GPU from this many windows (sum of max(len - k + 1, 0) over the reads).  There is no crossover
# worth a constant: in the sweep of tools/spectrum_probe.py (profiles/spectrum.json; the first r reads of PhiX
# N = 10,000, l = 100, p = 0.01, k = 12; ms, median (max - min) of five, host form on an EPYC 9575F) the device call is
# ahead by more than both spreads from the first point: r = 8 (712 windows) 0.343 (0.039) on the host against 0.267
# (0.013); r = 64 2.691 (0.086) against 0.307 (0.012); r = 8,192 63.1 (0.3) against 0.718 (0.034).  So "auto" takes the
# device whenever one is visible.
CORRECT_DEVICE_MIN_WINDOWS = 0


def _check_k(k: int) -> None:
    if not 1 <= k <= 31:
        raise OvlError(-1, f"k {k} outside [1, 31]")


def _key(read: str, o: int, k: int):
    """The key of the window read[o:o+k], or None when a byte of it has no code."""
    key = 0
    for j in range(k):
        c = _CODE.get(read[o + j])
        if c is None:
            return None
        key += c << (2 * (k - 1 - j))
    return key


def kmer_spectrum_loop(reads: Sequence[str], k: int) -> Tuple[np.ndarray, np.ndarray]:
    """The spectrum as literal loops: (keys uint64 ascending, counts int32)."""
    _check_k(k)
    count: Dict[int, int] = {}
    for r in reads:
        for o in range(len(r) - k + 1):
            key = _key(r, o, k)
            if key is not None:
                count[key] = count.get(key, 0) + 1
    keys = sorted(count)
    return np.asarray(keys, dtype=np.uint64).reshape(len(keys)), \
        np.asarray([count[x] for x in keys], dtype=np.int32).reshape(len(keys))


def solid_threshold(counts) -> int:
    """The smallest c >= 1 with c >= max count or h[c+1] >= h[c], h[c] the number of keys with count c."""
    counts = [int(c) for c in counts]
    most = max(counts, default=0)
    h = [0] * (most + 2)
    for c in counts:
        h[c] += 1
    c = 1
    while not (c >= most or h[c + 1] >= h[c]):
        c += 1
    return c


def correct_reads_loop(reads: Sequence[str], k: int, min_count="auto") -> Tuple[List[str], Dict[str, object]]:
    """One round of the rule as literal loops (slow; what the native forms are checked against).  Returns the
    corrected reads and the stats: ``STATS`` as ints and ``changed_per_read`` (int32)."""
    reads = list(reads)
    keys, counts = kmer_spectrum_loop(reads, k)
    count = dict(zip(keys.tolist(), counts.tolist()))
    if min_count in ("auto", 0):
        min_count = solid_threshold(counts)

    def solid(key) -> bool:
        return key is not None and count.get(key, 0) >= min_count

    out, per_read = [], []
    n_solid = n_untrusted = n_ties = windows = 0
    for r in reads:
        L = len(r)
        new = list(r)
        changed = 0
        if L >= k:
            windows += L - k + 1
            is_solid = [solid(_key(r, o, k)) for o in range(L - k + 1)]
            n_solid += sum(is_solid)
            for i in range(L):
                covering = range(max(0, i - k + 1), min(i, L - k) + 1)
                if any(is_solid[o] for o in covering):
                    continue
                n_untrusted += 1
                if r[i] not in _CODE:
                    continue
                others = [x for x in _BASE if x != r[i]]
                s = []
                for x in others:
                    replaced = r[:i] + x + r[i + 1:]
                    s.append(sum(solid(_key(replaced, o, k)) for o in covering))
                best = max(s)
                if best >= 1 and s.count(best) == 1:
                    new[i] = others[s.index(best)]
                    changed += 1
                elif best >= 1:
                    n_ties += 1
        out.append("".join(new))
        per_read.append(changed)
    n = len(reads)
    stats = {"kmers": int(counts.sum()), "distinct": len(keys), "solid": n_solid, "untrusted": n_untrusted,
             "changed": sum(per_read), "ties": n_ties, "threshold": int(min_count), "windows": windows,
             "changed_per_read": np.asarray(per_read, dtype=np.int32).reshape(n)}
    return out, stats


def _encode(reads):
    from .engine import encode_reads
    try:
        "".join(reads).encode("latin-1")
    except UnicodeEncodeError:
        raise OvlError(-4, "read correction works on the reads' bytes: characters above 255 are not supported")
    return encode_reads(reads)


def _windows(offs: np.ndarray, k: int) -> int:
    return int(np.maximum(np.diff(offs) - k + 1, 0).sum())


def _use_device(form: str, engine, windows: int) -> bool:
    from .engine import use_device
    if form not in FORMS:
        raise ValueError(f"form must be one of {FORMS}")
    return use_device({"auto": None, "device": True}.get(form, False), windows, CORRECT_DEVICE_MIN_WINDOWS, engine)


def kmer_spectrum(reads: Sequence[str], k: int, engine=None, form: str = "auto") -> Tuple[np.ndarray, np.ndarray]:
    """The spectrum of ``reads``: (keys uint64 ascending, counts int32).  ``form``: "device" (ovl_kmer_spectrum),
    "host" (ovl_kmer_spectrum_host), "loop", or "auto": the device when a GPU is visible and the reads hold at least
    ``CORRECT_DEVICE_MIN_WINDOWS`` windows, falling back to the host form beyond the device form's limits."""
    from .engine import default_engine, kmer_spectrum_host
    reads = list(reads)
    _check_k(k)
    if form == "loop":
        return kmer_spectrum_loop(reads, k)
    enc = _encode(reads)
    if _use_device(form, engine, _windows(enc[1], k)):
        try:
            return (engine or default_engine()).kmer_spectrum(reads, k, enc)
        except OvlError as e:
            if e.code != -4 or form == "device":
                raise
    return kmer_spectrum_host(reads, k, enc)


def _one_round(reads: List[str], k: int, min_count: int, engine, form: str):
    from .engine import correct_reads_host, default_engine
    if form == "loop":
        return correct_reads_loop(reads, k, min_count)
    enc = _encode(reads)
    res = None
    if _use_device(form, engine, _windows(enc[1], k)):
        try:
            res = (engine or default_engine()).correct_reads(reads, k, min_count, enc)
        except OvlError as e:
            if e.code != -4 or form == "device":
                raise
    if res is None:
        res = correct_reads_host(reads, k, min_count, enc)
    out, changed, stats = res
    text = out.tobytes().decode("latin-1")
    off = enc[1].tolist()
    stats["changed_per_read"] = changed
    return [text[off[r]:off[r + 1]] for r in range(len(reads))], stats


def correct_reads(reads: Sequence[str], k: int, min_count="auto", rounds: int = 1, engine=None,
                  form: str = "auto") -> Tuple[List[str], Dict[str, object]]:
    """``reads`` corrected by the rule of this module's docstring: (the corrected reads, the stats).

    ``min_count``: "auto" (the threshold rule, ``solid_threshold``) or an int >= 1.  ``rounds`` > 1 repeats the whole
    stage on its own output, the spectrum recounted each round; the stats are the last round's, and ``per_round`` lists
    every round's.  ``form`` as in ``kmer_spectrum``.  The stats: ``STATS`` as ints (k-mers, distinct keys, solid
    windows, untrusted positions, changed bases, ties, the threshold used, windows) and ``changed_per_read``."""
    reads = list(reads)
    _check_k(k)
    if form not in FORMS:
        raise ValueError(f"form must be one of {FORMS}")
    if min_count == "auto":
        min_count = 0
    elif not (isinstance(min_count, (int, np.integer)) and min_count >= 1):
        raise OvlError(-1, 'min_count must be "auto" or an int >= 1')
    if rounds < 1:
        raise OvlError(-1, "rounds must be >= 1")
    per_round = []
    for _ in range(rounds):
        reads, stats = _one_round(reads, k, int(min_count), engine, form)
        per_round.append(stats)
    stats = dict(per_round[-1])
    stats["per_round"] = per_round
    return reads, stats
