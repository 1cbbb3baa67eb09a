"""OverlapEngine — Python face of libovl.so (one context on one or more GPUs).

The engine keeps a read set resident in HBM (bit-plane packed by a gfx950
kernel) and scores candidate pairs in one batched call, replacing the
per-pair Python->Numba call of overlapGraphs.py:53.  A multi-GPU engine
(``OverlapEngine(devices=[...])`` or ``devices="all"``) shards every host-array
call over its GPUs from this one thread.  Results come back in
pinned host arrays (``hostmem.PinnedPool``) unless ``out=`` is given.  It never
computes on the CPU: a missing library or GPU raises ``OvlError``.

The stages that also have a host form (the graph reductions, read depth, consensus,
layout, read correction) are marshalled in ``stages.py``; the engine's methods of those
names are the device form of the same call.  ``use_device`` is the one rule by which
the package's entry points choose between the two forms.
"""
from __future__ import annotations

import ctypes
import os
import threading
import weakref
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._lib import OvlError, _ptr, check, read_out
from .hostmem import pinned_empty
# (the stage names are also this module's: callers import the host forms and encode_reads from here)
from .stages import (CORRECT_STATS, LAYOUT_COUNTS, UNITIGS_COUNTS, _consensus_call, _correct_call,  # noqa: F401
                     _layout_call, _layout_outputs, _layout_result, _placed_call, _reach_call, _read_best_call,
                     _spectrum_call, _transitive_call, _unitigs_call, consensus_host, consensus_placed_host,
                     correct_reads_host, encode_reads, kmer_spectrum_host, last_layout_host, last_unitigs_host,
                     layout_host, reach_reduce_host, read_best_host, transitive_reduce_host, unitigs_host,
                     unitigs_walk_host)

INDEL_DEFAULT = -(2 ** 31)  # aligners.py:7 default indel (the report's "-inf", REPORT p.3)

_LIVE: "weakref.WeakSet[OverlapEngine]" = weakref.WeakSet()  # open contexts (quiesce_all)


def quiesce_all() -> None:
    """ovl_quiesce on every open context of this process: their resident scoring grids leave the device, so a
    whole-device synchronisation (torch.cuda.synchronize) that follows does not wait for the grids' idle deadline.
    Call it from the thread that drives the contexts."""
    for eng in list(_LIVE):
        if getattr(eng, "_ctx", None):
            eng.quiesce()


def _outputs(n: int, out) -> Tuple[np.ndarray, np.ndarray]:
    """Result arrays: the caller's ``out=(score, end)`` (int32, contiguous, >= n) or pinned ones."""
    if out is None:
        return pinned_empty(n), pinned_empty(n)
    sc, en = out
    for x in (sc, en):
        if not (isinstance(x, np.ndarray) and x.dtype == np.int32 and x.flags.c_contiguous and x.ndim == 1
                and x.shape[0] >= n and x.flags.writeable):
            raise OvlError(-1, "out must be two writeable contiguous 1-D int32 arrays of >= n_pairs elements")
    return sc[:n], en[:n]


def _pair_arrays(a_idx, b_idx) -> Tuple[np.ndarray, np.ndarray]:
    """A host pair list as the two contiguous int32 arrays the C ABI takes."""
    a = np.ascontiguousarray(a_idx, dtype=np.int32)
    b = np.ascontiguousarray(b_idx, dtype=np.int32)
    if a.shape != b.shape or a.ndim != 1:
        raise OvlError(-1, "a_idx and b_idx must be 1-D arrays of equal length")
    return a, b


def host_pool() -> Dict[str, int]:
    """The host thread pool's plan, recounted now (ovl_host_pool): {threads, sharers, cpus, packed}."""
    return dict(zip(("threads", "sharers", "cpus", "packed"), read_out(_lib.load().ovl_host_pool)))


def device_count() -> int:
    n = ctypes.c_int32(0)
    rc = _lib.load().ovl_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def use_device(device: Optional[bool], work, min_work: int, engine) -> bool:
    """Whether a stage takes its device form: ``device`` when the caller forced it (True / False), else whether the
    ``work`` (a number, or a function that counts it) reaches the stage's threshold and a device can serve it -- an
    engine was given, or one is visible.  The count is asked for last: on a box without a GPU it loads the library,
    which small inputs do not pay for."""
    if device is not None:
        return device
    if callable(work):
        work = work()
    return work >= min_work and (engine is not None or device_count() > 0)


class OverlapEngine:
    """A libovl context on one HIP device (``device``; -1 = the current one) or on several
    (``devices``: a list of ordinals, or "all")."""

    def __init__(self, device: int = -1, devices: Union[None, str, Sequence[int]] = None):
        self._L = _lib.load()
        n = ctypes.c_int32(0)
        rc = self._L.ovl_device_count(ctypes.byref(n))
        if rc != 0 or n.value <= 0:
            raise OvlError(-2, "no HIP device visible to libovl: the overlap engine has no CPU fallback "
                               f"({_lib.last_error()})")
        ctx = ctypes.c_void_p()
        if devices == "all":
            check(self._L.ovl_create(0, ctypes.byref(ctx)))
        elif devices is not None:
            ids = np.ascontiguousarray(list(devices), dtype=np.int32)
            check(self._L.ovl_create_on_devices(_ptr(ids), int(ids.shape[0]), ctypes.byref(ctx)))
        elif int(device) < 0:
            check(self._L.ovl_create(1, ctypes.byref(ctx)))
        else:
            ids = np.array([int(device)], dtype=np.int32)
            check(self._L.ovl_create_on_devices(_ptr(ids), 1, ctypes.byref(ctx)))
        self._ctx = ctx
        self._reads_key = None
        self._dev0 = self.devices[0]  # device pointers given to score_device / score_tensors live here
        _LIVE.add(self)

    def _get(self, fn, keys, *args) -> dict:
        """``keys`` zipped with the out-parameters of ``fn(ctx, *args, ...)``."""
        return dict(zip(keys, read_out(fn, self._ctx, *args, ctx=self._ctx)))

    def _tensor_args(self, what: str, a, b, out_score, out_end, stream) -> Tuple[int, int]:
        """(n_pairs, stream handle) of a scoring launch over contiguous int32 tensors on this engine's first device
        (kernels there read and write them), on torch's current stream unless ``stream`` is given."""
        import torch
        for t in (a, b, out_score, out_end):
            if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous():
                raise OvlError(-1, f"{what} needs contiguous int32 device tensors")
            if t.device.index != self._dev0:
                raise OvlError(-1, f"{what}: tensor on cuda:{t.device.index}, but this engine's kernels run on "
                                   f"cuda:{self._dev0}")
        n = a.numel()
        if b.numel() != n or out_score.numel() < n or out_end.numel() < n:
            raise OvlError(-1, "tensor sizes disagree")
        s = stream if stream is not None else torch.cuda.current_stream(a.device)
        return n, s.cuda_stream

    @property
    def devices(self) -> List[int]:
        """Device ordinals of this context (results are sharded over them in this order)."""
        n = ctypes.c_int32()
        ids = np.zeros(64, dtype=np.int32)
        check(self._L.ovl_ctx_devices(self._ctx, _ptr(ids), 64, ctypes.byref(n)), self._ctx)
        return ids[: n.value].tolist()

    def set_timing(self, on: bool = True) -> None:
        """Record kernel time inside host-array scoring calls (HIP events; see ``last_timing``)."""
        check(self._L.ovl_set_timing(self._ctx, 1 if on else 0), self._ctx)

    def last_timing(self) -> Dict[str, float]:
        """{kernel_ms: summed kernel time of the busiest device, call_ms: wall time} of the last call."""
        return self._get(self._L.ovl_last_timing, ("kernel_ms", "call_ms"))

    def last_launches(self) -> List[Dict[str, float]]:
        """The scoring launches of the last host-array call made with timing on (ovl_last_launches):
        [{device, sink (0 HBM, 1 int32 into host memory, 2 packed into host staging), pairs, ms}]."""
        n = ctypes.c_int32()
        check(self._L.ovl_last_launches(self._ctx, 0, None, None, None, None, ctypes.byref(n)), self._ctx)
        k = n.value
        dev, sink = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.int32)
        pairs, ms = np.zeros(max(k, 1), np.int64), np.zeros(max(k, 1), np.float64)
        check(self._L.ovl_last_launches(self._ctx, k, _ptr(dev), _ptr(sink), _ptr(pairs), _ptr(ms),
                                        ctypes.byref(n)), self._ctx)
        return [{"device": int(dev[i]), "sink": int(sink[i]), "pairs": int(pairs[i]), "ms": float(ms[i])}
                for i in range(min(k, n.value))]

    def last_transfer(self) -> Dict[str, int]:
        """{link_bytes, packed_pairs} of the last host-array scoring call (ovl_last_transfer) and its results'
        part: result_bytes, record_pairs (crossed as tile records), escapes (ovl_last_results)."""
        return {**self._get(self._L.ovl_last_transfer, ("link_bytes", "packed_pairs")),
                **self._get(self._L.ovl_last_results, ("result_bytes", "record_pairs", "escapes"))}

    def last_pair_list(self) -> Dict[str, int]:
        """{in_place_pairs, decoded_pairs} of the last host-array call (ovl_last_pair_list): how the compact
        host pair list reached the kernels (read in place by uniform_kernel, or decoded into HBM first)."""
        return self._get(self._L.ovl_last_pair_list, ("in_place_pairs", "decoded_pairs"))

    # ---------------------------------------------------------------- lifecycle
    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._L.ovl_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- reads
    def set_reads(self, reads: Sequence[str], encoded: Optional[Tuple[np.ndarray, np.ndarray]] = None) -> None:
        """Upload, encode and bit-plane pack a read set; it stays resident in HBM."""
        buf, offs = encoded if encoded is not None else encode_reads(reads)
        n = offs.shape[0] - 1
        check(self._L.ovl_set_reads(self._ctx, _ptr(buf), _ptr(offs), n), self._ctx)
        self._reads_key = id(reads)

    def info(self) -> Dict[str, int]:
        return self._get(self._L.ovl_reads_info, ("n_reads", "lmax", "planes", "device_bytes"))

    def plan(self, match: int = 10, mismatch: int = -1, indel: int = INDEL_DEFAULT, band: int = -1) -> str:
        k = ctypes.c_int32()
        check(self._L.ovl_plan(self._ctx, match, mismatch, indel, band, ctypes.byref(k)), self._ctx)
        return _lib.KERNELS[k.value]

    def last_score_form(self) -> Dict[str, object]:
        """The form the first scoring launch of the last scoring call took on this engine's first device
        (ovl_last_score_form; host-array calls, ``score_tensors`` and ``launcher`` alike): ``kernel`` ("none" when
        nothing was launched, else as ``plan``), ``key64`` (for a banded call, its seed's), ``wide``, ``lane`` (the
        lane-per-pair full DP ran) with its arguments ``prof``, ``sfx``, ``ho`` (0 int32 / 1 int16 hand-off column,
        2 four-bit steps in LDS) and ``h2`` (packed f16 cells), ``band_form`` ("none", "strip", "rows", "fast", "diag"
        or "lane": the band form as launched), ``split`` (the band lane kernel's two lanes per pair) and ``rs_log2`` (an
        ungapped launch: 0 in throughput mode)."""
        names = ("kernel", "key64", "wide", "lane", "prof", "sfx", "ho", "h2", "band_form", "split", "rs_log2")
        form: Dict[str, object] = self._get(self._L.ovl_last_score_form, names)
        form["kernel"] = _lib.KERNELS[form["kernel"]]
        form["band_form"] = _lib.BAND_FORMS[form["band_form"]]
        return form

    # ---------------------------------------------------------------- candidates
    def candidates(self, k: int = 5) -> Tuple[np.ndarray, np.ndarray]:
        """k-mer candidate pairs over the resident (distinct) reads, enumerated on the GPU.

        Same list and order as ``candidates.enumerate_candidates`` (overlapGraphs.py:30-52);
        the list also stays resident for ``score_candidates``.
        """
        return self.candidates_copy(self.enumerate_candidates(k))

    def candidates_copy(self, n: int) -> Tuple[np.ndarray, np.ndarray]:
        """The resident candidate list (``n`` pairs, from ``enumerate_candidates``) in pinned host arrays."""
        a = pinned_empty(n)
        b = pinned_empty(n)
        if n:
            check(self._L.ovl_candidates_copy(self._ctx, _ptr(a), _ptr(b)), self._ctx)
        return a, b

    def enumerate_candidates(self, k: int = 5) -> int:
        """Enumerate the candidate list on the device (kept resident); returns its length."""
        if k < 0:
            raise AssertionError("k-mer length must be non-negative")
        n = ctypes.c_int64()
        check(self._L.ovl_candidates(self._ctx, int(k), ctypes.byref(n)), self._ctx)
        return int(n.value)

    def enumerate_seed_candidates(self, k: int) -> int:
        """Enumerate the seed candidate list on the device (ovl_seed_candidates): every k-mer of a read at offsets
        >= 1 looked up among the reads' prefixes, the list and order of ``candidates.enumerate_seed_candidates``.
        It becomes the resident candidate list (``candidates_copy``, ``score_candidates``, ...); returns its
        length."""
        n = ctypes.c_int64()
        check(self._L.ovl_seed_candidates(self._ctx, int(k), ctypes.byref(n)), self._ctx)
        return int(n.value)

    def seed_offsets(self) -> np.ndarray:
        """The offset of each pair of the resident seed candidate list (ovl_seed_offsets_copy); OVL_E_STATE when
        the resident list did not come from ``enumerate_seed_candidates``."""
        n = self.candidates_device()[2]  # (OVL_E_STATE without any list)
        out = np.zeros(max(n, 1), dtype=np.int32)
        check(self._L.ovl_seed_offsets_copy(self._ctx, _ptr(out)), self._ctx)
        return out[:n]

    def seed_candidates(self, k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``(a, b, offset)`` of the seed candidate list, enumerated on the GPU and kept resident."""
        a, b = self.candidates_copy(self.enumerate_seed_candidates(k))
        return a, b, self.seed_offsets()

    def last_seed_timing(self) -> Dict[str, float]:
        """Device times (ms) of the last ``enumerate_seed_candidates`` made with timing on
        (ovl_last_seed_timing): keys_ms, sort_ms, count_ms (the count kernel and the scan), emit_ms."""
        return self._get(self._L.ovl_last_seed_timing, ("keys_ms", "sort_ms", "count_ms", "emit_ms"))

    def candidates_device(self) -> Tuple[int, int, int]:
        """(device ptr of a_idx, device ptr of b_idx, n_pairs) of the resident candidate list."""
        pa, pb, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        check(self._L.ovl_candidates_device(self._ctx, ctypes.byref(pa), ctypes.byref(pb), ctypes.byref(n)),
              self._ctx)
        return pa.value or 0, pb.value or 0, int(n.value)

    def score_candidates(self, match: int = 10, mismatch: int = -1, indel: int = INDEL_DEFAULT,
                         band: int = -1, out=None) -> Tuple[np.ndarray, np.ndarray]:
        """Score the resident candidate list (no pair upload) -> (score, end) host arrays.

        Sharded over the engine's devices; each device's results land in its slice of the
        arrays by DMA (pinned arrays unless ``out=(score, end)`` is given)."""
        n = self.candidates_device()[2]
        sc, en = _outputs(n, out)
        check(self._L.ovl_score_candidates(self._ctx, match, mismatch, indel, band, _ptr(sc), _ptr(en)),
              self._ctx)
        return sc, en

    def score_candidates_range(self, lo: int, hi: int, match: int = 10, mismatch: int = -1,
                               indel: int = INDEL_DEFAULT, band: int = -1, out=None) -> Tuple[np.ndarray, np.ndarray]:
        """(score, end) of candidate pairs [lo, hi) (a shard of a multi-process job)."""
        sc, en = _outputs(int(hi) - int(lo), out)
        check(self._L.ovl_score_candidates_range(self._ctx, int(lo), int(hi), match, mismatch, indel, band,
                                                 _ptr(sc), _ptr(en)), self._ctx)
        return sc, en

    def range_scorer(self, lo: int, hi: int, out, match: int = 10, mismatch: int = -1, indel: int = INDEL_DEFAULT,
                     band: int = -1):
        """Pre-bound ``score_candidates_range(lo, hi, ..., out=out)`` for repeated steps over the same shard and
        arrays: every argument converted to its ctypes form once, so a step costs one foreign call (the
        sharded step of a multi-process job calls it every step).  ``out`` must stay alive while it is used."""
        sc, en = _outputs(int(hi) - int(lo), out)
        fn = self._L.ovl_score_candidates_range
        ctx = self._ctx
        args = (ctx, ctypes.c_int64(int(lo)), ctypes.c_int64(int(hi)), ctypes.c_int32(match), ctypes.c_int32(mismatch),
                ctypes.c_int64(indel), ctypes.c_int32(band), _ptr(sc), _ptr(en))
        check(self._L.ovl_plan(ctx, match, mismatch, indel, band, ctypes.byref(ctypes.c_int32())), ctx)

        keep = (self, sc, en)  # the closure owns the result arrays (and the engine) its pointers name

        def score() -> None:
            if keep[0]._ctx is None:
                raise RuntimeError("range_scorer: the engine is closed")
            rc = fn(*args)
            if rc:
                check(rc, ctx)
        return score

    def devices_for(self, n_pairs: int) -> int:
        """How many of this context's devices a host-array call over n_pairs uses (ovl_devices_for)."""
        return read_out(self._L.ovl_devices_for, self._ctx, int(n_pairs), ctx=self._ctx)[0]

    def quiesce(self) -> None:
        """Make this context's resident scoring grids leave the device now (ovl_quiesce): before a whole-device
        synchronisation (torch.cuda.synchronize), which would otherwise wait for their idle deadline.  The next
        eligible scoring call relaunches them."""
        check(self._L.ovl_quiesce(self._ctx), self._ctx)

    def resident_stats(self) -> Dict[str, int]:
        """{alive, launches, relaunches, broken} of this context's resident grids (ovl_resident_stats)."""
        return self._get(self._L.ovl_resident_stats, ("alive", "launches", "relaunches", "broken"))

    def candidate_shards(self, n_shards: int) -> List[int]:
        """Shard bounds of the resident candidate list balanced by sum len(a)*len(b) + 1 (on the device)."""
        bounds = np.zeros(int(n_shards) + 1, dtype=np.int64)
        check(self._L.ovl_candidates_shards(self._ctx, int(n_shards), _ptr(bounds)), self._ctx)
        return bounds.tolist()

    # ---------------------------------------------------------------- local alignment
    def local_align(self, query: str, reference: str, match: int = 10, mismatch: int = -1, indel: int = -1,
                    traceback: bool = True):
        """local_alignment's DP (aligners.py:105-160) on the GPU for one (possibly large) pair.

        Returns (score, end_i, end_j, start_i, start_j, ops) with ops the walk's codes
        (1 diag, 2 up, 3 left) in walk order (None without traceback).
        """
        buf, offs = encode_reads([query, reference])
        n, m = len(query), len(reference)
        qb = np.ascontiguousarray(buf[:n]) if n else np.zeros(1, np.uint8)
        rb = np.ascontiguousarray(buf[n:n + m]) if m else np.zeros(1, np.uint8)
        outs = [ctypes.c_int32() for _ in range(5)]
        k = ctypes.c_int64()
        cap = n + m + 1
        ops = np.zeros(cap, dtype=np.int8) if traceback else None
        check(self._L.ovl_local_align(self._ctx, _ptr(qb), n, _ptr(rb), m, int(match), int(mismatch), int(indel),
                                      *[ctypes.byref(o) for o in outs], _ptr(ops) if traceback else None,
                                      cap if traceback else 0, ctypes.byref(k)), self._ctx)
        sc, ei, ej, si, sj = (o.value for o in outs)
        return sc, ei, ej, si, sj, (ops[: k.value] if traceback else None)

    def local_align_batch(self, queries: Sequence[str], reference: str, windows=None, match: int = 10,
                          mismatch: int = -1, indel: int = -1, traceback: bool = True):
        """``local_align`` of every query against ``reference`` in one call (ovl_local_align_batch).

        ``windows`` (optional): one ``(lo, length)`` per query, the slice of the reference it is aligned
        to; positions are relative to that slice.  Returns ``(score, end_i, end_j, start_i, start_j, ops)``:
        five int32 arrays and a list of per-query op arrays (walk order; ``None`` without traceback).
        """
        queries = list(queries)
        nq = len(queries)
        buf, offs = encode_reads(queries + [reference])
        G = len(reference)
        q_off = np.ascontiguousarray(offs[: nq + 1])
        ref = np.ascontiguousarray(buf[int(offs[nq]): int(offs[nq]) + G]) if G else np.zeros(1, np.uint8)
        if windows is None:
            lo = ln = None
            m = np.full(nq, G, dtype=np.int64)
        else:
            w = np.asarray(list(windows), dtype=np.int64).reshape(-1, 2)
            if w.shape[0] != nq:
                raise OvlError(-1, "windows must hold one (lo, length) per query")
            if w.size and (w.min() < -2 ** 31 or w.max() >= 2 ** 31):
                raise OvlError(-1, "window outside the int32 range")
            lo = np.ascontiguousarray(w[:, 0], dtype=np.int32)
            ln = np.ascontiguousarray(w[:, 1], dtype=np.int32)
            m = w[:, 1]
        outs = [np.zeros(max(nq, 1), dtype=np.int32) for _ in range(5)]
        n_ops = np.zeros(max(nq, 1), dtype=np.int64)
        ops = ops_off = None
        if traceback:
            ops_off = np.zeros(nq + 1, dtype=np.int64)
            np.cumsum(np.diff(q_off) + np.maximum(m, 0), out=ops_off[1:])
            ops = np.zeros(max(int(ops_off[-1]), 1), dtype=np.int8)
        check(self._L.ovl_local_align_batch(
            self._ctx, _ptr(buf), _ptr(q_off), nq, _ptr(ref), G, _ptr(lo) if lo is not None else None,
            _ptr(ln) if ln is not None else None, int(match), int(mismatch), int(indel),
            *[_ptr(o) for o in outs], _ptr(ops) if traceback else None, _ptr(ops_off) if traceback else None,
            _ptr(n_ops)), self._ctx)
        walks = None
        if traceback:
            walks = [ops[int(ops_off[k]): int(ops_off[k]) + int(n_ops[k])] for k in range(nq)]
        return tuple(o[:nq] for o in outs) + (walks,)

    def last_local_batch(self) -> Dict[str, int]:
        """{batched, single, waves} of the last ``local_align_batch`` (ovl_last_local_batch): the queries that took
        the batch kernel, those that took the single-pair path, and the batch kernel's wavefronts."""
        return self._get(self._L.ovl_last_local_batch, ("batched", "single", "waves"))

    def read_best(self, reads, contigs, read_length: int, match: int = 10, mismatch: int = -1, indel: int = -1,
                  scores: bool = False) -> Dict[str, np.ndarray]:
        """Every read against every contig by ``align_read_or_contig_to_reference`` (ovl_read_best), reduced per
        read: ``best_score``, ``first_best`` (the first contig position that attains it, -1 without contigs),
        ``n_best``, ``start`` and ``end`` (the aligned stretch on that contig) as int32 arrays, ``tie_bits``
        (reads x ceil(contigs / 32) uint32: bit c of row r set iff contig c attains the best score) and, with
        ``scores=True``, the reads x contigs score matrix."""
        return _read_best_call(self._L.ovl_read_best, (self._ctx,), reads, contigs, read_length, match, mismatch,
                               indel, scores)

    def last_read_best(self) -> Dict[str, int]:
        """{lane_pairs, fallback_pairs, launches} of the last ``read_best`` (ovl_last_read_best): the (read, contig)
        pairs the lane-per-read kernel scored, those that went through the existing local-alignment kernels, and
        the lane kernel's launches."""
        return self._get(self._L.ovl_last_read_best, ("lane_pairs", "fallback_pairs", "launches"))

    def consensus(self, reads, contigs, place, read_length: int, match: int = 10, mismatch: int = -1,
                  indel: int = -1, min_depth: int = 3, counts: bool = True) -> Dict[str, object]:
        """The read pileup and the per-base vote (ovl_consensus): read r, aligned to contig position ``place[r]`` (-1:
        no vote) by ``align_read_or_contig_to_reference``, votes along its walk.  Returns ``called`` (uint8 over the
        concatenated contigs), ``n_changed``, ``n_other`` (read bytes outside ACGT on a diagonal), ``aln`` (reads x 3
        int32: score, first column, one past the last column, in the contig's own coordinates) and, with
        ``counts=True``, ``counts`` (bases x 6 int32: A, C, G, T, gap, ins)."""
        return _consensus_call(self._L.ovl_consensus, (self._ctx,), reads, contigs, place, read_length, match,
                               mismatch, indel, min_depth, counts)

    def last_consensus(self) -> Dict[str, float]:
        """{batch_reads, single_reads, ops, launches} of the last ``consensus`` (ovl_last_consensus): the reads that
        took the batch kernel and the single-pair path, the ops piled up and the batch kernel's launches; with timing
        on also {align_ms, pileup_ms, vote_ms} (ovl_last_consensus_timing)."""
        return {**self._get(self._L.ovl_last_consensus, ("batch_reads", "single_reads", "ops", "launches")),
                **self._get(self._L.ovl_last_consensus_timing, ("align_ms", "pileup_ms", "vote_ms"))}

    def consensus_placed(self, reads, contigs, contig, offset, slack: int = 8, weights=None, rounds: int = 1,
                         min_depth: int = 3, min_vote_score: int = 1, match: int = 10, mismatch: int = -1,
                         indel: int = -1, counts: bool = True) -> Dict[str, object]:
        """Placed consensus (ovl_consensus_placed; the rule: include/ovl.h and ``consensus.pileup_placed_loop``): read
        r votes with ``weights[r]`` (None: 1) on contig position ``contig[r]`` (-1: no vote), aligned inside the band of
        ``slack`` diagonals around its placement ``offset[r]``, for up to ``rounds`` rounds on the device.  Returns
        what ``consensus`` returns, of the last round, plus ``total_changed`` and ``rounds``."""
        return _placed_call(self._L.ovl_consensus_placed, (self._ctx,), reads, contigs, contig, offset, slack, weights,
                            rounds, min_depth, min_vote_score, match, mismatch, indel, counts)

    def last_consensus_placed(self) -> Dict[str, float]:
        """{voted_reads, windowless_reads, ops, launches, rounds} of the last ``consensus_placed``
        (ovl_last_consensus_placed): the reads that voted in the last round, the placed reads without a window, the
        ops of the last round's walks, the band kernel's launches and the rounds; with timing on also {band_ms,
        vote_ms} over all rounds (ovl_last_consensus_placed_timing)."""
        return {**self._get(self._L.ovl_last_consensus_placed,
                            ("voted_reads", "windowless_reads", "ops", "launches", "rounds")),
                **self._get(self._L.ovl_last_consensus_placed_timing, ("band_ms", "vote_ms"))}

    def layout(self, reads, a, b, score, end, min_score: int = 1, min_overlap: int = 1,
               encoded=None) -> Dict[str, object]:
        """The best-successor layout of scored pairs (ovl_layout; the rule: ``ovlgraph.layout``): ``succ``, ``link``,
        ``contig``, ``offset`` (int32 per read), ``on_path`` (uint8 per read), ``bases`` (the contigs' bytes) with
        ``c_off`` and ``n_contigs``, and the counts of ``last_layout``."""
        return _layout_call(self._L.ovl_layout, (self._ctx,), self.last_layout, reads, a, b, score, end, min_score,
                            min_overlap, encoded)

    def layout_candidates(self, match: int = 10, mismatch: int = -1, indel: int = INDEL_DEFAULT, band: int = -1,
                          min_score: int = 1, min_overlap: int = 1) -> Dict[str, object]:
        """``layout`` of the resident candidate list on the resident reads (ovl_layout_candidates): the list is scored
        into device columns and laid out there; only the outputs come back, and the list stays as it was."""
        i = self.info()
        n = max(i["n_reads"], 0)
        # (the contigs hold at most the reads' bytes, which n * lmax bounds)
        outs, on_path, bases, c_off = _layout_outputs(n, n * i["lmax"])
        nc = ctypes.c_int32(0)
        check(self._L.ovl_layout_candidates(self._ctx, int(match), int(mismatch), int(indel), int(band),
                                            int(min_score), int(min_overlap), *[_ptr(o) for o in outs], _ptr(on_path),
                                            _ptr(bases), _ptr(c_off), ctypes.byref(nc)), self._ctx)
        return _layout_result(n, outs, on_path, bases, c_off, nc.value, self.last_layout())

    def last_layout(self) -> Dict[str, float]:
        """{links, cycles, levels, on_path_reads} of the last ``layout`` / ``layout_candidates`` (ovl_last_layout): the
        links of the forest after the cuts, the cycles cut, the doubling levels and the reads on contig paths; with
        timing on also {score_ms, link_ms, forest_ms, spell_ms} (ovl_last_layout_timing)."""
        return {**self._get(self._L.ovl_last_layout, LAYOUT_COUNTS),
                **self._get(self._L.ovl_last_layout_timing, ("score_ms", "link_ms", "forest_ms", "spell_ms"))}

    def kmer_spectrum(self, reads, k: int, encoded=None):
        """The k-mer spectrum of ``reads`` (ovl_kmer_spectrum; the rule: ``ovlgraph.correct``): the distinct keys
        ascending (uint64) and their counts (int32)."""
        buf, offs = encoded if encoded is not None else encode_reads(reads)
        return _spectrum_call(self._L.ovl_kmer_spectrum, (self._ctx,), buf, offs, k)

    def correct_reads(self, reads, k: int, min_count: int = 0, encoded=None):
        """One round of k-mer spectrum correction (ovl_correct_reads): the corrected bytes in the layout of
        ``encode_reads``, the changed bases per read (int32) and the stats ``engine.CORRECT_STATS`` as a dict.
        ``min_count`` 0 takes the threshold rule."""
        buf, offs = encoded if encoded is not None else encode_reads(reads)
        return _correct_call(self._L.ovl_correct_reads, (self._ctx,), buf, offs, k, min_count)

    def last_correct(self) -> Dict[str, float]:
        """With timing on, {keys_ms, sort_ms, count_ms, correct_ms} of the last ``kmer_spectrum`` / ``correct_reads``
        (ovl_last_correct_timing); zeros with timing off."""
        return self._get(self._L.ovl_last_correct_timing, ("keys_ms", "sort_ms", "count_ms", "correct_ms"))

    # ---------------------------------------------------------------- graph stages
    def transitive_reduce(self, off, heads, weights) -> np.ndarray:
        """The reference's transitive reduction (overlapGraphs.py:235-303) of a CSR graph on the GPU
        (ovl_transitive_reduce): a uint8 mask over the CSR edges, 1 where the reference removes the edge."""
        return _transitive_call(self._L.ovl_transitive_reduce, (self._ctx,), off, heads, weights)

    def last_transitive(self) -> Dict[str, int]:
        """{window, passes, two_hop_steps} of the last ``transitive_reduce`` (ovl_last_transitive): the out-row
        entries held in LDS per pass, the passes per node, and the two-hop paths walked."""
        return self._get(self._L.ovl_last_transitive, ("window", "passes", "two_hop_steps"))

    def reach_reduce(self, off, heads, closure: bool = False):
        """The reference's ``transitive_reduction2`` (overlapGraphs.py:354-367) of a weightless CSR graph on the GPU
        (ovl_reach_reduce): a uint8 mask over the CSR edges, 1 where the reference removes the edge -- edge (v, w)
        goes iff a successor of v that stands before w reaches w.  ``closure=True`` returns ``(mask, matrix)``, the
        matrix n x ceil(n / 64) uint64: bit x & 63 of word x >> 6 of row u is set iff a path of at least one edge
        leads from u to x."""
        return _reach_call(self._L.ovl_reach_reduce, (self._ctx,), off, heads, closure)

    def last_reach(self) -> Dict[str, int]:
        """{words_per_row, pivot_blocks, window_bits} of the last ``reach_reduce`` (ovl_last_reach): the bit matrix's
        row width, the closure's pivot blocks of 64 nodes, and the columns the marking holds in registers per pass."""
        return self._get(self._L.ovl_last_reach, ("words_per_row", "pivot_blocks", "window_bits"))

    def unitigs(self, encoded, ids, score, end, self_score=None, self_end=None) -> Dict[str, object]:
        """The unitig pipeline from host score columns on the GPU (ovl_unitigs; the rule: ``ovlgraph.unitigs``): the
        paths (``path_off``, ``path_nodes``), the contigs' bytes (``bases``, ``c_off``, ``n_contigs``), the kept edge
        columns (``tail``, ``head``, ``weight``, ``end_position``), ``n_edges``, ``n_kept``, ``cycle_node`` and the
        counts of ``last_unitigs``."""
        return _unitigs_call(self._L.ovl_unitigs, (self._ctx,), self.last_unitigs, encoded, ids,
                             (score, end, self_score, self_end))

    def unitigs_candidates(self, encoded, ids, match: int = 10, mismatch: int = -1, indel: int = INDEL_DEFAULT,
                           band: int = -1) -> Dict[str, object]:
        """``unitigs`` of the raw list ``ids`` over the resident reads (``encoded``: their bytes, for the spelling) and
        the resident k = 0 candidate list (ovl_unitigs_candidates): the list and the repeated reads' self pairs are
        scored into device columns; only ``ids``, the per-node arrays and the outputs cross the link."""
        return _unitigs_call(self._L.ovl_unitigs_candidates, (self._ctx,), self.last_unitigs, encoded, ids, None,
                             (match, mismatch, indel, band))

    def last_unitigs(self) -> Dict[str, float]:
        """{edges, kept, paths, words_per_row} of the last ``unitigs`` / ``unitigs_candidates`` (ovl_last_unitigs);
        with timing on also {score_ms, build_ms, reduce_ms, facts_ms} (ovl_last_unitigs_timing)."""
        return {**self._get(self._L.ovl_last_unitigs, UNITIGS_COUNTS),
                **self._get(self._L.ovl_last_unitigs_timing, ("score_ms", "build_ms", "reduce_ms", "facts_ms"))}

    # ---------------------------------------------------------------- scoring
    def score_pairs(self, reads: Sequence[str], a_idx, b_idx, match: int = 10, mismatch: int = -1,
                    indel: int = INDEL_DEFAULT, band: int = -1, out=None,
                    encoded: Optional[Tuple[np.ndarray, np.ndarray]] = None) -> Tuple[np.ndarray, np.ndarray]:
        """The one-shot ABI call ``ovl_score_pairs``: host reads + host pair list -> host
        (score, end); the reads are uploaded, packed and left resident (as ``set_reads``)."""
        buf, offs = encoded if encoded is not None else encode_reads(reads)
        a, b = _pair_arrays(a_idx, b_idx)
        sc, en = _outputs(a.shape[0], out)
        check(self._L.ovl_score_pairs(self._ctx, _ptr(buf), _ptr(offs), offs.shape[0] - 1, _ptr(a), _ptr(b),
                                      a.shape[0], match, mismatch, indel, band, _ptr(sc), _ptr(en)), self._ctx)
        self._reads_key = id(reads)
        return sc, en

    def score(self, a_idx, b_idx, match: int = 10, mismatch: int = -1, indel: int = INDEL_DEFAULT,
              band: int = -1, out=None) -> Tuple[np.ndarray, np.ndarray]:
        """Score pairs (host arrays) against the resident reads -> (score, end) int32 arrays
        (pinned unless ``out=(score, end)`` is given); sharded over the engine's devices."""
        a, b = _pair_arrays(a_idx, b_idx)
        sc, en = _outputs(a.shape[0], out)
        check(self._L.ovl_score_host(self._ctx, _ptr(a), _ptr(b), a.shape[0], match, mismatch, indel, band,
                                     _ptr(sc), _ptr(en)), self._ctx)
        return sc, en

    def score_device(self, a_ptr: int, b_ptr: int, n_pairs: int, score_ptr: int, end_ptr: int,
                     match: int = 10, mismatch: int = -1, indel: int = INDEL_DEFAULT, band: int = -1,
                     stream: int = 0) -> None:
        """Asynchronous scoring with device pointers (e.g. torch tensors' data_ptr()) on `stream`."""
        check(self._L.ovl_score_device(self._ctx, ctypes.c_void_p(a_ptr), ctypes.c_void_p(b_ptr), int(n_pairs),
                                       match, mismatch, indel, band, ctypes.c_void_p(score_ptr),
                                       ctypes.c_void_p(end_ptr), ctypes.c_void_p(stream or None)), self._ctx)

    def score_tensors(self, a, b, out_score, out_end, match: int = 10, mismatch: int = -1,
                      indel: int = INDEL_DEFAULT, band: int = -1, stream=None) -> None:
        """torch int32 device tensors in/out, launched on torch's current stream (or `stream`)."""
        n, s = self._tensor_args("score_tensors", a, b, out_score, out_end, stream)
        self.score_device(a.data_ptr(), b.data_ptr(), n, out_score.data_ptr(), out_end.data_ptr(),
                          match, mismatch, indel, band, stream=s)

    def launcher(self, a, b, out_score, out_end, match: int = 10, mismatch: int = -1,
                 indel: int = INDEL_DEFAULT, band: int = -1, stream=None):
        """Pre-bound scoring launch for repeated steps over the same device buffers.

        Converts every argument to its ctypes form once, so each call costs one
        foreign call (the launch itself) instead of per-call tensor checks.
        The tensors must stay alive while the launcher is used.
        """
        n, s = self._tensor_args("launcher", a, b, out_score, out_end, stream)
        fn = self._L.ovl_score_device
        ctx = self._ctx
        args = (ctx, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), ctypes.c_int64(n),
                ctypes.c_int32(match), ctypes.c_int32(mismatch), ctypes.c_int64(indel), ctypes.c_int32(band),
                ctypes.c_void_p(out_score.data_ptr()), ctypes.c_void_p(out_end.data_ptr()),
                ctypes.c_void_p(s or None))
        check(self._L.ovl_plan(ctx, match, mismatch, indel, band, ctypes.byref(ctypes.c_int32())), ctx)

        def launch() -> None:
            rc = fn(*args)
            if rc:
                check(rc, ctx)
        return launch

    def check_device_errors(self) -> None:
        check(self._L.ovl_check_device_errors(self._ctx), self._ctx)

    def align_one(self, a: int, b: int, n: int, m: int, match: int = 10, mismatch: int = -1,
                  indel: int = INDEL_DEFAULT, traceback: bool = False):
        """One resident pair through the DP kernel; optionally the int8 traceback table."""
        sc, en = ctypes.c_int32(), ctypes.c_int32()
        tb = np.zeros((n + 1) * (m + 1), dtype=np.int8) if traceback else None
        check(self._L.ovl_align_one(self._ctx, a, b, match, mismatch, indel, ctypes.byref(sc), ctypes.byref(en),
                                    _ptr(tb) if tb is not None else None), self._ctx)
        if traceback:
            return sc.value, en.value, tb.reshape(n + 1, m + 1)
        return sc.value, en.value


_default: Optional[OverlapEngine] = None
_default_lock = threading.Lock()


def placement(count: int, env=None, pid: Optional[int] = None) -> Union[int, str, List[int]]:
    """Which device(s) the process-wide engine uses, given ``count`` visible devices.

    1. ``OVL_DEVICES``: "all" or a comma list -> one engine over several GPUs (single process);
    2. ``OVL_DEVICE``: that ordinal;
    3. ``LOCAL_RANK`` (torch.distributed.run and similar launchers): local_rank % count;
    4. otherwise the process id modulo count, so the reference's joblib workers
       (experiments.py:537, n_jobs=-1: one process each) spread over the visible GPUs.
    """
    env = os.environ if env is None else env
    if count <= 0:
        raise OvlError(-2, "no HIP device visible to libovl")
    many = env.get("OVL_DEVICES")
    if many:
        if many.strip().lower() == "all":
            return "all"
        ids = [int(x) for x in many.split(",") if x.strip()]
        if not ids or any(not 0 <= i < count for i in ids):
            raise OvlError(-1, f"OVL_DEVICES={many!r}: ordinals must lie in [0, {count})")
        return ids
    one = env.get("OVL_DEVICE")
    if one not in (None, ""):
        d = int(one)
        if not 0 <= d < count:
            raise OvlError(-1, f"OVL_DEVICE={d} outside [0, {count})")
        return d
    lr = env.get("LOCAL_RANK")
    if lr not in (None, ""):
        return int(lr) % count
    return (os.getpid() if pid is None else pid) % count


def default_engine() -> OverlapEngine:
    """Process-wide engine (created on first use) on the device(s) ``placement`` picks."""
    global _default
    with _default_lock:
        if _default is None:
            where = placement(device_count())
            if isinstance(where, int):
                _default = OverlapEngine(where)
            else:
                _default = OverlapEngine(devices=where)
        return _default


def score_reads(reads: Sequence[str], a_idx, b_idx, match: int = 10, mismatch: int = -1,
                indel: int = INDEL_DEFAULT, band: int = -1,
                engine: Optional[OverlapEngine] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Upload `reads` and score the pair list in one batch on the GPU."""
    eng = engine or default_engine()
    eng.set_reads(reads)
    return eng.score(a_idx, b_idx, match, mismatch, indel, band)
