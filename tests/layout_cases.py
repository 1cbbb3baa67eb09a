"""Shared small cases of the best-successor layout (ovlgraph/layout.py carries the rule), for test_layout_cpu.py and
test_gpu_layout.py: scored pair lists made by hand, each a few reads of 4 to 12 bases unless its name says otherwise,
and the helpers that compare two forms of the layout array for array and call the C ABI with raw pointers.

A case is ``Case(name, reads, a, b, score, end, min_score, min_overlap, expect)``; ``expect`` names what the case is
about as {array name: {read: value}}, checked against every form beside the form-to-form comparison.  The reads'
letters are random: the rule never compares bases, it concatenates them.
"""
import ctypes
import random
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name reads a b score end min_score min_overlap expect")

ARRAYS = ("succ", "link", "contig", "offset", "on_path")
COUNTS = ("links", "cycles", "on_path_reads")


def _reads(rng, n, lo=4, hi=12):
    return ["".join(rng.choice("ACGT") for _ in range(rng.randint(lo, hi))) for _ in range(n)]


def random_reads(n, seed, lo=16, hi=24):
    """n random ACGT reads of lo to hi bases."""
    return _reads(random.Random(seed), n, lo, hi)


def _case(name, reads, pairs, min_score=1, min_overlap=1, expect=None):
    cols = [[p[k] for p in pairs] for k in range(4)]
    return Case(name, reads, *cols, min_score, min_overlap, expect or {})


def _ring(lo, n, scores, end=2):
    return [(lo + i, lo + (i + 1) % n, scores[i], end) for i in range(n)]


def _one_read_with(rng, k, lead):
    """Read 0 with k pairs (its best score twice: the first of them wins), after `lead` pairs of read 1, so that the
    run starts inside a wavefront; k = 300 with lead = 37 crosses two wavefront boundaries and the block's."""
    reads = _reads(rng, k + 2)
    pairs = [(1, 2 + (i % k), 7, 2) for i in range(lead)]
    top = (2 * k) // 3
    for i in range(k):
        sc = 90 if i in (top, min(k - 1, top + 5)) else 10 + (i * 7) % 60
        pairs.append((0, 2 + i, sc, 3))
    return reads, pairs, lead + top


def build_cases():
    rng = random.Random(20261020)
    cases = []
    r = _reads(rng, 5)
    cases.append(_case("chain", r, [(i, i + 1, 30, 2) for i in range(4)],
                       expect={"succ": {0: 1, 3: 4, 4: -1}, "contig": {0: 0, 4: 0}, "on_path": {2: 1}}))
    r = _reads(rng, 4)
    cases.append(_case("score_tie_smallest_p", r, [(0, 3, 20, 2), (0, 1, 40, 2), (0, 2, 40, 2), (0, 3, 40, 2)],
                       expect={"link": {0: 1}, "succ": {0: 1}}))
    # every ineligibility on its own edge (read 1 is "ACGTAC": 6 bases)
    r = ["ACGTACGT", "ACGTAC", "TTTTT"]
    cases.append(_case("score_below_min", r, [(0, 1, 4, 2)], 5, 1, {"link": {0: -1}}))
    cases.append(_case("score_at_min", r, [(0, 1, 5, 2)], 5, 1, {"link": {0: 0}}))
    cases.append(_case("end_below_min_overlap", r, [(0, 1, 50, 2)], 1, 3, {"link": {0: -1}}))
    cases.append(_case("end_at_min_overlap", r, [(0, 1, 50, 3)], 1, 3, {"link": {0: 0}}))
    cases.append(_case("end_is_len_b", r, [(0, 1, 50, 6)], 1, 1, {"link": {0: -1}}))
    cases.append(_case("end_is_len_b_minus_1", r, [(0, 1, 50, 5)], 1, 1, {"link": {0: 0}, "offset": {1: 3}}))
    cases.append(_case("a_equals_b", r, [(0, 0, 90, 2), (0, 1, 10, 2)], 1, 1, {"link": {0: 1}}))
    cases.append(_case("a_equals_b_only", r, [(2, 2, 90, 2)], 1, 1, {"link": {2: -1}}))
    # negative scores under a negative min_score: the key's bias orders them; -9 is below the bound
    r = _reads(rng, 4)
    cases.append(_case("negative_scores", r, [(0, 1, -5, 2), (0, 2, -3, 2), (0, 3, -9, 2), (1, 2, -9, 2),
                                              (2, 3, -(2 ** 31), 2), (3, 0, 2 ** 31 - 1, 2)], -6, 1,
                       {"link": {0: 1, 1: -1, 2: -1, 3: 5}}))
    for n in (2, 3, 5, 100):
        r = _reads(rng, n)
        sc = [50 + (i * 37) % 41 for i in range(n)]
        sc[n // 2] = 7  # the weakest link
        cases.append(_case(f"cycle_{n}", r, _ring(0, n, sc), expect={"succ": {n // 2: -1}, "contig": {0: 0}}))
    r = _reads(rng, 80)
    pairs = _ring(0, 10, [60, 61, 62, 9, 64, 65, 66, 67, 68, 69]) + [(10 + i, 11 + i, 30, 2) for i in range(69)]
    pairs.append((79, 5, 30, 2))
    cases.append(_case("cycle_with_70_tail", r, pairs, expect={"succ": {3: -1, 79: 5}, "on_path": {10: 1, 3: 1}}))
    r = _reads(rng, 9)
    cases.append(_case("two_cycles", r, _ring(0, 4, [30, 20, 40, 50]) + _ring(4, 5, [9, 8, 7, 6, 5]),
                       expect={"succ": {1: -1, 8: -1}}))
    r = _reads(rng, 6)
    cases.append(_case("cycle_tie_greatest_p", r, _ring(0, 6, [25] * 6), expect={"succ": {5: -1, 4: 5}}))
    # the same ring listed backwards: the greatest p is now read 0's pair
    cases.append(_case("cycle_tie_greatest_p_reversed", r, list(reversed(_ring(0, 6, [25] * 6))),
                       expect={"succ": {0: -1, 5: 0}}))
    r = _reads(rng, 130)
    cases.append(_case("chain_130", r, [(i, i + 1, 30 + i % 7, 1 + i % 3) for i in range(129)],
                       expect={"succ": {128: 129}, "offset": {0: 0}}))
    r = _reads(rng, 200)
    cases.append(_case("star_200", r, [(i, 199, 10 + i % 50, 2) for i in range(199)], expect={"succ": {0: 199}}))
    for k, lead in ((1, 0), (64, 0), (65, 37), (300, 37)):
        r, pairs, best = _one_read_with(rng, k, lead)
        cases.append(_case(f"one_read_{k}_pairs", r, pairs, expect={"link": {0: best}}))
        if k == 300:
            order = list(range(len(pairs)))
            random.Random(7).shuffle(order)
            shuffled = [pairs[i] for i in order]
            # read 0's two best pairs tie: the one that now stands first in the list wins, under its new number
            first = min(order.index(best), order.index(best + 5))
            cases.append(_case("one_read_300_pairs_shuffled", r, shuffled,
                               expect={"link": {0: first}, "succ": {0: shuffled[first][1]}}))
    # two leaves of equal span into one read: the smaller index heads
    r = ["ACGTAC", "TTGGCC", "ACGTACGT"]
    cases.append(_case("span_tie", r, [(1, 2, 30, 3), (0, 2, 30, 3)], expect={"on_path": {0: 1, 1: 0}, "offset": {1: 0}}))
    r = [("ACGT" * 3)[:n] for n in (4, 12, 5, 11, 6, 10, 7, 9, 8)]
    cases.append(_case("variable_lengths", r, [(i, i + 1, 20, 1 + i % 3) for i in range(8)] + [(8, 0, 5, 3)]))
    cases.append(_case("no_pairs", _reads(rng, 4), [], expect={"contig": {0: 0, 3: 3}, "on_path": {2: 1}}))
    cases.append(_case("one_read", ["ACGTAC"], [], expect={"succ": {0: -1}, "offset": {0: 0}}))
    cases.append(_case("one_read_one_self_pair", ["ACGTAC"], [(0, 0, 50, 2)], expect={"succ": {0: -1}}))
    cases.append(_case("no_reads", [], []))
    for seed in (1, 2, 3):
        g = random.Random(seed)
        r = _reads(g, 300)
        pairs = [(g.randrange(300), g.randrange(300), g.randint(0, 5), g.randint(0, 13)) for _ in range(3000)]
        cases.append(_case(f"random_{seed}", r, pairs, 1, 1))
    return cases


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}


def case_args(c):
    return (c.reads, np.asarray(c.a, np.int32), np.asarray(c.b, np.int32), np.asarray(c.score, np.int64).astype(np.int32),
            np.asarray(c.end, np.int32), c.min_score, c.min_overlap)


def with_contigs(res):
    """A native form's result with ``contigs`` (list of str) from its bytes."""
    from ovlgraph.layout import _with_contigs
    return _with_contigs(res) if "contigs" not in res else res


def assert_same(got, want, what=""):
    """Two forms of one layout: array for array, contig for contig, count for count."""
    for k in ARRAYS:
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(np.asarray(got[k]) != np.asarray(want[k]))[:8])
        assert got[k].dtype == want[k].dtype, (what, k)
    assert list(got["contigs"]) == list(want["contigs"]), (what, "contigs")
    assert got["n_contigs"] == want["n_contigs"] == len(want["contigs"]), what
    for k in COUNTS:
        assert got[k] == want[k], (what, k, got[k], want[k])


def assert_expect(c, res):
    for name, at in c.expect.items():
        for r, v in at.items():
            assert int(res[name][r]) == v, (c.name, name, r, int(res[name][r]), v)


def spell(reads, res, end):
    """The contigs spelled again in Python from succ / link: per contig from its head (the one read on its path with
    offset 0), along succ."""
    succ, link = res["succ"].tolist(), res["link"].tolist()
    heads = {}
    for r in range(len(reads)):
        if res["on_path"][r] and res["offset"][r] == 0:
            heads[int(res["contig"][r])] = r
    out = []
    for c in range(res["n_contigs"]):
        x = heads[c]
        text = reads[x]
        while succ[x] >= 0:
            text += reads[succ[x]][end[link[x]]:]
            x = succ[x]
        out.append(text)
    return out


# ----------------------------------------------------------------------------- the C ABI with raw pointers
SENTINEL = 77


class RawCall:
    """One call of ovl_layout_host (ctx None) or ovl_layout (ctx given) with sentinel-filled outputs;
    ``untouched()`` tells whether the call wrote nothing."""

    def __init__(self, reads, a, b, score, end):
        from ovlgraph.engine import encode_reads
        self.buf, self.offs = encode_reads(reads)
        self.n = len(reads)
        self.cols = [np.ascontiguousarray(x, dtype=np.int32) for x in (a, b, score, end)]
        total = int(self.offs[-1])
        self.i32 = [np.full(max(self.n, 1), SENTINEL, np.int32) for _ in range(4)]
        self.on_path = np.full(max(self.n, 1), SENTINEL, np.uint8)
        self.bases = np.full(max(total, 1), SENTINEL, np.uint8)
        self.c_off = np.full(self.n + 1, SENTINEL, np.int64)
        self.nc = ctypes.c_int32(SENTINEL)

    def __call__(self, ctx=None, lib=None, n_reads=None, n_pairs=None, min_score=1, min_overlap=1, null=(),
                 offsets=None):
        from ovlgraph import _lib
        L = lib or _lib.load()
        p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
        offs = self.offs if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
        self._keep = offs
        named = {"seqs": p(self.buf), "offsets": p(offs), "a": p(self.cols[0]), "b": p(self.cols[1]),
                 "score": p(self.cols[2]), "end": p(self.cols[3]), "n_contigs": ctypes.byref(self.nc)}
        for k in null:
            named[k] = None
        args = [named["seqs"], named["offsets"], self.n if n_reads is None else n_reads, named["a"], named["b"],
                named["score"], named["end"], self.cols[0].shape[0] if n_pairs is None else n_pairs, min_score,
                min_overlap, *[p(o) for o in self.i32], p(self.on_path), p(self.bases), p(self.c_off),
                named["n_contigs"]]
        if ctx is None:
            return L.ovl_layout_host(*args)
        return L.ovl_layout(ctx, *args)

    def untouched(self):
        return (all((o == SENTINEL).all() for o in self.i32) and (self.on_path == SENTINEL).all()
                and (self.bases == SENTINEL).all() and (self.c_off == SENTINEL).all() and self.nc.value == SENTINEL)


# (what, keyword arguments of RawCall.__call__, the code): every argument check of the layout entry points
def bad_calls(n_reads=3):
    return [
        ("n_contigs NULL", {"null": ("n_contigs",)}, -1),
        ("offsets NULL", {"null": ("offsets",)}, -1),
        ("a NULL", {"null": ("a",)}, -1),
        ("b NULL", {"null": ("b",)}, -1),
        ("score NULL", {"null": ("score",)}, -1),
        ("end NULL", {"null": ("end",)}, -1),
        ("seqs NULL", {"null": ("seqs",)}, -1),
        ("n_reads < 0", {"n_reads": -1}, -1),
        ("n_pairs < 0", {"n_pairs": -1}, -1),
        ("offsets decrease", {"offsets": [0, 8, 6, 19]}, -1),
        ("min_overlap 0", {"min_overlap": 0}, -1),
        ("n_pairs 2^31", {"n_pairs": 2 ** 31}, -4),
        ("sum len 2^31", {"offsets": [0, 8, 14, 2 ** 31]}, -4),
    ]
