"""The three dict builders of ``ovlgraph._digraph`` (csrc/ovl_digraph.c; no GPU) called directly, on graphs of a few
dozen nodes: ``build`` (edge arrays), ``build_overlap`` (pair columns and an alive mask) and ``build_overlap_stream``
(pair columns, the cycle replay beside it) return the same ``node`` / ``succ`` / ``pred`` dicts in the same key
order; the shared attribute template is taken or replaced by the same rule; every error exit raises what it raised
before and leaves nothing held.  What ``test_lazy_graph_cpu.py`` pins through networkx views is not repeated here."""
import ctypes
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

from ovlgraph import _lib
from ovlgraph import overlapGraphs as og

INT_LO, INT_HI = -4096, 8192  # the builders' cache of attribute ints covers [INT_LO, INT_HI)
PLAIN = {"weight": 1, "end_position": 2}


def _mod():
    mod = og._digraph()
    assert mod is not None, "ovlgraph._digraph is not built"
    return mod


def _replay_fn():
    return ctypes.cast(_lib.load().ovl_remove_cycles_stream, ctypes.c_void_p).value


class Case:
    """Pair columns over reads with copy counts, their node names, and the expanded edges in insertion order
    (pair, copy of a, copy of b) with each edge's CSR index."""

    def __init__(self, counts, a, b, score, end, keep=None):
        self.counts = np.asarray(counts, np.int32)
        self.a, self.b = np.asarray(a, np.int32), np.asarray(b, np.int32)
        self.score, self.end = np.asarray(score, np.int32), np.asarray(end, np.int32)
        self.keep = None if keep is None else np.asarray(keep, np.uint8)
        self.names = [f"r{r}_{c}" for r, n in enumerate(self.counts) for c in range(n)]
        self.off, self.heads, self.w = (np.frombuffer(x, dt) for x, dt in zip(
            _mod().overlap_csr(self.counts, self.a, self.b, self.score, self.keep), (np.int64, np.int32, np.int64)))
        self.n_edges = int(self.off[-1])
        self.heads, self.w = self.heads[:self.n_edges].copy(), self.w[:self.n_edges].copy()
        first = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        rowlen = np.zeros(len(self.counts), np.int64)
        u, v, wt, en, idx = [], [], [], [], []
        for p in range(len(self.a)):
            if self.keep is not None and not self.keep[p]:
                continue
            ra, rb = int(self.a[p]), int(self.b[p])
            for ca in range(self.counts[ra]):
                for cb in range(self.counts[rb]):
                    u.append(first[ra] + ca)
                    v.append(first[rb] + cb)
                    wt.append(self.score[p])
                    en.append(self.end[p])
                    idx.append(self.off[first[ra] + ca] + rowlen[ra] + cb)
            rowlen[ra] += self.counts[rb]
        self.u, self.v = np.asarray(u, np.int64), np.asarray(v, np.int64)
        self.wt, self.en = np.asarray(wt, np.int32), np.asarray(en, np.int32)
        self.idx = np.asarray(idx, np.int64)
        assert len(self.idx) == self.n_edges and sorted(idx) == list(range(self.n_edges))

    def columns(self):
        return (self.names, self.counts, self.a, self.b, self.score, self.end)

    def stream(self, shared=None, **repl):
        c = dict(off=self.off, heads=self.heads, w=self.w, names=self.names, score=self.score, end=self.end)
        c.update(repl)
        return _mod().build_overlap_stream(c["names"], self.counts, self.a, self.b, c["score"], c["end"], self.keep,
                                           shared, _replay_fn(), c["off"], c["heads"], c["w"])

    def overlap(self, alive, *shared):
        return _mod().build_overlap(*self.columns(), self.keep, alive, *shared)

    def edges(self, alive, *shared):
        k = np.ones(self.n_edges, bool) if alive is None else alive[self.idx].astype(bool)
        return _mod().build(self.names, self.u[k], self.v[k], self.wt[k], self.en[k], *shared)


def _random_case(seed, reads=12, pairs=40, max_copies=3, keep_share=None, lo=1, hi=9):
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, max_copies + 1, reads)
    a = rng.integers(0, reads, pairs)
    b = (a + rng.integers(1, reads, pairs)) % reads  # (no pair of a read with itself)
    keep = None if keep_share is None else rng.random(pairs) < keep_share
    return Case(counts, a, b, rng.integers(lo, hi, pairs), rng.integers(0, 99, pairs), keep)


def _case_copies():
    c = _random_case(1)
    assert c.counts.max() > 1
    return c


def _case_keep():
    c = _random_case(2, keep_share=0.6)
    assert 0 < c.keep.sum() < len(c.keep)
    return c


def _case_same_b_twice():
    """read 0's kept pairs name read 1 twice, with other attributes: the later pair's dict replaces the earlier
    one's in place (the streamed builder then owns the references it keeps per edge)"""
    return Case([2, 2, 1, 2], [0, 2, 0, 1, 0, 3], [1, 0, 1, 3, 2, 0], [5, 3, 7, 4, 6, 2], [10, 11, 12, 13, 14, 15])


def _case_int_cache_edges():
    vals = [INT_LO - 1, INT_LO, INT_LO + 1, INT_HI - 2, INT_HI - 1, INT_HI]
    n = len(vals)
    return Case([2] * (n + 1), range(n), range(1, n + 1), vals, vals[::-1])  # (a chain: every edge survives)


def _case_empty():
    z = np.zeros(0, np.int32)
    return Case(z, z, z, z, z)


CASES = {"copies": _case_copies, "keep": _case_keep, "same_b_twice": _case_same_b_twice,
         "int_cache_edges": _case_int_cache_edges, "empty": _case_empty}


def _assert_same(got, want):
    for g, w in zip(got[:3], want[:3]):  # node, succ, pred
        assert list(g) == list(w) and g == w
        for name in w:
            assert list(g[name]) == list(w[name])
    for (_, succ, pred) in (got[:3], want[:3]):
        for u, row in succ.items():
            for v, d in row.items():
                assert d is pred[v][u] and list(d) == ["weight", "end_position"]
                assert type(d["weight"]) is int and type(d["end_position"]) is int


def _three(case, shared=None):
    """The streamed result, and the two other builders' for the replay's alive mask; all three must agree."""
    node, succ, pred, rem, n_rem = case.stream(shared)
    alive = np.ones(case.n_edges, np.uint8)
    alive[np.frombuffer(rem, np.int64)[:n_rem]] = 0
    extra = () if shared is None else (shared,)
    by_cols, by_edges = case.overlap(alive, *extra), case.edges(alive, *extra)
    _assert_same(by_cols, (node, succ, pred))
    _assert_same(by_edges, (node, succ, pred))
    assert sum(len(r) for r in succ.values()) == sum(len(r) for r in pred.values()) <= int(alive.sum())
    return node, succ, pred, alive


def _agree_on_every_case():
    for make in CASES.values():
        case = make()
        _, succ, _, alive = _three(case, og._attr_template())
        if case.n_edges:  # all alive, and an alive mask of the caller's, through the two serial builders
            _assert_same(case.overlap(None), case.edges(None))
            mask = (np.arange(case.n_edges) % 3 != 0).astype(np.uint8)
            _assert_same(case.overlap(mask), case.edges(mask))
    c = _case_copies()
    assert (_three(c)[3] == 0).any()  # (the random cases do hold cycles: the alive mask drops edges)
    c = _case_int_cache_edges()  # (the values themselves, not only that the builders agree on them)
    succ = _three(c)[1]
    for p in range(len(c.a)):
        for d in succ[f"r{c.a[p]}_1"].values():
            assert (d["weight"], d["end_position"]) == (int(c.score[p]), int(c.end[p]))
    assert _three(_case_empty())[:3] == ({}, {}, {})


def test_builders_agree():
    _agree_on_every_case()


@pytest.mark.parametrize("scc", ["0", "1", "2"])
def test_builders_agree_in_each_helper_mode(scc):
    """OVL_STREAM_SCC is read from the environment by each streamed call: a fresh child process per setting."""
    code = ("import sys; sys.path[:0] = %r\n"
            "import test_digraph_builders_cpu as t\n"
            "t._agree_on_every_case(); print('agree')\n") % [os.path.dirname(os.path.abspath(__file__)),
                                                             os.path.dirname(os.path.dirname(og.__file__))]
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OVL_STREAM_SCC=scc), capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "agree", out.stderr


def _attr_dicts(result):
    return [d for row in result[1].values() for d in row.values()]


def test_shared_template_rule():
    """A dict of exactly the two keys is the template (a key-sharing one keeps its key table in every attribute
    dict); anything else -- other keys, None, nothing -- is replaced by a fresh template with equal results."""
    case = _case_copies()
    want = _three(case)[:3]
    split = og._attr_template()
    for shared in (split, dict(PLAIN), {"weight": None, "other": None}, {"weight": 0, "end_position": 0, "x": 0}):
        before = dict(shared)
        got = _three(case, shared)[:3]
        _assert_same(got, want)
        assert shared == before  # (the template itself is only copied)
    alive = _three(case)[3]
    taken = [case.stream(split), case.overlap(alive, split), case.edges(alive, split)]
    fresh = [case.stream(None), case.overlap(alive), case.edges(alive), case.stream({"weight": None, "other": None})]
    if sys.getsizeof(split.copy()) < sys.getsizeof(dict(PLAIN)):  # (this CPython copies a split table as one)
        for r in taken:
            assert {sys.getsizeof(d) for d in _attr_dicts(r)} == {sys.getsizeof(split.copy())}
    for r in fresh:
        assert {sys.getsizeof(d) for d in _attr_dicts(r)} == {sys.getsizeof(dict(PLAIN))}
    for call in (lambda: case.overlap(alive, None), lambda: case.edges(alive, None)):
        with pytest.raises(TypeError):  # (their optional argument is a dict or absent)
            call()


def _errors(case):
    """(name, call, exception type, message) of every error exit"""
    short = case.score[:-1].copy()
    alive = np.ones(case.n_edges, np.uint8)
    tmpl = og._attr_template()
    m = _mod()
    n = len(case.names)
    extra_node = np.concatenate([case.off, case.off[-1:]])  # a CSR of its own, of one node more
    per_pair = "score and end must have one entry per pair"
    no_match = "names / CSR do not match the columns' graph"
    return tmpl, [
        ("overlap score", lambda: m.build_overlap(case.names, case.counts, case.a, case.b, short, case.end, case.keep,
                                                  alive, tmpl), ValueError, per_pair),
        ("overlap end", lambda: m.build_overlap(case.names, case.counts, case.a, case.b, case.score, short, case.keep,
                                                alive, tmpl), ValueError, per_pair),
        ("overlap names", lambda: m.build_overlap(case.names[:-1], case.counts, case.a, case.b, case.score, case.end,
                                                  case.keep, alive, tmpl), ValueError, f"{n - 1} names for {n} nodes"),
        ("overlap alive", lambda: case.overlap(alive[:-1].copy(), tmpl), ValueError,
         "alive must have one entry per edge"),
        ("stream score", lambda: case.stream(tmpl, score=short), ValueError, per_pair),
        ("stream end", lambda: case.stream(tmpl, end=short), ValueError, per_pair),
        ("stream names", lambda: case.stream(tmpl, names=case.names[:-1]), ValueError, no_match),
        ("stream csr", lambda: case.stream(tmpl, off=extra_node), ValueError, no_match),  # (the replay has started)
        ("edges end", lambda: m.build(case.names, case.u, case.v, case.wt, case.en[:-1].copy(), tmpl), ValueError,
         "u, v, weight and end must have the same length"),
        ("edges names", lambda: m.build(case.names[:-1], case.u, case.v, case.wt, case.en, tmpl), IndexError,
         f"node id outside [0, {n - 1})"),
    ]


def test_error_exits():
    case = _case_copies()
    assert (case.v == len(case.names) - 1).any()  # (so that a names list one short is noticed by build)
    tmpl, errors = _errors(case)
    for name, call, exc, text in errors:
        with pytest.raises(exc) as info:
            call()
        assert text in str(info.value), name
        if exc is ValueError:
            assert str(info.value) == text, name
    _three(case, tmpl)  # a valid call on the same inputs after them: nothing was left held or running


def _holds_nothing(call, watched):
    """`call` (its result dropped, its exception caught) changes no reference count of `watched` and, repeated 50
    times, leaves the collector's object count where it was."""
    def once():
        try:
            call()
        except (ValueError, IndexError):
            pass
    once()  # (first use: interned keys, the builder's import of gc)
    gc.collect()
    refs = [sys.getrefcount(x) for x in watched]
    once()
    gc.collect()
    assert [sys.getrefcount(x) for x in watched] == refs
    n0 = len(gc.get_objects())
    for _ in range(50):
        once()
    gc.collect()
    assert len(gc.get_objects()) == n0
    assert [sys.getrefcount(x) for x in watched] == refs


ERROR_EXITS = ["overlap score", "overlap end", "overlap names", "overlap alive", "stream score", "stream end",
               "stream names", "stream csr", "edges end", "edges names"]
SUCCESS_EXITS = ["stream", "overlap masked", "edges masked", "overlap", "edges", "stream same_b_twice",
                 "stream other keys"]
_leak_state = []


def _leak_calls():
    """One case for every parameter of the test below: a small int that the edges carry as score and end position
    (one of CPython's own shared ints, so its reference count can be read), the template, and every call."""
    if not _leak_state:
        small = 201
        rng = np.random.default_rng(3)
        a = rng.integers(0, 12, 40)
        case = Case(rng.integers(1, 4, 12), a, (a + rng.integers(1, 12, 40)) % 12,
                    np.where(np.arange(40) % 2, small, rng.integers(1, 9, 40)), np.full(40, small))
        tmpl, errors = _errors(case)
        assert [e[0] for e in errors] == ERROR_EXITS
        alive = _three(case, tmpl)[3]
        assert (alive == 0).any()
        dup = _case_same_b_twice()  # (the streamed builder's owned-reference path)
        calls = dict(zip(SUCCESS_EXITS, (
            lambda: case.stream(tmpl), lambda: case.overlap(alive, tmpl), lambda: case.edges(alive, tmpl),
            lambda: case.overlap(None), lambda: case.edges(None), lambda: dup.stream(tmpl),
            lambda: case.stream({"weight": None, "other": None}))))
        calls.update((e[0], e[1]) for e in errors)
        _leak_state.append((calls, [tmpl, case.names[0], case.names[-1], small]))
    return _leak_state[0]


@pytest.mark.parametrize("which", SUCCESS_EXITS + ERROR_EXITS)
def test_no_leaked_references(which):
    """Success and every error exit of each builder: the shared template, a name string and a small int that the
    edges carry are referenced afterwards exactly as before, and no object stays behind."""
    calls, watched = _leak_calls()
    gc_was = gc.isenabled()
    gc.disable()  # (only the explicit collections of _holds_nothing)
    try:
        _holds_nothing(calls[which], watched)
    finally:
        if gc_was:
            gc.enable()
