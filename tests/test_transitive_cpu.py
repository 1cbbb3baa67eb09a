"""The string pipeline without a GPU: transitive_reduction through the library's host loop and
assemble_contigs_string with oracle scores, against the reference's own results (tests/golden/string_graph.json,
written by tools/gen_golden_string.py from overlapGraphs.py:235-329)."""
import ctypes

import networkx as nx
import numpy as np
import pytest

from conftest import assert_graph_matches_record, load_golden
from ovlgraph import _lib
from ovlgraph import overlapGraphs as og
from ovlgraph.engine import transitive_reduce_host


@pytest.fixture(scope="module")
def golden_string():
    return load_golden("string_graph.json")


def _oracle_scorer(oracle_mod):
    return lambda reads, a, b: oracle_mod.batch_dp(reads, a, b)


def hand_graph(rec):
    G = nx.DiGraph()
    G.add_nodes_from(f"n{i}" for i in range(rec["n_nodes"]))
    for u, v, w in rec["edges"]:
        G.add_edge(f"n{u}", f"n{v}", weight=w)
    return G


def assert_hand_graph_matches(R, rec):
    assert list(R.nodes()) == [f"n{i}" for i in rec["nodes"]]
    got = []
    for u, v, d in R.edges(data=True):
        assert list(d.keys()) == ["weight"] and type(d["weight"]) is int
        got.append((u, v, d["weight"]))
    assert got == [(f"n{u}", f"n{v}", w) for u, v, w in rec["reduced_edges"]]
    for node, preds in zip(R.nodes(), rec["pred"]):
        assert list(R.pred[node]) == [f"n{p}" for p in preds]


def closed_form(off, heads, weights):
    """reduced[e] for e = (v, x): some w in succ(v) has (w, x) with weight(v, w) + weight(w, x) >= weight(v, x),
    evaluated on dense matrices."""
    n = off.shape[0] - 1
    has = np.zeros((n, n), bool)
    wt = np.zeros((n, n), np.int64)
    tails = np.repeat(np.arange(n), np.diff(off))
    has[tails, heads] = True
    wt[tails, heads] = weights
    out = np.zeros(heads.shape[0], np.uint8)
    for e, (v, x) in enumerate(zip(tails.tolist(), heads.tolist())):
        via = has[v, :] & has[:, x]
        out[e] = bool(np.any(via & (wt[v, :] + wt[:, x] >= wt[v, x])))
    return out


def random_csr(rng, n, density, lo, hi, self_loops=True, full_rows=0):
    """A random CSR graph (successors in shuffled order); the first ``full_rows`` nodes point at every node."""
    m = rng.random((n, n)) < density
    m[:full_rows, :] = True
    if not self_loops:
        np.fill_diagonal(m, False)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(m.sum(axis=1), out=off[1:])
    heads = np.concatenate([rng.permutation(np.flatnonzero(row)) for row in m] or [np.zeros(0, np.int64)])
    weights = rng.integers(lo, hi + 1, size=heads.shape[0], dtype=np.int64)
    return off, heads.astype(np.int32), weights


def test_golden_records_cover_the_edge_cases(golden_string):
    recs = golden_string["graphs"]
    assert len(recs) >= 40 and 8 <= len(golden_string["reads"]) <= 12
    loops = [(w, r) for r in recs for u, v, w in r["edges"] if u == v]
    assert any(w >= 0 for w, _ in loops) and any(w < 0 for w, _ in loops)
    assert any(w == 0 for r in recs for _, _, w in r["edges"]) and any(w < 0 for r in recs for _, _, w in r["edges"])

    def copy_reorders(r):  # the surviving edges' predecessor order is not the input's
        alive = {(u, v) for u, v, _ in r["reduced_edges"]}
        kept = [[p for p in preds if (p, n) in alive] for n, preds in zip(r["nodes"], r["input_pred"])]
        return kept != r["pred"]
    assert any(copy_reorders(r) for r in recs)
    assert any(len({u for u, _, _ in r["edges"]}) < r["n_nodes"] for r in recs)
    assert any(len(r["reduced_edges"]) not in (0, len(r["edges"])) for r in recs)


def test_hand_graphs_match_reference(golden_string):
    for rec in golden_string["graphs"]:
        G = hand_graph(rec)
        before = [(u, v, dict(d)) for u, v, d in G.edges(data=True)]
        pred_before = {n: list(G.pred[n]) for n in G}
        R = og.transitive_reduction(G, device=False)
        assert_hand_graph_matches(R, rec)
        # the input is untouched and shares no attribute dict with the result
        assert R is not G and [(u, v, dict(d)) for u, v, d in G.edges(data=True)] == before
        assert {n: list(G.pred[n]) for n in G} == pred_before
        assert all(R[u][v] is not G[u][v] for u, v in R.edges())


def test_hand_graphs_python_csr_path(golden_string):
    """A DiGraph subclass takes the Python CSR and removal passes."""
    class Sub(nx.DiGraph):
        pass
    for rec in golden_string["graphs"][:20]:
        G = Sub(hand_graph(rec))
        R = og.transitive_reduction(G, device=False)
        assert type(R) is Sub
        want = og.transitive_reduction(hand_graph(rec), device=False)
        assert list(R.edges(data=True)) == list(want.edges(data=True))
        assert [list(R.pred[n]) for n in R] == [list(want.pred[n]) for n in want]


def test_read_sets_match_reference(golden_string, oracle_mod):
    for rec in golden_string["reads"]:
        G, copies = og.construct_overlap_graph_string(rec["reads"], scorer=_oracle_scorer(oracle_mod))
        assert G.number_of_edges() == rec["overlap_edges"]
        lazy = isinstance(G, og.LazyOverlapDiGraph)
        R = og.transitive_reduction(G, device=False)
        if lazy:
            assert not G.is_materialised and type(R) is nx.DiGraph  # the input is still columns
        assert_graph_matches_record(R, rec, copies)
        assert G.number_of_edges() == rec["overlap_edges"]
        # the same through the materialised graph (G.copy() and removals)
        P = nx.DiGraph(G)
        R2 = og.transitive_reduction(P, device=False)
        assert_graph_matches_record(R2, rec, copies)
        assert P.number_of_edges() == rec["overlap_edges"]


def test_k_filtered_lazy_graph_matches_plain_path(golden_graphs, oracle_mod):
    """A k-filtered graph with read copies, still lazy, against the plain path on its materialised copy (G.copy()
    and removals): same edges, same predecessor order."""
    seen = 0
    for rec in golden_graphs["graphs"]:
        if rec["fn"] != "construct_overlap_graph_nx_k" or len(rec["reads"]) > 100:
            continue
        G, copies = og.construct_overlap_graph_nx_k(rec["reads"], scorer=_oracle_scorer(oracle_mod), **rec["kwargs"])
        assert isinstance(G, og.LazyOverlapDiGraph) and max(copies.values()) > 1
        R = og.transitive_reduction(G, device=False)
        assert not G.is_materialised
        P = og.transitive_reduction(nx.DiGraph(G), device=False)
        assert list(R.nodes()) == list(P.nodes()) and list(R.edges(data=True)) == list(P.edges(data=True))
        assert [list(R.pred[n]) for n in R] == [list(P.pred[n]) for n in P]
        seen += R.number_of_edges() < G.number_of_edges()
    assert seen >= 1  # (not vacuous: edges were removed, survivors' predecessor lists compared)


def test_contigs_match_reference(golden_string, oracle_mod, capsys):
    for rec in golden_string["reads"]:
        contigs = og.assemble_contigs_string(rec["reads"], scorer=_oracle_scorer(oracle_mod), device=False)
        assert contigs == rec["contigs"]
    assert capsys.readouterr().out == ""
    rec = golden_string["reads"][0]
    og.assemble_contigs_string(rec["reads"], scorer=_oracle_scorer(oracle_mod), device=False, verbose=True)
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 2 and out[0].startswith("overlap_graph: [") and out[1].startswith("reduced_graph: [")


def test_exported_from_package():
    import ovlgraph
    assert ovlgraph.transitive_reduction is og.transitive_reduction
    assert ovlgraph.assemble_contigs_string is og.assemble_contigs_string


def test_host_form_matches_closed_form():
    rng = np.random.default_rng(20261019)
    total = removed = 0
    for n in (1, 2, 3, 5, 8, 13, 30, 64):
        for density in (0.1, 0.5, 1.0):
            for lo, hi in ((1, 12), (-3, 6), (0, 2), (-(2 ** 30) + 1, 2 ** 30 - 1)):
                off, heads, weights = random_csr(rng, n, density, lo, hi)
                got = transitive_reduce_host(off, heads, weights)
                assert np.array_equal(got, closed_form(off, heads, weights))
                total += got.shape[0]
                removed += int(got.sum())
    assert 0 < removed < total


def test_default_routing_takes_host_form_for_small_graphs(golden_string):
    """device=None: a handful of two-hop paths never reaches for a GPU (none is visible to the CPU suite)."""
    rec = golden_string["graphs"][0]
    assert_hand_graph_matches(og.transitive_reduction(hand_graph(rec)), rec)


def test_weight_must_be_integer():
    G = nx.DiGraph()
    G.add_edge("a", "b", weight=1.5)
    with pytest.raises(TypeError):
        og.transitive_reduction(G, device=False)
    G = nx.DiGraph()
    G.add_edge("a", "b", weight=True)
    with pytest.raises(TypeError):
        og.transitive_reduction(G, device=False)


def _call_host(off, heads, weights, n_nodes, reduced):
    n = ctypes.c_int64(-7)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = _lib.load().ovl_transitive_reduce_host(p(off), p(heads), p(weights), n_nodes, p(reduced), ctypes.byref(n))
    return rc, n.value


def test_host_form_error_codes():
    off = np.array([0, 2, 3, 3], np.int64)
    heads = np.array([1, 2, 2], np.int32)
    weights = np.array([1, 5, 4], np.int64)
    reduced = np.full(3, 9, np.uint8)
    assert _call_host(off, heads, weights, 3, reduced) == (0, 1) and reduced.tolist() == [0, 1, 0]
    cases = [
        (np.array([0, 2, 1, 3], np.int64), heads, weights, 3, -1),   # off decreases
        (np.array([1, 2, 3, 3], np.int64), heads, weights, 3, -1),   # off[0] != 0
        (off, heads, weights, -1, -1),                               # negative size
        (off, np.array([1, 3, 2], np.int32), weights, 3, -7),        # head == n_nodes
        (off, np.array([1, -1, 2], np.int32), weights, 3, -7),       # negative head
        (off, heads, np.array([1, 2 ** 30, 4], np.int64), 3, -5),    # weight 2^30
        (off, heads, np.array([1, 5, -(2 ** 30)], np.int64), 3, -5),  # weight -2^30
    ]
    for o, h, w, n, want in cases:
        reduced = np.full(3, 9, np.uint8)
        rc, count = _call_host(o, h, w, n, reduced)
        assert rc == want and count == -7 and reduced.tolist() == [9, 9, 9]
        assert _lib.last_error()
    L = _lib.load()
    n = ctypes.c_int64(0)
    assert L.ovl_transitive_reduce_host(None, None, None, 0, None, ctypes.byref(n)) == -1
    # the widest accepted weights: sums of two stay exact
    big = 2 ** 30 - 1
    got = transitive_reduce_host(off, heads, np.array([big, big, big], np.int64))
    assert got.tolist() == [0, 1, 0]
    got = transitive_reduce_host(off, heads, np.array([-big, -big, -big], np.int64))
    assert got.tolist() == [0, 0, 0]
    # an empty graph and a graph without edges
    assert transitive_reduce_host(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64)).shape == (0,)
    assert transitive_reduce_host(np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64)).shape == (0,)
