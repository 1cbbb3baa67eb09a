"""The unitig pipeline without a GPU: transitive_reduction2 through the library's host form, find_unitigs and
assemble_contigs with oracle scores, against the reference's own results (tests/golden/unitigs.json, written by
tools/gen_golden_unitigs.py from overlapGraphs.py:354-412), and the host form against a dense closure."""
import ctypes

import networkx as nx
import numpy as np
import pytest

from conftest import assert_graph_matches_record, load_golden
from ovlgraph import _lib
from ovlgraph import overlapGraphs as og
from ovlgraph.engine import reach_reduce_host
from unitig_graphs import assert_hand_graph_matches, dense_reference, families, hand_graph, literal_loop

SIZES = (1, 2, 3, 8, 63, 64, 65, 129, 300)


@pytest.fixture(scope="module")
def golden_unitigs():
    return load_golden("unitigs.json")


def _oracle_scorer(oracle_mod):
    return lambda reads, a, b: oracle_mod.batch_dp(reads, a, b)


# ------------------------------------------------------------------ golden records
def test_golden_records_cover_the_edge_cases(golden_unitigs):
    recs = golden_unitigs["graphs"]
    assert len(recs) >= 38 and 7 <= len(golden_unitigs["reads"]) <= 10
    names = {r["name"] for r in recs}
    assert {"self_loop_first", "self_loop_last", "two_cycle", "diamond", "chain_shortcut_after",
            "chain_shortcut_before", "sinks_and_isolated", "shuffled_insertion"} <= names
    assert any(len(r["reduced_edges"]) not in (0, len(r["edges"])) for r in recs)

    def copy_reorders(r):  # the surviving edges' predecessor order is not the input's
        alive = {(u, v) for u, v in r["reduced_edges"]}
        kept = [[p for p in preds if (p, n) in alive] for n, preds in zip(r["nodes"], r["input_pred"])]
        return kept != r["pred"]
    assert any(copy_reorders(r) for r in recs)
    sets = golden_unitigs["reads"]
    assert sum(r["cyclic"] for r in sets) >= 2 and sum(not r["cyclic"] for r in sets) >= 2


def test_hand_graphs_match_reference(golden_unitigs):
    for rec in golden_unitigs["graphs"]:
        G = hand_graph(rec)
        for u, v in G.edges():
            G[u][v]["tag"] = [u, v]
        before = [(u, v, dict(d)) for u, v, d in G.edges(data=True)]
        pred_before = {n: list(G.pred[n]) for n in G}
        R = og.transitive_reduction2(G, device=False)
        assert_hand_graph_matches(R, rec)
        # the input is untouched and shares no attribute dict with the result
        assert R is not G and [(u, v, dict(d)) for u, v, d in G.edges(data=True)] == before
        assert {n: list(G.pred[n]) for n in G} == pred_before
        assert all(R[u][v] is not G[u][v] and R[u][v] == G[u][v] for u, v in R.edges())


def test_hashable_nodes_and_python_removal_path(golden_unitigs):
    """Tuple nodes, and a DiGraph subclass (which takes networkx's own remove_edges_from)."""
    class Sub(nx.DiGraph):
        pass
    for rec in golden_unitigs["graphs"][:20]:
        want = og.transitive_reduction2(hand_graph(rec), device=False)
        G = Sub()
        G.add_nodes_from((i, "x") for i in range(rec["n_nodes"]))
        G.add_edges_from(((u, "x"), (v, "x")) for u, v in rec["edges"])
        R = og.transitive_reduction2(G, device=False)
        assert type(R) is Sub
        assert [(f"n{u[0]}", f"n{v[0]}") for u, v in R.edges()] == list(want.edges())
        assert [[f"n{p[0]}" for p in R.pred[n]] for n in R] == [list(want.pred[n]) for n in want]


def _reduced(rec, oracle_mod, capsys):
    G = og.construct_string_graph(rec["reads"], scorer=_oracle_scorer(oracle_mod))
    assert capsys.readouterr().out.startswith("graph: [")  # called directly it keeps its line
    assert G.number_of_edges() == rec["graph_edges"]
    return G, og.transitive_reduction2(G, device=False)


def test_read_sets_match_reference(golden_unitigs, oracle_mod, capsys):
    for rec in golden_unitigs["reads"]:
        G, R = _reduced(rec, oracle_mod, capsys)
        assert_graph_matches_record(R, rec)
        assert G.number_of_edges() == rec["graph_edges"]
        assert og.find_unitigs(R) == rec["unitigs"]
    assert capsys.readouterr().out == ""


def test_contigs_match_reference(golden_unitigs, oracle_mod, capsys):
    for rec in golden_unitigs["reads"]:
        contigs = og.assemble_contigs(rec["reads"], scorer=_oracle_scorer(oracle_mod), device=False)
        assert contigs == rec["contigs"]
    assert capsys.readouterr().out == ""
    rec = golden_unitigs["reads"][0]
    og.assemble_contigs(rec["reads"], scorer=_oracle_scorer(oracle_mod), device=False, verbose=True)
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 1 and out[0].startswith("graph: [")


def test_exported_from_package():
    import ovlgraph
    assert ovlgraph.transitive_reduction2 is og.transitive_reduction2
    assert ovlgraph.find_unitigs is og.find_unitigs
    assert ovlgraph.assemble_contigs is og.assemble_contigs
    assert {"transitive_reduction2", "find_unitigs", "assemble_contigs"} <= set(ovlgraph.__all__)


# ------------------------------------------------------------------ host form
@pytest.mark.parametrize("n", SIZES)
def test_host_form_matches_dense_closure(n):
    for name, off, heads, _ in families(n, 1):
        mask, closure = reach_reduce_host(off, heads, closure=True)
        want_mask, want_closure = dense_reference(off, heads)
        assert np.array_equal(mask, want_mask), name
        assert closure.shape == want_closure.shape and np.array_equal(closure, want_closure), name
        assert np.array_equal(reach_reduce_host(off, heads), mask), name  # without the closure output


@pytest.mark.parametrize("n", [n for n in SIZES if n >= 2])
def test_families_mix_kept_and_removed_edges(n):
    """0 < removed < edges for the c >= 1.5, DAG and chain families, so the comparisons above are not vacuous: at
    every size from which the family can hold a removable edge (unitig_graphs.families says which and why; one node
    has one self-loop at most, and a first successor always stays)."""
    asserted = 0
    for name, off, heads, mix_from in families(n, 1):
        if mix_from is not None and n >= mix_from:
            mask = reach_reduce_host(off, heads)
            assert 0 < int(mask.sum()) < mask.shape[0], name
            asserted += 1
    assert asserted >= 2


@pytest.mark.parametrize("n", (1, 2, 3, 8, 30))
def test_literal_has_path_loop_matches_host_form(n):
    for seed in (1, 2, 3):
        for name, off, heads, _ in families(n, seed):
            assert np.array_equal(reach_reduce_host(off, heads), literal_loop(off, heads)), name


def test_repeated_head_gets_the_positional_rule():
    # 0 -> [1, 1, 2, 2], 1 -> [1], 2 -> []: the second (0, 1) goes because 1 reaches 1; the first (0, 2) stays, no
    # earlier entry reaches 2; the second (0, 2) stays too: R[2][2] is false
    off = np.array([0, 4, 5, 5], np.int64)
    heads = np.array([1, 1, 2, 2, 1], np.int32)
    assert reach_reduce_host(off, heads).tolist() == [0, 1, 0, 0, 0]
    # 1 -> [2] as well: now 1 reaches 2 and both (0, 2) entries go
    off = np.array([0, 4, 6, 6], np.int64)
    heads = np.array([1, 1, 2, 2, 1, 2], np.int32)
    assert reach_reduce_host(off, heads).tolist() == [0, 1, 1, 1, 0, 1]


def _call_host(off, heads, n_nodes, reduced, closure):
    n = ctypes.c_int64(-7)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
    rc = _lib.load().ovl_reach_reduce_host(p(off), p(heads), n_nodes, p(reduced), ctypes.byref(n), p(closure))
    return rc, n.value


def test_host_form_error_codes():
    off = np.array([0, 2, 3, 3], np.int64)
    heads = np.array([1, 2, 2], np.int32)
    reduced = np.full(3, 9, np.uint8)
    closure = np.full(3, 99, np.uint64)
    assert _call_host(off, heads, 3, reduced, closure) == (0, 1) and reduced.tolist() == [0, 1, 0]
    assert closure.tolist() == [0b110, 0b100, 0]
    cases = [
        (np.array([0, 2, 1, 3], np.int64), heads, 3, -1),   # off decreases
        (np.array([1, 2, 3, 3], np.int64), heads, 3, -1),   # off[0] != 0
        (off, heads, -1, -1),                               # negative size
        (off, np.array([1, 3, 2], np.int32), 3, -7),        # head == n_nodes
        (off, np.array([1, -1, 2], np.int32), 3, -7),       # negative head
        (None, heads, 3, -1),                               # null off
        (off, None, 3, -1),                                 # null head
    ]
    for o, h, n, want in cases:
        reduced = np.full(3, 9, np.uint8)
        closure = np.full(3, 99, np.uint64)
        rc, count = _call_host(o, h, n, reduced, closure)
        assert rc == want and count == -7 and reduced.tolist() == [9, 9, 9] and closure.tolist() == [99, 99, 99]
        assert _lib.last_error()
    closure = np.full(3, 99, np.uint64)
    assert _call_host(off, heads, 3, None, closure) == (-1, -7) and closure.tolist() == [99, 99, 99]  # null reduced
    L = _lib.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert L.ovl_reach_reduce_host(p(off), p(heads), 3, p(reduced), None, None) == -1  # null n_reduced
    # an empty graph and a graph without edges
    assert reach_reduce_host(np.zeros(1, np.int64), np.zeros(0, np.int32)).shape == (0,)
    mask, closure = reach_reduce_host(np.zeros(4, np.int64), np.zeros(0, np.int32), closure=True)
    assert mask.shape == (0,) and closure.shape == (3, 1) and not closure.any()


# ------------------------------------------------------------------ Python stages
def test_graph_without_weights_and_default_routing():
    """No edge attribute is read, and device=None takes the host form on a small graph (no GPU is visible to the
    CPU suite)."""
    G = nx.DiGraph()
    G.add_edges_from([("a", "b"), ("b", "c"), ("a", "c"), ("c", "d")])
    R = og.transitive_reduction2(G)
    assert list(R.edges()) == [("a", "b"), ("b", "c"), ("c", "d")]
    assert all(d == {} for _, _, d in R.edges(data=True))
    assert og.REACH_DEVICE_MIN_WORK > 4  # (its unit is nodes)


def _walk_graph(edges):
    G = nx.DiGraph()
    for u, v in edges:
        G.add_edge(u, v, end_position=1)
    return G


def test_find_unitigs_raises_where_the_reference_never_returns():
    with pytest.raises(ValueError, match="'AC'"):
        og.find_unitigs(_walk_graph([("AC", "AC")]))
    with pytest.raises(ValueError, match="'AC'"):
        og.find_unitigs(_walk_graph([("AC", "CA"), ("CA", "AC")]))
    # a self-loop whose node has a second edge: two successors, the walk stops at once
    assert og.find_unitigs(_walk_graph([("AC", "AC"), ("AC", "CG")])) == ["AC", "CG"]


def test_find_unitigs_appends_a_node_with_several_predecessors():
    # only the path's last node is tested: CG has two predecessors, is appended, and ends the path
    G = _walk_graph([("AC", "CG"), ("TC", "CG"), ("CG", "GT")])
    G.add_edge("XA", "AC", end_position=1)
    assert list(G.nodes()) == ["AC", "CG", "TC", "GT", "XA"]
    assert og.find_unitigs(G) == ["ACG", "TC", "GT", "XA"]
