"""Reachability reduction on the GPU (ovl_reach_reduce, ovl_reach.hip) and the unitig pipeline on top of it, bit for
bit against the library's host form and the reference's recorded results.

The closure runs a pivot and an update launch per block of 64 nodes; the update gives a row to a lane group whose
width is the power of two that covers the row's words, the marking gives a node to one.  The shapes here have one
word per row, the word and pivot-block boundary (63, 64, 65, 127, 128, 129), several blocks with a ragged last one
(300), 18 words per row so that two rows share a wavefront (1,100), and 65 words, a second trip of a full
wavefront (4,160); with OVL_REACH_WINDOW the marking takes several column windows per node.
"""
import ctypes

import numpy as np
import pytest

from conftest import assert_graph_matches_record, load_golden
from unitig_graphs import (assert_hand_graph_matches, csr_from_lists, families, hand_graph, random_dag,
                           relabelled_chain)

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 300)


@pytest.fixture(scope="module")
def engine():
    from ovlgraph import OverlapEngine
    eng = OverlapEngine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def golden_unitigs():
    return load_golden("unitigs.json")


@pytest.fixture(scope="module")
def family_graphs():
    """(name, off, heads, host mask, host closure) of every family at every size."""
    from ovlgraph.engine import reach_reduce_host
    out = []
    for n in SIZES:
        for name, off, heads, _ in families(n, 2):
            out.append((name, off, heads) + reach_reduce_host(off, heads, closure=True))
    return out


@pytest.fixture(scope="module")
def large_graphs():
    """The chain family (diameter n) and the DAG at 0.05 at 1,100 nodes (18 words per row) and 4,160 (65 words)."""
    from ovlgraph.engine import reach_reduce_host
    out = []
    for n in (1100, 4160):
        rng = np.random.default_rng(n)
        for name, (off, heads) in ((f"chain_n{n}", relabelled_chain(rng, n)), (f"dag_n{n}", random_dag(rng, n, 0.05))):
            out.append((name, off, heads) + reach_reduce_host(off, heads, closure=True))
    return out


def assert_padding_is_zero(closure, n):
    if n % 64:
        assert not (closure[:, -1] >> np.uint64(n % 64)).any()


def test_families_match_host_form(engine, family_graphs):
    removed = 0
    for name, off, heads, want, want_closure in family_graphs:
        n = off.shape[0] - 1
        got, closure = engine.reach_reduce(off, heads, closure=True)
        assert np.array_equal(got, want), name
        assert closure.shape == (n, -(-n // 64)) and np.array_equal(closure, want_closure), name
        assert_padding_is_zero(closure, n)
        info = engine.last_reach()
        assert info["pivot_blocks"] == -(-n // 64) and info["words_per_row"] == -(-n // 64), name
        assert np.array_equal(engine.reach_reduce(off, heads), want), name  # without the closure output
        removed += int(got.sum())
    assert removed > 0


def test_rows_sharing_and_exceeding_a_wavefront(engine, large_graphs):
    for name, off, heads, want, want_closure in large_graphs:
        n = off.shape[0] - 1
        assert 0 < int(want.sum()) < want.shape[0], name
        got, closure = engine.reach_reduce(off, heads, closure=True)
        assert np.array_equal(got, want), name
        assert np.array_equal(closure, want_closure), name
        assert_padding_is_zero(closure, n)
        assert engine.last_reach()["words_per_row"] == {1100: 18, 4160: 65}[n]


def test_default_window_marking_forms(engine, family_graphs, large_graphs):
    """The default window (16,384 columns) on both forms of the marking: rows of up to 64 words -- every graph
    below 4,096 nodes, the form the string graphs take -- hold one word per lane with sixteen successor rows in
    flight; 65 words take four words per lane.  Long successor lists (the complete graph's 300, several trips of
    sixteen with a ragged last one) and short ones, against the host form."""
    seen = set()
    for name, off, heads, want, _ in family_graphs + large_graphs:
        n = off.shape[0] - 1
        if n not in (129, 300, 1100, 4160):
            continue
        got = engine.reach_reduce(off, heads)
        info = engine.last_reach()
        assert info["window_bits"] == 16384 and info["words_per_row"] == -(-n // 64), name
        assert np.array_equal(got, want), name
        seen.add(info["words_per_row"] <= 64)
    assert seen == {True, False}
    assert any(name == "complete_n300" and int(np.diff(off).max()) == 300 for name, off, *_ in family_graphs)


def test_out_degree_boundaries_in_one_graph(engine):
    """Out-degrees 0, 1, 2, 64, 65 and n in one graph: the marking's successor walk takes its boundary trip
    counts."""
    from ovlgraph.engine import reach_reduce_host
    n = 130
    rng = np.random.default_rng(7)
    succ = [rng.choice(n, size=int(rng.integers(0, 6)), replace=False) for _ in range(n)]
    for v, deg in ((3, 0), (10, 1), (20, 2), (64, 64), (65, 65), (129, n)):
        succ[v] = rng.choice(n, size=deg, replace=False)
    off, heads = csr_from_lists(rng, succ)
    assert {0, 1, 2, 64, 65, n} <= set(np.diff(off).tolist())
    want, want_closure = reach_reduce_host(off, heads, closure=True)
    assert 0 < int(want.sum()) < want.shape[0]
    got, closure = engine.reach_reduce(off, heads, closure=True)
    assert np.array_equal(got, want) and np.array_equal(closure, want_closure)


def test_several_windows_per_node(family_graphs, large_graphs, monkeypatch):
    from ovlgraph import OverlapEngine
    monkeypatch.setenv("OVL_REACH_WINDOW", "128")
    seen = 0
    with OverlapEngine(0) as eng:
        for name, off, heads, want, _ in family_graphs + large_graphs:
            if off.shape[0] - 1 not in (300, 1100):
                continue
            got = eng.reach_reduce(off, heads)
            assert eng.last_reach()["window_bits"] == 128, name
            assert np.array_equal(got, want), name
            seen += 1
    assert seen >= 9


def test_hand_graphs_match_reference(engine, golden_unitigs):
    from ovlgraph import overlapGraphs as og
    for rec in golden_unitigs["graphs"]:
        assert_hand_graph_matches(og.transitive_reduction2(hand_graph(rec), engine=engine, device=True), rec)


def test_read_sets_match_reference(engine, golden_unitigs, capsys):
    from ovlgraph import overlapGraphs as og
    for rec in golden_unitigs["reads"]:
        G = og.construct_string_graph(rec["reads"], engine=engine)
        assert G.number_of_edges() == rec["graph_edges"]
        R = og.transitive_reduction2(G, engine=engine, device=True)
        assert_graph_matches_record(R, rec)
        assert og.find_unitigs(R) == rec["unitigs"]
        capsys.readouterr()
        assert og.assemble_contigs(rec["reads"], engine=engine, device=True) == rec["contigs"]
        assert capsys.readouterr().out == ""


def test_string_graph_of_400_reads(engine):
    from ovlgraph import overlapGraphs as og
    from ovlgraph.engine import reach_reduce_host
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads
    reads = list(dict.fromkeys(simulate_reads(read_genome_from_fasta(), 60, 440, 0.01, seed=5)))[:400]
    assert len(reads) == 400
    G = og._string_graph(reads, engine, None)
    off, heads = og._csr_heads(list(G), G._adj)
    assert heads.shape[0] > 50_000
    want = reach_reduce_host(off, heads)
    assert 0 < int(want.sum()) < want.shape[0]
    assert np.array_equal(engine.reach_reduce(off, heads), want)


def test_error_codes_leave_outputs_untouched(engine):
    from ovlgraph import _lib
    L = _lib.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    off = np.array([0, 2, 3, 3], np.int64)
    heads = np.array([1, 2, 2], np.int32)
    cases = [
        (off, np.array([1, 3, 2], np.int32), 3, -7),            # head == n_nodes: OVL_E_INDEX
        (off, np.array([1, -1, 2], np.int32), 3, -7),           # a negative head
        (np.array([0, 2, 1, 3], np.int64), heads, 3, -1),       # a decreasing off: OVL_E_ARG
        (np.array([1, 2, 3, 3], np.int64), heads, 3, -1),       # off[0] != 0
        (off, heads, -1, -1),                                   # a negative node count
    ]
    for o, h, n_nodes, want in cases:
        reduced = np.full(3, 9, np.uint8)
        closure = np.full(3, 99, np.uint64)
        n = ctypes.c_int64(-7)
        rc = L.ovl_reach_reduce(engine._ctx, p(o), p(h), n_nodes, p(reduced), ctypes.byref(n), p(closure))
        assert rc == want and n.value == -7 and reduced.tolist() == [9, 9, 9] and closure.tolist() == [99, 99, 99]
    reduced = np.full(3, 9, np.uint8)
    n = ctypes.c_int64(-7)
    assert L.ovl_reach_reduce(engine._ctx, None, p(heads), 3, p(reduced), ctypes.byref(n), None) == -1
    assert L.ovl_reach_reduce(engine._ctx, p(off), None, 3, p(reduced), ctypes.byref(n), None) == -1
    assert n.value == -7 and reduced.tolist() == [9, 9, 9]
    mask, closure = engine.reach_reduce(off, heads, closure=True)
    assert mask.tolist() == [0, 1, 0] and closure[:, 0].tolist() == [0b110, 0b100, 0]


def test_buffers_reused_across_sizes(engine, family_graphs):
    """Larger then smaller on one engine: the smaller call's matrix has its own row width and clean padding."""
    by_name = {name: rest for name, *rest in family_graphs}
    for big, small in (("complete_n300", "chain_n65"), ("complete_n300", "digraph_c3_n63"),
                       ("complete_n129", "complete_n2")):
        off, heads, want, want_closure = by_name[big]
        assert np.array_equal(engine.reach_reduce(off, heads), want)
        off, heads, want, want_closure = by_name[small]
        got, closure = engine.reach_reduce(off, heads, closure=True)
        assert np.array_equal(got, want) and np.array_equal(closure, want_closure), small
        assert_padding_is_zero(closure, off.shape[0] - 1)


def test_timing_covers_a_calls_launches(engine):
    """Four nodes, one removable edge: 0 -> 2 goes, since 0's earlier successor 1 reaches 2."""
    from ovlgraph.engine import reach_reduce_host
    from stage_timing import assert_kernel_inside_call, timed_and_untimed
    off, heads = [0, 2, 3, 4, 4], [1, 2, 2, 3]
    got_on, on, got_off, off_t = timed_and_untimed(engine, lambda: engine.reach_reduce(off, heads), engine.last_reach)
    assert on["words_per_row"] == 1
    assert_kernel_inside_call(on, off_t)
    want = reach_reduce_host(off, heads)
    assert want.tolist() == [0, 1, 0, 0] and np.array_equal(got_on, want) and np.array_equal(got_off, want)
