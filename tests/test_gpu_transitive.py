"""Transitive reduction on the GPU (ovl_transitive_reduce, ovl_reduce.hip) and the string pipeline on top of it,
bit for bit against the library's host loop and the reference's recorded results.

The kernel gives a node to a workgroup of 512 threads: the threads stride over the node's edges to fill, write
and reset a window of its out-row in LDS, and lane groups share the node's successors and stride over each
successor's list.  The shapes here have out-degrees below, at and above a wavefront, above the workgroup's lane
groups and above its 512 threads (so the fill and the write / reset loops take a second and a third trip), one
node and one window, and (with OVL_TR_WINDOW) several windows per node.
"""
import ctypes
from collections import Counter

import networkx as nx
import numpy as np
import pytest

from conftest import assert_graph_matches_record, load_golden
from test_transitive_cpu import assert_hand_graph_matches, hand_graph, random_csr

pytestmark = pytest.mark.gpu

BIG = 2 ** 30 - 1


@pytest.fixture(scope="module")
def engine():
    from ovlgraph import OverlapEngine
    eng = OverlapEngine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def golden_string():
    return load_golden("string_graph.json")


@pytest.fixture(scope="module")
def random_graphs():
    """(name, off, heads, weights, host mask): every size and density, small weights (ties), mixed signs and the
    widest weights; isolated nodes and self-loops come with the densities."""
    from ovlgraph.engine import transitive_reduce_host
    rng = np.random.default_rng(300)
    out = []
    for n in (1, 2, 63, 64, 65, 300):
        for density in (0.05, 0.5, 1.0):
            for lo, hi in ((0, 3), (-40, 400), (-BIG, BIG)):
                off, heads, weights = random_csr(rng, n, density, lo, hi)
                if weights.shape[0] >= 2 and hi == BIG:
                    weights[0], weights[-1] = BIG, -BIG
                out.append((f"n{n}_d{density}_w{hi}", off, heads, weights, transitive_reduce_host(off, heads, weights)))
    return out


@pytest.fixture(scope="module")
def wide_graphs():
    """Nodes with more out-edges than the workgroup has threads, so that the fill and the write / reset loops take
    a second trip (complete graphs of 600 nodes, self-loops included) and a third (1,100 nodes, the first eight
    pointing at every node, the others at 5 %).  The weights are mostly negative, so that a sum of two reaches only
    the more negative direct edges and the masks mix kept and removed edges."""
    from ovlgraph.engine import transitive_reduce_host
    rng = np.random.default_rng(512)
    out = []
    for n, density, full, lo, hi in ((600, 1.0, 0, -BIG, -1), (600, 1.0, 0, -400, 40), (1100, 0.05, 8, -400, -1),
                                     (1100, 0.05, 8, -BIG, 40)):
        off, heads, weights = random_csr(rng, n, density, lo, hi, full_rows=full)
        out.append((f"n{n}_d{density}_w{lo}", off, heads, weights, transitive_reduce_host(off, heads, weights)))
    return out


def test_out_degree_above_workgroup_threads(engine, wide_graphs):
    for name, off, heads, weights, want in wide_graphs:
        assert int(np.diff(off).max()) == off.shape[0] - 1 > 512 and 0 < int(want.sum()) < want.shape[0], name
        got = engine.transitive_reduce(off, heads, weights)
        assert np.array_equal(got, want), name
        assert engine.last_transitive()["passes"] == 1


def test_out_degree_above_workgroup_threads_several_windows(wide_graphs, monkeypatch):
    from ovlgraph import OverlapEngine
    monkeypatch.setenv("OVL_TR_WINDOW", "64")
    with OverlapEngine(0) as eng:
        for name, off, heads, weights, want in wide_graphs:
            got = eng.transitive_reduce(off, heads, weights)
            info = eng.last_transitive()
            assert info["window"] == 64 and info["passes"] == -(-(off.shape[0] - 1) // 64), info
            assert np.array_equal(got, want), name


def test_random_graphs_match_host_form(engine, random_graphs):
    removed = 0
    for name, off, heads, weights, want in random_graphs:
        got = engine.transitive_reduce(off, heads, weights)
        assert np.array_equal(got, want), name
        info = engine.last_transitive()
        assert info["passes"] == 1 and info["two_hop_steps"] == int(np.diff(off)[heads].sum()), name
        removed += int(got.sum())
    assert removed > 0
    deg = max(int(np.diff(off).max()) for _, off, _, _, _ in random_graphs)
    assert deg >= 299  # above a wavefront and above a workgroup's lane groups (above its threads: wide_graphs)


def test_several_windows_per_node(random_graphs, monkeypatch):
    from ovlgraph import OverlapEngine
    monkeypatch.setenv("OVL_TR_WINDOW", "64")
    with OverlapEngine(0) as eng:
        for name, off, heads, weights, want in random_graphs:
            if off.shape[0] - 1 != 300:
                continue
            got = eng.transitive_reduce(off, heads, weights)
            info = eng.last_transitive()
            assert info["window"] == 64 and info["passes"] >= 5, info
            assert np.array_equal(got, want), name


def test_hand_graphs_match_reference(engine, golden_string):
    from ovlgraph import overlapGraphs as og
    for rec in golden_string["graphs"]:
        assert_hand_graph_matches(og.transitive_reduction(hand_graph(rec), engine=engine, device=True), rec)


def test_read_sets_match_reference(engine, golden_string):
    from ovlgraph import overlapGraphs as og
    for rec in golden_string["reads"]:
        G, copies = og.construct_overlap_graph_string(rec["reads"], engine=engine)
        R = og.transitive_reduction(G, engine=engine, device=True)
        assert_graph_matches_record(R, rec, copies)
        assert og.assemble_contigs_string(rec["reads"], engine=engine, device=True) == rec["contigs"]


def _phix_reads(n_reads, length, p, seed):
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads
    return simulate_reads(read_genome_from_fasta(), length, n_reads, p, seed=seed)


def test_string_graph_of_400_reads(engine):
    from ovlgraph import overlapGraphs as og
    from ovlgraph.engine import transitive_reduce_host
    reads = list(dict.fromkeys(_phix_reads(440, 60, 0.01, 5)))[:400]
    assert len(reads) == 400
    G, _ = og.construct_overlap_graph_string(reads, engine=engine)
    off, heads, weights = G.__dict__["_ovl_edges"].csr()
    assert heads.shape[0] > 150_000
    got = engine.transitive_reduce(off, heads, weights)
    steps = int(np.diff(off)[heads].sum())
    assert steps > 5 * 10 ** 7 and engine.last_transitive()["two_hop_steps"] == steps
    assert np.array_equal(got, transitive_reduce_host(off, heads, weights))


def test_k_filtered_graph_passed_lazy(engine):
    from ovlgraph import overlapGraphs as og
    reads = _phix_reads(2000, 100, 0.01, 9)
    G, _ = og.construct_overlap_graph_nx_k(reads, k=5, engine=engine)
    assert isinstance(G, og.LazyOverlapDiGraph) and not G.is_materialised
    R = og.transitive_reduction(G, engine=engine, device=True)
    H = og.transitive_reduction(G, device=False)
    assert not G.is_materialised and type(R) is nx.DiGraph
    assert 0 < R.number_of_edges() < G.number_of_edges()
    assert list(R.nodes()) == list(H.nodes()) and list(R.edges(data=True)) == list(H.edges(data=True))
    assert all(list(R.pred[n]) == list(H.pred[n]) for n in R)
    # and what the plain path makes of the same graph (G.copy() and removals): the lazy build's predecessor order
    # is the copy's, read copies included
    assert max(Counter(reads).values()) > 1
    P = og.transitive_reduction(nx.DiGraph(G), device=False)
    assert list(R.nodes()) == list(P.nodes()) and list(R.edges(data=True)) == list(P.edges(data=True))
    assert all(list(R.pred[n]) == list(P.pred[n]) for n in R)


def test_error_codes_leave_reduced_untouched(engine):
    from ovlgraph import _lib
    L = _lib.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    off = np.array([0, 2, 3, 3], np.int64)
    heads = np.array([1, 2, 2], np.int32)
    weights = np.array([1, 5, 4], np.int64)
    cases = [
        (off, np.array([1, 3, 2], np.int32), weights, -7),            # a bad head: OVL_E_INDEX
        (off, heads, np.array([1, 2 ** 30, 4], np.int64), -5),        # a weight of 2^30: OVL_E_RANGE
        (np.array([0, 2, 1, 3], np.int64), heads, weights, -1),       # a decreasing off: OVL_E_ARG
    ]
    for o, h, w, want in cases:
        reduced = np.full(3, 9, np.uint8)
        n = ctypes.c_int64(-7)
        rc = L.ovl_transitive_reduce(engine._ctx, p(o), p(h), p(w), 3, p(reduced), ctypes.byref(n))
        assert rc == want and n.value == -7 and reduced.tolist() == [9, 9, 9]
    assert engine.transitive_reduce(off, heads, weights).tolist() == [0, 1, 0]


def test_timing_covers_the_reduction_kernel(engine):
    """Four nodes, one two-hop path (0 -> 1 -> 2) beside the edge it removes."""
    from ovlgraph.engine import transitive_reduce_host
    from stage_timing import assert_kernel_inside_call, timed_and_untimed
    off, heads, weights = [0, 2, 3, 4, 4], [1, 2, 2, 3], [3, 5, 4, 1]
    got_on, on, got_off, off_t = timed_and_untimed(engine, lambda: engine.transitive_reduce(off, heads, weights),
                                                   engine.last_transitive)
    assert on["two_hop_steps"] == 3
    assert_kernel_inside_call(on, off_t)
    want = transitive_reduce_host(off, heads, weights)
    assert want.sum() >= 1 and np.array_equal(got_on, want) and np.array_equal(got_off, want)
