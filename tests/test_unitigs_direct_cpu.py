"""The unitig pipeline from the score columns without a GPU: ovl_unitigs_host through ``assemble_contigs_direct`` and
``reduced_string_graph`` with oracle scores, against the reference's recorded results (tests/golden/unitigs.json) and
against ``assemble_contigs`` / ``transitive_reduction2(_string_graph(...))`` on raw lists with copies; the walk alone
(ovl_unitigs_walk_host) against ``find_unitigs`` on hand and random digraphs; and the host form's argument checks."""
import ctypes

import networkx as nx
import numpy as np
import pytest

from conftest import assert_graph_matches_record, load_golden
from ovlgraph import _lib
from ovlgraph import overlapGraphs as og
from ovlgraph.engine import encode_reads, last_unitigs_host, unitigs_host, unitigs_walk_host
from ovlgraph.unitigs import ReducedStringGraph, assemble_contigs_direct, reduced_string_graph
from unitig_graphs import hand_graph

R = ["ACGTACGGTC", "CGGTCTTAGA", "TTAGACCATG", "CCATGACGTA", "GGGGGCCCCC"]  # a chain, its wrap-around, a stranger


@pytest.fixture(scope="module")
def golden_unitigs():
    return load_golden("unitigs.json")


@pytest.fixture(scope="module")
def scorer(oracle_mod):
    return lambda reads, a, b: oracle_mod.batch_dp(reads, a, b)


def assert_same_graph(got, want):
    """Nodes, successor order, predecessor order and attributes."""
    assert list(got.nodes()) == list(want.nodes())
    assert [(u, v, dict(d)) for u, v, d in got.edges(data=True)] == [(u, v, dict(d)) for u, v, d in
                                                                      want.edges(data=True)]
    for node in want:
        assert list(got.pred[node]) == list(want.pred[node])
        assert list(got.succ[node]) == list(want.succ[node])


# ------------------------------------------------------------------ golden records
def test_read_sets_match_reference(golden_unitigs, scorer, capsys):
    for rec in golden_unitigs["reads"]:
        assert assemble_contigs_direct(rec["reads"], scorer=scorer, device=False) == rec["contigs"]
        red = reduced_string_graph(rec["reads"], scorer=scorer, device=False)
        assert isinstance(red, ReducedStringGraph)
        assert_graph_matches_record(red.to_digraph(), rec)
        assert red.n_edges == rec["graph_edges"]
        assert red.n_kept == len(rec["edges"]) == red.tail.shape[0]
        stats = last_unitigs_host()
        assert stats["edges"] == red.n_edges and stats["kept"] == red.n_kept
        assert stats["paths"] == len(rec["contigs"]) and stats["words_per_row"] == -(-len(red.nodes) // 64)
    assert capsys.readouterr().out == ""


# ------------------------------------------------------------------ raw lists with copies
DUPLICATE_LISTS = {
    "copy_before_the_other": [R[0], R[0], R[1], R[2]],
    "copy_after_the_other": [R[0], R[1], R[0], R[2]],
    "adjacent_copies_inside": [R[0], R[1], R[1], R[2], R[3]],
    "a_triple": [R[1], R[0], R[1], R[2], R[1], R[4]],
    "x_y_x": [R[0], R[1], R[0]],
    "copies_of_several": [R[2], R[0], R[1], R[2], R[0], R[3], R[4], R[4]],
    "copy_of_a_later_read_before_the_other": [R[1], R[0], R[0], R[2]],
    "copy_of_a_later_read_after_the_other": [R[1], R[0], R[2], R[0], R[3]],
    "empty": [],
    "single": [R[0]],
    "no_copies": list(R),
}


@pytest.mark.parametrize("name", list(DUPLICATE_LISTS))
def test_raw_lists_with_copies_match_the_graph_route(name, scorer):
    reads = DUPLICATE_LISTS[name]
    G = og._string_graph(reads, None, scorer)
    want = og.transitive_reduction2(G, device=False)
    red = reduced_string_graph(reads, scorer=scorer, device=False)
    assert_same_graph(red.to_digraph(), want)
    assert red.n_edges == G.number_of_edges() and red.n_kept == want.number_of_edges()
    try:
        contigs = og.assemble_contigs(reads, scorer=scorer, device=False)
    except ValueError as e:
        with pytest.raises(ValueError) as got:
            assemble_contigs_direct(reads, scorer=scorer, device=False)
        assert str(got.value) == str(e)
    else:
        assert assemble_contigs_direct(reads, scorer=scorer, device=False) == contigs


def test_the_lists_hold_self_loops_removed_edges_and_both_outcomes(scorer):
    """A copy of the list's first read puts its self-loop first, which removes every other successor and leaves the
    cycle that raises; a copy of a later read does not."""
    loops = removed = raised = spelled = 0
    for reads in DUPLICATE_LISTS.values():
        red = reduced_string_graph(reads, scorer=scorer, device=False)
        loops += int((red.tail == red.head).sum())
        removed += red.n_edges - red.n_kept
        raised += red.cycle_node >= 0
        spelled += red.cycle_node < 0 and len(set(reads)) < len(reads)
    assert loops >= 2 and removed >= 2 and raised >= 3 and spelled >= 3


def test_two_copies_of_one_read_raise_in_both_routes(scorer):
    reads = [R[0], R[0]]
    with pytest.raises(ValueError) as want:
        og.assemble_contigs(reads, scorer=scorer, device=False)
    with pytest.raises(ValueError) as got:
        assemble_contigs_direct(reads, scorer=scorer, device=False)
    assert str(got.value) == str(want.value) and repr(R[0]) in str(got.value)
    red = reduced_string_graph(reads, scorer=scorer, device=False)  # the graph itself is there: one self-loop
    assert red.cycle_node == 0 and red.n_kept == 1 and list(red.to_digraph().edges()) == [(R[0], R[0])]


# ------------------------------------------------------------------ the walk alone
def _walk_reference(G):
    """find_unitigs' paths as node lists, or the node its ValueError names.  Node strings of one character and
    end_position 0, so that a unitig spells its path."""
    H = nx.DiGraph()
    H.add_nodes_from(chr(0x100 + v) for v in G)
    H.add_edges_from((chr(0x100 + u), chr(0x100 + v), {"end_position": 0}) for u, v in G.edges())
    try:
        return [[ord(ch) - 0x100 for ch in unitig] for unitig in og.find_unitigs(H)], -1
    except ValueError:
        return None, 0


def _walk_native(G):
    nodes = list(G)
    index = {v: i for i, v in enumerate(nodes)}
    off, heads = og._csr_heads(nodes, G._adj)
    path_off, path_nodes, cyc = unitigs_walk_host(off, heads)
    if cyc >= 0:
        return None, nodes[cyc] if isinstance(nodes[cyc], int) else cyc
    assert sorted(path_nodes.tolist()) == list(range(len(nodes)))  # every node on exactly one path
    return [[nodes[i] for i in path_nodes[a:b]] for a, b in zip(path_off[:-1], path_off[1:])], -1


def test_walk_matches_find_unitigs_on_hand_graphs(golden_unitigs):
    seen_cycle = 0
    for rec in golden_unitigs["graphs"]:
        for which in ("edges", "reduced_edges"):
            G = nx.DiGraph()
            G.add_nodes_from(rec["nodes"])
            G.add_edges_from(rec[which])
            want, want_cyc = _walk_reference(G)
            got, cyc = _walk_native(G)
            assert (cyc >= 0) == (want_cyc >= 0), rec["name"]
            assert got == want, rec["name"]
            seen_cycle += cyc >= 0
    assert seen_cycle >= 1


def test_walk_matches_find_unitigs_on_random_digraphs():
    rng = np.random.default_rng(20261021)
    cycles = shared_terminals = 0
    for trial in range(3000):
        n = int(rng.integers(1, 13))
        order = rng.permutation(n).tolist()
        G = nx.DiGraph()
        G.add_nodes_from(order)
        m = rng.random((n, n)) < rng.choice([0.6, 1.0, 1.6]) / n
        for u in order:
            G.add_edges_from((u, int(v)) for v in rng.permutation(np.flatnonzero(m[u])))
        want, want_cyc = _walk_reference(G)
        got, cyc = _walk_native(G)
        assert (cyc >= 0) == (want_cyc >= 0), trial
        assert got == want, trial
        if cyc >= 0:
            cycles += 1
            # the node named lies on a cycle of nodes with one successor and one predecessor
            assert G.out_degree(cyc) == 1 and G.in_degree(cyc) == 1
            continue
        # a terminal (a node the walk cannot leave) that several chains of non-branching nodes run into
        chain = [v for v in G if G.out_degree(v) == 1 and G.in_degree(v) == 1]
        for t in G:
            if t not in chain and sum(1 for p in G.pred[t] if p in chain) >= 2:
                shared_terminals += 1
                break
    assert cycles >= 20 and shared_terminals >= 20


# ------------------------------------------------------------------ the host form's ABI
def _host_call(buf, offs, n, ids, n_raw, score, end, self_sc, self_en, outs, n_contigs=True, scalars=True):
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    nc, cyc = ctypes.c_int32(-7), ctypes.c_int32(-7)
    ne, nk = ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = _lib.load().ovl_unitigs_host(p(buf), p(offs), n, p(ids), n_raw, p(score), p(end), p(self_sc), p(self_en),
                                      *[p(o) for o in outs], ctypes.byref(nc) if n_contigs else None,
                                      ctypes.byref(ne), ctypes.byref(nk), ctypes.byref(cyc))
    return rc, (nc.value, ne.value, nk.value, cyc.value)


def _fresh_outputs(n, total):
    return [np.full(n + 1, -9, np.int64), np.full(max(n, 1), -9, np.int32), np.full(max(total, 1), 9, np.uint8),
            np.full(n + 1, -9, np.int64)]


def test_host_form_error_codes_leave_outputs_untouched(scorer):
    reads = [R[0], R[1], R[2]]
    buf, offs = encode_reads(reads)
    ids = np.array([0, 1, 1, 2], np.int32)
    x = np.repeat(np.arange(3, dtype=np.int32), 2)
    y = np.array([1, 2, 0, 2, 0, 1], np.int32)
    score, end = (np.ascontiguousarray(v, np.int32) for v in scorer(reads, x, y))
    self_sc, self_en = np.array([0, 100, 0], np.int32), np.array([0, 10, 0], np.int32)
    good = unitigs_host((buf, offs), ids, score, end, self_sc, self_en)
    assert good["n_edges"] >= 3 and good["cycle_node"] == -1 and good["path_nodes"].shape == (3,)
    bad_offs = offs.copy()
    bad_offs[1], bad_offs[2] = offs[2], offs[1]
    cases = [
        (dict(n=-1), -1), (dict(n_raw=-1), -1), (dict(offs=None), -1), (dict(ids=None), -1),
        (dict(offs=bad_offs), -1),                                 # offsets decrease
        (dict(n_raw=2), -1),                                       # fewer raw reads than distinct reads
        (dict(ids=np.array([0, 1, 3, 2], np.int32)), -7),          # an id outside [0, n)
        (dict(ids=np.array([0, -1, 1, 2], np.int32)), -7),
        (dict(ids=np.array([0, 2, 1, 2], np.int32)), -1),          # not numbered by first occurrence
        (dict(ids=np.array([1, 0, 1, 2], np.int32)), -1),
        (dict(ids=np.array([0, 1, 1, 1], np.int32)), -1),          # a distinct read never occurs
        (dict(score=None), -1), (dict(end=None), -1),
        (dict(self_sc=None), -1), (dict(self_en=None), -1),        # read 1 has two copies
        (dict(buf=None), -1),                                      # bases to spell and no bytes
    ]
    base = dict(buf=buf, offs=offs, n=3, ids=ids, n_raw=4, score=score, end=end, self_sc=self_sc, self_en=self_en)
    for change, want in cases:
        a = {**base, **change}
        outs = _fresh_outputs(3, int(offs[-1]))
        before = [o.copy() for o in outs]
        rc, scalars = _host_call(a["buf"], a["offs"], a["n"], a["ids"], a["n_raw"], a["score"], a["end"], a["self_sc"],
                                 a["self_en"], outs)
        assert rc == want, change
        assert scalars == (-7, -7, -7, -7), change
        assert all(np.array_equal(o, b) for o, b in zip(outs, before)), change
        assert _lib.last_error()
    outs = _fresh_outputs(3, int(offs[-1]))
    rc, _ = _host_call(buf, offs, 3, ids, 4, score, end, self_sc, self_en, outs, n_contigs=False)
    assert rc == -1 and outs[0][0] == -9
    # every output but n_contigs may be NULL, and without bases no bytes are needed
    rc, scalars = _host_call(None, offs, 3, ids, 4, score, end, self_sc, self_en, [None] * 4)
    assert rc == 0 and scalars == (good["n_contigs"], good["n_edges"], good["n_kept"], -1)
    # without a repeated read the self columns may be NULL
    rc, _ = _host_call(buf, offs, 3, np.arange(3, dtype=np.int32), 3, score, end, None, None, _fresh_outputs(3, 30))
    assert rc == 0
    # the cycle status writes the counts and the node, and nothing else
    one = encode_reads([R[0]])
    outs = _fresh_outputs(1, 10)
    rc, scalars = _host_call(*one, 1, np.zeros(2, np.int32), 2, None, None, np.array([100], np.int32),
                             np.array([10], np.int32), outs)
    assert rc == 1 and scalars == (-7, 1, 1, 0) and outs[0].tolist() == [-9, -9] and outs[2].tolist() == [9] * 10


def test_walk_entry_error_codes():
    L = _lib.load()
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    off, heads = np.array([0, 1, 2], np.int64), np.array([1, 2], np.int32)
    for o, h, n, want in ((off, heads, 2, -7), (np.array([0, 2, 1], np.int64), heads, 2, -1), (None, heads, 2, -1),
                          (off, None, 2, -1), (off, heads, -1, -1)):
        path_off, path_nodes = np.full(3, -9, np.int64), np.full(2, -9, np.int32)
        n_paths, cyc = ctypes.c_int32(-7), ctypes.c_int32(-7)
        rc = L.ovl_unitigs_walk_host(p(o), p(h), n, p(path_off), p(path_nodes), ctypes.byref(n_paths), ctypes.byref(cyc))
        assert rc == want and n_paths.value == -7 and cyc.value == -7
        assert path_off.tolist() == [-9] * 3 and path_nodes.tolist() == [-9] * 2
    assert L.ovl_unitigs_walk_host(p(off), p(np.array([1, 0], np.int32)), 2, None, None, None, None) == -1


def test_hand_walks():
    # only the path's last node is tested: node 1 has two predecessors, is appended, and ends the path
    G = nx.DiGraph()
    G.add_nodes_from(range(5))
    G.add_edges_from([(0, 1), (2, 1), (1, 3), (4, 0)])
    assert _walk_native(G) == ([[0, 1], [2], [3], [4]], -1)
    assert _walk_native(hand_graph({"n_nodes": 1, "edges": [(0, 0)]}))[1] == 0  # a lone self-loop


def test_host_check_program_under_sanitizers():
    """The host form as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
    import os
    import subprocess
    from ovlgraph._lib import CSRC
    out = subprocess.run(["make", "-s", "-C", CSRC, "unitigs-host-check"], capture_output=True, text=True)
    assert out.returncode == 0 and "unitigs_host_check: ok" in out.stdout, out.stdout + out.stderr
    assert os.path.exists(os.path.join(CSRC, "..", "build", "unitigs_host_check"))


def test_stage_block_check_program_under_sanitizers():
    """The carver of ovl_stage.h and the device blocks of the layout, the read correction and this pipeline, sized and
    then placed over host memory, as a stand-alone program under the same two sanitizers."""
    import subprocess
    from ovlgraph._lib import CSRC
    out = subprocess.run(["make", "-s", "-C", CSRC, "stage-block-check"], capture_output=True, text=True)
    assert out.returncode == 0 and "stage_block_check: ok" in out.stdout, out.stdout + out.stderr


def test_exported_from_package():
    import ovlgraph
    from ovlgraph import unitigs
    assert ovlgraph.assemble_contigs_direct is unitigs.assemble_contigs_direct
    assert ovlgraph.reduced_string_graph is unitigs.reduced_string_graph
    assert {"assemble_contigs_direct", "reduced_string_graph"} <= set(ovlgraph.__all__)
    assert og.UNITIGS_DEVICE_MIN_WORK > 2  # (its unit is distinct reads)


def test_default_routing_takes_the_host_form_without_a_gpu(scorer, monkeypatch):
    from ovlgraph import engine
    monkeypatch.setattr(engine, "device_count", lambda: 0)
    reads = DUPLICATE_LISTS["a_triple"]
    assert assemble_contigs_direct(reads, scorer=scorer) == og.assemble_contigs(reads, scorer=scorer, device=False)
