"""The unitig pipeline from the score columns on the GPU (ovl_unitigs, ovl_unitigs_candidates; ovl_unitigs.hip and the
launches of ovl_reach.hip on the resident CSR), element for element against the library's host form, and against
``assemble_contigs`` and the reference's recorded results.

A wavefront walks a row's raw positions 64 at a time, and the matrix has one word per 64 nodes: the raw lists here have
1, 2, 3, 63, 64, 65, 129 and 300 reads with copies inserted, so that a row ends inside, at and past a trip and the
distinct count stands on both sides of the word boundary; the 400-read set has rows of seven trips and seven words."""
import ctypes

import numpy as np
import pytest

from conftest import assert_graph_matches_record, load_golden

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 63, 64, 65, 129, 300)
ARRAYS = ("path_off", "path_nodes", "bases", "c_off", "tail", "head", "weight", "end_position")
SCALARS = ("n_edges", "n_kept", "cycle_node", "edges", "kept", "paths", "words_per_row")


@pytest.fixture(scope="module")
def engine():
    from ovlgraph import OverlapEngine
    eng = OverlapEngine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def golden_unitigs():
    return load_golden("unitigs.json")


def raw_list(n_raw, length=40, seed=3):
    """The first n_raw of 300 PhiX reads; every third position from the third on is a copy of an earlier read other
    than the first (a copy of the first read puts its self-loop first and always leaves the cycle that raises)."""
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads
    raw = simulate_reads(read_genome_from_fasta(), length, 300, 0.01, seed=seed)[:n_raw]
    for j in range(2, n_raw, 3):
        raw[j] = raw[1 + (j * 5) % (j - 1)]
    return raw


@pytest.fixture(scope="module")
def raw_lists(engine):
    """(raw reads, the host form's result over columns scored by the engine) per size."""
    from ovlgraph.unitigs import _run
    out = {}
    for n_raw in SIZES:
        raw = raw_list(n_raw)
        out[n_raw] = (raw, _run(raw, engine, None, False, None)[1])
    return out


def engine_scorer(engine):
    from ovlgraph import overlapGraphs as og
    return lambda distinct, a, b: og._score(distinct, a, b, engine)


def assert_same_result(got, want, what):
    for key in SCALARS:
        assert got[key] == want[key], (what, key)
    if want["cycle_node"] >= 0:
        assert "bases" not in got and "bases" not in want, what
    for key in ARRAYS:
        if key in want:
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (what, key)


def contigs_or_error(fn):
    try:
        return fn()
    except ValueError as e:
        return str(e)


def test_golden_read_sets_through_both_device_calls(engine, golden_unitigs, capsys):
    from ovlgraph.unitigs import assemble_contigs_direct, reduced_string_graph
    for rec in golden_unitigs["reads"]:
        for scorer in (None, engine_scorer(engine)):  # ovl_unitigs_candidates, then ovl_unitigs over uploaded columns
            assert assemble_contigs_direct(rec["reads"], engine, scorer, device=True) == rec["contigs"]
            red = reduced_string_graph(rec["reads"], engine, scorer, device=True)
            assert_graph_matches_record(red.to_digraph(), rec)
            assert red.n_edges == rec["graph_edges"] and red.n_kept == len(rec["edges"])
            stats = engine.last_unitigs()
            assert stats["edges"] == red.n_edges and stats["kept"] == red.n_kept
            assert stats["paths"] == len(rec["contigs"]) and stats["words_per_row"] == -(-len(red.nodes) // 64)
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("n_raw", SIZES)
def test_raw_lists_match_the_host_form_and_the_graph_route(engine, raw_lists, n_raw):
    from ovlgraph import overlapGraphs as og
    from ovlgraph.unitigs import _run, assemble_contigs_direct
    raw, want = raw_lists[n_raw]
    assert n_raw < 3 or len(set(raw)) < len(raw)
    assert_same_result(_run(raw, engine, None, True, None)[1], want, "ovl_unitigs_candidates")
    assert_same_result(_run(raw, engine, engine_scorer(engine), True, None)[1], want, "ovl_unitigs")
    assert contigs_or_error(lambda: assemble_contigs_direct(raw, engine, device=True)) == \
        contigs_or_error(lambda: og.assemble_contigs(raw, engine, device=False))


def test_raw_lists_reach_what_they_are_for(raw_lists):
    spelled = [n for n, (_, res) in raw_lists.items() if res["cycle_node"] < 0]
    assert len(spelled) >= 5 and max(spelled) >= 129
    big = raw_lists[300][1]
    assert big["words_per_row"] >= 2 and 0 < big["n_kept"] < big["n_edges"]
    assert int((big["tail"] == big["head"]).sum()) >= 1  # a kept self-loop: the self column was read


def test_string_graph_of_400_reads(engine):
    from ovlgraph import overlapGraphs as og
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads
    from ovlgraph.unitigs import assemble_contigs_direct
    reads = list(dict.fromkeys(simulate_reads(read_genome_from_fasta(), 60, 440, 0.01, seed=5)))[:400]
    assert len(reads) == 400
    got = contigs_or_error(lambda: assemble_contigs_direct(reads, engine, device=True))
    stats = engine.last_unitigs()
    assert stats["edges"] > 50_000 and 0 < stats["kept"] < stats["edges"] and stats["words_per_row"] == 7
    assert got == contigs_or_error(lambda: og.assemble_contigs(reads, engine, device=True))
    assert isinstance(got, list) and len(got) == stats["paths"]


def test_a_larger_call_then_a_smaller_one(engine, raw_lists):
    from ovlgraph.unitigs import _run
    for big, small in ((300, 65), (300, 3), (129, 1)):
        assert_same_result(_run(raw_lists[big][0], engine, None, True, None)[1], raw_lists[big][1], big)
        assert_same_result(_run(raw_lists[small][0], engine, None, True, None)[1], raw_lists[small][1], small)
        assert_same_result(_run(raw_lists[small][0], engine, engine_scorer(engine), True, None)[1],
                           raw_lists[small][1], small)


def test_blocks_regrown_and_reused_equal_the_host_form():
    """3 reads, then 70 (past one wavefront; two words per matrix row), then the 3 again, on one fresh engine and
    through both device calls: the input, node and edge blocks are laid out in new buffers, in regrown ones and inside
    buffers larger than they need."""
    from layout_cases import random_reads
    from ovlgraph import OverlapEngine
    from ovlgraph.unitigs import _run
    small, big = random_reads(3, 20261021), random_reads(70, 20261022)
    with OverlapEngine(0) as eng:
        for raw in (small, big, small):
            want = _run(raw, eng, None, False, None)[1]
            assert want["n_edges"] > 0
            assert_same_result(_run(raw, eng, None, True, None)[1], want, (len(raw), "ovl_unitigs_candidates"))
            assert_same_result(_run(raw, eng, engine_scorer(eng), True, None)[1], want, (len(raw), "ovl_unitigs"))


def test_several_marking_windows_per_node(raw_lists, monkeypatch):
    from ovlgraph import OverlapEngine
    from ovlgraph.unitigs import _run
    monkeypatch.setenv("OVL_REACH_WINDOW", "128")
    raw, want = raw_lists[300]
    assert want["words_per_row"] > 2  # more columns than one window of 128
    with OverlapEngine(0) as eng:
        assert_same_result(_run(raw, eng, None, True, None)[1], want, "window 128")


def test_two_copies_of_one_read_raise_as_find_unitigs_does(engine):
    from ovlgraph import overlapGraphs as og
    from ovlgraph.unitigs import assemble_contigs_direct, reduced_string_graph
    r = raw_list(1)[0]
    with pytest.raises(ValueError) as want:
        og.assemble_contigs([r, r], engine, device=False)
    for scorer in (None, engine_scorer(engine)):
        with pytest.raises(ValueError) as got:
            assemble_contigs_direct([r, r], engine, scorer, device=True)
        assert str(got.value) == str(want.value)
        red = reduced_string_graph([r, r], engine, scorer, device=True)
        assert red.cycle_node == 0 and list(red.to_digraph().edges()) == [(r, r)]


def _candidates_call(eng, buf, ids, outs):
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    nc, cyc = ctypes.c_int32(-7), ctypes.c_int32(-7)
    ne, nk = ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = eng._L.ovl_unitigs_candidates(eng._ctx, p(buf), p(ids), 0 if ids is None else ids.shape[0], 10, -1,
                                       -(2 ** 31), -1, *[p(o) for o in outs], ctypes.byref(nc), ctypes.byref(ne),
                                       ctypes.byref(nk), ctypes.byref(cyc))
    return rc, (nc.value, ne.value, nk.value, cyc.value)


def test_state_and_error_codes_leave_outputs_untouched():
    from ovlgraph import OverlapEngine
    from ovlgraph.engine import encode_reads
    raw = raw_list(8)
    distinct = list(dict.fromkeys(raw))
    index = {r: i for i, r in enumerate(distinct)}
    ids = np.array([index[r] for r in raw], np.int32)
    buf, offs = encode_reads(distinct)
    n = len(distinct)

    def fresh():
        return [np.full(n + 1, -9, np.int64), np.full(n, -9, np.int32), np.full(int(offs[-1]), 9, np.uint8),
                np.full(n + 1, -9, np.int64)]

    def untouched(outs):
        return all((o == (9 if o.dtype == np.uint8 else -9)).all() for o in outs)

    with OverlapEngine(0) as eng:
        outs = fresh()
        assert _candidates_call(eng, buf, ids, outs) == (-6, (-7, -7, -7, -7)) and untouched(outs)  # no reads
        eng.set_reads(distinct, (buf, offs))
        assert _candidates_call(eng, buf, ids, outs) == (-6, (-7, -7, -7, -7)) and untouched(outs)  # no list
        eng.enumerate_candidates(5)
        assert _candidates_call(eng, buf, ids, outs) == (-1, (-7, -7, -7, -7)) and untouched(outs)  # a k = 5 list
        assert eng.enumerate_candidates(0) == n * (n - 1)
        far, swapped = ids.copy(), ids.copy()
        far[3], swapped[0] = 99, 1  # an id outside [0, n); ids that do not start at 0
        for bad, want in ((far, -7), (swapped, -1), (ids[: n - 1], -1), (None, -1)):
            assert _candidates_call(eng, buf, bad, outs) == (want, (-7, -7, -7, -7)) and untouched(outs)
        assert _candidates_call(eng, None, ids, outs) == (-1, (-7, -7, -7, -7)) and untouched(outs)  # bases, no bytes
        p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
        assert eng._L.ovl_unitigs_candidates(eng._ctx, p(buf), p(ids), ids.shape[0], 10, -1, -(2 ** 31), -1, None,
                                             None, None, None, None, None, None, None) == -1  # n_contigs is NULL
        assert eng._L.ovl_unitigs_edges_copy(eng._ctx, None, None, None, None) == -6  # nothing ran yet
        rc, scalars = _candidates_call(eng, buf, ids, outs)
        assert rc in (0, 1) and scalars[1] > 0 and untouched(outs[:1]) == (rc != 0)
        # the uploaded form's checks are the host form's
        sc = np.zeros(n * (n - 1), np.int32)
        nc = ctypes.c_int32(-7)
        outs = fresh()
        for bad_ids, n_raw, want in ((far, far.shape[0], -7), (ids, n - 1, -1)):
            assert eng._L.ovl_unitigs(eng._ctx, p(buf), p(offs), n, p(bad_ids), n_raw, p(sc), p(sc), p(sc[:n]),
                                      p(sc[:n]), *[p(o) for o in outs], ctypes.byref(nc), None, None, None) == want
        assert eng._L.ovl_unitigs(eng._ctx, p(buf), p(offs), n, p(ids), ids.shape[0], None, p(sc), p(sc[:n]),
                                  p(sc[:n]), *[p(o) for o in outs], ctypes.byref(nc), None, None, None) == -1
        assert nc.value == -7 and untouched(outs)


def test_timing_covers_a_calls_launches(engine, raw_lists):
    from stage_timing import assert_kernel_inside_call, timed_and_untimed
    from ovlgraph.unitigs import _run
    raw, want = raw_lists[129]
    got_on, on, got_off, off = timed_and_untimed(engine, lambda: _run(raw, engine, None, True, None)[1],
                                                 engine.last_unitigs)
    assert_kernel_inside_call(on, off)
    parts = [on[k] for k in ("score_ms", "build_ms", "reduce_ms", "facts_ms")]
    assert all(v > 0.0 for v in parts) and abs(sum(parts) - on["kernel_ms"]) < 1e-6
    assert all(off[k] == 0.0 for k in ("score_ms", "build_ms", "reduce_ms", "facts_ms"))
    assert_same_result(got_on, want, "timing on")
    assert_same_result(got_off, want, "timing off")
    # the uploaded form scores nothing
    engine.set_timing(True)
    try:
        _run(raw, engine, engine_scorer(engine), True, None)
        assert engine.last_unitigs()["score_ms"] == 0.0 and engine.last_unitigs()["build_ms"] > 0.0
    finally:
        engine.set_timing(False)
