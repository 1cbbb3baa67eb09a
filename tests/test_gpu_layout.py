"""The best-successor layout on the GPU (ovl_layout and ovl_layout_candidates: the kernels of ovl_layout.hip,
ovl_layout_api.cpp) against the host form element for element.

The cases of tests/layout_cases.py are shaped for the kernels: runs of one read's pairs of 1, 64, 65 and 300 pairs that
start inside a wavefront and cross the wavefront's and the block's boundary, the same list shuffled (no runs at all),
both forms of the link kernel, cycles of 2 to 100 reads (the 100-cycle needs seven doubling levels), a tail of 70 reads
running into a cycle, two cycles in one launch, tied cycle minima, a chain of 130 reads (three wavefronts, not a power
of two), a star of 200 reads on one root (the head kernel's per-root reduction), negative scores (the key's bias) and
empty inputs.  The host results are computed once per module and shared."""
import numpy as np
import pytest

from layout_cases import (CASES, COUNTS, RawCall, assert_expect, assert_same, bad_calls, case_args, random_reads,
                          with_contigs)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from ovlgraph import OverlapEngine
    eng = OverlapEngine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def host_results():
    from ovlgraph.engine import layout_host
    return {c.name: with_contigs(layout_host(*case_args(c))) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_device_form_equals_the_host_form(engine, host_results, case):
    got = with_contigs(engine.layout(*case_args(case)))
    assert_same(got, host_results[case.name], case.name)
    assert_expect(case, got)
    assert np.array_equal(got["c_off"], host_results[case.name]["c_off"])
    n = len(case.reads)
    assert got["levels"] == (0 if n <= 1 else (n - 1).bit_length())


def test_blocks_regrown_and_reused_equal_the_host_form():
    """3 reads, then 70 (past one wavefront), then the 3 again, on one fresh engine: the upload and the per-read block
    are laid out in new buffers, in regrown ones and inside buffers larger than they need."""
    import random
    from ovlgraph import OverlapEngine
    from ovlgraph.engine import layout_host
    calls = []
    for n in (3, 70):
        g = random.Random(20261021 + n)
        pairs = [(g.randrange(n), g.randrange(n), g.randint(0, 5), g.randint(0, 13)) for _ in range(10 * n)]
        cols = [np.asarray([p[k] for p in pairs], np.int32) for k in range(4)]
        calls.append((random_reads(n, 20261021 + n), *cols, 1, 1))
    with OverlapEngine(0) as eng:
        for args in (calls[0], calls[1], calls[0]):
            got, want = with_contigs(eng.layout(*args)), with_contigs(layout_host(*args))
            assert_same(got, want, len(args[0]))
            assert np.array_equal(got["c_off"], want["c_off"]) and want["links"] > 0


def test_plain_link_kernel_equals_the_runs_form(host_results, monkeypatch):
    """OVL_LAYOUT_LINK=plain: one atomic per eligible pair, the form the runs form was measured against."""
    from ovlgraph import OverlapEngine
    monkeypatch.setenv("OVL_LAYOUT_LINK", "plain")
    with OverlapEngine(0) as eng:
        for c in CASES:
            assert_same(with_contigs(eng.layout(*case_args(c))), host_results[c.name], c.name)


def test_timing_reports_the_parts(engine, host_results):
    c = next(c for c in CASES if c.name == "random_1")
    engine.set_timing(True)
    try:
        got = with_contigs(engine.layout(*case_args(c)))
    finally:
        engine.set_timing(False)
    assert_same(got, host_results[c.name])
    assert got["score_ms"] == 0.0 and got["link_ms"] > 0.0 and got["forest_ms"] > 0.0 and got["spell_ms"] > 0.0
    assert engine.last_timing()["call_ms"] > 0.0


def _phix(n_reads):
    from ovlgraph.candidates import dedup_reads
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads
    return dedup_reads(simulate_reads(read_genome_from_fasta(), 100, n_reads, 0.01, seed=0))[0]


@pytest.mark.parametrize("n_reads", (200, 2000))
@pytest.mark.parametrize("seeds,k", (("any", 12), ("suffix", 5)))
def test_candidates_form_equals_the_host_route(engine, n_reads, seeds, k):
    """ovl_layout_candidates against: the list copied, score_candidates, ovl_layout_host; the list is unchanged."""
    from ovlgraph.engine import layout_host
    distinct = _phix(n_reads)
    engine.set_reads(distinct)
    n = engine.enumerate_seed_candidates(k) if seeds == "any" else engine.enumerate_candidates(k)
    a, b = (x.copy() for x in engine.candidates_copy(n))
    got = with_contigs(engine.layout_candidates())
    stats = engine.last_layout()
    a2, b2 = engine.candidates_copy(n)
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and engine.candidates_device()[2] == n
    sc, en = engine.score_candidates()
    want = with_contigs(layout_host(distinct, a, b, sc, en))
    assert_same(got, want, (n_reads, seeds))
    assert all(stats[key] == want[key] for key in COUNTS) and want["links"] > 0
    # another bound on the scores and the overlaps changes the layout, through the same columns
    got2 = with_contigs(engine.layout_candidates(min_score=600, min_overlap=70))
    assert_same(got2, with_contigs(layout_host(distinct, a, b, sc, en, 600, 70)), (n_reads, seeds, "bounds"))
    assert got2["links"] < got["links"]


def test_state_errors_without_reads_or_list():
    from ovlgraph import OverlapEngine, OvlError
    with OverlapEngine(0) as eng:
        with pytest.raises(OvlError) as e:
            eng.layout_candidates()
        assert e.value.code == -6
        eng.set_reads(["ACGTACGT", "GTACGTTT"])
        with pytest.raises(OvlError) as e:
            eng.layout_candidates()
        assert e.value.code == -6
        eng.enumerate_candidates(3)
        assert eng.layout_candidates()["n_contigs"] >= 1


def test_argument_checks_return_their_code_and_write_nothing(engine):
    reads = ["ACGTACGT", "GGGTTTAACC", "TTTACGATC"]
    cols = ([0, 1, 2], [1, 2, 0], [30, 20, 10], [2, 2, 2])
    for what, kw, code in bad_calls():
        call = RawCall(reads, *cols)
        assert call(ctx=engine._ctx, **kw) == code, what
        assert call.untouched(), what
    for bad_a, bad_b in (([0, 3, 2], cols[1]), (cols[0], [-5, 2, 0])):
        call = RawCall(reads, bad_a, bad_b, cols[2], cols[3])
        assert call(ctx=engine._ctx) == -7 and call.untouched()
    ok = RawCall(reads, *cols)
    assert ok(ctx=engine._ctx) == 0 and ok.nc.value == 1
    # the candidates form's own checks, on a context with reads and a list
    engine.set_reads(reads)
    engine.enumerate_candidates(2)
    import ctypes
    nc = ctypes.c_int32(77)
    L = engine._L
    assert L.ovl_layout_candidates(engine._ctx, 10, -1, -(2 ** 31), -1, 1, 0, *([None] * 7), ctypes.byref(nc)) == -1
    assert L.ovl_layout_candidates(engine._ctx, 10, -1, -(2 ** 31), -1, 1, 1, *([None] * 7), None) == -1
    assert nc.value == 77
    assert L.ovl_layout_candidates(engine._ctx, 10, -1, -(2 ** 31), -1, 1, 1, *([None] * 7), ctypes.byref(nc)) == 0
    assert nc.value >= 1


def test_counts_match_the_host(engine, host_results):
    for c in CASES:
        engine.layout(*case_args(c))
        stats = engine.last_layout()
        assert all(stats[k] == host_results[c.name][k] for k in COUNTS), c.name


@pytest.mark.parametrize("seeds,k", (("any", 12), ("suffix", 5)))
def test_pipeline_equals_its_host_route(engine, seeds, k):
    from ovlgraph.layout import assemble_contigs_best_successor
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads
    reads = simulate_reads(read_genome_from_fasta(), 100, 600, 0.01, seed=3)
    dev, host = {}, {}
    stages = {}
    got = assemble_contigs_best_successor(reads, k=k, seeds=seeds, engine=engine, layout_out=dev, timing=stages)
    want = assemble_contigs_best_successor(reads, k=k, seeds=seeds, engine=engine, candidates="host", layout_out=host)
    assert got == want and len(got) >= 1
    assert "enumerate" in stages and "candidates_and_scores" not in stages  # the resident route was taken
    for key in ("succ", "link", "contig", "offset", "on_path"):
        assert np.array_equal(dev[key], host[key]), key
    assert all(dev[key] == host[key] for key in COUNTS) and dev["reads"] == host["reads"]
    # layout(device=True) over host columns is the third way to the same contigs
    from ovlgraph import overlapGraphs as og
    from ovlgraph.layout import layout
    a, b, sc, en = og.candidates_and_scores(dev["reads"], k, engine, None, "host", None, seeds)
    assert layout(dev["reads"], a, b, sc, en, engine=engine, device=True)["contigs"] == want
