"""Placed consensus on the GPU: ovl_consensus_placed against the host form, element for element, on every case of
tests/consensus_placed_cases.py, in one chunk and in several; its counters; the slack it does not take; at slack 15 on
short sequences against ovl_consensus; and the pipeline with polishing against its host route."""
import random

import numpy as np
import pytest

from consensus_placed_cases import BY_NAME, CASES, RawCall, assert_same, native_args
from ovlgraph.engine import consensus_placed_host

pytestmark = pytest.mark.gpu

IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def engine():
    from ovlgraph import OverlapEngine
    eng = OverlapEngine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def host_results():
    """The host form's result per case, computed once and shared by the tests below."""
    out = {}
    for c in CASES:
        a, kw = native_args(c)
        out[c.name] = consensus_placed_host(*a, **kw)
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_form_equals_the_host_form(engine, host_results, case):
    a, kw = native_args(case)
    got = engine.consensus_placed(*a, **kw)
    assert_same(got, host_results[case.name], case.name)
    last = engine.last_consensus_placed()
    ref = host_results[case.name]
    # the reads that voted went through the band kernel, in one launch per round
    assert last["voted_reads"] == int((ref["aln"][:, 0] > 0).sum())
    assert last["rounds"] == ref["rounds"]
    assert last["launches"] == (ref["rounds"] if _items(case) else 0)
    assert last["ops"] >= last["voted_reads"]


def _items(case) -> int:
    """The reads of the case that have a window: what the band kernel takes."""
    n = 0
    for r, q in enumerate(case.reads):
        c = case.contig[r]
        wt = 1 if case.weights is None else case.weights[r]
        if c < 0 or not q or wt == 0:
            continue
        lo = max(0, case.offset[r] - case.slack)
        hi = min(len(case.contigs[c]), case.offset[r] + len(q) + case.slack)
        n += hi > lo
    return n


@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_several_chunks_equal_one(monkeypatch, host_results, chunk):
    from ovlgraph import OverlapEngine
    monkeypatch.setenv("OVL_CONSENSUS_CHUNK", str(chunk))
    eng = OverlapEngine(0)
    try:
        for name in ("count_130", "len_mixed", "weights", "rounds_5", "contigs_edge", "no_window"):
            case = BY_NAME[name]
            a, kw = native_args(case)
            got = eng.consensus_placed(*a, **kw)
            assert_same(got, host_results[name], f"{name}, chunks of {chunk}")
            last = eng.last_consensus_placed()
            assert last["launches"] == -(-_items(case) // chunk) * last["rounds"], name
            windowless = sum(1 for r, q in enumerate(case.reads) if case.contig[r] >= 0 and q
                             and (case.weights is None or case.weights[r] > 0)) - _items(case)
            assert last["windowless_reads"] == windowless, name
    finally:
        eng.close()


def test_counts_and_aln_may_be_null(engine, host_results):
    case = BY_NAME["slack_9"]
    a, kw = native_args(case)
    got = engine.consensus_placed(*a, counts=False, **kw)
    assert "counts" not in got and np.array_equal(got["called"], host_results[case.name]["called"])
    raw = RawCall(case)
    assert engine._L.ovl_consensus_placed(*raw.args(head=[engine._ctx], aln=None, counts=None)) == 0
    assert np.array_equal(raw.called, host_results[case.name]["called"]) and (raw.aln == 77).all()


def test_slack_16_is_unsupported_and_writes_nothing(engine):
    case = BY_NAME["slack_15"]
    raw = RawCall(case)
    assert engine._L.ovl_consensus_placed(*raw.args(head=[engine._ctx], slack=16)) == -4
    assert raw.untouched()
    raw = RawCall(case)
    assert engine._L.ovl_consensus_placed(*raw.args(head=[engine._ctx], slack=15)) == 0 and not raw.untouched()
    # so is a positive score whose sums could leave int32 in the band kernel; the host form takes it
    raw = RawCall(case)
    assert engine._L.ovl_consensus_placed(*raw.args(head=[engine._ctx], mismatch=1 << 25)) == -4
    assert raw.untouched()
    assert engine._L.ovl_consensus_placed_host(*raw.args(mismatch=1 << 25)) == 0


def test_slack_15_on_short_sequences_equals_ovl_consensus(engine):
    rng = random.Random(15)
    contigs = ["".join(rng.choice("ACGTN") for _ in range(rng.randint(0, 15))) for _ in range(6)]
    reads, contig, offset = [], [], []
    for _ in range(150):
        c = rng.randrange(-1, 6)
        reads.append("".join(rng.choice("ACGTa") for _ in range(rng.randint(0, 15))))
        contig.append(c)
        offset.append(rng.randint(-3, 3))
    for scoring in ((10, -1, -1), (2, -3, -5), (1, -1, -1)):
        # offset 0 keeps |(j - i) - d| <= 15 for every cell of a table of at most 15 x 15
        got = engine.consensus_placed(reads, contigs, contig, [0] * 150, 15, None, 1, 2, 1, *scoring)
        ref = engine.consensus(reads, contigs, contig, 0, *scoring, 2)
        for k in ("counts", "called", "n_changed", "n_other", "aln"):
            assert np.array_equal(got[k], ref[k]), (scoring, k)
        # and any placement gives what the host form gives
        got = engine.consensus_placed(reads, contigs, contig, offset, 15, None, 1, 2, 1, *scoring)
        assert_same(got, consensus_placed_host(reads, contigs, contig, offset, 15, None, 1, 2, 1, *scoring), "short")


def test_pipeline_with_polish_equals_its_host_route(engine):
    from ovlgraph.layout import assemble_contigs_best_successor
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads
    reads = simulate_reads(read_genome_from_fasta(), 100, 2000, 0.01, seed=0)
    out, ref_out = {}, {}
    got = assemble_contigs_best_successor(reads, k=12, polish=2, engine=engine, layout_out=out)
    plain = assemble_contigs_best_successor(reads, k=12, engine=engine, candidates="host", layout_out=ref_out)
    assert plain == out["contigs"] and "pileup" not in ref_out
    ref = consensus_placed_host(ref_out["reads"], plain, ref_out["contig"], ref_out["offset"], 8, out["copies"], 2)
    assert "".join(got) == ref["called"].tobytes().decode()
    pile = out["pileup"]
    assert (pile.rounds, pile.total_changed, pile.n_changed) == (ref["rounds"], ref["total_changed"], ref["n_changed"])
    assert np.array_equal(np.concatenate(pile.counts), ref["counts"]) and np.array_equal(pile.aln, ref["aln"])
    assert pile.total_changed > 0 and engine.last_consensus_placed()["voted_reads"] > 1900


def test_timing_reports_the_band_and_the_vote(engine, host_results):
    """The smallest case that runs two rounds (eight reads of 20 bases): band_ms and vote_ms are summed over the
    rounds, and kernel_ms is their sum."""
    from stage_timing import timed_and_untimed
    case = BY_NAME["rounds_2"]
    a, kw = native_args(case, rounds=2)
    got_on, on, got_off, off = timed_and_untimed(engine, lambda: engine.consensus_placed(*a, **kw),
                                                 engine.last_consensus_placed)
    assert on["band_ms"] > 0.0 and on["vote_ms"] > 0.0, on
    assert abs(on["kernel_ms"] - (on["band_ms"] + on["vote_ms"])) <= 1e-6 and on["kernel_ms"] <= on["call_ms"], on
    assert off["band_ms"] == off["vote_ms"] == off["kernel_ms"] == 0.0 and off["call_ms"] > 0.0, off
    want = host_results[case.name]
    assert want["rounds"] == on["rounds"] == 2
    assert_same(got_on, want, "timing on")
    assert_same(got_off, want, "timing off")


def test_timer_made_by_a_later_call_and_used_again(host_results):
    """A fresh engine whose first call has timing off makes its events only when timing is turned on, and the next
    timed call uses them again: both report every phase, and all three calls give the same result."""
    from ovlgraph import OverlapEngine
    case = BY_NAME["rounds_2"]
    a, kw = native_args(case)
    with OverlapEngine(0) as eng:
        first = eng.consensus_placed(*a, **kw)
        assert eng.last_consensus_placed()["band_ms"] == 0.0
        eng.set_timing(True)
        for what in ("first timed call", "second timed call"):
            got = eng.consensus_placed(*a, **kw)
            last = eng.last_consensus_placed()
            assert last["band_ms"] > 0.0 and last["vote_ms"] > 0.0, (what, last)
            assert last["rounds"] == 2
            assert_same(got, first, what)
    assert_same(first, host_results[case.name], "timing off")
