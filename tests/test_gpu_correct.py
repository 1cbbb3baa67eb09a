"""k-mer spectrum read correction on the GPU (ovl_kmer_spectrum and ovl_correct_reads: the kernels of ovl_spectrum.hip,
ovl_spectrum_api.cpp) against the host form element for element: spectrum, bytes, per-read counts and stats.

The cases of tests/correct_cases.py are shaped for the kernels: reads of 63, 64, 65 and 129 windows (the wavefront's
steps), k = 1, 16 and 31 (the key's 32-bit boundary and its top field), a read with more than 64 untrusted positions
(the position chunks and the work-item stepping), a window without a key beside the key of k T's (the sort's extra
bit), more than 2,000 reads (several blocks), empty reads and no reads.  The host results are computed once per module
and shared."""
import numpy as np
import pytest

from correct_cases import (BY_NAME, CASES, RawCorrect, RawSpectrum, assert_same, assert_same_spectrum,
                           bad_correct_calls, bad_spectrum_calls, genome, quality, small_quality_reads, with_errors)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from ovlgraph import OverlapEngine
    eng = OverlapEngine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def host_results():
    from ovlgraph.correct import correct_reads, kmer_spectrum
    return {c.name: (kmer_spectrum(c.reads, c.k, form="host"), correct_reads(c.reads, c.k, c.min_count, form="host"))
            for c in CASES}


def _check_case(eng, host_results, c):
    from ovlgraph.correct import correct_reads, kmer_spectrum
    want_spectrum, want = host_results[c.name]
    assert_same_spectrum(kmer_spectrum(c.reads, c.k, engine=eng, form="device"), want_spectrum, c.name)
    assert_same(correct_reads(c.reads, c.k, c.min_count, engine=eng, form="device"), want, c.name)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_device_form_equals_the_host_form(engine, host_results, case):
    _check_case(engine, host_results, case)


def test_blocks_regrown_and_reused_equal_the_host_form():
    """3 reads, then 70 (past one wavefront), then the 3 again, on one fresh engine: the upload and the tables are laid
    out in new buffers, in regrown ones and inside buffers larger than they need.  With k = 4 and the rule's threshold
    the 3 reads change 5 bases; with k = 5 and min_count 2 the 70 reads change 59 and tie at 21 (the host form)."""
    from layout_cases import random_reads
    from ovlgraph import OverlapEngine
    from ovlgraph.correct import correct_reads, kmer_spectrum
    small, big = random_reads(3, 20261021), random_reads(70, 20261022)
    with OverlapEngine(0) as eng:
        for reads in (small, big, small):
            for k, min_count in ((4, "auto"), (5, 2)):
                what = (len(reads), k)
                assert_same_spectrum(kmer_spectrum(reads, k, engine=eng, form="device"),
                                     kmer_spectrum(reads, k, form="host"), what)
                assert_same(correct_reads(reads, k, min_count, engine=eng, form="device"),
                            correct_reads(reads, k, min_count, form="host"), what)


def test_three_slot_context_equals_the_host_form(host_results, monkeypatch):
    from ovlgraph import OverlapEngine
    monkeypatch.setenv("OVL_SHARE_DEVICES", "1")
    with OverlapEngine(devices=[0, 0, 0]) as eng:
        for c in CASES:
            _check_case(eng, host_results, c)


@pytest.mark.parametrize("vote", ("atomic", "ballot"))
def test_both_forms_of_the_vote_count_equal_the_host_form(host_results, monkeypatch, vote):
    """OVL_SPECTRUM_VOTE: the solid work items counted by LDS atomics and by ballot."""
    from ovlgraph import OverlapEngine
    monkeypatch.setenv("OVL_SPECTRUM_VOTE", vote)
    with OverlapEngine(0) as eng:
        for c in CASES:
            _check_case(eng, host_results, c)


def test_longest_read_the_device_takes_and_the_first_it_refuses(engine):
    from ovlgraph import OvlError
    from ovlgraph.correct import correct_reads, kmer_spectrum
    k = 12
    text = genome(k + 8192, 5)
    fits = [text[:-1]] * 3 + [with_errors(text[:-1], [0, 4000, k + 8190])]
    want = correct_reads(fits, k, 3, form="host")
    assert want[0] == [text[:-1]] * 4
    assert_same(correct_reads(fits, k, 3, engine=engine, form="device"), want)
    assert_same_spectrum(kmer_spectrum(fits, k, engine=engine, form="device"), kmer_spectrum(fits, k, form="host"))
    too_long = ["ACGTACGTACGTACGT", text]
    for call in (lambda: correct_reads(too_long, k, 3, engine=engine, form="device"),
                 lambda: kmer_spectrum(too_long, k, engine=engine, form="device")):
        with pytest.raises(OvlError) as e:
            call()
        assert e.value.code == -4 and "read 1" in str(e.value)
    # "auto" serves it through the host form
    reads = [text] * 3 + [with_errors(text, [5, k + 8191])]
    assert_same(correct_reads(reads, k, 3, engine=engine, form="auto"), correct_reads(reads, k, 3, form="host"))
    assert_same_spectrum(kmer_spectrum(reads, k, engine=engine, form="auto"), kmer_spectrum(reads, k, form="host"))
    raw = RawCorrect(too_long)
    assert raw(engine._L, ctx=engine._ctx, k=k) == -4 and raw.untouched()


def test_argument_checks_return_their_code_and_write_nothing(engine):
    L = engine._L
    reads = BY_NAME["duplicated_reads"].reads
    for what, kw, code in bad_correct_calls():
        call = RawCorrect(reads)
        assert call(L, ctx=engine._ctx, **kw) == code, what
        assert call.untouched(), what
    call = RawCorrect(reads)
    call.offs[2] = call.offs[1] - 1
    assert call(L, ctx=engine._ctx) == -1 and call.untouched()
    ok = RawCorrect(reads)
    assert ok(L, ctx=engine._ctx, k=12, min_count=3) == 0 and ok.stats[4] == 2 and ok.stats[6] == 3
    assert (ok.out[int(ok.offs[-1]):] == 0x5A).all() and (ok.changed[ok.n:] == -77).all()
    for what, kw, code in bad_spectrum_calls():
        call = RawSpectrum(reads, 100)
        assert call(L, ctx=engine._ctx, **kw) == code, what
        assert call.arrays_untouched() and call.nd.value == -77, what
    # the sizing protocol
    from ovlgraph.correct import kmer_spectrum
    kmer_keys = kmer_spectrum(reads, 12, form="host")[0]
    n = len(kmer_keys)
    small = RawSpectrum(reads, n - 1)
    assert small(L, ctx=engine._ctx, k=12) == -5 and small.nd.value == n and small.arrays_untouched()
    exact = RawSpectrum(reads, n)
    assert exact(L, ctx=engine._ctx, k=12) == 0 and np.array_equal(exact.keys[:n], kmer_keys)
    assert (exact.keys[n:] == 0x5A5A).all() and (exact.counts[n:] == -77).all()


def test_timing_reports_the_parts(engine, host_results):
    from ovlgraph.correct import correct_reads
    c = BY_NAME["many_short_reads"]
    engine.set_timing(True)
    try:
        got = correct_reads(c.reads, c.k, c.min_count, engine=engine, form="device")
        t = engine.last_correct()
        call_ms = engine.last_timing()["call_ms"]
    finally:
        engine.set_timing(False)
    assert_same(got, host_results[c.name][1])
    assert set(t) == {"keys_ms", "sort_ms", "count_ms", "correct_ms"} and all(v > 0.0 for v in t.values()), t
    assert call_ms > 0.0
    correct_reads(c.reads, c.k, c.min_count, engine=engine, form="device")
    assert all(v == 0.0 for v in engine.last_correct().values())


def test_threshold_past_the_histogram_bins_equals_the_host_form(engine, monkeypatch):
    """The device form takes the threshold from a histogram with a last bin for every greater count.  Counts above
    the 1,024 bins (k = 1) land there; and with OVL_SPECTRUM_BINS=4 the small quality case's first valley (threshold
    5) lies past the exact bins, so the rule is taken from the counts themselves."""
    from ovlgraph import OverlapEngine
    from ovlgraph.correct import correct_reads
    reads = ["A"] * 1100 + ["C"] * 1100 + ["G"] * 1 + ["T"] * 1
    want = correct_reads(reads, 1, form="host")
    assert want[1]["threshold"] == 2
    assert_same(correct_reads(reads, 1, engine=engine, form="device"), want)
    noisy, _ = small_quality_reads()
    want = correct_reads(noisy, 8, form="host")
    assert want[1]["threshold"] == 5
    monkeypatch.setenv("OVL_SPECTRUM_BINS", "4")
    with OverlapEngine(0) as eng:
        assert_same(correct_reads(noisy, 8, engine=eng, form="device"), want)


def test_small_quality_case_on_the_device(engine):
    from ovlgraph.correct import correct_reads
    noisy, clean = small_quality_reads()
    out, stats = correct_reads(noisy, 8, engine=engine, form="device")
    before, after, wrong, changes = quality(noisy, out, clean)
    print(f"threshold {stats['threshold']}: errors {before} -> {after}, {wrong} of {changes} changes wrong")
    assert stats["threshold"] == 5 and changes == stats["changed"]
    assert after <= before / 4
    assert wrong <= changes / 10
    assert_same(correct_reads(noisy, 8, rounds=2, engine=engine, form="device"),
                correct_reads(noisy, 8, rounds=2, form="host"))


def test_assembly_of_device_corrected_reads_equals_host_corrected(engine):
    from ovlgraph.correct import correct_reads
    from ovlgraph.layout import assemble_contigs_best_successor
    reads = BY_NAME["phix_300"].reads
    dev = correct_reads(reads, 12, engine=engine, form="device")[0]
    host = correct_reads(reads, 12, form="host")[0]
    assert dev == host != reads
    assert assemble_contigs_best_successor(dev, k=12, engine=engine) == \
        assemble_contigs_best_successor(host, k=12, engine=engine)
    assert engine.correct_reads(reads, 12)[2]["changed"] > 0  # the engine's thin wrapper, threshold by the rule


def test_timing_of_the_two_entry_points(engine):
    """A dozen 40-base reads, k = 8 (every read has windows): ovl_correct_reads times four parts that add up to
    kernel_ms, ovl_kmer_spectrum the first three, and with timing off all are zero."""
    from stage_timing import timed_and_untimed
    reads = small_quality_reads()[0][:12]
    parts = ("keys_ms", "sort_ms", "count_ms", "correct_ms")
    got_on, on, got_off, off = timed_and_untimed(engine, lambda: engine.correct_reads(reads, 8), engine.last_correct)
    assert all(on[p] > 0.0 for p in parts), on
    assert abs(on["kernel_ms"] - sum(on[p] for p in parts)) <= 1e-6 and on["kernel_ms"] <= on["call_ms"], on
    assert all(off[p] == 0.0 for p in parts) and off["kernel_ms"] == 0.0 and off["call_ms"] > 0.0, off
    assert np.array_equal(got_on[0], got_off[0]) and np.array_equal(got_on[1], got_off[1]) and got_on[2] == got_off[2]
    sp_on, on, sp_off, off = timed_and_untimed(engine, lambda: engine.kmer_spectrum(reads, 8), engine.last_correct)
    assert on["correct_ms"] == 0.0 and all(on[p] > 0.0 for p in parts[:3]), on
    assert abs(on["kernel_ms"] - sum(on[p] for p in parts)) <= 1e-6, on
    assert all(off[p] == 0.0 for p in parts) and off["kernel_ms"] == 0.0, off
    assert np.array_equal(sp_on[0], sp_off[0]) and np.array_equal(sp_on[1], sp_off[1])
