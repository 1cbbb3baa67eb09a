"""k-mer spectrum read correction without a GPU: ovl_kmer_spectrum_host and ovl_correct_reads_host against the rule as
literal loops (kmer_spectrum_loop, correct_reads_loop) on every case of tests/correct_cases.py, element for element;
solid_threshold on hand-made histograms; every argument check of the ABI (its code, and nothing written) and the
OVL_E_RANGE sizing protocol; rounds; and what the stage does to simulated errors.

Quality bounds: errors after <= a quarter of errors before, and correct bases changed by mistake <= a
tenth of all changes.  Measured with the host form: the small case (threshold 5) 282 -> 26 errors with 10 of 276 changes
wrong; PhiX N = 2,000, p = 0.01 (threshold 5) 2,006 -> 91 with 25 of 1,966 changes wrong."""
import ctypes

import numpy as np
import pytest

from correct_cases import (BY_NAME, CASES, RawCorrect, RawSpectrum, assert_same, assert_same_spectrum,
                           bad_correct_calls, bad_spectrum_calls, quality, small_quality_reads)
from ovlgraph import _lib
from ovlgraph.correct import (correct_reads, correct_reads_loop, kmer_spectrum, kmer_spectrum_loop, solid_threshold)


@pytest.fixture(scope="module")
def loops():
    return {c.name: (kmer_spectrum_loop(c.reads, c.k), correct_reads_loop(c.reads, c.k, c.min_count)) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_form_equals_the_loop_form(loops, case):
    want_spectrum, want = loops[case.name]
    assert_same_spectrum(kmer_spectrum(case.reads, case.k, form="host"), want_spectrum, case.name)
    got = correct_reads(case.reads, case.k, case.min_count, form="host")
    assert_same(got, want, case.name)
    assert [len(r) for r in got[0]] == [len(r) for r in case.reads]
    if case.min_count == "auto":
        assert got[1]["threshold"] == solid_threshold(want_spectrum[1])
    assert got[1]["kmers"] == int(want_spectrum[1].sum()) and got[1]["distinct"] == len(want_spectrum[0])


def test_the_cases_reach_what_they_are_named_for(loops):
    res = {name: v[1] for name, v in loops.items()}
    assert res["no_reads"][0] == [] and res["no_reads"][1]["threshold"] == 1
    for n_win in (63, 64, 65, 129):
        c = BY_NAME[f"windows_{n_win}"]
        assert len(c.reads[0]) - c.k + 1 == n_win
        assert res[c.name][0] == [c.reads[0]] * len(c.reads), c.name  # every error repaired, ends included
    c = BY_NAME["lengths_around_k"]
    assert sorted(len(r) for r in c.reads)[:4] == [c.k - 1, c.k, c.k, c.k + 1]
    assert res["error_at_0_and_last"][0] == [BY_NAME["error_at_0_and_last"].reads[0]] * 8
    assert res["two_errors_closer_than_k"][0] == [BY_NAME["two_errors_closer_than_k"].reads[0]] * 8
    c = BY_NAME["damaged_read"]
    assert res[c.name][1]["untrusted"] > 150 > 64  # read 5 alone: every position, 150 * 3 * k work items
    c = BY_NAME["tie_stays"]
    assert res[c.name][0] == c.reads and res[c.name][1]["ties"] == 1 and res[c.name][1]["changed"] == 0
    c = BY_NAME["n_and_lower_case"]
    assert res[c.name][0][4] == c.reads[0] and res[c.name][0][5:9] == c.reads[5:9]
    assert res[c.name][0][9] == c.reads[0][:20] + "N" + c.reads[0][21:]  # the N stays, the error beside it goes
    assert res[c.name][1]["kmers"] < res[c.name][1]["windows"]
    for name in ("min_count_1", "min_count_above_all"):
        assert res[name][0] == BY_NAME[name].reads and res[name][1]["changed"] == 0
    assert res["min_count_1"][1]["untrusted"] == 0
    assert res["min_count_above_all"][1]["untrusted"] == 5 * 60 and res["min_count_above_all"][1]["solid"] == 0
    c = BY_NAME["duplicated_reads"]
    assert res[c.name][0] == [c.reads[1]] * 6 and res[c.name][1]["changed_per_read"].tolist() == [1, 0, 0, 0, 0, 1]
    assert len(BY_NAME["many_short_reads"].reads) > 2000 and res["many_short_reads"][1]["changed"] > 100
    assert res["phix_300"][1]["changed"] > 0
    keys, counts = loops["all_t_beside_keyless"][0]
    assert int(keys[-1]) == 0xFF and int(counts[-1]) > 20 and res["all_t_beside_keyless"][1]["changed"] == 1
    keys, _ = loops["k_31"][0]
    assert int(keys[-1]) == (1 << 62) - 1  # 31 T's: the greatest key there is


def test_solid_threshold_on_hand_made_histograms():
    assert solid_threshold([]) == 1
    assert solid_threshold([7]) == 1                      # a single count: h[1] = h[2] = 0
    assert solid_threshold([1]) == 1
    assert solid_threshold([1, 1, 1, 2, 2, 3]) == 3       # a histogram that only decreases: the max count
    assert solid_threshold([1] * 9 + [2] * 4 + [3] * 2 + [4] * 2 + [9] * 5) == 3  # h[4] >= h[3]
    assert solid_threshold([1] * 9 + [2] * 4 + [3] * 0 + [10] * 5) == 3           # h[4] = h[3] = 0
    assert solid_threshold([1] * 3 + [2] * 5) == 1        # rising at once
    assert solid_threshold(np.asarray([5, 5, 5], dtype=np.int32)) == 1  # h[1] = h[2] = 0
    # the native forms use the same rule: counts 1 x 4, 2 x 2, 3 x 1, 4 x 1 over k = 1
    reads = ["A"] * 1 + ["C"] * 2 + ["G"] * 3 + ["T"] * 4
    assert solid_threshold(kmer_spectrum(reads, 1, form="host")[1]) == 1  # h[1] = h[2] = 1
    assert correct_reads(reads, 1, form="host")[1]["threshold"] == 1
    # a first valley past the device histogram's exact bins is found by the host form all the same
    reads = ["A"] * 1500 + ["C"] * 1400
    assert correct_reads(reads, 1, form="host")[1]["threshold"] == solid_threshold([1500, 1400]) == 1


def test_argument_checks_return_their_code_and_write_nothing():
    L = _lib.load()
    reads = BY_NAME["duplicated_reads"].reads
    for what, kw, code in bad_correct_calls():
        call = RawCorrect(reads)
        assert call(L, **kw) == code, what
        assert call.untouched(), what
        assert _lib.last_error(), what
    call = RawCorrect(reads)
    call.offs[2] = call.offs[1] - 1
    assert call(L) == -1 and call.untouched()
    ok = RawCorrect(reads)
    assert ok(L, k=12, min_count=3) == 0 and ok.stats[4] == 2 and ok.stats[6] == 3
    assert (ok.out[int(ok.offs[-1]):] == 0x5A).all() and (ok.changed[ok.n:] == -77).all()
    for what, kw, code in bad_spectrum_calls():
        call = RawSpectrum(reads, 100)
        assert call(L, **kw) == code, what
        assert call.arrays_untouched() and call.nd.value == -77, what
    assert L.ovl_last_correct_timing(None, None, None, None, None) == -1
    assert L.ovl_correct_reads(None, *([None] * 2), 0, 4, 0, *([None] * 3)) == -1
    assert L.ovl_kmer_spectrum(None, *([None] * 2), 0, 4, None, None, 0, None) == -1


def test_range_sizing_protocol():
    L = _lib.load()
    c = BY_NAME["duplicated_reads"]
    want_keys, want_counts = kmer_spectrum_loop(c.reads, c.k)
    n = len(want_keys)
    sizing = RawSpectrum(c.reads, 0)
    assert sizing(L, k=c.k, out_keys=True, out_counts=True) == -5 and sizing.nd.value == n
    small = RawSpectrum(c.reads, n - 1)
    assert small(L, k=c.k) == -5 and small.nd.value == n and small.arrays_untouched()
    exact = RawSpectrum(c.reads, n)
    assert exact(L, k=c.k) == 0 and exact.nd.value == n
    assert np.array_equal(exact.keys[:n], want_keys) and np.array_equal(exact.counts[:n], want_counts)
    assert (exact.keys[n:] == 0x5A5A).all() and (exact.counts[n:] == -77).all()
    empty = RawSpectrum([], 0)
    assert empty(L, k=c.k, out_keys=True, out_counts=True) == 0 and empty.nd.value == 0


def test_rounds_2_equals_two_calls():
    c = BY_NAME["many_short_reads"]
    once, s1 = correct_reads(c.reads, c.k, form="host")
    twice, s2 = correct_reads(once, c.k, form="host")
    both, s = correct_reads(c.reads, c.k, rounds=2, form="host")
    assert both == twice and once != twice
    assert_same((both, s), (twice, s2))
    assert len(s["per_round"]) == 2
    assert_same((once, s["per_round"][0]), (once, s1))
    assert_same(correct_reads(c.reads[:300], c.k, rounds=2, form="loop"),
                correct_reads(c.reads[:300], c.k, rounds=2, form="host"))


def test_python_checks_and_package_names():
    import ovlgraph
    assert ovlgraph.correct_reads is correct_reads and ovlgraph.kmer_spectrum is kmer_spectrum
    assert ovlgraph.solid_threshold is solid_threshold
    with pytest.raises(_lib.OvlError):
        correct_reads(["ACΔT", "ACGT"], 2, form="host")
    for bad in (dict(k=0), dict(k=32), dict(k=4, min_count=0), dict(k=4, rounds=0)):
        with pytest.raises(_lib.OvlError):
            correct_reads(["ACGTACGT"], form="host", **bad)
    with pytest.raises(ValueError):
        correct_reads(["ACGTACGT"], 4, form="gpu")
    from ovlgraph.engine import device_count
    if device_count() == 0:  # "auto" serves without a GPU
        c = BY_NAME["duplicated_reads"]
        assert_same(correct_reads(c.reads, c.k, c.min_count), correct_reads_loop(c.reads, c.k, c.min_count))
        assert_same_spectrum(kmer_spectrum(c.reads, c.k), kmer_spectrum_loop(c.reads, c.k))


def test_a_read_beyond_the_device_limit_is_served_by_the_host_form():
    from correct_cases import genome, with_errors
    long_read = genome(12 + 8192, 5)
    reads = [long_read] * 3 + [with_errors(long_read, [0, 4000, 8203])]
    out, stats = correct_reads(reads, 12, 3, form="host")
    assert out == [long_read] * 4 and stats["changed"] == 3 and stats["windows"] == 4 * 8193


def _check_quality(noisy, clean, k, threshold):
    out, stats = correct_reads(noisy, k, form="host")
    before, after, wrong, changes = quality(noisy, out, clean)
    print(f"threshold {stats['threshold']}: errors {before} -> {after}, {wrong} of {changes} changes wrong")
    assert stats["threshold"] == threshold and changes == stats["changed"]
    assert after <= before / 4
    assert wrong <= changes / 10


def test_small_quality_case():
    noisy, clean = small_quality_reads()
    _check_quality(noisy, clean, 8, 5)


def test_phix_quality_case():
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads
    g = read_genome_from_fasta()
    _check_quality(simulate_reads(g, 100, 2000, 0.01, seed=0), simulate_reads(g, 100, 2000, 0.0, seed=0), 12, 5)


def test_error_free_reads_do_not_change():
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads
    noisy, clean = small_quality_reads()
    out, stats = correct_reads(clean, 8, form="host")
    assert out == clean and stats["changed"] == 0
    phix = simulate_reads(read_genome_from_fasta(), 100, 2000, 0.0, seed=0)
    out, stats = correct_reads(phix, 12, form="host")
    assert out == phix and stats["changed"] == 0
