"""Consensus polishing without a GPU: ovl_consensus_host and ovlgraph.consensus against the reference's own
alignments (tests/golden/consensus.json, written by tools/gen_golden_consensus.py from aligners.py:85-202), piled up by
a restatement of the rule written in tests/consensus_cases.py; the planted-error inputs; the coverage sum property
against read_depth; the Python layer's choices and the argument errors of the ABI."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from consensus_cases import assert_same, planted, restate, window
from ovlgraph import _lib
from ovlgraph import consensus as cs
from ovlgraph import performanceMeasures as pm
from ovlgraph.engine import consensus_host, encode_reads


@pytest.fixture(scope="module")
def golden():
    return load_golden("consensus.json")


def _scoring(g):
    return g["match"], g["mismatch"], g["indel"]


def _mismatches(a, b):
    assert len(a) == len(b)
    return sum(x != y for x, y in zip(a, b))


def test_fixture_covers_the_edge_cases(golden):
    reads, contigs, place, rec, L = (golden[k] for k in ("reads", "contigs", "place", "records", "read_length"))
    case = golden["meta"]["cases"]
    assert len(place) == len(rec) == len(reads) and all((r is None) == (p < 0) for r, p in zip(rec, place))
    tails = [r for r, read in enumerate(reads) if 0 < len(read) < L and 0 <= place[r]
             and len(read) < len(contigs[place[r]])]
    assert len(tails) >= 10
    r = case["negative_shift"]
    assert len(contigs[place[r]]) < len(reads[r]) < L and rec[r][3] < 0
    assert reads[case["empty_read"]] == "" and contigs[place[case["empty_contig"]]] == ""
    assert place[case["unplaced"]] == -1 and rec[case["score_zero"]][2] == 0
    assert rec[case["gap_read"]][1].count("-") == 60 and rec[case["ins_read"]][0].count("-") == 30
    assert "N" in reads[case["n_in_read"]] and any("N" in c for c in contigs)
    assert len(set(contigs)) < len(contigs)
    # the read placed away from its best contig scores more on contig 0, which holds it whole
    r = case["not_its_best"]
    assert reads[r] in contigs[0] and place[r] == 1 and rec[r][2] < 10 * len(reads[r])


def test_host_form_equals_the_restatement_over_the_reference_alignments(golden):
    reads, contigs, place, rec, L = (golden[k] for k in ("reads", "contigs", "place", "records", "read_length"))
    for min_depth in (1, 3):
        want = restate(contigs, reads, place, L, rec, min_depth)
        got = consensus_host(reads, contigs, place, L, *_scoring(golden), min_depth)
        assert_same(got, want, min_depth)
    # aln: the reference's score, and the real columns from its start / end and the window rule
    for r, read in enumerate(reads):
        if place[r] < 0 or rec[r][2] == 0:
            assert got["aln"][r].tolist() == [0, 0, 0]
            continue
        lo, _, shift = window(len(read), len(contigs[place[r]]), L)
        assert got["aln"][r].tolist() == [rec[r][2], rec[r][3] - shift + lo, rec[r][4] - shift + lo], r
    case = golden["meta"]["cases"]
    off = np.concatenate(([0], np.cumsum([len(c) for c in contigs])))
    counts = got["counts"]
    gap = counts[off[4]:off[5]]
    assert gap[20:80, 4].tolist() == [1] * 60 and gap[:, 4].sum() == 60
    ins = counts[off[5]:off[6]]
    assert ins[:, 5].sum() == 30 and ins[:, 5].max() == 30 and ins[:, 4].sum() == 0
    r = case["negative_shift"]
    assert got["aln"][r, 1] >= 0 and got["aln"][r, 2] <= len(contigs[place[r]])
    assert got["n_other"] == 1  # the N of a read on a diagonal; the contig's N only receives votes
    # both copies of the repeated contig hold votes of their own
    assert counts[off[1]:off[2], :4].sum() > 0 and counts[off[2]:off[3], :4].sum() == len(reads[-1])
    # the two tie columns of the last contig: A = C = 2 under an A (kept), A = C = 2 under a G (A wins)
    tie = counts[off[8]:off[9]]
    assert tie[10].tolist() == [2, 2, 0, 0, 0, 0] and tie[20].tolist() == [2, 2, 0, 0, 0, 0]
    called = got["called"][off[8]:off[9]].tobytes().decode()
    assert contigs[8][10] == "A" and called[10] == "A" and contigs[8][20] == "G" and called[20] == "A"
    # without the counts the results are the same
    lean = consensus_host(reads, contigs, place, L, *_scoring(golden), 3, counts=False)
    assert "counts" not in lean and np.array_equal(lean["called"], got["called"])
    assert np.array_equal(lean["aln"], got["aln"]) and lean["n_changed"] == got["n_changed"]


def test_result_does_not_depend_on_the_order_of_the_reads(golden):
    reads, contigs, place, L = (golden[k] for k in ("reads", "contigs", "place", "read_length"))
    a = consensus_host(reads, contigs, place, L, *_scoring(golden))
    b = consensus_host(reads[::-1], contigs, place[::-1], L, *_scoring(golden))
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["called"], b["called"])
    assert np.array_equal(a["aln"], b["aln"][::-1]) and a["n_other"] == b["n_other"]


def test_planted_errors_are_removed_by_error_free_reads():
    g, truth, contigs, reads = planted()
    assert [_mismatches(c, t) for c, t in zip(contigs, truth)] == [6, 3, 0]
    polished, pile = cs.polish_contigs(contigs, reads, 40, device=False)
    assert polished == truth
    assert pile.n_changed == 9 and pile.n_other == 0 and pile.rounds == 1
    assert [c.shape for c in pile.counts] == [(300, 6), (300, 6), (60, 6)] and pile.called == truth
    assert pile.place.dtype == np.int32 and pile.aln.shape == (len(reads), 3)


def test_rounds_stop_after_a_round_that_changed_nothing():
    g, truth, contigs, reads = planted()
    polished, pile = cs.polish_contigs(contigs, reads, 40, rounds=2, device=False)
    assert polished == truth and pile.n_changed == 0 and pile.rounds == 2
    polished, pile = cs.polish_contigs(contigs, reads, 40, rounds=5, device=False)
    assert polished == truth and pile.n_changed == 0 and pile.rounds == 2
    with pytest.raises(_lib.OvlError):
        cs.polish_contigs(contigs, reads, 40, rounds=0)


@pytest.mark.parametrize("seed", ["1", "2", "3", "4"])
def test_noisy_reads_leave_fewer_mismatches(golden, seed):
    g, truth, contigs, _ = planted()
    reads = golden["noisy"][seed]
    assert len(reads) == 281 and sum(_mismatches(r, g[p:p + 40]) for r, p in zip(reads, range(0, 561, 2))) > 200
    polished, pile = cs.polish_contigs(contigs, reads, 40, device=False)
    before = [_mismatches(c, t) for c, t in zip(contigs, truth)]
    after = [_mismatches(c, t) for c, t in zip(polished, truth)]
    print(f"seed {seed}: mismatches {before} -> {after}")
    assert [len(c) for c in polished] == [300, 300, 60]
    assert after[0] < before[0] and after[1] < before[1] and polished[2] == contigs[2]


def test_counts_sum_to_read_depth_coverage(golden):
    """Reads of upper-case ACGT, none longer than its contig: A + C + G + T + gap per base is the coverage that
    read_depth's [start:end) += 1 gives for the same placement."""
    reads, contigs, L = golden["reads"], golden["contigs"], golden["read_length"]

    class First:
        def randint(self, lo, hi):
            return 0

    keep = [c for c in contigs if len(c) >= 150]  # three contigs, one of them repeated
    assert len(keep) == 3 and len(set(keep)) == 2
    rs = [r for r in reads[:60] if set(r) <= set("ACGT")]
    depth = pm.read_depth(keep, rs, L, *_scoring(golden), device=False, rng=First())
    assert np.array_equal(depth.chosen, depth.first_best)
    pile = cs.pileup(keep, rs, L, depth=depth, device=False)
    assert np.array_equal(pile.place, depth.chosen)
    coverage = [np.zeros(len(c)) for c in keep]  # per position: a repeated contig's copies apart
    for r in range(len(rs)):
        coverage[depth.chosen[r]][int(depth.start[r]):int(depth.end[r])] += 1
    for k in range(len(keep)):
        assert np.array_equal(pile.counts[k][:, :5].sum(axis=1), coverage[k]), k
    assert sum(c.sum() for c in coverage) > 1500
    # place=None without a depth object: first_best of read_best_host, the same placement
    again = cs.pileup(keep, rs, L, device=False)
    assert np.array_equal(again.place, pile.place) and again.called == pile.called


def test_min_depth_above_every_depth_changes_nothing():
    g, truth, contigs, reads = planted()
    pile = cs.pileup(contigs, reads, 40, min_depth=1000, device=False)
    assert pile.n_changed == 0 and pile.called == contigs
    assert max(int(c[:, :4].sum(axis=1).max()) for c in pile.counts) < 1000


def test_device_none_follows_the_cell_threshold():
    """Below CONSENSUS_DEVICE_MIN_CELLS the host form runs even when an engine is given; from it the engine is
    asked.  The stand-in engine answers with the host form's results, so no GPU is needed."""
    g, truth, contigs, reads = planted()

    class Engine:
        calls = 0

        def consensus(self, reads, contigs, place, read_length, match, mismatch, indel, min_depth):
            self.calls += 1
            return consensus_host(reads, contigs, place, read_length, match, mismatch, indel, min_depth)

    eng = Engine()
    place = np.zeros(len(reads), dtype=np.int32)
    few = 3
    assert few * 40 * 300 < cs.CONSENSUS_DEVICE_MIN_CELLS <= len(reads) * 40 * 300
    a = cs.pileup(contigs, reads[:few], 40, place=place[:few], engine=eng)
    assert eng.calls == 0
    b = cs.pileup(contigs, reads, 40, place=place, engine=eng)
    assert eng.calls == 1
    cs.pileup(contigs, reads, 40, place=place, engine=eng, device=False)
    assert eng.calls == 1
    c = cs.pileup(contigs, reads[:few], 40, place=place[:few], engine=eng, device=True)
    assert eng.calls == 2 and c.called == a.called and len(b.called) == 3
    with pytest.raises(_lib.OvlError) as e:
        cs.pileup(contigs, reads, 40, place=place[:few], device=False)
    assert e.value.code == -1


def test_argument_errors_of_the_abi():
    L = _lib.load()
    buf, offs = encode_reads(["ACGT", "ACGTACGT"])
    r_off, c_off = np.ascontiguousarray(offs[:2]), np.ascontiguousarray(offs[1:])
    place = np.zeros(1, dtype=np.int32)
    counts = np.full((8, 6), 77, dtype=np.int32)
    called = np.full(8, 77, dtype=np.uint8)
    aln = np.full(3, 77, dtype=np.int32)
    n_changed, n_other = ctypes.c_int64(77), ctypes.c_int64(77)
    P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731

    def call(reads=buf, ro=r_off, nr=1, contigs=buf, co=c_off, nc=1, pl=place, rl=4, match=10, min_depth=3,
             out=called, changed=ctypes.byref(n_changed)):
        return L.ovl_consensus_host(P(reads), P(ro), nr, P(contigs), P(co), nc, P(pl), rl, match, -1, -1, min_depth,
                                    P(counts), P(out), changed, ctypes.byref(n_other), P(aln))

    bad = np.array([4, 0], dtype=np.int64)
    far = np.array([0, 1 << 20], dtype=np.int64)
    cases = [(dict(nr=-1), -1), (dict(nc=-1), -1), (dict(rl=-1), -1), (dict(ro=None), -1), (dict(co=None), -1),
             (dict(pl=None), -1), (dict(reads=None), -1), (dict(contigs=None), -1), (dict(ro=bad), -1),
             (dict(co=bad), -1), (dict(out=None), -1), (dict(changed=None), -1), (dict(min_depth=0), -1),
             (dict(pl=np.array([1], dtype=np.int32)), -7), (dict(pl=np.array([-2], dtype=np.int32)), -7),
             (dict(match=1 << 22), -4), (dict(ro=far), -4), (dict(co=far), -4)]
    for kw, code in cases:
        assert call(**kw) == code, kw
        assert _lib.last_error()
    for a in (counts, called, aln):
        assert (a == 77).all()
    assert n_changed.value == 77 and n_other.value == 77
    assert call(min_depth=1) == 0
    assert counts[:4, :4].tolist() == np.eye(4, dtype=int).tolist() and not counts[4:].any()
    assert called.tobytes() == b"ACGTACGT" and aln.tolist() == [40, 0, 4] and n_changed.value == n_other.value == 0
    # a read beyond the pair limits that is not placed is no error
    assert call(ro=far, reads=np.zeros(1 << 20, dtype=np.uint8), pl=np.array([-1], dtype=np.int32)) == 0
    assert set(("ovl_consensus", "ovl_consensus_host", "ovl_last_consensus")) <= set(_lib.SIGNATURES)


def test_python_layer_argument_errors_one_per_code():
    with pytest.raises(_lib.OvlError) as e:
        consensus_host(["ACGT"], ["ACGT"], [0], 4, min_depth=0)
    assert e.value.code == -1
    with pytest.raises(_lib.OvlError) as e:
        consensus_host(["ACGT"], ["ACGT"], [1], 4)
    assert e.value.code == -7
    with pytest.raises(_lib.OvlError) as e:
        consensus_host(["ACGT" * 8], ["ACGT" * 8], [0], 4, match=1 << 22)
    assert e.value.code == -4
    with pytest.raises(_lib.OvlError) as e:
        consensus_host(["ACGΔ"], ["ACGT"], [0], 4)
    assert e.value.code == -4
    res = consensus_host([], ["ACGT", ""], [], 4)
    assert res["called"].tobytes() == b"ACGT" and res["aln"].shape == (0, 3) and res["counts"].shape == (4, 6)
    res = consensus_host(["ACGT"], [], [-1], 4)
    assert res["called"].shape == (0,) and res["aln"].tolist() == [[0, 0, 0]]

