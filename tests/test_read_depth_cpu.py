"""Read-depth coverage without a GPU: ovl_read_best_host and performanceMeasures.read_depth against the reference's
own per-pair results (tests/golden/read_depth.json, written by tools/gen_golden_read_depth.py from
aligners.py:170-202), the selection and accumulation of plots.py:115-135 restated literally, the draw pinned
against np.random.choice, and the argument errors of the ABI."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from ovlgraph import _lib
from ovlgraph import performanceMeasures as pm
from ovlgraph.engine import encode_reads, read_best_host


@pytest.fixture(scope="module")
def golden():
    return load_golden("read_depth.json")


def _scoring(g):
    return g["match"], g["mismatch"], g["indel"]


def literal_depth(contigs, triples, choice):
    """plots.py:115-135 over recorded (score, start, end) triples, with the six-tuple's indices.  ``choice`` is
    given the list of tied contig positions; the reference draws from the contig strings, which consumes the stream
    the same way."""
    coverage = {contig: np.zeros(len(contig), dtype=float) for contig in contigs}
    picked = []
    for row in triples:
        best_score = -float("inf")
        best_contigs = []
        best_start = best_end = None
        for c, (score, start, end) in enumerate(row):
            if score > best_score:
                best_score = score
                best_contigs = [c]
                best_start, best_end = start, end
            elif score == best_score:
                best_contigs.append(c)
        if best_contigs:
            chosen = int(choice(best_contigs))
            coverage[contigs[chosen]][best_start:best_end] += 1
            picked.append((best_score, best_contigs, chosen, best_start, best_end))
    return coverage, picked


def assert_depth_matches(depth, contigs, coverage, picked):
    assert list(depth.coverage) == list(coverage)  # first-occurrence order
    for contig in coverage:
        assert depth.coverage[contig].dtype == np.float64
        assert np.array_equal(depth.coverage[contig], coverage[contig]), contig
    for name in ("best_score", "first_best", "n_best", "chosen", "start", "end"):
        arr = getattr(depth, name)
        assert arr.dtype == np.int32 and arr.shape == (len(picked),), name
    for r, (best, ties, chosen, start, end) in enumerate(picked):
        got = (int(depth.best_score[r]), int(depth.first_best[r]), int(depth.n_best[r]), int(depth.chosen[r]),
               int(depth.start[r]), int(depth.end[r]))
        assert got == (best, ties[0], len(ties), chosen, start, end), r
        assert list(depth.ties(r)) == ties, r


def test_fixture_covers_the_edge_cases(golden):
    reads, contigs, triples, L = golden["reads"], golden["contigs"], golden["triples"], golden["read_length"]
    assert len(triples) == len(reads) and all(len(row) == len(contigs) for row in triples)
    n_best = [sum(1 for t in row if t[0] == max(x[0] for x in row)) for row in triples]
    assert sum(k >= 2 for k in n_best) >= 20 and any(k >= 3 for k in n_best)
    assert any(0 < len(r) < L for r in reads) and "" in reads and any(len(r) > L for r in reads)
    assert "" in contigs and len(set(contigs)) < len(contigs) and any(0 < len(c) < L for c in contigs)
    gr, gc = golden["meta"]["gap_read"], golden["meta"]["gap_contig"]
    score, start, end = triples[gr][gc]
    assert score == 340 and end - start > 2 * len(reads[gr])


def test_host_form_matches_the_reference_pair_by_pair(golden):
    reads, contigs, triples = golden["reads"], golden["contigs"], golden["triples"]
    res = read_best_host(reads, contigs, golden["read_length"], *_scoring(golden), scores=True)
    want = np.array([[t[0] for t in row] for row in triples], dtype=np.int32)
    assert res["scores"].dtype == np.int32 and np.array_equal(res["scores"], want)
    _, picked = literal_depth(contigs, triples, lambda ties: ties[0])
    for r, (best, ties, _, start, end) in enumerate(picked):
        got = (int(res["best_score"][r]), int(res["first_best"][r]), int(res["n_best"][r]), int(res["start"][r]),
               int(res["end"][r]))
        assert got == (best, ties[0], len(ties), start, end), r
        bits = [c for c in range(len(contigs)) if (int(res["tie_bits"][r, c >> 5]) >> (c & 31)) & 1]
        assert bits == ties, r
    # without the score matrix the results are the same
    lean = read_best_host(reads, contigs, golden["read_length"], *_scoring(golden))
    assert "scores" not in lean
    for k in ("best_score", "first_best", "n_best", "start", "end", "tie_bits"):
        assert np.array_equal(lean[k], res[k]), k


def test_read_depth_equals_the_literal_loop(golden):
    reads, contigs, triples = golden["reads"], golden["contigs"], golden["triples"]
    np.random.seed(1234)
    coverage, picked = literal_depth(contigs, triples, np.random.choice)
    after = np.random.randint(0, 1 << 30)
    assert len({p[2] for p in picked if len(p[1]) > 1}) > 1  # the draws do pick different positions
    np.random.seed(1234)
    depth = pm.read_depth(contigs, reads, golden["read_length"], *_scoring(golden), device=False)
    assert np.random.randint(0, 1 << 30) == after  # one draw per read, no more
    assert_depth_matches(depth, contigs, coverage, picked)
    # a RandomState of its own, the module's stream untouched
    ref_rng = np.random.RandomState(77)
    coverage, picked = literal_depth(contigs, triples, ref_rng.choice)
    np.random.seed(5)
    depth = pm.read_depth(contigs, reads, golden["read_length"], *_scoring(golden), device=False,
                          rng=np.random.RandomState(77))
    np.random.seed(5)
    first = np.random.randint(0, 1 << 30)
    np.random.seed(5)
    assert np.random.randint(0, 1 << 30) == first
    assert_depth_matches(depth, contigs, coverage, picked)


def test_device_none_follows_the_cell_threshold(golden):
    """Below READ_DEPTH_DEVICE_MIN_CELLS the host form runs even when an engine is given; from it the engine is
    asked.  The stand-in engine answers with the host form's results, so no GPU is needed."""
    reads, contigs, L = golden["reads"], golden["contigs"], golden["read_length"]

    class Engine:
        calls = 0

        def read_best(self, reads, contigs, read_length, match, mismatch, indel):
            self.calls += 1
            return read_best_host(reads, contigs, read_length, match, mismatch, indel)

    small_r, small_c = reads[:5], contigs[:3]
    assert sum(map(len, small_r)) * sum(map(len, small_c)) < pm.READ_DEPTH_DEVICE_MIN_CELLS
    assert sum(map(len, reads)) * sum(map(len, contigs)) >= pm.READ_DEPTH_DEVICE_MIN_CELLS
    eng = Engine()
    a = pm.read_depth(small_c, small_r, L, engine=eng, rng=np.random.RandomState(3))
    assert eng.calls == 0
    b = pm.read_depth(small_c, small_r, L, device=False, rng=np.random.RandomState(3))
    assert np.array_equal(a.chosen, b.chosen) and all(np.array_equal(a.coverage[c], b.coverage[c]) for c in small_c)
    big = pm.read_depth(contigs, reads, L, engine=eng, rng=np.random.RandomState(3))
    assert eng.calls == 1
    pm.read_depth(contigs, reads, L, engine=eng, device=False, rng=np.random.RandomState(3))
    assert eng.calls == 1
    forced = pm.read_depth(small_c, small_r, L, engine=eng, device=True, rng=np.random.RandomState(3))
    assert eng.calls == 2 and np.array_equal(forced.chosen, a.chosen) and big.chosen.shape == (len(reads),)


def test_draw_consumes_the_stream_as_np_random_choice():
    """plots.py:134 calls np.random.choice(best_contigs); read_depth calls rng.randint(0, n).  Same index, same
    stream afterwards, n = 1 included, for the module's stream and for a RandomState."""
    sizes = [1, 2, 3, 1, 8, 2, 1, 1, 5, 33, 2, 65, 1]
    for make in (lambda: np.random, lambda: np.random.RandomState(99)):
        np.random.seed(42)
        rng = make()
        by_choice = [int(rng.choice(list(range(100, 100 + n)))) - 100 for n in sizes]
        tail_choice = rng.randint(0, 1 << 30, size=4).tolist()
        np.random.seed(42)
        rng = make()
        by_randint = [int(rng.randint(0, n)) for n in sizes]
        tail_randint = rng.randint(0, 1 << 30, size=4).tolist()
        assert by_choice == by_randint and tail_choice == tail_randint
    # contig strings, as the reference passes them
    np.random.seed(7)
    picked = np.random.choice(["ACGT", "GG", "ACGT"])
    np.random.seed(7)
    assert ["ACGT", "GG", "ACGT"][np.random.randint(0, 3)] == picked


def test_repeated_contigs_share_one_array_and_slices_clip():
    # both reads score best on the long contig at position 0 and tie with its copy at position 2
    long, short = "ACGTTGCAAGGCTTAACCGG", "ACGTT"
    contigs = [long, short, long]
    reads = [long[8:20], long[0:12]]

    class Pick:
        def __init__(self, picks):
            self.picks, self.seen = list(picks), []

        def randint(self, lo, hi):
            self.seen.append((lo, hi))
            return self.picks.pop(0)

    rng = Pick([1, 0])
    depth = pm.read_depth(contigs, reads, 12, device=False, rng=rng)
    assert rng.seen == [(0, 2), (0, 2)]
    assert list(depth.coverage) == [long, short] and depth.chosen.tolist() == [2, 0]
    want = np.zeros(20)
    want[8:20] += 1
    want[0:12] += 1
    assert np.array_equal(depth.coverage[long], want) and not depth.coverage[short].any()
    # the stretch comes from the first best contig, the array from the chosen one: a shorter chosen contig clips
    contigs = ["TTTTTTTT" + "ACGTACGTAC", "ACGTACGTAC"]
    depth = pm.read_depth(contigs, ["ACGTACGTAC"], 10, device=False, rng=Pick([1]))
    assert (int(depth.start[0]), int(depth.end[0]), depth.n_best[0], depth.chosen[0]) == (8, 18, 2, 1)
    assert np.array_equal(depth.coverage[contigs[1]], [0] * 8 + [1] * 2) and not depth.coverage[contigs[0]].any()


def test_no_contigs_and_no_reads():
    class Never:
        def randint(self, lo, hi):
            raise AssertionError("a read without contigs draws nothing")

    depth = pm.read_depth([], ["ACGT", ""], 4, device=False, rng=Never())
    assert depth.coverage == {} and depth.first_best.tolist() == [-1, -1] and depth.chosen.tolist() == [-1, -1]
    for name in ("best_score", "n_best", "start", "end"):
        assert getattr(depth, name).tolist() == [0, 0]
    assert list(depth.ties(0)) == []
    depth = pm.read_depth(["ACGT", "ACGT", "GG"], [], 4, device=False, rng=Never())
    assert list(depth.coverage) == ["ACGT", "GG"] and not any(v.any() for v in depth.coverage.values())
    assert depth.best_score.shape == (0,) and depth.chosen.shape == (0,)
    res = read_best_host([], [], 4)
    assert res["best_score"].shape == (0,) and res["tie_bits"].shape == (0, 0)


def test_argument_errors_of_the_abi():
    L = _lib.load()
    buf, offs = encode_reads(["ACGT", "ACGTACGT"])
    r_off, c_off = np.ascontiguousarray(offs[:2]), np.ascontiguousarray(offs[1:])
    outs = [np.full(2, 77, dtype=np.int32) for _ in range(5)]
    bits = np.full(2, 77, dtype=np.uint32)
    scores = np.full(2, 77, dtype=np.int32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731

    def call(reads=buf, ro=r_off, nr=1, contigs=buf, co=c_off, nc=1, rl=4, match=10, best=outs[0]):
        return L.ovl_read_best_host(P(reads), P(ro), nr, P(contigs), P(co), nc, rl, match, -1, -1, P(best),
                                    *[P(o) for o in outs[1:]], P(bits), P(scores))

    bad = np.array([4, 0], dtype=np.int64)
    far = np.array([0, 1 << 20], dtype=np.int64)
    cases = [(dict(nr=-1), -1), (dict(nc=-1), -1), (dict(rl=-1), -1), (dict(ro=None), -1), (dict(co=None), -1),
             (dict(reads=None), -1), (dict(contigs=None), -1), (dict(ro=bad), -1), (dict(co=bad), -1),
             (dict(best=None), -1), (dict(match=1 << 22), -4), (dict(ro=far), -4), (dict(co=far), -4)]
    for kw, code in cases:
        assert call(**kw) == code, kw
        assert _lib.last_error()
    for a in outs + [bits, scores]:
        assert (a == 77).all()
    assert call() == 0 and outs[0][0] == 40 and outs[0][1] == 77 and scores[0] == 40 and bits[0] == 1
    assert set(("ovl_read_best", "ovl_read_best_host", "ovl_last_read_best")) <= set(_lib.SIGNATURES)


def test_plot_reconstructed_coverage_calls_the_hook_per_contig_position(golden):
    reads, contigs, L = golden["reads"], golden["contigs"], golden["read_length"]

    class Plots:
        def __init__(self):
            self.calls = []

        def plot_contig_depth(self, *args):
            self.calls.append(args)

    plots = Plots()
    genome = "A" * 600
    depth = pm.plot_reconstructed_coverage(contigs, reads, len(reads), L, genome, "exp", 3, "some/path",
                                           device=False, rng=np.random.RandomState(11), plots=plots)
    want = pm.read_depth(contigs, reads, L, device=False, rng=np.random.RandomState(11))
    assert np.array_equal(depth.chosen, want.chosen)
    assert len(plots.calls) == len(contigs)
    for idx, (contig, args) in enumerate(zip(contigs, plots.calls)):
        contig_idx, cov, expected, name, it, path = args
        assert (contig_idx, name, it, path) == (idx, "exp", 3, "some/path")
        assert expected == len(reads) * L / len(genome)
        assert cov is depth.coverage[contig] and np.array_equal(cov, want.coverage[contig])
    # no plots object: nothing is called, the result is the same
    quiet = pm.plot_reconstructed_coverage(contigs, reads, len(reads), L, genome, "exp", 3, "some/path",
                                           device=False, rng=np.random.RandomState(11))
    assert np.array_equal(quiet.chosen, want.chosen)
