"""Read-depth coverage on the GPU (ovl_read_best: ovl_local_lane.hip, ovl_depth_api.cpp) against the oracle's
``align_read_or_contig_to_reference`` for every (read, contig) pair, the host form and the reference's recorded
results (tests/golden/read_depth.json).

The lane kernel gives one lane one read and sweeps a contig with a wavefront's 64 reads: the shapes here mix every
read length that takes another path inside one wavefront (empty, shorter than read_length and so aligned to the
contig's tail, longer than the contig, at the 64-row boundary, beyond the kernel's 128 rows and so sent through the
batched kernel in the same call), cross the wavefront boundary in reads and the 32-bit tie word in contigs, and
repeat contigs.  One oracle matrix per scoring is computed once and sliced by every shape.
"""
import random

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

SCORINGS = ((10, -1, -1), (2, -3, -5), (1, -1, -1))  # test_gpu_local_batch.py's
READ_LENGTH = 50
READ_LENGTHS = (0, 1, 7, READ_LENGTH - 1, READ_LENGTH, 63, 64, 65, 100, 129)
CONTIG_LENGTHS = (0, 1, 5, 63, 64, 65, 127, 300, 700)
N_READS, N_CONTIGS = 130, 65
SHAPES = ((130, 65), (1, 1), (63, 2), (64, 31), (65, 32), (64, 33), (1, 65), (65, 65))


@pytest.fixture(scope="module")
def engine():
    from ovlgraph import OverlapEngine
    eng = OverlapEngine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def inputs():
    from ovlgraph.reads import read_genome_from_fasta
    genome = read_genome_from_fasta()
    rng = random.Random(950)
    st = rng.randint(0, len(genome) - 1000)
    g = genome[st:st + 1000]
    # the long gap: A + B against A + 60 x "T" + B, one gap of 60 for 250 points of matches
    a = "".join(rng.choice("ACG") for _ in range(25))
    b = "".join(rng.choice("ACG") for _ in range(25))
    contigs = []
    for k in range(N_CONTIGS):
        m = CONTIG_LENGTHS[k % len(CONTIG_LENGTHS)]
        lo = rng.randint(0, len(g) - m)
        contigs.append(g[lo:lo + m])
    contigs[1], contigs[2] = a + "T" * 60 + b, contigs[7]    # the gap contig early; 2 and 7 repeat (300 bases)
    contigs[40], contigs[64] = contigs[7], contigs[8]        # repeats across the tie words
    reads = []
    for k in range(N_READS):
        n = READ_LENGTHS[k % len(READ_LENGTHS)]
        src = contigs[rng.choice((2, 7, 8, 16, 17, 25, 26))]  # a 300- or 700-base contig
        lo = rng.randint(0, len(src) - n)
        s = list(src[lo:lo + n])
        for i in range(len(s)):
            if rng.random() < 0.03:
                s[i] = rng.choice("ACGT")
        if n > 20 and rng.random() < 0.3:
            del s[rng.randint(5, n - 5)]
            s.append(rng.choice("ACGT"))
        reads.append("".join(s))
    reads[4] = a + b
    assert len(reads[4]) == READ_LENGTH
    return reads, contigs


_TRIPLES = {}


@pytest.fixture(scope="module")
def triples(inputs, oracle_mod):
    """scoring -> (reads x contigs x 3) int64: the oracle's (score, start, end), computed once per scoring."""
    reads, contigs = inputs

    def get(params):
        if params not in _TRIPLES:
            t = np.zeros((len(reads), len(contigs), 3), dtype=np.int64)
            for r, read in enumerate(reads):
                for c, contig in enumerate(contigs):
                    t[r, c] = oracle_mod.align_read_or_contig_to_reference(read, contig, READ_LENGTH, *params)[3:6]
            t.setflags(write=False)
            _TRIPLES[params] = t
        return _TRIPLES[params]
    return get


def expected(t):
    """The selection of plots.py:126-131 over a (reads x contigs x 3) block of triples."""
    R, C = t.shape[:2]
    best = t[:, :, 0].max(axis=1)
    tie = t[:, :, 0] == best[:, None]
    first = tie.argmax(axis=1)
    idx = np.arange(R)
    bits = np.zeros((R, (C + 31) // 32), dtype=np.uint32)
    for c in range(C):
        bits[:, c >> 5] |= tie[:, c].astype(np.uint32) << np.uint32(c & 31)
    return {"best_score": best, "first_best": first, "n_best": tie.sum(axis=1), "start": t[idx, first, 1],
            "end": t[idx, first, 2], "tie_bits": bits}


def assert_matches(res, t, what):
    want = expected(t)
    if "scores" in res:
        bad = np.argwhere(res["scores"] != t[:, :, 0])
        assert bad.size == 0, (what, "scores", bad[:5].tolist())
    for k, w in want.items():
        assert res[k].shape == w.shape, (what, k)
        bad = np.flatnonzero((res[k] != w).reshape(w.shape[0], -1).any(axis=1))
        assert bad.size == 0, (what, k, bad[:5].tolist(), res[k][bad[:5]].tolist(), w[bad[:5]].tolist())


def test_inputs_mix_every_path_in_one_wavefront(inputs):
    reads, contigs = inputs
    first_wave = {len(r) for r in reads[:64]}
    assert first_wave == set(READ_LENGTHS) and {len(c) for c in contigs} >= set(CONTIG_LENGTHS) - {1}
    assert len(set(contigs)) < len(contigs) and max(map(len, reads)) > 128


@pytest.mark.parametrize("params", SCORINGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_read_best_matches_the_oracle(engine, inputs, triples, params, shape):
    reads, contigs = inputs
    nr, nc = shape
    t = triples(params)[:nr, :nc]
    res = engine.read_best(reads[:nr], contigs[:nc], READ_LENGTH, *params, scores=True)
    assert_matches(res, t, (params, shape))
    last = engine.last_read_best()
    n_long = sum(len(r) > 128 for r in reads[:nr])
    assert last["lane_pairs"] == (nr - n_long) * nc and last["fallback_pairs"] == n_long * nc
    assert last["launches"] == 1
    if shape == SHAPES[0]:
        # without this the test could pass on the existing kernels alone
        assert last["lane_pairs"] > 0 and last["fallback_pairs"] > 0
        if params == SCORINGS[0]:
            score, start, end = t[4, 1]
            assert score == 440 and end - start == 110 > 2 * len(reads[4]) and res["first_best"][4] == 1


def test_without_the_score_matrix_and_reused_buffers(engine, inputs, triples):
    """The same engine serves a large call, a small one and the large one again: its buffers are reused."""
    reads, contigs = inputs
    params = SCORINGS[0]
    big = engine.read_best(reads, contigs, READ_LENGTH, *params)
    assert "scores" not in big
    assert_matches(big, triples(params), "big")
    small = engine.read_best(reads[60:67], contigs[30:35], READ_LENGTH, *params)
    assert_matches(small, triples(params)[60:67, 30:35], "small")
    again = engine.read_best(reads, contigs, READ_LENGTH, *params)
    for k in big:
        assert np.array_equal(big[k], again[k]), k


def test_several_chunks_of_contigs(monkeypatch, inputs, triples):
    """OVL_READ_BEST_CHUNK=32: three launches over 65 contigs, a read's best moving from chunk to chunk."""
    from ovlgraph import OverlapEngine
    reads, contigs = inputs
    monkeypatch.setenv("OVL_READ_BEST_CHUNK", "32")
    with OverlapEngine(0) as eng:
        for params in SCORINGS[:2]:
            res = eng.read_best(reads, contigs, READ_LENGTH, *params, scores=True)
            assert eng.last_read_best()["launches"] == 3
            assert_matches(res, triples(params), ("chunks", params))
            # contigs reversed: improvements arrive late, so earlier tie words are cleared
            rev = eng.read_best(reads, contigs[::-1], READ_LENGTH, *params)
            assert_matches(rev, triples(params)[:, ::-1], ("chunks reversed", params))


def test_wavefronts_that_sweep_several_contigs(engine):
    """More contigs than the launch has wavefronts per read group (eight per CU): a wavefront sweeps one contig
    after another and must start each from a cleared column.  Checked against the host form, which the tests above
    and tests/test_read_depth_cpu.py pin to the oracle and the reference."""
    from ovlgraph.engine import read_best_host
    from ovlgraph.reads import read_genome_from_fasta
    genome = read_genome_from_fasta()
    rng = random.Random(7)
    contigs = []
    for _ in range(4500):
        m = rng.randint(0, 40)
        lo = rng.randint(0, len(genome) - m)
        contigs.append(genome[lo:lo + m])
    reads = []
    for n in (0, 12, 33, 39, 40, 41, 64, 90):
        lo = rng.randint(0, len(genome) - n)
        reads.append(genome[lo:lo + n])
    dev = engine.read_best(reads, contigs, 40, scores=True)
    assert engine.last_read_best() == {"lane_pairs": 8 * 4500, "fallback_pairs": 0, "launches": 1}
    host = read_best_host(reads, contigs, 40, scores=True)
    for k in host:
        assert np.array_equal(dev[k], host[k]), k


def test_scorings_outside_the_lane_kernel_take_the_existing_kernels(engine, inputs, oracle_mod):
    reads, contigs = inputs
    reads, contigs = reads[:12], contigs[:9]
    params = (3, 1, -2)  # a positive mismatch score: padding rows could win
    t = np.array([[oracle_mod.align_read_or_contig_to_reference(r, c, READ_LENGTH, *params)[3:6] for c in contigs]
                  for r in reads], dtype=np.int64)
    res = engine.read_best(reads, contigs, READ_LENGTH, *params, scores=True)
    assert_matches(res, t, params)
    assert engine.last_read_best() == {"lane_pairs": 0, "fallback_pairs": 12 * 9, "launches": 0}


def test_host_form_matches_the_oracle(inputs, triples):
    from ovlgraph.engine import read_best_host
    reads, contigs = inputs
    params = SCORINGS[0]
    res = read_best_host(reads[:70], contigs[:33], READ_LENGTH, *params, scores=True)
    assert_matches(res, triples(params)[:70, :33], "host")


def test_read_depth_on_the_device_equals_the_host_form_and_the_fixture(engine):
    from ovlgraph import performanceMeasures as pm
    g = load_golden("read_depth.json")
    reads, contigs, L = g["reads"], g["contigs"], g["read_length"]
    args = (g["match"], g["mismatch"], g["indel"])
    np.random.seed(2026)
    dev = pm.read_depth(contigs, reads, L, *args, engine=engine, device=True)
    assert engine.last_read_best()["lane_pairs"] == len(reads) * len(contigs)
    np.random.seed(2026)
    host = pm.read_depth(contigs, reads, L, *args, device=False)
    t = np.array(g["triples"], dtype=np.int64)
    want = expected(t)
    for d in (dev, host):
        for k in ("best_score", "first_best", "n_best", "start", "end"):
            assert np.array_equal(getattr(d, k), want[k]), k
    assert np.array_equal(dev.chosen, host.chosen) and list(dev.coverage) == list(host.coverage)
    for r in range(len(reads)):
        assert list(dev.ties(r)) == list(host.ties(r)) == np.flatnonzero(t[r, :, 0] == want["best_score"][r]).tolist()
    for contig in host.coverage:
        assert np.array_equal(dev.coverage[contig], host.coverage[contig])
    assert sum(v.sum() for v in dev.coverage.values()) > 0


def test_argument_errors_leave_the_outputs_alone(engine):
    from ovlgraph._lib import OvlError
    with pytest.raises(OvlError) as e:
        engine.read_best(["ACGT"], ["ACGT"], -1)
    assert e.value.code == -1
    with pytest.raises(OvlError) as e:
        engine.read_best(["ACGT" * 8], ["ACGT" * 8], 4, match=1 << 22)
    assert e.value.code == -4
    res = engine.read_best(["ACGT"], [], 4)
    assert res["first_best"].tolist() == [-1] and res["best_score"].tolist() == [0]
    assert engine.read_best([], ["ACGT"], 4)["best_score"].shape == (0,)


def test_timing_covers_the_score_pass(engine):
    """Eight 32-base reads against three contigs of about 100 bases at the default scoring: the lane kernel takes them
    all, and kernel_ms is its launches and folds."""
    from ovlgraph.reads import read_genome_from_fasta
    from stage_timing import assert_kernel_inside_call, timed_and_untimed
    genome = read_genome_from_fasta()
    contigs = [genome[0:100], genome[80:185], genome[150:248]]
    reads = [genome[lo:lo + 32] for lo in (0, 20, 60, 85, 110, 150, 190, 215)]
    got_on, on, got_off, off = timed_and_untimed(engine, lambda: engine.read_best(reads, contigs, 32),
                                                 engine.last_read_best)
    assert on["lane_pairs"] == off["lane_pairs"] == 8 * 3 and on["launches"] == 1
    assert_kernel_inside_call(on, off)
    for k in got_on:
        assert np.array_equal(got_on[k], got_off[k]), k
