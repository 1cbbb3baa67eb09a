"""Consensus on the GPU (ovl_consensus: the batch alignment kernel, consensus_pileup_kernel and
consensus_vote_kernel of ovl_consensus.hip, ovl_consensus_api.cpp) against the host form bit for bit and, on the
smaller shapes, against the rule restated over the oracle's aligned strings (tests/consensus_cases.py).

The pileup kernel gives one wavefront one read and consumes its walk 64 ops at a time, carrying two prefix counts
from chunk to chunk: the shapes here put walks of 63, 64, 65, 127, 128, 129 and 200 ops next to each other, runs of
left and of up ops inside one chunk and across a chunk boundary, every window rule in one launch, many reads on the
same columns, read counts around the wavefront boundary, several chunks of reads, a read that leaves the batch
kernel for the single-pair path, and the two reads on either side of that boundary (1,024 and 1,025 bases) through
both callers of the routing rule.  One oracle restatement per scoring is computed once and shared.
"""
import random

import numpy as np
import pytest

from conftest import load_golden
from consensus_cases import assert_same, oracle_records, planted, restate

pytestmark = pytest.mark.gpu

SCORINGS = ((10, -1, -1), (2, -3, -5), (1, -1, -1))  # test_gpu_local_batch.py's
READ_LENGTH = 50
EXACT = (63, 64, 65, 127, 128, 129, 200)
N_POOL = 130


@pytest.fixture(scope="module")
def engine():
    from ovlgraph import OverlapEngine
    eng = OverlapEngine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def pool():
    """130 reads on a 300- and a 700-base contig: first error-free reads of the exact walk lengths, then reads of
    63 to 130 bases with 3 % substitutions and some single-base deletions; then the four gap cases."""
    from ovlgraph.reads import read_genome_from_fasta
    genome = read_genome_from_fasta()
    rng = random.Random(950)
    st = rng.randint(0, len(genome) - 1000)
    g = genome[st:st + 1000]
    contigs = [g[0:300], g[300:1000]]
    reads, place = [], []
    for n in EXACT:
        for c in (0, 1):
            lo = rng.randint(1, len(contigs[c]) - n - 1)
            reads.append(contigs[c][lo:lo + n])
            place.append(c)
    while len(reads) < N_POOL:
        c = len(reads) & 1
        n = rng.randint(63, 130)
        lo = rng.randint(0, len(contigs[c]) - n)
        s = list(contigs[c][lo:lo + n])
        for i in range(len(s)):
            if rng.random() < 0.03:
                s[i] = rng.choice("ACGT")
        if rng.random() < 0.3:
            del s[rng.randint(5, n - 5)]
        reads.append("".join(s))
        place.append(c)

    def acg(n):
        return "".join(rng.choice("ACG") for _ in range(n))
    gaps = {}
    for name, nb, run, kind in (("left_across", 25, 60, "left"), ("left_inside", 65, 60, "left"),
                                ("up_inside", 25, 30, "up"), ("up_across", 50, 30, "up")):
        a, b = acg(25), acg(nb)
        long, short = a + "T" * run + b, a + b
        contigs.append(long if kind == "left" else short)
        reads.append(short if kind == "left" else long)
        place.append(len(contigs) - 1)
        gaps[name] = (len(reads) - 1, len(contigs) - 1, nb, run, kind)
    return contigs, reads, np.array(place, dtype=np.int32), gaps


_WANT = {}


@pytest.fixture(scope="module")
def want(pool, oracle_mod):
    """scoring -> the oracle's records for the pool, computed once per scoring."""
    contigs, reads, place, _ = pool

    def get(params):
        if params not in _WANT:
            _WANT[params] = oracle_records(oracle_mod, contigs, reads, place.tolist(), READ_LENGTH, params)
        return _WANT[params]
    return get


def check(engine, contigs, reads, place, read_length, params=SCORINGS[0], min_depth=3, records=None, what=""):
    from ovlgraph.engine import consensus_host
    dev = engine.consensus(reads, contigs, place, read_length, *params, min_depth)
    host = consensus_host(reads, contigs, place, read_length, *params, min_depth)
    assert_same(dev, host, (what, "host"))
    if records is not None:
        assert_same(dev, restate(contigs, reads, list(place), read_length, records, min_depth), (what, "oracle"))
    return dev


def test_pool_holds_the_walk_lengths_and_the_gap_runs(pool, want):
    contigs, reads, place, gaps = pool
    rec = want(SCORINGS[0])
    walks = {len(r[0]) for r in rec}
    assert set(EXACT) <= walks and len(reads) == N_POOL + 4
    for name, (r, c, nb, run, kind) in gaps.items():
        a_ref, a_query = rec[r][0], rec[r][1]
        dashes = a_query if kind == "left" else a_ref
        assert dashes.count("-") == run and dashes[25:25 + run] == "-" * run, name
        first, last = nb, nb + run - 1  # the run's ops in walk order, from the alignment's end
        assert (first // 64 == last // 64) == name.endswith("inside"), name


@pytest.mark.parametrize("params", SCORINGS)
@pytest.mark.parametrize("n_reads", (1, 63, 64, 65, N_POOL, N_POOL + 4))
def test_device_equals_host_and_oracle(engine, pool, want, params, n_reads):
    contigs, reads, place, gaps = pool
    if n_reads > N_POOL:
        reads, place, rec = reads[N_POOL - 60:], place[N_POOL - 60:], want(params)[N_POOL - 60:]
    else:
        reads, place, rec = reads[:n_reads], place[:n_reads], want(params)[:n_reads]
    dev = check(engine, contigs, reads, place, READ_LENGTH, params, 3, rec, (params, n_reads))
    last = engine.last_consensus()
    assert last["batch_reads"] == len(reads) and last["single_reads"] == 0 and last["launches"] == 1
    assert last["ops"] == sum(len(r[0]) for r in rec if r[2] > 0)
    if n_reads > N_POOL and params == SCORINGS[0]:
        off = np.concatenate(([0], np.cumsum([len(c) for c in contigs])))
        for name, (r, c, nb, run, kind) in gaps.items():
            col = dev["counts"][off[c]:off[c + 1]]
            if kind == "left":
                assert col[25:25 + run, 4].tolist() == [1] * run and col[:, 4].sum() == run, name
            else:
                assert col[24, 5] == run and col[:, 5].sum() == run, name


def test_every_window_rule_in_one_launch(engine):
    """The golden input of tests/test_consensus_cpu.py: tail windows, the short read longer than its contig, an
    empty read, an empty contig, place = -1, a read that scores 0, N bytes, ties -- against the reference's own
    aligned strings."""
    g = load_golden("consensus.json")
    for min_depth in (1, 3):
        dev = check(engine, g["contigs"], g["reads"], g["place"], g["read_length"],
                    (g["match"], g["mismatch"], g["indel"]), min_depth, g["records"], "golden")
    assert dev["n_other"] == 1
    votes = sum(1 for r, p in zip(g["reads"], g["place"]) if p >= 0 and r and g["contigs"][p])
    assert engine.last_consensus()["batch_reads"] == votes


def test_many_reads_on_the_same_columns(engine, oracle_mod):
    _, truth, _, _ = planted()
    contig = truth[2]  # 60 bases
    rng = random.Random(7)
    same = [contig[10:50]] * 200
    dev = check(engine, [contig], same, [0] * 200, 40, what="200 copies")
    assert dev["counts"][10:50, :4].sum(axis=1).tolist() == [200] * 40 and dev["counts"][:, :4].sum() == 8000
    distinct = set()
    while len(distinct) < 65:
        p = rng.randint(0, 20)
        s = list(contig[p:p + 40])
        k = rng.randint(3, 36)
        s[k] = rng.choice([ch for ch in "ACGT" if ch != s[k]])
        distinct.add("".join(s))
    distinct = sorted(distinct)
    rec = oracle_records(oracle_mod, [contig], distinct, [0] * 65, 40, SCORINGS[0])
    dev = check(engine, [contig], distinct, [0] * 65, 40, records=rec, what="65 distinct")
    assert dev["counts"][20:40, :4].sum(axis=1).min() >= 60  # more than one wavefront of reads per column


def test_chunks_of_reads_give_the_same_result(monkeypatch, engine, pool):
    from ovlgraph import OverlapEngine
    contigs, reads, place, _ = pool
    reads, place = reads[:N_POOL], place[:N_POOL]
    whole = engine.consensus(reads, contigs, place, READ_LENGTH)
    assert engine.last_consensus()["launches"] == 1
    monkeypatch.setenv("OVL_CONSENSUS_CHUNK", "7")
    with OverlapEngine(0) as eng:
        parts = eng.consensus(reads, contigs, place, READ_LENGTH)
        last = eng.last_consensus()
    assert last["launches"] == (N_POOL + 6) // 7 and last["batch_reads"] == N_POOL
    assert_same(parts, whole, "chunks")


def test_a_long_read_takes_the_single_pair_path(engine, pool):
    from ovlgraph.reads import read_genome_from_fasta
    genome = read_genome_from_fasta()
    long_contig = genome[2000:3200]
    s = list(long_contig[40:1140])
    rng = random.Random(11)
    for i in range(0, len(s), 97):
        s[i] = rng.choice([ch for ch in "ACGT" if ch != s[i]])
    del s[500]
    contigs, reads, place, _ = pool
    contigs = contigs[:2] + [long_contig]
    reads = reads[:20] + ["".join(s)] + reads[20:40] + [long_contig[1000:1100]]
    place = place[:20].tolist() + [2] + place[20:40].tolist() + [2]
    dev = check(engine, contigs, reads, place, READ_LENGTH, what="single")
    last = engine.last_consensus()
    assert last["single_reads"] == 1 and last["batch_reads"] == 41
    assert dev["aln"][20, 0] > 10000 and dev["counts"][1000:, :4].sum() >= 1099 + 100 - 13
    assert last["ops"] == int(dev["counts"].sum()) + dev["n_other"]


def test_the_strip_boundary_routes_alike_in_both_callers(engine):
    """1,024 bases are the batch kernel's 16 strips, 1,025 one more: ovl_consensus and ovl_local_align_batch, which
    share one routing rule, send the first read to the batch kernel and the second down the single-pair path."""
    from ovlgraph.reads import read_genome_from_fasta
    contig = read_genome_from_fasta()[3300:4400]
    reads = []
    for lo, n in ((30, 1024), (60, 1025)):
        s = list(contig[lo:lo + n + 1])
        for i in range(50, n, 101):
            s[i] = "A" if s[i] != "A" else "C"
        del s[700]
        reads.append("".join(s))
    assert [len(r) for r in reads] == [1024, 1025]
    dev = check(engine, [contig], reads, [0, 0], READ_LENGTH, what="boundary")
    last = engine.last_consensus()
    assert last["batch_reads"] == 1 and last["single_reads"] == 1
    assert dev["aln"][:, 0].min() > 9000
    score = engine.local_align_batch(reads, contig, None, *SCORINGS[0])[0]
    last = engine.last_local_batch()
    assert last["batched"] == 1 and last["single"] == 1
    assert score.tolist() == dev["aln"][:, 0].tolist()


def test_polish_contigs_on_the_device_returns_the_true_sequences(engine):
    from ovlgraph import consensus as cs
    _, truth, contigs, reads = planted()
    polished, pile = cs.polish_contigs(contigs, reads, 40, rounds=2, engine=engine, device=True)
    assert polished == truth and pile.rounds == 2 and pile.n_changed == 0
    assert engine.last_consensus()["batch_reads"] == len(reads)
    host, _ = cs.polish_contigs(contigs, reads, 40, rounds=2, device=False)
    assert host == polished


def test_timing_and_argument_errors(engine):
    from ovlgraph._lib import OvlError
    _, truth, contigs, reads = planted()
    place = [0] * len(reads)
    engine.set_timing(True)
    try:
        engine.consensus(reads, contigs, place, 40)
        t, last = engine.last_timing(), engine.last_consensus()
    finally:
        engine.set_timing(False)
    assert 0 < last["align_ms"] and 0 < last["pileup_ms"] and 0 < last["vote_ms"]
    assert abs(t["kernel_ms"] - (last["align_ms"] + last["pileup_ms"] + last["vote_ms"])) < 1e-6
    assert t["kernel_ms"] <= t["call_ms"]
    for kw, code in ((dict(min_depth=0), -1), (dict(read_length=-1), -1), (dict(match=1 << 22), -4)):
        args = dict(read_length=40, match=10, min_depth=3)
        args.update(kw)
        with pytest.raises(OvlError) as e:
            engine.consensus(["ACGT" * 8], ["ACGT" * 8], [0], args["read_length"], args["match"], -1, -1,
                             args["min_depth"])
        assert e.value.code == code, kw
    with pytest.raises(OvlError) as e:
        engine.consensus(["ACGT"], ["ACGT"], [1], 4)
    assert e.value.code == -7
    res = engine.consensus(["ACGT"], [], [-1], 4)
    assert res["called"].shape == (0,) and res["aln"].tolist() == [[0, 0, 0]]
    res = engine.consensus([], ["ACGT"], [], 4)
    assert res["called"].tobytes() == b"ACGT" and res["n_changed"] == 0
