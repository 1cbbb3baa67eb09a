"""Batched local alignment (ovl_local_align_batch, ovl_local_batch.hip) and the evaluation stage on top of it,
bit-exact against the oracle, the single-pair path and the reference's recorded outputs.

The batch kernel gives one wavefront one query: the shapes here cross every strip (64 rows) and chunk (64 steps)
boundary, make a wavefront reuse its traceback slab for a shorter query after a longer one, and send a query that
is too long for one wavefront through the single-pair path inside the same call.
"""
import ctypes
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCORINGS = ((10, -1, -1), (2, -3, -5), (1, -1, -1))


@pytest.fixture(scope="module")
def engine():
    from ovlgraph import OverlapEngine
    eng = OverlapEngine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def genome():
    from ovlgraph.reads import read_genome_from_fasta
    return read_genome_from_fasta()


def _mutated(rng, src, n, p_sub=0.02, p_indel=0.01):
    """`src` with substitutions and indels (test_gpu_local._genome_pair's rule), cut or padded to n bases."""
    out = []
    for ch in src:
        u = rng.random()
        if u < p_indel / 2:
            continue
        if u < p_indel:
            out.append(rng.choice("ACGT"))
        out.append(rng.choice("ACGT") if rng.random() < p_sub else ch)
    while len(out) < n:
        out.append(rng.choice("ACGT"))
    return "".join(out[:n])


def _boundary_batch(genome):
    rng = random.Random(64)
    st = rng.randint(0, len(genome) - 1000)
    ref = genome[st:st + 1000]
    queries, windows = [], []
    for n in (0, 1, 63, 64, 65, 128, 129, 200):
        for m in (0, 1, 63, 64, 65, 127, 129, 300, 700):
            lo = rng.randint(0, len(ref) - m)
            o = rng.randint(0, max(0, m - n))
            queries.append(_mutated(rng, ref[lo + o:lo + o + n], n))
            windows.append((lo, m))
    for n, m in ((70, 300), (200, 129), (33, 700), (129, 64)):  # unrelated
        queries.append("".join(rng.choice("ACGT") for _ in range(n)))
        windows.append((rng.randint(0, len(ref) - m), m))
    return queries, ref, windows


def _assert_batch_matches(engine, oracle_mod, queries, ref, windows, params, got, singles=True):
    from ovlgraph import aligners
    sc, ei, ej, si, sj, ops = got
    for arr in (sc, ei, ej, si, sj):
        assert arr.dtype == np.int32 and arr.shape == (len(queries),)
    for k, q in enumerate(queries):
        lo, m = windows[k] if windows is not None else (0, len(ref))
        r = ref[lo:lo + m]
        a_r, a_q = aligners._local_strings(q, r, int(ei[k]), int(ej[k]), ops[k].tolist())
        to_print = f"\nTarget:   {a_r}\n          {'|' * len(a_r)}\nQuery:    {a_q}"
        exp = oracle_mod.local_alignment(q, r, *params)
        assert (to_print, a_r, a_q, int(sc[k]), int(sj[k]), int(ej[k])) == exp, (k, len(q), m, params)
        if singles:
            one = engine.local_align(q, r, *params)
            assert (int(sc[k]), int(ei[k]), int(ej[k]), int(si[k]), int(sj[k])) == one[:5], (k, len(q), m, params)
            assert ops[k].dtype == np.int8 and ops[k].tolist() == one[5].tolist(), (k, len(q), m, params)


@pytest.mark.parametrize("params", SCORINGS)
def test_batch_boundary_shapes(engine, oracle_mod, genome, params):
    queries, ref, windows = _boundary_batch(genome)
    got = engine.local_align_batch(queries, ref, windows, *params)
    _assert_batch_matches(engine, oracle_mod, queries, ref, windows, params, got)
    stats = engine.last_local_batch()
    n_empty = sum(1 for q, (_, m) in zip(queries, windows) if not q or not m)
    assert stats["batched"] == len(queries) - n_empty and stats["single"] == 0 and stats["waves"] >= 1


def test_batch_whole_reference_default(engine, oracle_mod, genome):
    """windows=None: every query against the whole reference (several strips over a 1,000-base row)."""
    rng = random.Random(5)
    ref = genome[2000:3000]
    queries = [_mutated(rng, ref[o:o + n], n) for o, n in ((0, 100), (900, 100), (400, 257), (10, 64), (700, 1))]
    got = engine.local_align_batch(queries, ref)
    _assert_batch_matches(engine, oracle_mod, queries, ref, None, (10, -1, -1), got)


@pytest.mark.parametrize("m", [8129, 8130])
def test_batch_row_in_lds_and_in_global_memory(engine, oracle_mod, genome, m):
    """The row a strip leaves for the next one lives in LDS up to 8,192 int32 (windows up to 8,129 bases: 128 chunks
    of 64 steps) and in a global row of the wavefront's own beyond: the last size of the one, the first of the
    other, with queries of two and three strips."""
    rng = random.Random(m)
    ref = _mutated(rng, genome + genome[:3000], m, 0.1, 0.0)
    queries = [_mutated(rng, ref[8000:8100], 100), _mutated(rng, ref[40:170], 130), _mutated(rng, ref[5000:5065], 65),
               _mutated(rng, ref[3000:3040], 40)]
    windows = [(0, m), (0, m), (0, m), (2900, 300)]
    got = engine.local_align_batch(queries, ref, windows)
    assert engine.last_local_batch()["batched"] == 4
    _assert_batch_matches(engine, oracle_mod, queries, ref, windows, (10, -1, -1), got)


@pytest.mark.parametrize("waves", [2, 3])
def test_batch_slab_reuse(monkeypatch, oracle_mod, genome, waves):
    """Few wavefronts, many queries: each wavefront's slab still holds a long query's codes when a short one
    follows."""
    from ovlgraph import OverlapEngine
    monkeypatch.setenv("OVL_LOCAL_BATCH_WAVES", str(waves))
    rng = random.Random(waves)
    ref = genome[1000:1700]
    queries, windows = [], []
    for k in range(40):
        n, m = ((190, 600), (20, 50), (150, 333), (70, 64))[k % 4] if k % 2 == 0 else \
               ((20, 50), (9, 130), (64, 64), (3, 700))[(k // 2) % 4]
        lo = rng.randint(0, len(ref) - m)
        o = rng.randint(0, max(0, m - n))
        queries.append(_mutated(rng, ref[lo + o:lo + o + n], n, 0.05, 0.05))
        windows.append((lo, m))
    eng = OverlapEngine(0)
    try:
        for params in SCORINGS[:2]:
            got = eng.local_align_batch(queries, ref, windows, *params)
            assert eng.last_local_batch() == {"batched": 40, "single": 0, "waves": waves}
            _assert_batch_matches(eng, oracle_mod, queries, ref, windows, params, got, singles=False)
    finally:
        eng.close()


def test_batch_routing_long_query(engine, oracle_mod, genome):
    """A 1,500-base query (24 strips) among short ones takes the single-pair path inside the same call."""
    rng = random.Random(15)
    ref = genome[300:1800]
    queries = [_mutated(rng, ref[100:160], 60), _mutated(rng, ref, 1500), _mutated(rng, ref[1400:1500], 100), "",
               _mutated(rng, ref[700:830], 130)]
    windows = [(0, 1500), (0, 1500), (1300, 200), (0, 1500), (640, 300)]
    got = engine.local_align_batch(queries, ref, windows)
    _assert_batch_matches(engine, oracle_mod, queries, ref, windows, (10, -1, -1), got)
    stats = engine.last_local_batch()
    assert stats["single"] >= 1 and stats["batched"] + stats["single"] == 4  # the empty query takes neither
    assert got[0][1] > 10000


def test_batch_score_only(engine, genome):
    queries, ref, windows = _boundary_batch(genome)
    full = engine.local_align_batch(queries, ref, windows)
    sc, ei, ej, si, sj, ops = engine.local_align_batch(queries, ref, windows, traceback=False)
    assert ops is None
    assert sc.tolist() == full[0].tolist() and ei.tolist() == full[1].tolist() and ej.tolist() == full[2].tolist()
    assert si.tolist() == ei.tolist() and sj.tolist() == ej.tolist()


def test_align_to_reference_batch_golden(engine):
    """The 20 align_to_reference records.  Each record has a reference and a read length of its own, and
    align_to_reference_batch takes one of each, so it is called per record; the one call over all 20 is made a
    layer below, on the concatenated references with a window per item."""
    from conftest import load_golden
    from ovlgraph import aligners
    recs = load_golden("local_alignment.json")["align_to_reference"]
    assert len(recs) == 20
    want = [(r["to_print"], r["aligned_reference"], r["aligned_query"], r["score"], r["start"], r["end"])
            for r in recs]
    for rec, exp in zip(recs, want):
        got = aligners.align_to_reference_batch([rec["item"], rec["item"]], rec["reference"], rec["read_length"],
                                                engine=engine)
        assert got == [exp, exp]
        assert all(type(x) is int for x in got[0][3:])
    # one call: item k against its own window of all the references laid end to end
    refs = "".join(r["reference"] for r in recs)
    windows, shifts, base = [], [], 0
    for r in recs:
        G, L = len(r["reference"]), len(r["item"])
        tail = 0 < L < r["read_length"]
        windows.append((base + G - L, L) if tail else (base, G))
        shifts.append(G - L if tail else 0)
        base += G
    sc, ei, ej, si, sj, ops = engine.local_align_batch([r["item"] for r in recs], refs, windows)
    for k, (r, exp) in enumerate(zip(recs, want)):
        lo, m = windows[k]
        a_r, a_q = aligners._local_strings(r["item"], refs[lo:lo + m], int(ei[k]), int(ej[k]), ops[k].tolist())
        assert (a_r, a_q, int(sc[k]), shifts[k] + int(sj[k]), shifts[k] + int(ej[k])) == exp[1:]


def test_calculate_measures_end_to_end(engine, capsys):
    from conftest import load_golden
    from ovlgraph import performanceMeasures as pm

    class Plots:
        def __init__(self):
            self.fired = []

        def plot_genome_coverage(self, *a):
            self.fired.append("plot_genome_coverage")

        def plot_genome_depth(self, *a):
            self.fired.append("plot_genome_depth")

    for case in load_golden("measures.json")["cases"]:
        a = case["args"]
        plots = Plots()
        measures, details = pm.calculate_measures(a["contigs"], a["contigs"], a["num_reads"], a["reads_length"],
                                                  a["error_prob"], a["k"], a["ref_genome"], a["experiment_name"],
                                                  a["num_iteration"], engine=engine, plots=plots)
        assert list(measures.items()) == list(case["measures"].items()), case["name"]
        assert [type(v) for v in measures.values()] == [int, float, int, float, float]
        got = [[c, d["Print"], d["Alignment_reference"], d["Alignment_query"], d["Alignment Score"],
                d["Start Position"], d["End Position"]] for c, d in details.items()]
        assert got == case["details"], case["name"]
        assert all(list(d) == ["Print", "Alignment_reference", "Alignment_query", "Alignment Score",
                               "Start Position", "End Position"] for d in details.values())
        assert all(type(d["Alignment Score"]) is int and type(d["Start Position"]) is int
                   and type(d["End Position"]) is int for d in details.values())
        assert plots.fired == case["plots_fired"], case["name"]
    capsys.readouterr()


def _raw_call(engine, queries, ref, windows, match, slot_slack=0):
    """ovl_local_align_batch through ctypes with sentinel-filled outputs -> (rc, error text, outputs)."""
    from ovlgraph import _lib
    from ovlgraph.engine import encode_reads
    buf, offs = encode_reads(queries + [ref])
    nq = len(queries)
    q_off = np.ascontiguousarray(offs[:nq + 1])
    rb = np.ascontiguousarray(buf[int(offs[nq]):])
    lo = np.array([w[0] for w in windows], dtype=np.int32)
    ln = np.array([w[1] for w in windows], dtype=np.int32)
    outs = [np.full(nq, 77, dtype=np.int32) for _ in range(5)]
    n_ops = np.full(nq, 77, dtype=np.int64)
    ops_off = np.zeros(nq + 1, dtype=np.int64)
    np.cumsum(np.diff(q_off) + ln + slot_slack, out=ops_off[1:])
    ops = np.full(max(int(ops_off[-1]), 1), 77, dtype=np.int8)
    P = ctypes.c_void_p
    rc = engine._L.ovl_local_align_batch(engine._ctx, P(buf.ctypes.data), P(q_off.ctypes.data), nq,
                                         P(rb.ctypes.data), len(ref), P(lo.ctypes.data), P(ln.ctypes.data), match,
                                         -1, -1, *[P(o.ctypes.data) for o in outs], P(ops.ctypes.data),
                                         P(ops_off.ctypes.data), P(n_ops.ctypes.data))
    return rc, _lib.last_error(engine._ctx), outs + [n_ops, ops]


def test_batch_errors_write_nothing(engine):
    from ovlgraph import OvlError
    ref = "ACGTTGCAAC" * 5
    queries = ["", "ACGTTGCA", "TTGCAACACG"]
    windows = [(0, 50), (0, 50), (10, 30)]

    def untouched(arrays):
        return all((a == 77).all() for a in arrays)

    rc, msg, arrays = _raw_call(engine, queries, ref, windows, 10)
    assert rc == 0 and not untouched(arrays[:5]) and arrays[0].tolist() == [0, 80, 100]
    rc, msg, arrays = _raw_call(engine, queries, ref, windows, 10, slot_slack=-1)  # every slot one short of n + m
    assert rc == -1 and "ops slot" in msg and untouched(arrays)
    rc, msg, arrays = _raw_call(engine, queries, ref, windows, 2 ** 22)
    assert rc == -4 and "query 1" in msg and untouched(arrays)
    rc, msg, arrays = _raw_call(engine, queries, ref, [(0, 50), (0, 50), (30, 21)], 10)
    assert rc == -1 and "query 2" in msg and untouched(arrays)
    rc, msg, arrays = _raw_call(engine, queries, ref, [(0, 50), (-1, 20), (30, 20)], 10)
    assert rc == -1 and untouched(arrays)
    with pytest.raises(OvlError, match="OVL_E_UNSUPPORTED.*query 1"):
        engine.local_align_batch(queries, ref, windows, 2 ** 22, -1, -1)
    with pytest.raises(OvlError, match="OVL_E_ARG"):
        engine.local_align_batch(queries, ref, [(0, 50), (0, 50), (30, 21)])
    # the context still works
    assert engine.local_align_batch(queries, ref, windows)[0].tolist() == [0, 80, 100]


def test_timing_covers_the_batch_kernel(engine, genome):
    """Four 50-base queries against a 300-base reference: all take the batch kernel."""
    from stage_timing import assert_kernel_inside_call, timed_and_untimed
    rng = random.Random(4)
    ref = genome[1000:1300]
    queries = [_mutated(rng, ref[lo:lo + 50], 50) for lo in (0, 70, 140, 250)]
    got_on, on, got_off, off = timed_and_untimed(engine, lambda: engine.local_align_batch(queries, ref),
                                                 engine.last_local_batch)
    assert on["batched"] == off["batched"] == 4 and on["single"] == 0
    assert_kernel_inside_call(on, off)
    for x, y in zip(got_on[:5], got_off[:5]):
        assert np.array_equal(x, y)
    assert all(np.array_equal(x, y) for x, y in zip(got_on[5], got_off[5])) and len(got_on[5]) == 4
    assert (got_on[0] > 0).all()
