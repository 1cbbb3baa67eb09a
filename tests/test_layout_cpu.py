"""The best-successor layout without a GPU: ovl_layout_host against the rule as literal loops (layout_loop) on every
case of tests/layout_cases.py, array for array and contig for contig; the spelled bases against a spelling from succ and
link alone; every argument check of the ABI (its code, and nothing written); and the pipeline on PhiX reads scored by
the oracle."""
import numpy as np
import pytest

from layout_cases import (BY_NAME, CASES, RawCall, assert_expect, assert_same, bad_calls, case_args, spell,
                          with_contigs)
from ovlgraph import _lib
from ovlgraph.engine import last_layout_host, layout_host
from ovlgraph.layout import assemble_contigs_best_successor, layout, layout_loop


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_form_equals_the_loop_form(case):
    args = case_args(case)
    want = layout_loop(*args)
    got = with_contigs(layout_host(*args))
    assert_same(got, want, case.name)
    assert_expect(case, want)
    assert_expect(case, got)
    assert got["contigs"] == spell(case.reads, got, case.end)
    assert got["c_off"].tolist() == np.concatenate(([0], np.cumsum([len(c) for c in want["contigs"]]))).tolist()
    assert {k: got[k] for k in ("links", "cycles", "on_path_reads")} == \
        {k: last_layout_host()[k] for k in ("links", "cycles", "on_path_reads")}


def test_the_cases_reach_what_they_are_named_for():
    loops = {c.name: layout_loop(*case_args(c)) for c in CASES}
    assert [loops[f"cycle_{n}"]["cycles"] for n in (2, 3, 5, 100)] == [1, 1, 1, 1]
    assert loops["two_cycles"]["cycles"] == 2 and loops["cycle_with_70_tail"]["cycles"] == 1
    # the tail's 70 reads and the nine of the ring from where it enters to the cut; read 4 hangs off the path
    assert loops["cycle_with_70_tail"]["on_path_reads"] == 79 and loops["cycle_with_70_tail"]["on_path"][4] == 0
    assert loops["chain_130"]["n_contigs"] == 1 and loops["chain_130"]["on_path_reads"] == 130
    assert loops["star_200"]["n_contigs"] == 1 and loops["star_200"]["on_path_reads"] == 2
    assert loops["no_pairs"]["n_contigs"] == 4 and loops["no_reads"]["n_contigs"] == 0
    assert all(loops[f"random_{s}"]["cycles"] >= 1 for s in (1, 2, 3))
    # the shuffled list holds the same pairs under other numbers: read 0's two best pairs tie, and whichever of them
    # has the smaller p in each list wins there
    plain, mixed = loops["one_read_300_pairs"], loops["one_read_300_pairs_shuffled"]
    assert plain["succ"][0] == 202 and mixed["succ"][0] in (202, 207)
    want = BY_NAME["one_read_300_pairs_shuffled"].expect
    assert mixed["link"][0] == want["link"][0] != plain["link"][0] and mixed["succ"][0] == want["succ"][0]
    assert BY_NAME["one_read_300_pairs_shuffled"].a[:4] != BY_NAME["one_read_300_pairs"].a[:4]


def test_outputs_may_be_null():
    import ctypes
    c = BY_NAME["cycle_with_70_tail"]
    call = RawCall(c.reads, c.a, c.b, c.score, c.end)
    L = _lib.load()
    p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    rc = L.ovl_layout_host(p(call.buf), p(call.offs), call.n, *[p(x) for x in call.cols], len(c.a), 1, 1, None, None,
                           None, None, None, None, None, ctypes.byref(call.nc))
    assert rc == 0 and call.nc.value == 1
    # and without the bytes no seqs are needed
    rc = L.ovl_layout_host(None, p(call.offs), call.n, *[p(x) for x in call.cols], len(c.a), 1, 1, p(call.i32[0]),
                           None, None, None, None, None, None, ctypes.byref(call.nc))
    assert rc == 0 and call.i32[0][3] == -1


def test_argument_checks_return_their_code_and_write_nothing():
    c = BY_NAME["two_cycles"]
    reads = c.reads[:3]
    cols = ([0, 1, 2], [1, 2, 0], [30, 20, 10], [2, 2, 2])
    for what, kw, code in bad_calls():
        call = RawCall(reads, *cols)
        assert call(**kw) == code, what
        assert call.untouched(), what
        assert _lib.last_error(), what
    for bad_a, bad_b in (([0, 3, 2], cols[1]), ([0, -1, 2], cols[1]), (cols[0], [1, 2, 3]), (cols[0], [-5, 2, 0])):
        call = RawCall(reads, bad_a, bad_b, cols[2], cols[3])
        assert call() == -7 and call.untouched()
    ok = RawCall(reads, *cols)
    assert ok() == 0 and not ok.untouched() and ok.nc.value == 1
    assert _lib.load().ovl_last_layout_timing(None, None, None, None, None) == -1
    assert _lib.load().ovl_layout(None, *([None] * 2), 0, *([None] * 4), 0, 1, 1, *([None] * 8)) == -1
    assert _lib.load().ovl_layout_candidates(None, 10, -1, -1, -1, 1, 1, *([None] * 8)) == -1


def test_layout_takes_the_host_form_without_a_gpu_and_checks_its_text():
    c = BY_NAME["variable_lengths"]
    args = case_args(c)
    assert_same(layout(*args, device=False), layout_loop(*args))
    from ovlgraph.engine import device_count
    if device_count() == 0:
        assert_same(layout(*args), layout_loop(*args))
    with pytest.raises(_lib.OvlError):
        layout(["ACΔT", "ACGT"], [], [], [], [])
    with pytest.raises(_lib.OvlError):
        layout(c.reads, [0, 1], [1], [5, 5], [2, 2], device=False)


def test_package_level_names_are_stable_in_either_import_order():
    """The three lazy names of the package, taken twice, before and after the submodule is imported, in a fresh
    interpreter per order: each is the same function every time, and ovlgraph.layout is the module."""
    import os
    import subprocess
    import sys
    script = """
import sys, types
first = sys.argv[1]
if first == "submodule":
    import ovlgraph.layout
import ovlgraph
names = ("best_successor_layout", "layout_loop", "assemble_contigs_best_successor")
took = [[getattr(ovlgraph, n) for n in names] for _ in range(2)]
from ovlgraph import best_successor_layout, layout_loop, assemble_contigs_best_successor
took.append([best_successor_layout, layout_loop, assemble_contigs_best_successor])
import ovlgraph.layout
from ovlgraph.layout import layout
took.append([getattr(ovlgraph, n) for n in names])
from ovlgraph import best_successor_layout as again
assert all(t == took[0] for t in took) and all(isinstance(f, types.FunctionType) for f in took[0])
assert again is layout is took[0][0] and took[0][1] is ovlgraph.layout.layout_loop
assert isinstance(ovlgraph.layout, types.ModuleType) and ovlgraph.layout is sys.modules["ovlgraph.layout"]
assert set(names) <= set(ovlgraph.__all__) and "layout" not in ovlgraph.__all__
r = ovlgraph.best_successor_layout(["ACGTAC", "TACGGG"], [0], [1], [30], [3], device=False)
assert ovlgraph.best_successor_layout(["ACGTAC", "TACGGG"], [0], [1], [30], [3], device=False)["contigs"] == \
    r["contigs"] == ["ACGTACGGG"]
print("ok", first)
"""
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__)))
    env = dict(os.environ, PYTHONPATH=pkg)
    for first in ("package", "submodule"):
        out = subprocess.run([sys.executable, "-c", script, first], env=env, capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.strip() == f"ok {first}", out.stderr


@pytest.fixture(scope="module")
def phix(oracle_mod):
    """PhiX, N = 2,000 reads of 100 bases with 1 % errors (seed 0), k = 12 seed candidates, scored by the oracle."""
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads
    genome = read_genome_from_fasta()
    reads = simulate_reads(genome, 100, 2000, 0.01, seed=0)
    seen = {}

    def scorer(distinct, a, b):
        seen["pairs"] = len(a)
        return oracle_mod.batch_dp(distinct, a, b)

    out, stages = {}, {}
    contigs = assemble_contigs_best_successor(reads, k=12, seeds="any", scorer=scorer, layout_out=out, timing=stages)
    return genome, reads, scorer, contigs, out, stages, seen


def test_phix_pipeline_equals_the_loop_form(phix, oracle_mod):
    from ovlgraph.candidates import dedup_reads, enumerate_seed_candidates
    genome, reads, scorer, contigs, out, stages, seen = phix
    distinct, _ = dedup_reads(reads)
    assert out["reads"] == distinct
    a, b, _o = enumerate_seed_candidates(distinct, 12)
    assert seen["pairs"] == len(a) > 10000
    sc, en = oracle_mod.batch_dp(distinct, a, b)
    want = layout_loop(distinct, a, b, sc, en)
    assert contigs == want["contigs"] == out["contigs"]
    for k in ("succ", "link", "contig", "offset", "on_path"):
        assert np.array_equal(out[k], want[k]), k
    for k in ("links", "cycles", "on_path_reads"):
        assert out[k] == want[k], k
    assert {"dedup", "candidates_and_scores", "layout"} <= set(stages)


def test_phix_layout_has_no_cycle_and_spans_the_genome(phix):
    genome, reads, scorer, contigs, out, stages, seen = phix
    assert out["cycles"] == 0
    assert max(len(c) for c in contigs) >= 0.9 * len(genome)
    # min_contig_length drops the short contigs in Python and nothing else
    long_only = assemble_contigs_best_successor(reads, k=12, seeds="any", scorer=scorer, min_contig_length=200)
    assert last_layout_host()["cycles"] == 0 and last_layout_host()["links"] == out["links"]
    assert long_only == [c for c in contigs if len(c) >= 200] and 1 <= len(long_only) < len(contigs)
