"""The evaluation stage's host arithmetic (ovlgraph/performanceMeasures.py) against the reference's recorded
outputs (tests/golden/measures.json, tools/gen_golden_measures.py), bit-exact, without a GPU: the golden
alignment details go in, the reference's coverage, mismatch rates, N50 and plot-hook firing must come out."""
import pytest

from conftest import load_golden


class RecordingPlots:
    def __init__(self):
        self.fired = []

    def plot_genome_coverage(self, coverage, genome_length, experiment_name, num_iteration, path):
        assert len(coverage) == genome_length
        self.fired.append("plot_genome_coverage")

    def plot_genome_depth(self, coverage, expected_coverage, genome_length, experiment_name, num_iteration, path):
        assert len(coverage) == genome_length
        self.fired.append("plot_genome_depth")


@pytest.fixture(scope="module")
def cases():
    return load_golden("measures.json")["cases"]


def details_of(case):
    return {c: {"Print": tp, "Alignment_reference": a_r, "Alignment_query": a_q, "Alignment Score": sc,
                "Start Position": st, "End Position": en}
            for c, tp, a_r, a_q, sc, st, en in case["details"]}


def test_fixture_covers_the_cases(cases):
    assert len(cases) >= 4
    by_name = {c["name"]: c for c in cases}
    assert by_name["full_coverage_exact"]["measures"]["Genome Coverage"] == 1.0
    assert by_name["full_coverage_exact"]["measures"]["Mismatch Rate Genome Level"] == 0.0
    assert any("-" in d[2] or "-" in d[3] for d in by_name["errors_with_indels"]["details"])
    short = by_name["short_and_repeated"]
    assert any(0 < len(c) < short["args"]["reads_length"] for c in short["args"]["contigs"])
    assert len(short["details"]) < len(short["args"]["contigs"])
    assert by_name["uncovered_bases"]["measures"]["Genome Coverage"] < 1.0
    uni = by_name["uniform_second_iteration"]
    assert uni["args"]["num_iteration"] == 2 and uni["plots_fired"] == []


def test_coverage_and_mismatch_rates(cases):
    from ovlgraph import performanceMeasures as pm
    for case in cases:
        a = case["args"]
        plots = RecordingPlots()
        expected_coverage = a["num_reads"] * a["reads_length"] / len(a["ref_genome"])
        got = pm.calculate_genome_coverage_and_mismatch_rate(details_of(case), a["ref_genome"], expected_coverage,
                                                             a["experiment_name"], a["num_iteration"], plots=plots)
        m = case["measures"]
        assert got == (m["Genome Coverage"], m["Mismatch Rate Aligned Regions"], m["Mismatch Rate Genome Level"]), \
            case["name"]
        assert all(type(x) is float for x in got)
        assert plots.fired == case["plots_fired"], case["name"]
        # without a plots object nothing is called and the numbers are the same
        assert pm.calculate_genome_coverage_and_mismatch_rate(details_of(case), a["ref_genome"], expected_coverage,
                                                              a["experiment_name"], a["num_iteration"]) == got


def test_n50(cases):
    from ovlgraph import performanceMeasures as pm
    for case in cases:
        got = pm.calculate_n50(case["args"]["contigs"])
        assert got == case["measures"]["N50"] and type(got) is int, case["name"]
    assert pm.calculate_n50([]) == 0
    assert pm.calculate_n50(["AAAA", "CC", "G"]) == 4
    assert pm.calculate_n50(["AA", "CC", "GG", "TT"]) == 2


def test_signatures_list_the_batch_calls():
    from ovlgraph import _lib
    assert "ovl_local_align_batch" in _lib.SIGNATURES
    assert "ovl_last_local_batch" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ovl_local_align_batch"][1]) == 19
    assert _lib.ABI_VERSION == 4
