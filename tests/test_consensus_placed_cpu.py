"""Placed consensus without a GPU: ovl_consensus_placed_host against the rule as literal loops (pileup_placed_loop) on
every case of tests/consensus_placed_cases.py, element for element; at full slack against ovl_consensus_host; rounds
against single rounds; read order; every argument check of the ABI (its code, and nothing written); the stand-alone
sanitizer program; and the pipeline on PhiX reads scored by the oracle, polished at the layout's own placement."""
import os
import subprocess

import numpy as np
import pytest

from consensus_placed_cases import (BY_NAME, CASES, KEYS, RawCall, assert_same, bad_calls, full_slack, loop_args,
                                    native_args, permuted, want)
from conftest import PKG
from ovlgraph import _lib
from ovlgraph.consensus import pileup_placed, pileup_placed_loop
from ovlgraph.engine import consensus_host, consensus_placed_host

IDS = [c.name for c in CASES]


def host(case, **over):
    a, kw = native_args(case, **over)
    return consensus_placed_host(*a, **kw)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_form_equals_the_loop_form(case):
    assert_same(host(case), want(case), case.name)


def test_the_cases_reach_what_they_are_named_for():
    w = {c.name: want(c) for c in CASES}
    # every window that should exist does, every one that should not casts no vote
    assert (w["clip_start"]["aln"][:, 0] > 0).sum() >= 4 and (w["clip_end"]["aln"][:, 0] > 0).sum() >= 4
    assert w["no_window"]["aln"][:6].tolist() == [[0, 0, 0]] * 6 and w["no_window"]["aln"][6, 0] == 120
    # gaps of up to slack bases are walked through (gap and ins votes); a gap of slack + 1 leaves the band
    for s in (1, 4, 5, 8, 9, 15):
        counts = w[f"slack_{s}"]["counts"]
        assert counts[:, 4].sum() >= 1 + s and counts[:, 5].sum() >= 1, s
    assert w["slack_0"]["counts"][:, 4:].sum() == 0
    for s in (4, 8):
        # reads 4 and 6 lack s contig bases and are walked across the gap; reads 8 and 10 lack s + 1, which only a
        # slack of s + 1 lets them cross
        c = BY_NAME[f"slack_{s}"]
        a, kw = loop_args(c, slack=s + 1)
        wider, aln = pileup_placed_loop(*a, **kw)["aln"], w[c.name]["aln"]
        for r in (4, 6):
            assert aln[r, 2] - aln[r, 1] >= 30 + s and aln[r, 0] == wider[r, 0], (s, r)
        for r in (8, 10):
            assert aln[r, 0] < wider[r, 0] and wider[r, 2] - wider[r, 1] >= 30 + s, (s, r)
    # a positive indel walks out of the band and stops there
    assert w["scoring_positive_indel"]["counts"][:, 4:].sum() > 0
    assert w["scoring_never_taken"]["counts"][:, 4:].sum() == 0
    assert w["other_bytes"]["n_other"] >= 3
    assert w["weights"]["counts"].sum() > 0 and w["pile_200"]["counts"][:, :4].max() == 200
    assert w["pile_200"]["n_changed"] > 0
    assert w["vote_edge"]["aln"][:, 0].tolist() == [50, 0]
    a, kw = loop_args(BY_NAME["vote_edge"], min_vote_score=49)
    assert pileup_placed_loop(*a, **kw)["aln"][:, 0].tolist() == [50, 49]
    assert [(w[f"rounds_{r}"]["rounds"], w[f"rounds_{r}"]["total_changed"], w[f"rounds_{r}"]["n_changed"])
            for r in (1, 2, 3, 5)] == [(1, 1, 1), (2, 2, 1), (3, 2, 0), (3, 2, 0)]
    assert w["contigs_edge"]["aln"][:, 0].tolist()[:3] == [0, 10, 10]


@pytest.mark.parametrize("case", [c for c in CASES if c.full], ids=[c.name for c in CASES if c.full])
def test_full_slack_equals_ovl_consensus(case):
    got = host(case, slack=full_slack(case), weights=None, rounds=1, min_vote_score=1)
    ref = consensus_host(case.reads, case.contigs, case.contig, 0, *case.scoring, case.min_depth)
    for k in ("counts", "called", "n_changed", "n_other", "aln"):
        assert np.array_equal(got[k], ref[k]), k


@pytest.mark.parametrize("name", ["rounds_5", "len_100", "slack_8", "pile_200"])
def test_rounds_equal_single_rounds(name):
    case = BY_NAME[name]
    for R in (1, 2, 3):
        got = host(case, rounds=R)
        contigs, step, done = list(case.contigs), None, 0
        for _ in range(R):
            a, kw = native_args(case, rounds=1)
            step = consensus_placed_host(a[0], contigs, a[2], a[3], **kw)
            done += 1
            text = step["called"].tobytes().decode("latin-1")
            cut = np.concatenate(([0], np.cumsum([len(c) for c in contigs])))
            contigs = [text[cut[k]:cut[k + 1]] for k in range(len(contigs))]
            if step["n_changed"] == 0:
                break
        for k in ("counts", "called", "n_changed", "n_other", "aln"):
            assert np.array_equal(got[k], step[k]), (R, k)
        assert got["rounds"] == done
        assert got["total_changed"] == sum(x != y for x, y in zip("".join(contigs), "".join(case.contigs)))


@pytest.mark.parametrize("name", ["len_mixed", "weights", "contigs_edge", "rounds_3", "slack_5"])
def test_result_does_not_depend_on_read_order(name):
    case = BY_NAME[name]
    mixed, order = permuted(case)
    got, ref = host(mixed), host(case)
    for k in KEYS:
        if k != "aln":
            assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["aln"], ref["aln"][order])


def test_outputs_may_be_null_and_weights_default_to_one():
    case = BY_NAME["count_65"]
    L = _lib.load()
    raw = RawCall(case)
    assert L.ovl_consensus_placed_host(*raw.args(counts=None, aln=None, weight=None)) == 0
    ref = host(case)
    assert np.array_equal(raw.called, ref["called"]) and raw.i64[0].value == ref["n_changed"]
    assert raw.done.value == 1 and (raw.counts == 77).all() and (raw.aln == 77).all()
    ones = host(case, weights=[1] * len(case.reads))
    assert_same(ones, ref, "weights of one")


def test_every_argument_check_returns_its_code_and_writes_nothing():
    case = BY_NAME["count_1"]
    L = _lib.load()
    calls = bad_calls(case)
    assert len(calls) >= 26
    for name, over, code in calls:
        raw = RawCall(case)
        assert L.ovl_consensus_placed_host(*raw.args(**over)) == code, name
        assert raw.untouched(), name
        assert _lib.last_error(None), name
    # the host form takes any slack
    raw = RawCall(case)
    assert L.ovl_consensus_placed_host(*raw.args(slack=2 ** 31 - 1)) == 0 and not raw.untouched()


def test_python_surface():
    import ovlgraph
    assert {"ovl_consensus_placed", "ovl_consensus_placed_host", "ovl_last_consensus_placed",
            "ovl_last_consensus_placed_timing"} <= set(_lib.SIGNATURES)
    assert "pileup_placed" in ovlgraph.__all__ and ovlgraph.pileup_placed is pileup_placed
    case = BY_NAME["contigs_edge"]
    pile = pileup_placed(case.contigs, case.reads, case.contig, case.offset, case.slack, min_depth=case.min_depth,
                         device=False)
    ref = want(case)
    assert [len(c) for c in pile.counts] == [len(c) for c in case.contigs]
    assert "".join(pile.called) == ref["called"].tobytes().decode() and pile.rounds == 1
    assert pile.place.tolist() == case.contig and pile.offset.tolist() == case.offset
    assert pile.total_changed == ref["total_changed"] and pile.n_other == ref["n_other"]
    # slack beyond the device form's goes to the host form whatever is visible
    wide = pileup_placed(case.contigs, case.reads, case.contig, case.offset, 16, min_depth=case.min_depth)
    a, kw = native_args(case, slack=16)
    assert "".join(wide.called) == consensus_placed_host(*a, **kw)["called"].tobytes().decode()


def test_host_check_program_under_sanitizers():
    """The host form as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (no Python)."""
    out = subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc"), "consensus-placed-host-check"],
                         capture_output=True, text=True)
    assert out.returncode == 0 and "consensus_placed_host_check: ok" in out.stdout, out.stdout + out.stderr


# ----------------------------------------------------------------------------- the pipeline on PhiX


def mismatches_against(genome: str, contig: str) -> int:
    """Ungapped mismatches of the contig against the genome where an exact 30-base anchor of it places it."""
    for a in range(0, len(contig) - 30, 30):
        at = genome.find(contig[a:a + 30])
        if at >= 0:
            shift = at - a  # contig base i lies on genome base i + shift
            lo, hi = max(0, -shift), min(len(contig), len(genome) - shift)
            return sum(contig[i] != genome[i + shift] for i in range(lo, hi))
    raise AssertionError("no exact 30-base anchor")


@pytest.fixture(scope="module")
def phix(oracle_mod):
    """test_layout_cpu.py's workload: PhiX, N = 2,000 reads of 100 bases with 1 % errors (seed 0), k = 12 seed
    candidates, scored by the oracle (once: the second run takes the first's scores)."""
    from ovlgraph.layout import assemble_contigs_best_successor
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads
    genome = read_genome_from_fasta()
    reads = simulate_reads(genome, 100, 2000, 0.01, seed=0)
    memo = {}

    def scorer(distinct, a, b):
        key = (len(distinct), len(a))
        if key not in memo:
            memo[key] = oracle_mod.batch_dp(distinct, a, b)
        return memo[key]

    plain_out, out, stages = {}, {}, {}
    plain = assemble_contigs_best_successor(reads, k=12, seeds="any", scorer=scorer, layout_out=plain_out)
    polished = assemble_contigs_best_successor(reads, k=12, seeds="any", scorer=scorer, layout_out=out, timing=stages,
                                               polish=1)
    return genome, reads, plain, plain_out, polished, out, stages


def test_phix_polish_takes_the_spanning_contig_to_the_genome(phix):
    genome, reads, plain, plain_out, polished, out, stages = phix
    assert [len(c) for c in polished] == [len(c) for c in plain]
    k = max(range(len(plain)), key=lambda i: len(plain[i]))
    assert len(plain[k]) >= 0.9 * len(genome)
    before, after = mismatches_against(genome, plain[k]), mismatches_against(genome, polished[k])
    print(f"longest contig, {len(plain[k])} bases: {before} -> {after} mismatches against the genome")
    assert (before, after) == (62, 0)
    pile = out["pileup"]
    assert pile.rounds == 1 and pile.total_changed == sum(a != b for a, b in zip("".join(plain), "".join(polished)))
    assert sum(out["copies"]) == len(reads) and len(out["copies"]) == len(out["reads"])
    assert out["polished"] == polished and out["contigs"] == plain and "polish" in stages


def test_phix_polish_0_changes_nothing(phix):
    genome, reads, plain, plain_out, polished, out, stages = phix
    assert set(plain_out) == {"succ", "link", "contig", "offset", "on_path", "links", "cycles", "levels",
                              "on_path_reads", "contigs", "reads"}
    assert set(out) == set(plain_out) | {"copies", "polished", "pileup"}
    assert plain == plain_out["contigs"] == out["contigs"]
    for key in ("succ", "link", "contig", "offset", "on_path"):
        assert np.array_equal(plain_out[key], out[key]), key
    with pytest.raises(ValueError):
        from ovlgraph.layout import assemble_contigs_best_successor
        assemble_contigs_best_successor(reads[:10], polish=-1)
