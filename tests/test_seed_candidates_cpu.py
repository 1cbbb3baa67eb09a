"""Seed candidates on the host (no GPU): the vectorised host form against the rule's literal loops, the reference's
rule as a subset, the ``seeds=`` keyword of the graph builders, and what the rule buys an assembly."""
import numpy as np
import pytest

from conftest import assert_graph_matches_record
from seed_inputs import input_sets, phix_reads

from ovlgraph import overlapGraphs as og
from ovlgraph.candidates import (dedup_reads, enumerate_candidates, enumerate_seed_candidates,
                                 enumerate_seed_candidates_loop)

SETS = input_sets()


def _oracle_scorer(oracle_mod):
    return lambda reads, a, b: oracle_mod.batch_dp(reads, a, b)


@pytest.mark.parametrize("name", sorted(SETS))
def test_host_form_equals_loop(name):
    distinct, k = SETS[name]
    got = enumerate_seed_candidates(distinct, k)
    want = enumerate_seed_candidates_loop(distinct, k)
    for g, w in zip(got, want):
        assert g.dtype == np.int32
        np.testing.assert_array_equal(g, w)
    if name in ("empty", "single"):
        assert got[0].shape[0] == 0
    elif name != "forty_bytes":  # (40 symbols at k = 5: a chance hit is one in 40^5)
        assert got[0].shape[0] > 0


def test_rule_by_hand():
    # a = 0: "ACGTAC" has k-mers CG, GT, TA, AC at offsets 1..4; its own prefix AC recurs at offset 4, where read 0
    # itself is dropped and read 3 ("ACT") is not.  Read 4 is shorter than k.
    distinct = ["ACGTAC", "GTT", "CGA", "ACT", "G", "TAC"]
    a, b, o = enumerate_seed_candidates(distinct, 2)
    rows = list(zip(a.tolist(), b.tolist(), o.tolist()))
    assert [r for r in rows if r[0] == 0] == [(0, 2, 1), (0, 1, 2), (0, 5, 3), (0, 3, 4)]
    assert 4 not in a.tolist() and 4 not in b.tolist()
    # a repeated k-mer emits at its first offset only: "ACACAC" meets AC at offsets 2 and 4
    a, b, o = enumerate_seed_candidates(["GACACAC", "ACT"], 2)
    assert list(zip(a.tolist(), b.tolist(), o.tolist())) == [(0, 1, 1)]


def test_short_reads_take_no_part():
    distinct, k = SETS["acgt"]
    short = {i for i, r in enumerate(distinct) if len(r) < k}
    assert short, "the set must hold reads shorter than k"
    a, b, _ = enumerate_seed_candidates(distinct, k)
    assert not short & set(a.tolist()) and not short & set(b.tolist())
    no_probe = {i for i, r in enumerate(distinct) if len(r) == k}  # a key, but no offset >= 1
    assert not no_probe & set(a.tolist())


def test_own_prefix_inside_the_read():
    distinct, k = SETS["own_prefix"]
    a, b, o = enumerate_seed_candidates(distinct, k)
    assert distinct[0][:k] in distinct[0][1:]
    sharing = [i for i, r in enumerate(distinct) if i != 0 and r[:k] == distinct[0][:k]]
    first = distinct[0].index(distinct[0][:k], 1)
    got = [(y, z) for x, y, z in zip(a.tolist(), b.tolist(), o.tolist()) if x == 0 and z == first]
    assert len(sharing) >= 3 and got == [(i, first) for i in sharing]  # read order kept around the dropped a


@pytest.mark.parametrize("name,k", [("phix200", 12), ("phix200", 5), ("repeats", 4)])
def test_reference_rule_is_a_subset(name, k):
    distinct = [r for r in SETS[name][0] if len(r) > k]
    ra, rb = enumerate_candidates(distinct, k)
    sa, sb, _ = enumerate_seed_candidates(distinct, k)
    ref = set(zip(ra.tolist(), rb.tolist()))
    assert ref and ref <= set(zip(sa.tolist(), sb.tolist()))


def test_k_below_one_is_an_error():
    for fn in (enumerate_seed_candidates, enumerate_seed_candidates_loop):
        with pytest.raises(ValueError):
            fn(["ACGT"], 0)


def test_keyword_suffix_gives_the_golden_graphs(golden_graphs, oracle_mod):
    n = 0
    for rec in golden_graphs["graphs"]:
        if rec["fn"] != "construct_overlap_graph_nx_k":
            continue
        G, copies = og.construct_overlap_graph_nx_k(rec["reads"], scorer=_oracle_scorer(oracle_mod), seeds="suffix",
                                                    **rec["kwargs"])
        assert_graph_matches_record(G, rec, copies)
        n += 1
    assert n > 0


def test_keyword_errors():
    reads = ["ACGTACGT", "GTACGTAA"]
    for fn in (og.construct_overlap_graph_nx_k, og.build_overlap_graph, og.overlap_edges_k,
               og.assemble_contigs_using_overlap_graphs):
        with pytest.raises(ValueError):
            fn(reads, k=3, seeds="bogus", candidates="host")
        with pytest.raises(ValueError):
            fn(reads, k=0, seeds="any", candidates="host")
    with pytest.raises(ValueError):
        og.candidates_and_scores(reads, 3, seeds="bogus")
    with pytest.raises(ValueError):
        og.candidates_and_scores(reads, 0, seeds="any")


def test_keyword_any_scores_the_seed_pairs(oracle_mod):
    reads = phix_reads(200) + phix_reads(200)[:20]  # with copies
    distinct, counts = dedup_reads(reads)
    E = og.overlap_edges_k(reads, k=12, scorer=_oracle_scorer(oracle_mod), seeds="any")
    a, b, _ = enumerate_seed_candidates(distinct, 12)
    sc, en = oracle_mod.batch_dp(distinct, a, b)
    assert E.reads == distinct and E.counts == counts
    for got, want in ((E.a, a), (E.b, b), (E.score, sc), (E.end, en)):
        np.testing.assert_array_equal(got, want)
    G, copies = og.construct_overlap_graph_nx_k(reads, k=12, scorer=_oracle_scorer(oracle_mod), seeds="any")
    assert G.number_of_edges() == E.n_edges() and copies == dict(zip(distinct, counts))


def test_assembly_quality(oracle_mod):
    """1,000 PhiX reads of 100 bases at p = 0.01, the oracle's scores: the longest contig under the seed rule at
    k = 12 is at least 5x the longest under the reference's rule at k = 5 (measured: 2,590 against 225)."""
    reads = phix_reads(1000)
    scorer = _oracle_scorer(oracle_mod)
    before = og.assemble_contigs_using_overlap_graphs(reads, k=5, scorer=scorer, seeds="suffix")
    after = og.assemble_contigs_using_overlap_graphs(reads, k=12, scorer=scorer, seeds="any")
    longest = max(map(len, before)), max(map(len, after))
    print(f"contigs {len(before)} -> {len(after)}, longest {longest[0]} -> {longest[1]}")
    assert longest[1] >= 5 * longest[0]
