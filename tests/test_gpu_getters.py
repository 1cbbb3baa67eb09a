"""Every getter of the Python face after one small call of its stage: the exact key set, the Python type of every
value (``int`` for the ABI's int32 / int64, ``float`` for its doubles) and the counts, which are literals recorded
from the commit before the getters shared one out-parameter reader.  Times are only floats >= 0.

One engine on device 0, four distinct reads of 16 bases; each stage runs once and its getters are read at once."""
import pytest

pytestmark = pytest.mark.gpu

GENOME = "ACGTTGCAATGCCGTAGGCTTAACGATC"
READS = [GENOME[o:o + 16] for o in (0, 4, 8, 12)]
CONTIG = GENOME + "GGTA"
CSR = ([0, 2, 3, 3], [1, 2, 2], [5, 8, 5])  # 0 -> 1 -> 2 and 0 -> 2, which both reductions remove

TIMES = {
    "last_timing": ("kernel_ms", "call_ms"),
    "last_seed_timing": ("keys_ms", "sort_ms", "count_ms", "emit_ms"),
    "last_consensus": ("align_ms", "pileup_ms", "vote_ms"),
    "last_consensus_placed": ("band_ms", "vote_ms"),
    "last_layout": ("score_ms", "link_ms", "forest_ms", "spell_ms"),
    "last_correct": ("keys_ms", "sort_ms", "count_ms", "correct_ms"),
}
# host_pool follows the box's CPUs: its keys and types are pinned, and what the plan guarantees on any box
BOX = ("host_pool",)

EXPECTED = {  # (times: any float >= 0 passes; host_pool: as recorded on a 16-CPU share)
    "info": {"n_reads": 4, "lmax": 16, "planes": 2, "device_bytes": 312},
    "candidates": 1,
    "last_seed_timing": {"keys_ms": 0.0, "sort_ms": 0.0, "count_ms": 0.0, "emit_ms": 0.0},
    "last_timing": {"kernel_ms": 0.0, "call_ms": 0.0},
    "last_transfer": {"link_bytes": 8, "packed_pairs": 0, "result_bytes": 8, "record_pairs": 0, "escapes": 0},
    "last_pair_list": {"in_place_pairs": 0, "decoded_pairs": 0},
    "last_score_form": {"kernel": "ungapped", "key64": 0, "wide": 0, "lane": 0, "prof": 0, "sfx": 0, "ho": 0, "h2": 0,
                        "band_form": "none", "split": 0, "rs_log2": 1},
    "resident_stats": {"alive": 0, "launches": 0, "relaunches": 0, "broken": 0},
    "devices_for": [1, 1, 1, 1],
    "last_read_best": {"lane_pairs": 4, "fallback_pairs": 0, "launches": 1},
    "last_consensus": {"batch_reads": 4, "single_reads": 0, "ops": 64, "launches": 1, "align_ms": 0.0,
                       "pileup_ms": 0.0, "vote_ms": 0.0},
    "last_consensus_placed": {"voted_reads": 0, "windowless_reads": 0, "ops": 0, "launches": 0, "rounds": 0,
                              "band_ms": 0.0, "vote_ms": 0.0},
    "layout_n_contigs": 3,
    "last_layout": {"links": 1, "cycles": 0, "levels": 2, "on_path_reads": 4, "score_ms": 0.0, "link_ms": 0.0,
                    "forest_ms": 0.0, "spell_ms": 0.0},
    "last_layout_host": {"links": 1, "cycles": 0, "levels": 0, "on_path_reads": 4},
    "last_correct": {"keys_ms": 0.0, "sort_ms": 0.0, "count_ms": 0.0, "correct_ms": 0.0},
    "transitive_mask": [0, 1, 0],
    "last_transitive": {"window": 20224, "passes": 1, "two_hop_steps": 1},
    "reach_mask": [0, 1, 0],
    "last_reach": {"words_per_row": 1, "pivot_blocks": 1, "window_bits": 16384},
    "last_local_batch": {"batched": 2, "single": 0, "waves": 2},
    "host_pool": {"threads": 12, "sharers": 1, "cpus": 16, "packed": 1},
}


def collect():
    """{getter name: what it returned} after the stage calls of this module's docstring."""
    from ovlgraph import OverlapEngine
    from ovlgraph.engine import host_pool, last_layout_host, layout_host
    got = {}
    with OverlapEngine(0) as eng:
        eng.set_timing(True)
        eng.set_reads(READS)
        got["info"] = eng.info()
        got["candidates"] = eng.enumerate_candidates(4)
        got["last_seed_timing"] = eng.last_seed_timing()
        sc, en = eng.score_candidates()
        for name in ("last_timing", "last_transfer", "last_pair_list", "last_score_form", "resident_stats"):
            got[name] = getattr(eng, name)()
        got["devices_for"] = [eng.devices_for(n) for n in (0, 1, got["candidates"], 1 << 20)]
        a, b = eng.candidates_copy(got["candidates"])
        eng.read_best(READS, [CONTIG], 16)
        got["last_read_best"] = eng.last_read_best()
        eng.consensus(READS, [CONTIG], [0, 0, 0, 0], 16)
        got["last_consensus"] = eng.last_consensus()
        got["last_consensus_placed"] = eng.last_consensus_placed()
        got["layout_n_contigs"] = eng.layout_candidates()["n_contigs"]
        got["last_layout"] = eng.last_layout()
        layout_host(READS, a, b, sc, en)
        got["last_layout_host"] = last_layout_host()
        eng.kmer_spectrum(READS, 4)
        got["last_correct"] = eng.last_correct()
        got["transitive_mask"] = eng.transitive_reduce(*CSR).tolist()
        got["last_transitive"] = eng.last_transitive()
        got["reach_mask"] = eng.reach_reduce(*CSR[:2]).tolist()
        got["last_reach"] = eng.last_reach()
        eng.local_align_batch(READS[:2], CONTIG)
        got["last_local_batch"] = eng.last_local_batch()
    got["host_pool"] = host_pool()
    return got


def test_every_getter_keeps_its_keys_types_and_counts():
    got = collect()
    assert set(got) == set(EXPECTED)
    for name, want in EXPECTED.items():
        have = got[name]
        if not isinstance(want, dict):
            assert type(have) is type(want) and have == want, name
            continue
        assert list(have) == list(want), name
        for key, value in want.items():
            assert type(have[key]) is type(value), (name, key)
            if key in TIMES.get(name, ()):
                assert type(have[key]) is float and have[key] >= 0, (name, key)
            elif name not in BOX:
                assert have[key] == value, (name, key)
    pool = got["host_pool"]
    assert pool["threads"] >= 1 and pool["sharers"] >= 1 and pool["cpus"] >= 1 and pool["packed"] in (0, 1)
