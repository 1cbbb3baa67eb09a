"""Seed candidates on the device (ovl_seed_candidates) against the host form, element for element: the lists and their
offsets, the key limit and the argument checks, the list's lifetime beside ovl_candidates, scoring the resident seed
list, and the assembly end to end.  ``candidates.enumerate_seed_candidates`` is itself pinned to the rule's literal
loops by tests/test_seed_candidates_cpu.py."""
import random

import numpy as np
import pytest

from seed_inputs import gpu_only_sets, input_sets, phix_reads

pytestmark = pytest.mark.gpu

SETS = dict(input_sets(), **gpu_only_sets())
E_ARG, E_UNSUPPORTED, E_STATE = -1, -4, -6


@pytest.fixture(scope="module")
def engine():
    from ovlgraph import OverlapEngine
    eng = OverlapEngine(0)
    yield eng
    eng.close()


def _host(distinct, k):
    from ovlgraph.candidates import enumerate_seed_candidates
    return enumerate_seed_candidates(distinct, k)


def _check(eng, distinct, k):
    eng.set_reads(distinct)
    n = eng.enumerate_seed_candidates(k)
    want = _host(distinct, k)
    assert n == want[0].shape[0]
    a, b = eng.candidates_copy(n)
    for got, w in zip((a, b, eng.seed_offsets()), want):
        np.testing.assert_array_equal(got, w)
    return n


def _code(call):
    from ovlgraph import OvlError
    with pytest.raises(OvlError) as err:
        call()
    return err.value.code


@pytest.mark.parametrize("name", sorted(SETS))
def test_device_list_equals_host_form(engine, name):
    distinct, k = SETS[name]
    n = _check(engine, distinct, k)
    if name == "long_group":
        a, b = engine.candidates_copy(n)
        assert np.bincount(a)[0] >= 200  # one read's group of more than three 64-member steps
    if name == "many_reads":
        assert len(distinct) > 2000 and n > 0


@pytest.mark.parametrize("name", ["phix200", "repeats", "own_prefix", "long_group", "long_reads"])
def test_groups_searched_again_in_the_emit_pass(monkeypatch, name):
    """OVL_SEED_GROUPS=search: the emit pass forms the keys and searches the groups again instead of reading what the
    count pass left in HBM -- the same list."""
    from ovlgraph import OverlapEngine
    monkeypatch.setenv("OVL_SEED_GROUPS", "search")
    with OverlapEngine(0) as eng:
        assert _check(eng, *SETS[name]) > 0


def _windows(seed, step, n=60, length=40):
    rng = random.Random(seed)
    text = "".join(rng.choice("ACGT") for _ in range(length + step * n))
    return [text[p:p + length] for p in range(0, step * n, step)]


def test_key_limit_and_argument_checks(engine, oracle_mod):
    from ovlgraph import OverlapEngine
    from ovlgraph.candidates import dedup_reads
    distinct = dedup_reads(_windows(31, 3))[0]
    assert _check(engine, distinct, 29) > 0  # 58 bits
    a, b = engine.candidates_copy(engine.candidates_device()[2])
    a, b, o = a.copy(), b.copy(), engine.seed_offsets().copy()
    ref = oracle_mod.batch_dp(distinct, a, b)
    for k, code in ((30, E_UNSUPPORTED), (0, E_ARG), (-1, E_ARG)):
        assert _code(lambda: engine.enumerate_seed_candidates(k)) == code
        # the previous list is intact and still scores
        a2, b2 = engine.candidates_copy(engine.candidates_device()[2])
        for got, want in ((a2, a), (b2, b), (engine.seed_offsets(), o)):
            np.testing.assert_array_equal(got, want)
        sc, en = engine.score_candidates()
        np.testing.assert_array_equal(sc, ref[0])
        np.testing.assert_array_equal(en, ref[1])
    with OverlapEngine(0) as fresh:
        assert _code(lambda: fresh.enumerate_seed_candidates(5)) == E_STATE
        assert _code(fresh.seed_offsets) == E_STATE


def test_list_lifetime(engine):
    from ovlgraph.candidates import enumerate_candidates
    distinct, k = SETS["phix200"]
    engine.set_reads(distinct)
    for rule in ("seed", "suffix", "seed"):
        if rule == "seed":
            n = engine.enumerate_seed_candidates(k)
            want = _host(distinct, k)
            np.testing.assert_array_equal(engine.seed_offsets(), want[2])
        else:
            n = engine.enumerate_candidates(5)
            want = enumerate_candidates(distinct, 5)
            assert _code(engine.seed_offsets) == E_STATE
        a, b = engine.candidates_copy(n)
        np.testing.assert_array_equal(a, want[0])
        np.testing.assert_array_equal(b, want[1])
    # other reads: the list is gone; the same reads again: gone too, as after ovl_candidates
    engine.set_reads(SETS["acgt"][0])
    assert _code(engine.candidates_device) == E_STATE
    assert _code(engine.seed_offsets) == E_STATE
    assert _code(engine.score_candidates) == E_STATE
    _check(engine, *SETS["acgt"])


def test_scoring_the_seed_list(engine, oracle_mod):
    from ovlgraph.candidates import dedup_reads
    distinct = dedup_reads(phix_reads(300))[0]
    engine.set_reads(distinct)
    n = engine.enumerate_seed_candidates(12)
    a, b = engine.candidates_copy(n)
    a, b = a.copy(), b.copy()
    assert n > 1000
    for args in ((), (10, -1, -2)):
        ref_s, ref_e = oracle_mod.batch_dp(distinct, a, b, *args)
        sc, en = engine.score_candidates(*args)
        np.testing.assert_array_equal(sc, ref_s)
        np.testing.assert_array_equal(en, ref_e)
        for lo, hi in ((0, n), (64, 700), (n // 3, n // 3 + 1), (n - 5, n), (7, 7)):
            rs, re_ = engine.score_candidates_range(lo, hi, *args)
            np.testing.assert_array_equal(rs, ref_s[lo:hi])
            np.testing.assert_array_equal(re_, ref_e[lo:hi])
    bounds = np.zeros(5, dtype=np.int64)
    from ovlgraph import _lib
    _lib.check(engine._L.ovl_candidates_shards(engine._ctx, 4, bounds.ctypes.data), engine._ctx)
    assert bounds[0] == 0 and bounds[4] == n and np.all(np.diff(bounds) > 0)


def test_auto_takes_the_host_form_when_the_keys_do_not_fit(engine, oracle_mod):
    from ovlgraph import overlapGraphs as og
    distinct = SETS["forty_bytes_overlaps"][0]  # 8 bits per symbol: k = 8 needs 64 bits
    a, b, _ = _host(distinct, 8)
    ref_s, ref_e = oracle_mod.batch_dp(distinct, a, b)
    assert a.shape[0] > 0
    got = og.candidates_and_scores(distinct, 8, engine=engine, seeds="any")
    for g, w in zip(got, (a, b, ref_s, ref_e)):
        np.testing.assert_array_equal(g, w)
    assert _code(lambda: og.candidates_and_scores(distinct, 8, engine=engine, seeds="any",
                                                  candidates="device")) == E_UNSUPPORTED


def test_every_device_of_the_context_enumerates(monkeypatch, oracle_mod):
    """A three-slot context (every slot on GPU 0): each slot enumerates the list from its own reads, and a scoring
    call sharded over the slots reads each slot's copy."""
    from ovlgraph import OverlapEngine
    monkeypatch.setenv("OVL_SHARE_DEVICES", "1")
    distinct, k = SETS["phix200"]
    with OverlapEngine(devices=[0, 0, 0]) as eng:
        n = _check(eng, distinct, k)
        a, b = eng.candidates_copy(n)
        ref_s, ref_e = oracle_mod.batch_dp(distinct, a, b)
        sc, en = eng.score_candidates()
        np.testing.assert_array_equal(sc, ref_s)
        np.testing.assert_array_equal(en, ref_e)


def test_seed_timing(engine):
    distinct, k = SETS["phix200"]
    engine.set_reads(distinct)
    engine.set_timing(True)
    try:
        engine.enumerate_seed_candidates(k)
        t = engine.last_seed_timing()
    finally:
        engine.set_timing(False)
    assert sorted(t) == ["count_ms", "emit_ms", "keys_ms", "sort_ms"] and all(v > 0.0 for v in t.values())
    engine.enumerate_seed_candidates(k)
    assert all(v == 0.0 for v in engine.last_seed_timing().values())


def test_end_to_end_parity(engine, oracle_mod):
    from ovlgraph import overlapGraphs as og
    reads = phix_reads(300)
    dev = og.assemble_contigs_using_overlap_graphs(reads, k=12, engine=engine, seeds="any", candidates="device")
    host = og.assemble_contigs_using_overlap_graphs(reads, k=12, seeds="any",
                                                    scorer=lambda r, a, b: oracle_mod.batch_dp(r, a, b))
    assert dev == host and max(map(len, dev)) > 100
    auto = og.assemble_contigs_using_overlap_graphs(reads, k=12, engine=engine, seeds="any")
    assert auto == host
