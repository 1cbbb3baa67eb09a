"""GPU: what a scoring launch is given -- its result sink, its error flag, its pair encoding and its timing events
(ovl_ctx.h LaunchIo) -- does not survive from one kind of call to the next on one engine.

1. One engine takes every kind of call in turn: packed and direct chunks into pinned arrays, a device call, a banded
   call whose seed stays in HBM while its results go to host memory, the layout's scoring of the resident list, a bad
   index through the host flag and through the device flag, and the first call again.
2. One call holds a chunk that uniform_kernel reads in place and a chunk that is decoded, in both orders, untimed and
   timed.
Every result is compared with the oracle."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _engine_env(env):
    from ovlgraph import OverlapEngine
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return OverlapEngine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _equal(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


def test_every_kind_of_call_in_turn_on_one_engine(oracle_mod):
    import torch
    from layout_cases import assert_same, with_contigs
    from ovlgraph import OvlError
    from ovlgraph.candidates import dedup_reads
    from ovlgraph.engine import host_pool, layout_host
    from ovlgraph.hostmem import pinned_empty
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads
    reads = dedup_reads(simulate_reads(read_genome_from_fasta(), 100, 400, 0.01, seed=0))[0]
    reads = [r for r in reads if len(r) == 100]  # one length <= 254: two bit planes, the packed sink applies
    nr = len(reads)
    assert nr >= 200
    rng = np.random.default_rng(20261021)
    n = 20_000
    a = rng.integers(0, nr, n, dtype=np.int32)
    b = rng.integers(0, nr, n, dtype=np.int32)
    ref = oracle_mod.batch_ungapped(reads, a, b)
    ref_band = oracle_mod.batch_banded(reads, a, b, 10, -1, -2, 8)
    dev = torch.device("cuda", 0)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    so, eo = torch.empty_like(ta), torch.empty_like(ta)
    pinned = (pinned_empty(n), pinned_empty(n))
    packs = host_pool()["threads"] >= 6  # (the library's own rule: fewer threads, and results cross as int32)

    def packed_call():
        pinned[0][:] = -9
        pinned[1][:] = -9
        eng.score(a, b, out=pinned)
        _equal(pinned, ref)
        if packs:  # four packed chunks of 4,096 pairs and a direct one
            assert eng.last_transfer()["packed_pairs"] > 0
        return pinned[0].copy(), pinned[1].copy()

    eng = _engine_env({"OVL_PACK_MIN": "0", "OVL_PIPE_CHUNK": "4096"})
    try:
        eng.set_reads(reads)
        first = packed_call()                                              # (a)
        eng.score_tensors(ta, tb, so, eo)                                  # (b)
        torch.cuda.synchronize(dev)
        eng.check_device_errors()
        _equal((so.cpu().numpy(), eo.cpu().numpy()), ref)
        eng.set_timing(True)                                               # (c)
        try:
            assert eng.plan(10, -1, -2, 8) == "banded"
            pinned[0][:] = -9
            eng.score(a, b, 10, -1, -2, band=8, out=pinned)
            launches = eng.last_launches()
        finally:
            eng.set_timing(False)
        _equal(pinned, ref_band)  # (seeds stored through the call's host sink would not have reached the band kernel)
        assert launches and all(x["ms"] > 0 and x["sink"] == 1 for x in launches), launches
        assert sum(x["pairs"] for x in launches) == n
        m = eng.enumerate_seed_candidates(12)                              # (d)
        assert m > 0
        ca, cb = (x.copy() for x in eng.candidates_copy(m))
        got = with_contigs(eng.layout_candidates())
        cs, ce = eng.score_candidates()
        _equal((cs, ce), oracle_mod.batch_ungapped(reads, ca, cb))
        assert_same(got, with_contigs(layout_host(reads, ca, cb, cs, ce)), "layout of the seed list")
        bad = b.copy()                                                     # (e)
        bad[n // 2 + 3] = nr
        pageable = (np.full(n, 7, np.int32), np.full(n, 7, np.int32))
        with pytest.raises(OvlError, match="OVL_E_INDEX"):
            eng.score(a, bad, out=pageable)
        ok = np.ones(n, bool)
        ok[n // 2 + 3] = False
        assert pageable[0][n // 2 + 3] == -1 and pageable[1][n // 2 + 3] == -1
        _equal((pageable[0][ok], pageable[1][ok]), (ref[0][ok], ref[1][ok]))
        so.fill_(-9)                                                       # (f)
        eng.score_tensors(ta, tb, so, eo)
        torch.cuda.synchronize(dev)
        eng.check_device_errors()  # the host call's flag did not leak into the device's
        _equal((so.cpu().numpy(), eo.cpu().numpy()), ref)
        eng.score_tensors(ta, torch.from_numpy(bad).to(dev), so, eo)
        torch.cuda.synchronize(dev)
        with pytest.raises(OvlError, match="OVL_E_INDEX"):
            eng.check_device_errors()
        _equal(eng.score(a, b, out=pageable), ref)  # ... nor the device call's into the host call's
        _equal(packed_call(), first)                                       # (g)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def two_chunks(oracle_mod):
    """2 * chunk a-major pairs (a = p // 512, b pseudo-random) over 600 reads of 60 bases, chunk the smallest that
    uniform_kernel reads in place (more than 8 tiles of 64 pairs per CU) and a margin; the oracle's results for the
    list as it is and with one tile of either chunk spoiled (an a more than 255 above its tile's first)."""
    import random
    import torch
    g = random.Random(20261021)
    reads = sorted({"".join(g.choice("ACGT") for _ in range(60)) for _ in range(600)})
    assert len(reads) == 600
    chunk = 64 * (8 * torch.cuda.get_device_properties(0).multi_processor_count + 64)
    p = np.arange(2 * chunk, dtype=np.int64)
    a = (p // 512).astype(np.int32)
    b = ((p * 2654435761 + 12345) % 600).astype(np.int32)
    lists = {}
    for spoiled in (0, 1):
        x = a.copy()
        at = spoiled * chunk + 64 * 5 + 10  # inside the chunk's sixth tile
        x[at] = x[at - 10] + 260
        assert int(x[at]) < len(reads)
        lists[spoiled] = (x, oracle_mod.batch_ungapped(reads, x, b))
    return reads, chunk, b, lists


@pytest.mark.parametrize("timing", [False, True], ids=["untimed", "timed"])
@pytest.mark.parametrize("spoiled", [1, 0], ids=["in_place_then_decoded", "decoded_then_in_place"])
def test_in_place_and_decoded_chunks_in_one_call(two_chunks, spoiled, timing):
    reads, chunk, b, lists = two_chunks
    a, ref = lists[spoiled]
    n = 2 * chunk
    eng = _engine_env({"OVL_PIPE_CHUNK": str(chunk)})
    try:
        eng.set_reads(reads)
        eng.set_timing(timing)
        out = (np.full(n, 7, np.int32), np.full(n, 7, np.int32))  # (pageable: the call is two chunks of `chunk`)
        eng.score(a, b, out=out)
        assert eng.last_pair_list() == {"in_place_pairs": chunk, "decoded_pairs": chunk}
        _equal(out, ref)
        if timing:
            launches = eng.last_launches()
            assert len(launches) == 2 and all(x["ms"] > 0 and x["pairs"] == chunk for x in launches), launches
    finally:
        eng.close()
