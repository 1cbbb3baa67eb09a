"""GPU: every scoring-range rule (csrc/ovl_score_range.h) on both sides of its edge, on reads that attain the bounds.

Each case takes its edge from the inequality (tests/extremal_reads.py ``edge`` / ``lane_form``, never from the
library), scores the extremal pairs of ``extremal_set`` -- identical reads, homopolymers, shifted copies, gap runs,
periodic reads, next to random reads and reads of length 1 and 0 -- and asserts two things: ``last_score_form`` (or
``last_local_batch`` / ``last_read_best``) shows the form the case was written for, and (score, end) equal the
oracle's bit for bit.  The lane forms are forced on these few hundred pairs with OVL_DP_FORM, OVL_LANE_FORM and
OVL_BAND_FORM.

Notation: sma = match - 2 indel, smm = mismatch - 2 indel, M = max(|match|, |mismatch|, |indel|), L = lmax.

Two edges cannot be reached through the API and are pinned on the host only (tests/c/score_range_check.cpp): the
band lane kernel's (6L + 2 band + 8) M < 2^30 (its byte scores keep M <= 254 and its reads L <= 1024), and
local_wide's top + M >= 2^31 through match (the best-cell key's match * min(n, m) < 2^24 is checked first); the
local cases below take local_wide at the edge that can decide, M = 2^30 through mismatch or indel."""
import functools
import os
import random

import numpy as np
import pytest

from extremal_reads import HOMO_A, R, assert_extremes, edge, extremal_set, h2_byte, lane_form

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


@pytest.fixture(scope="module")
def engines():
    """One engine per set of knobs (they are read once, when a context is created), shared by the cases."""
    cache = {}

    def get(**env):
        key = tuple(sorted(env.items()))
        if key not in cache:
            cache[key] = _engine_env(env)
        return cache[key]
    yield get
    for eng in cache.values():
        eng.close()


@functools.lru_cache(maxsize=None)
def _set(lmax):
    reads, a, b = extremal_set(lmax)
    if lmax >= 66:
        assert len(reads) == 25 and a.shape[0] % 64 and a.shape[0] % 128
    return reads, a, b


def _check(eng, oracle_fn, lmax, params, want, band=None):
    """Score the extremal pairs at ``params`` (and ``band``), assert the form fields in ``want`` and bit equality with
    the oracle; the oracle's own output must show the set's extremes."""
    reads, a, b = _set(lmax)
    args = params if band is None else (*params, band)
    rs, re_ = oracle_fn(reads, a, b, *args)
    assert_extremes(reads, a, b, rs, re_, params[0], params[1], params[2] if len(params) > 2 else None)
    eng.set_reads(reads)
    if len(params) == 2:
        sc, en = eng.score(a, b, *params)
    else:
        sc, en = eng.score(a, b, *params, -1 if band is None else band)
    eng.check_device_errors()
    form = eng.last_score_form()
    got = {k: form[k] for k in want}
    assert got == want, (params, form)
    np.testing.assert_array_equal(sc, rs, err_msg=str(params))
    np.testing.assert_array_equal(en, re_, err_msg=str(params))
    return form


# ----------------------------------------------------------------------------- full DP, lane kernels

LANE = {"OVL_DP_FORM": "lane"}


@pytest.mark.parametrize("params, ho", [((13, -1, -1), 2), ((15, -2, 0), 2), ((9, 3, -3), 2), ((14, -1, -1), 1),
                                        ((-1, -2, -1), 2), ((-3, -5, -3), 2), ((-4, -5, -3), 1)])
def test_four_bit_steps_at_step_15_and_16(engines, oracle_mod, params, ho):
    """step_max = max(match, mismatch) - 2 indel: 15 is in, 16 is out; the other clause, max(match, mismatch) >=
    indel, with both scores negative: (-3, -5, -3) sits on it, (-4, -5, -3) just outside."""
    want = lane_form(*params, 256)
    assert want["ho"] == ho
    _check(engines(**LANE), oracle_mod.batch_dp, 256, params, dict(want, kernel="dp", lane=1, wide=0))


@pytest.mark.parametrize("lmax, ho", [(256, 2), (257, 1)])
def test_four_bit_steps_at_256_and_257_bases(engines, oracle_mod, lmax, ho):
    """The LDS hand-off holds 256 rows: 257-base reads have no bit planes and take the int16 column."""
    want = lane_form(13, -1, -1, lmax, planes=lmax <= 256)
    assert want["ho"] == ho
    _check(engines(**LANE), oracle_mod.batch_dp, lmax, (13, -1, -1), {"lane": 1, "ho": ho, "sfx": want["sfx"]})


SMM = (0, -2, -112, -128, -127, -129)


@pytest.mark.parametrize("lmax", [256, 100])
@pytest.mark.parametrize("indel", [0, -1, -3])
@pytest.mark.parametrize("sma", range(1, 17))
def test_packed_f16_at_every_match_step(engines, oracle_mod, lmax, indel, sma):
    """dp_lane_h2_kernel at every sma from 1 to 16 with smm in {sma - 1 where it is a byte score, 0, -2, -112, -128}
    and the ineligible neighbours -127 (profile, no f16 form) and -129 (no profile): h2 is reported exactly where
    both diagonal scores are f16 byte scores under the 4-bit step rule -- up to the largest steps (14) and the most
    negative diagonal score (-128) on identical, homopolymer and gap-run reads, the exactness argument's worst case."""
    eng = engines(**LANE)
    n_h2 = 0
    for smm in ((sma - 1,) if h2_byte(sma - 1) else ()) + SMM:
        params = (sma + 2 * indel, smm + 2 * indel, indel)
        want = lane_form(*params, lmax)
        assert want["h2"] == int(h2_byte(sma) and h2_byte(smm) and sma <= 15 and smm >= -128
                                 and params[0] >= indel)
        _check(eng, oracle_mod.batch_dp, lmax, params, dict(want, kernel="dp", lane=1))
        n_h2 += want["h2"]
    assert n_h2 == (4 + h2_byte(sma - 1) if h2_byte(sma) and sma <= 15 and sma + 2 * indel >= indel else 0)


@pytest.mark.parametrize("form", ["7", "1"])
@pytest.mark.parametrize("params, prof", [((7, -1, -60), 1), ((8, -1, -60), 0), ((1, -248, -60), 1),
                                          ((1, -249, -60), 0)])
def test_int8_profile_at_127_and_minus_128(engines, oracle_mod, params, prof, form):
    """sma = 127 in, 128 out; smm = -128 in, -129 out; with the row symbols from the bit planes and without."""
    want = lane_form(*params, 256, sfx_on=form == "7")
    assert want["prof"] == prof and want["ho"] == 0
    _check(engines(OVL_LANE_FORM=form, **LANE), oracle_mod.batch_dp, 256, params, dict(want, lane=1))


def _through(M, lmax):
    """M reached once through each score (no 4-bit steps: the steps exceed 15 or the planes are off); beside an indel
    of -M the match is large enough for gaps to win (lmax * match > M), or the call would take the closed form"""
    return [(M, -1, -1), (1, -M, -1), (M // lmax + 2, -1, -M)]


@pytest.mark.parametrize("lmax", [100, 260])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_int16_column_at_its_largest_magnitude(engines, oracle_mod, lmax, which):
    """The largest M with (4L + 4) M < 2^15 takes the int16 hand-off column, M + 1 the int32 one (bit planes off:
    OVL_LANE_FORM=1, so that no scoring takes the 4-bit steps instead)."""
    M = edge("ho1", lmax)
    assert (4 * lmax + 4) * M < 2 ** 15 <= (4 * lmax + 4) * (M + 1)
    eng = engines(OVL_LANE_FORM="1", **LANE)
    _check(eng, oracle_mod.batch_dp, lmax, _through(M, lmax)[which], {"lane": 1, "ho": 1, "sfx": 0})
    _check(eng, oracle_mod.batch_dp, lmax, _through(M + 1, lmax)[which], {"lane": 1, "ho": 0, "sfx": 0})


@pytest.mark.parametrize("lmax", [100, 256])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_lane_int32_range_at_its_largest_magnitude(engines, oracle_mod, lmax, which):
    """The largest M with (4L + 4) M < 2^30 still takes the lane kernel (int32 column); M + 1 reports lane == 0 and
    the anti-diagonal kernel equals the oracle."""
    M = edge("lane_int32", lmax)
    assert (4 * lmax + 4) * M < 2 ** 30 <= (4 * lmax + 4) * (M + 1)
    eng = engines(**LANE)
    _check(eng, oracle_mod.batch_dp, lmax, _through(M, lmax)[which], {"kernel": "dp", "lane": 1, "ho": 0, "wide": 0})
    _check(eng, oracle_mod.batch_dp, lmax, _through(M + 1, lmax)[which], {"kernel": "dp", "lane": 0, "wide": 0})


@pytest.mark.parametrize("dp_form", ["fast", "classic"])
@pytest.mark.parametrize("lmax", [100, 256])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_int32_cells_at_their_largest_magnitude(engines, oracle_mod, lmax, which, dp_form):
    """The largest M with (2L + 1) M < 2^31 keeps int32 cells, M + 1 takes the wide ones, in dp_fast_kernel and in
    dp_kernel."""
    M = edge("wide", lmax)
    assert (2 * lmax + 1) * M < 2 ** 31 <= (2 * lmax + 1) * (M + 1)
    eng = engines(OVL_DP_FORM=dp_form)
    _check(eng, oracle_mod.batch_dp, lmax, _through(M, lmax)[which], {"kernel": "dp", "lane": 0, "wide": 0})
    _check(eng, oracle_mod.batch_dp, lmax, _through(M + 1, lmax)[which], {"kernel": "dp", "lane": 0, "wide": 1})


# ----------------------------------------------------------------------------- ungapped

def _key_cases():
    cases = []
    for L in (100, 256):
        amax = edge("key32", L)
        assert amax * (2 * L + 32) < 2 ** 15 <= (amax + 1) * (2 * L + 32)
        if amax < 128:  # through match and through mismatch
            cases += [(L, (amax, -1), 0), (L, (amax + 1, -1), 1), (L, (1, -amax), 0), (L, (1, -amax - 1), 1)]
        else:  # the two 128 clauses leave only mismatch = match - 127 < -127
            cases += [(L, (127 - amax, -amax), 0), (L, (126 - amax, -amax - 1), 1)]
    # |mismatch - match| = 127 / 128 and |match| = 127 / 128, where amax leaves room (L = 100: amax <= 141)
    cases += [(100, (100, -27), 0), (100, (100, -28), 1), (100, (-27, 100), 0), (100, (-28, 100), 1),
              (100, (127, 0), 0), (100, (128, 1), 1), (100, (127, -1), 1)]
    return cases


@pytest.mark.parametrize("lmax, params, key64", _key_cases())
def test_folded_keys_at_their_edges_latency_mode(engines, oracle_mod, lmax, params, key64):
    form = _check(engines(), oracle_mod.batch_ungapped, lmax, params, {"kernel": "ungapped", "key64": key64})
    assert form["rs_log2"] > 0  # a few hundred pairs: latency mode


@pytest.mark.parametrize("delta, key64", [(0, 0), (1, 1)])
def test_folded_keys_at_their_edge_throughput_mode(engines, oracle_mod, delta, key64):
    """The same extremal pairs tiled to just above the planner's latency cut (32 tiles of 64 pairs per CU for a device
    list), through ``score_tensors``: rs_log2 == 0 says the launch was a throughput-mode one."""
    import torch
    lmax = 256
    reads, a, b = _set(lmax)
    params = (edge("key32", lmax) + delta, -1)
    rs, re_ = oracle_mod.batch_ungapped(reads, a, b, *params)
    assert_extremes(reads, a, b, rs, re_, *params, None)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reps = cus * 32 * 64 // a.shape[0] + 2
    dev = torch.device("cuda", 0)
    ta, tb = torch.from_numpy(np.tile(a, reps)).to(dev), torch.from_numpy(np.tile(b, reps)).to(dev)
    so, eo = torch.empty_like(ta), torch.empty_like(ta)
    eng = engines()
    eng.set_reads(reads)
    eng.score_tensors(ta, tb, so, eo, *params)
    torch.cuda.synchronize(dev)
    eng.check_device_errors()
    form = eng.last_score_form()
    assert (form["kernel"], form["key64"], form["rs_log2"]) == ("ungapped", key64, 0), form
    np.testing.assert_array_equal(so.cpu().numpy(), np.tile(rs, reps))
    np.testing.assert_array_equal(eo.cpu().numpy(), np.tile(re_, reps))


@pytest.mark.parametrize("lmax", [100, 256])
@pytest.mark.parametrize("scores", [(10, -1), (3, 2), (-2, -3), (127, -127)])
def test_gaps_cannot_win_at_its_edge(engines, oracle_mod, lmax, scores):
    """indel exactly lo - hi reports the closed form, lo - hi + 1 the DP; both equal the reference DP -- the periodic
    and homopolymer pairs are where a gap path could tie."""
    lo, hi = min(0, lmax * min(scores)), max(0, lmax * max(scores))
    eng = engines()
    _check(eng, oracle_mod.batch_dp, lmax, (*scores, lo - hi), {"kernel": "ungapped"})
    _check(eng, oracle_mod.batch_dp, lmax, (*scores, lo - hi + 1), {"kernel": "dp"})


@pytest.mark.parametrize("lmax", [100, 256])
def test_ungapped_int32_stores_at_their_edge(engines, oracle_mod, lmax):
    """amax L < 2^31: the largest amax is scored by the closed form (64-bit keys), amax + 1 by the wide DP."""
    amax = edge("ungapped_int32", lmax)
    assert amax * lmax < 2 ** 31 <= (amax + 1) * lmax
    eng = engines()
    for m, kernel in ((amax, "ungapped"), (amax + 1, "dp")):
        indel = -lmax - lmax * m  # lo - hi of (m, -1): gaps cannot win on either side
        want = {"kernel": kernel, "key64": 1} if kernel == "ungapped" else {"kernel": kernel, "wide": 1}
        _check(eng, oracle_mod.batch_dp, lmax, (m, -1, indel), want)


def test_launcher_reports_its_form(engines, oracle_mod):
    """``launcher`` (the pre-bound device call) records the form like the other entry points, and a later call
    replaces it."""
    import torch
    reads, a, b = _set(100)
    eng = engines(**LANE)
    eng.set_reads(reads)
    dev = torch.device("cuda", 0)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    so, eo = torch.empty_like(ta), torch.empty_like(ta)
    launch = eng.launcher(ta, tb, so, eo, 13, -1, -1, -1)
    launch()
    torch.cuda.synchronize(dev)
    form = eng.last_score_form()
    assert {k: form[k] for k in ("kernel", "lane", "ho", "h2")} == {"kernel": "dp", "lane": 1, "ho": 2, "h2": 0}
    rs, re_ = oracle_mod.batch_dp(reads, a, b, 13, -1, -1)
    np.testing.assert_array_equal(so.cpu().numpy(), rs)
    np.testing.assert_array_equal(eo.cpu().numpy(), re_)
    eng.score(a, b)
    assert eng.last_score_form()["kernel"] == "ungapped" and eng.last_score_form()["lane"] == 0


# ----------------------------------------------------------------------------- band knob

BYTE_EDGES = [((1, 0, -63), True), ((2, 0, -63), False),        # sma 127 / 128
              ((0, 1, -63), True), ((0, 2, -63), False),        # smm 127 / 128
              ((1, -128, 0), True), ((1, -129, 0), False),      # smm -128 / -129
              ((-128, 1, 0), True), ((-129, 1, 0), False),      # sma -128 / -129
              ((1, -1, -63), True), ((-1, -2, -64), False)]     # -2 indel 126 / 128


@pytest.mark.parametrize("band", [8, 64])
@pytest.mark.parametrize("knob", ["lane1", "lane2"])
@pytest.mark.parametrize("params, lane_ok", BYTE_EDGES)
def test_band_lane_bytes_at_their_edges(engines, oracle_mod, knob, band, params, lane_ok):
    """The band lane kernels' byte scores: inside, the forced lane form runs (one or two lanes per pair as asked);
    one outside, the call falls back to an anti-diagonal form and still equals the oracle."""
    eng = engines(OVL_BAND_FORM=knob)
    if lane_ok:
        _check(eng, oracle_mod.batch_banded, 256, params,
               {"kernel": "banded", "band_form": "lane", "split": int(knob == "lane2")}, band)
    else:
        form = _check(eng, oracle_mod.batch_banded, 256, params, {"kernel": "banded", "split": 0}, band)
        assert form["band_form"] in ("diag", "fast"), form


@pytest.mark.parametrize("band", [8, 64])
@pytest.mark.parametrize("knob, inside, outside", [("diag", "diag", "fast"), ("rows", "rows", "strip")])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_band_minus_infinity_at_its_largest_magnitude(engines, oracle_mod, knob, inside, outside, band, which):
    """kBandNeg stays below every value while (4L + 2) M < 2^29: the diagonal and the row form at the largest such
    M, their fallbacks at M + 1."""
    lmax = 256
    M = edge("band_neg", lmax)
    assert (4 * lmax + 2) * M < 2 ** 29 <= (4 * lmax + 2) * (M + 1)
    eng = engines(OVL_BAND_FORM=knob)
    for m, form in ((M, inside), (M + 1, outside)):
        _check(eng, oracle_mod.batch_banded, lmax, _through(m, lmax)[which], {"kernel": "banded", "band_form": form},
               band)


# ----------------------------------------------------------------------------- local alignment stages

def _local_case():
    """The extremal families as (query, reference) pairs: the reference holds the random read, a homopolymer run and
    a periodic stretch; the queries are the set's reads."""
    reads, _, _ = _set(100)
    reference = reads[R] + reads[HOMO_A][:40] + reads[10]
    return [q for q in reads if q], reference


def _assert_local_equals_oracle(oracle_mod, res, queries, reference, params):
    score, _, end_j, _, start_j, _ = res
    for k, q in enumerate(queries):
        exp = oracle_mod.local_alignment(q, reference, *params)
        assert (int(score[k]), int(start_j[k]), int(end_j[k])) == tuple(exp[3:6]), (k, params)


@pytest.mark.parametrize("params, single", [((10, -(2 ** 30 - 1), -1), False), ((10, -(2 ** 30), -1), True),
                                            ((10, -1, -(2 ** 30 - 1)), False), ((10, -1, -(2 ** 30)), True)])
def test_local_wide_at_its_edge(engines, oracle_mod, params, single):
    """M = 2^30 - 1 keeps every query on the batch kernel, M = 2^30 sends each alone through the wide form."""
    queries, reference = _local_case()
    eng = engines()
    res = eng.local_align_batch(queries, reference, None, *params)
    last = eng.last_local_batch()
    assert (last["single"], last["batched"]) == ((len(queries), 0) if single else (0, len(queries)))
    _assert_local_equals_oracle(oracle_mod, res, queries, reference, params)


@pytest.mark.parametrize("params, single", [((10, -(2 ** 30 - 1), -1), False), ((10, -(2 ** 30), -1), True)])
def test_consensus_routes_at_the_local_wide_edge(engines, oracle_mod, params, single):
    """The same routing rule in ``consensus``: every read's alignment (score, first and last column) equals the
    oracle's on either side, and the whole result the host form's."""
    from ovlgraph.engine import consensus_host
    queries, reference = _local_case()
    place = np.zeros(len(queries), dtype=np.int32)
    eng = engines()
    res = eng.consensus(queries, [reference], place, 100, *params)
    last = eng.last_consensus()
    assert (last["single_reads"], last["batch_reads"]) == ((len(queries), 0) if single else (0, len(queries)))
    for k, q in enumerate(queries):
        score, start, end = oracle_mod.align_read_or_contig_to_reference(q, reference, 100, *params)[3:6]
        assert tuple(res["aln"][k]) == ((score, start, end) if score > 0 else (0, 0, 0)), (k, q)
    host = consensus_host(queries, [reference], place, 100, *params)
    for key in host:
        np.testing.assert_array_equal(res[key], host[key], err_msg=key)


def _raw_local_batch(eng, queries, reference, match):
    """ovl_local_align_batch with its outputs prefilled: (return code, the outputs)."""
    from ovlgraph.engine import _ptr, encode_reads
    nq = len(queries)
    buf, offs = encode_reads(list(queries) + [reference])
    q_off = np.ascontiguousarray(offs[: nq + 1])
    ref = np.ascontiguousarray(buf[int(offs[nq]):])
    outs = [np.full(nq, -7, dtype=np.int32) for _ in range(5)]
    n_ops = np.full(nq, -7, dtype=np.int64)
    rc = eng._L.ovl_local_align_batch(eng._ctx, _ptr(buf), _ptr(q_off), nq, _ptr(ref), len(reference), None, None,
                                      match, -1, -1, *[_ptr(o) for o in outs], None, None, _ptr(n_ops))
    return rc, outs + [n_ops]


@pytest.mark.parametrize("n", [1, 64])
def test_local_key_score_at_2_to_the_24(engines, oracle_mod, n):
    """match * min(n, m) below 2^24 (2^24 - 1 at one base, 2^24 - 64 at 64) equals the oracle; at 2^24 the call
    returns OVL_E_UNSUPPORTED with its outputs untouched."""
    rng = random.Random(n)
    q = "".join(rng.choice("ACGT") for _ in range(n))
    reference = "".join(rng.choice("ACGT") for _ in range(90)) + q + "ACGTTGCA"
    match = edge("local_key", n)
    assert match * n < 2 ** 24 <= (match + 1) * n
    eng = engines()
    res = eng.local_align_batch([q, q[: n // 2]], reference, None, match, -1, -1)
    assert int(res[0][0]) == match * n
    _assert_local_equals_oracle(oracle_mod, res, [q, q[: n // 2]], reference, (match, -1, -1))
    rc, outs = _raw_local_batch(eng, [q, q[: n // 2]], reference, match + 1)
    assert rc == -4
    assert all((o == -7).all() for o in outs)


@pytest.fixture(scope="module")
def long_contig():
    """A contig of 0xFFFFF bases over {A, C} whose last 64 bases are a read over {G, T}: the read occurs only there,
    so the best cell is (64, 0xFFFFF)."""
    rng = np.random.default_rng(5)
    read = "".join(rng.choice(list("GT"), 64))
    body = np.where(rng.integers(0, 2, 0xFFFFF - 64), ord("A"), ord("C")).astype(np.uint8).tobytes().decode()
    return read, body + read


def test_best_cell_in_column_0xFFFFF(engines, oracle_mod, long_contig):
    """The last column a cell key holds: the lane-per-read kernel's (bi << 20) | bestj word through ``read_best``,
    the batch kernel's 64-bit key through ``local_align_batch``; one more base is refused."""
    from ovlgraph._lib import OvlError
    read, contig = long_contig
    assert len(contig) == 0xFFFFF
    exp = oracle_mod.align_read_or_contig_to_reference(read, contig, 64)[3:6]
    assert tuple(exp) == (640, 0xFFFFF - 64, 0xFFFFF)
    eng = engines()
    res = eng.read_best([read], [contig], 64)
    assert eng.last_read_best()["lane_pairs"] == 1 and eng.last_read_best()["fallback_pairs"] == 0
    assert (int(res["best_score"][0]), int(res["start"][0]), int(res["end"][0])) == tuple(exp)
    out = eng.local_align_batch([read], contig, None, 10, -1, -1, traceback=False)
    assert eng.last_local_batch()["batched"] == 1
    assert (int(out[0][0]), int(out[1][0]), int(out[2][0])) == (640, 64, 0xFFFFF)  # (no walk asked for: no start)
    for call in (lambda: eng.read_best([read], ["A" + contig], 64),
                 lambda: eng.local_align_batch([read], "A" + contig, None, 10, -1, -1, traceback=False)):
        with pytest.raises(OvlError) as e:
            call()
        assert e.value.code == -4


@pytest.mark.parametrize("params, lane", [((65535, -1, -1), True), ((65536, -1, -1), False),
                                          ((10, 0, -1), True), ((10, 1, -1), False),
                                          ((10, -1, 0), True), ((10, -1, 1), False)])
def test_read_best_lane_scorings_at_their_edges(engines, oracle_mod, params, lane):
    """The lane-per-read kernel's scorings: match 65535 (the largest score in its v << 8 key on an identical
    128-base pair) / 65536, mismatch 0 / +1, indel 0 / +1 -- inside, every pair is a lane pair; outside, a fallback
    pair; both equal the oracle."""
    reads, _, _ = _set(128)
    pick = [reads[R], reads[HOMO_A], reads[4], reads[8], reads[9], reads[10]]
    contigs = [reads[R], reads[HOMO_A] + reads[11]]
    eng = engines()
    res = eng.read_best(pick, contigs, 128, *params, scores=True)
    last = eng.last_read_best()
    n = len(pick) * len(contigs)
    assert (last["lane_pairs"], last["fallback_pairs"]) == ((n, 0) if lane else (0, n))
    t = np.array([[oracle_mod.align_read_or_contig_to_reference(r, c, 128, *params)[3:6] for c in contigs]
                  for r in pick], dtype=np.int64)
    np.testing.assert_array_equal(res["scores"], t[:, :, 0])
    best = t[:, :, 0].max(axis=1)
    first = t[:, :, 0].argmax(axis=1)
    np.testing.assert_array_equal(res["best_score"], best)
    np.testing.assert_array_equal(res["first_best"], first)
    np.testing.assert_array_equal(res["start"], t[np.arange(len(pick)), first, 1])
    np.testing.assert_array_equal(res["end"], t[np.arange(len(pick)), first, 2])
    if params[0] >= 65535:
        assert best[0] == 128 * params[0]


@pytest.mark.parametrize("n_symbols, lane", [(255, True), (256, False)])
def test_read_best_symbols_at_255_and_256(engines, oracle_mod, n_symbols, lane):
    """255 distinct byte values leave the lane kernel its padding symbol; 256 do not."""
    alphabet = [chr(c) for c in range(n_symbols)]
    rng = random.Random(n_symbols)
    contig = "".join(alphabet) + "".join(rng.choice(alphabet) for _ in range(100))
    pick = [contig[40:140], contig[200:300], "".join(rng.choice(alphabet) for _ in range(100))]
    eng = engines()
    res = eng.read_best(pick, [contig], 100, scores=True)
    last = eng.last_read_best()
    assert (last["lane_pairs"], last["fallback_pairs"]) == ((3, 0) if lane else (0, 3))
    t = np.array([oracle_mod.align_read_or_contig_to_reference(r, contig, 100)[3:6] for r in pick], dtype=np.int64)
    np.testing.assert_array_equal(res["scores"][:, 0], t[:, 0])
    np.testing.assert_array_equal(res["start"], t[:, 1])
    np.testing.assert_array_equal(res["end"], t[:, 2])
