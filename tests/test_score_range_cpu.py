"""CPU: the scoring-range rules of csrc/ovl_score_range.h at their edges.

tests/c/score_range_check.cpp checks every rule on both sides of its edge and h2_byte_score against the IEEE half
encoding; here its edges are compared with the closed forms of tests/extremal_reads.py (the numbers the GPU tests of
tests/test_gpu_score_ranges.py use), its accepted f16 byte scores with numpy.float16, and the step claim that the
4-bit and packed-f16 cell forms rest on is checked by a numpy statement of the reference recurrence over the extremal
pairs: for every scoring the rules give the 4-bit hand-off, every vertical and horizontal step of
G = dp - indel * (i + j) lies in [0, max(match, mismatch) - 2 * indel]."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from extremal_reads import assert_extremes, edge, extremal_set, step_range

LMAX = (1, 100, 256, 257, 1024)


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("score_range") / "score_range_check"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        "-o", str(exe), os.path.join(ROOT, "tests", "c", "score_range_check.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok"
    return lines


def test_edges_match_closed_forms(check_output):
    """Every edge the program found by bisecting the library's predicate is the closed form's, and no edge is
    missing: each magnitude rule at each lmax (the 32-bit keys' where the two 128 clauses leave it reachable)."""
    got = {}
    for line in check_output:
        if line.startswith("edge "):
            _, rule, L, m_in, m_out = line.split()
            got[(rule, int(L))] = (int(m_in), int(m_out))
    want = {}
    for L in LMAX:
        for rule in ("wide", "lane_int32", "ho1", "band_neg", "ungapped_int32", "local_key", "local_int32"):
            want[(rule, L)] = (edge(rule, L), edge(rule, L) + 1)
        if edge("key32", L) < 254:  # above, |match| or |mismatch - match| reaches 128 first
            want[("key32", L)] = (edge("key32", L), edge("key32", L) + 1)
    for band in (8, 64):
        want[(f"band_lane_lmax{band}", 0)] = (edge("band_lane_lmax", 0, band), edge("band_lane_lmax", 0, band) + 1)
    assert got == want
    # a few of them written out: M = 31 for the int16 column at 256 bases, about 1.04e6 for the lane kernel's int32
    assert edge("ho1", 256) == 31 and edge("lane_int32", 256) == 1044495 and edge("key32", 100) == 141
    assert edge("key32", 256) == 60 and edge("local_int32", 64) == 33038209


def test_h2_byte_scores_match_numpy_float16(check_output):
    """h2_byte_score(v) for |v| <= 2048 is true exactly where numpy's float16 of v has a zero low byte."""
    line = [x for x in check_output if x.startswith("h2 ")][0]
    head, _, rest = line.partition(":")
    accepted = [int(x) for x in rest.split()]
    assert int(head.split()[1]) == len(accepted)
    v = np.arange(-2048, 2049)
    h = v.astype(np.float16)
    assert np.array_equal(h.astype(np.int64), v)  # every such integer is a half
    want = v[(h.view(np.uint16) & 0xFF) == 0]
    assert accepted == want.tolist()
    # the scores the GPU tests lean on: 1..16 without 9, 11, 13, 15; -112 and -128 but neither neighbour of -128
    pos = [x for x in accepted if 0 < x <= 16]
    assert pos == [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16]
    assert {-112, -128} <= set(accepted) and not {-127, -129} & set(accepted)


def _ho2(match, mismatch, indel, lcap=256):
    """The scorings that take the 4-bit hand-off on 2-bit reads, restated: the byte profile and the step rule."""
    sma, smm, top = match - 2 * indel, mismatch - 2 * indel, max(match, mismatch)
    prof = indel <= 0 and -128 <= sma <= 127 and -128 <= smm <= 127
    return prof and top >= indel and top - 2 * indel <= 15 and lcap <= 256


def _ho2_scorings(indel):
    out = set()
    for step in sorted({-indel, -indel + 1, 8, 14, 15}):
        top = step + 2 * indel
        for other in (top, top - 1, top - 7, 2 * indel, 2 * indel - 2, 2 * indel - 112, 2 * indel - 128):
            if other <= top:
                out |= {(top, other, indel), (other, top, indel)}
    assert all(_ho2(*s) for s in out)
    return sorted(out)


@pytest.fixture(scope="module")
def small_set():
    return extremal_set(40)


@pytest.mark.parametrize("indel", [0, -1, -3, -7])
def test_steps_stay_in_four_bits(oracle_mod, small_set, indel):
    """Every admitted scoring at this indel (largest steps 15, the clause max(match, mismatch) >= indel at equality,
    both scores negative, the most negative diagonal score -128 - 2 indel): all steps of G lie in
    [0, max(match, mismatch) - 2 indel]."""
    reads, a, b = small_set
    for k, (match, mismatch, ind) in enumerate(_ho2_scorings(indel)):
        sc, en, lo, hi = step_range(reads, a, b, match, mismatch, ind)
        top = max(match, mismatch) - 2 * ind
        assert 0 <= lo and hi <= top, (match, mismatch, ind, lo, hi)
        if k % 8 == 0:  # the numpy statement is the reference recurrence: the oracle agrees
            rs, re_ = oracle_mod.batch_dp(reads, a, b, match, mismatch, ind)
            np.testing.assert_array_equal(sc, rs)
            np.testing.assert_array_equal(en, re_)
            assert_extremes(reads, a, b, rs, re_, match, mismatch, ind)


def test_steps_at_full_length(oracle_mod):
    """The same at 256 bases, the longest reads the 4-bit form takes, at step 15."""
    reads, a, b = extremal_set(256)
    assert len(reads) == 25 and a.shape[0] == 625
    sc, en, lo, hi = step_range(reads, a, b, 13, -1, -1)
    assert (lo, hi) == (0, 15)
    rs, re_ = oracle_mod.batch_dp(reads, a, b, 13, -1, -1)
    np.testing.assert_array_equal(sc, rs)
    np.testing.assert_array_equal(en, re_)
    assert_extremes(reads, a, b, rs, re_, 13, -1, -1)


def test_steps_leave_four_bits_outside_the_rule(small_set):
    """The rule is tight: step_max 16 reaches a step of 16, and max(match, mismatch) < indel a step below 0 (or
    above step_max) on the boundary, where G[i][0] - G[i-1][0] = -indel."""
    reads, a, b = small_set
    assert not _ho2(14, -1, -1) and step_range(reads, a, b, 14, -1, -1)[3] == 16
    assert not _ho2(-4, -5, -3)
    lo, hi = step_range(reads, a, b, -4, -5, -3)[2:]
    assert hi > max(-4, -5) + 6
