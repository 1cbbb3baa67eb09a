"""Shared by tests/test_score_range_cpu.py and tests/test_gpu_score_ranges.py: read sets whose DP values attain the
bounds the scoring-range rules guard (csrc/ovl_score_range.h) -- identical reads (the largest score and the largest
step in every cell), homopolymers (every end ties, or everything mismatches), shifted copies (long suffix-prefix
overlaps that end at the 32-column strip edges), a deletion and a 60-base insertion (long gap runs), periodic reads
against their rotations (many equal paths) -- next to a few random reads and to reads of length 1 and 0, so that the
ordinary pairs and the virtual rows share tiles with the extremes.  Random ACGT reads match a quarter of the time and
never come near those bounds.

Also the closed forms of the rules' edges (``largest_below``) and a numpy statement of the reference recurrence with
the step bounds the narrow cell forms rest on (``step_range``)."""
import random

import numpy as np

# fixed places in the list that extremal_set returns (assert_extremes reads them)
R, R_AGAIN, HOMO_A, HOMO_C = 0, 1, 2, 3


def _rand(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _periodic(unit, n, rot=0):
    s = unit * (n // len(unit) + 2)
    return s[rot:rot + n]


def extremal_set(lmax, alphabet="ACGT"):
    """(reads, a, b): about 25 reads of at most ``lmax`` bases and every ordered pair of them (a-major).  Reads that
    do not fit ``lmax`` (a strip-edge length above it, a shift beyond it) are left out, whatever the count then is;
    from 66 bases on there are 25 reads and 625 pairs: full and partial tiles of 32, 64 and 128 pairs."""
    rng = random.Random(7919 * lmax + len(alphabet))
    x, y = alphabet[0], alphabet[1]
    z = alphabet[2 % len(alphabet)]
    r = _rand(rng, lmax, alphabet)
    reads = [r, r, x * lmax, y * max(lmax - 1, 1)]
    # shifted copies: r's suffix from k is the copy's prefix
    for k in (1, 31, 32, 33):
        if k < lmax:
            reads.append(r[k:] + _rand(rng, k, alphabet))
    # the gap cases: one base deleted; a run of 60 bases (a quarter of the read, where 60 do not fit) inserted
    mid = lmax // 2
    reads.append(r[:mid] + r[mid + 1:])
    run = 60 if lmax >= 120 else max(lmax // 4, 1)
    cut = (lmax - run) // 2
    reads.append((r[:cut] + _rand(rng, run, alphabet) + r[cut:lmax - run])[:lmax])
    # periodic reads and their rotations
    reads += [_periodic(x + y, lmax), _periodic(x + y, lmax, 1),
              _periodic(x + y + z, max(lmax - 1, 1)), _periodic(x + y + z, max(lmax - 1, 1), 1)]
    # ordinary reads
    reads += [_rand(rng, lmax, alphabet), _rand(rng, max(lmax - 1, 1), alphabet),
              _rand(rng, max(lmax * 2 // 3, 1), alphabet), _rand(rng, max(lmax // 3, 1), alphabet)]
    # strip edges: prefixes of r and homopolymers, so they are extremal against reads above
    for k in (31, 32, 33, 64, 65):
        if k < lmax:
            reads.append(r[:k] if k % 2 else x * k)
    reads += [x, ""]
    n = len(reads)
    a = np.repeat(np.arange(n, dtype=np.int32), n)
    b = np.tile(np.arange(n, dtype=np.int32), n)
    return reads, a, b


def assert_extremes(reads, a, b, scores, ends, match, mismatch, indel):
    """The set does what it is for, checked on the oracle's (scores, ends) of a full or banded DP or of the ungapped
    closed form (``indel`` None): the identical pair attains lmax * match, the homopolymer against itself ends at its
    length, the pair of two homopolymers scores 0 at end 0."""
    n = len(reads)
    assert a.shape[0] == n * n and reads[R] == reads[R_AGAIN] and len(set(reads[HOMO_A])) == 1
    lmax = len(reads[R])
    assert lmax == max(len(s) for s in reads)
    at = lambda i, j: i * n + j  # noqa: E731
    gaps_ok = indel is None or indel <= 0
    if match > 0 and match >= mismatch and gaps_ok and lmax * match < 2 ** 31:
        assert (scores[at(R, R_AGAIN)], ends[at(R, R_AGAIN)]) == (lmax * match, lmax)
        assert (scores[at(HOMO_A, HOMO_A)], ends[at(HOMO_A, HOMO_A)]) == (lmax * match, lmax)
    if mismatch < 0 and gaps_ok:
        assert (scores[at(HOMO_A, HOMO_C)], ends[at(HOMO_A, HOMO_C)]) == (0, 0)


def largest_below(bound, factor):
    """The largest integer M with factor * M < bound (the edge of a rule of that shape; M + 1 is outside)."""
    return (bound - 1) // factor


def edge(rule, L, band=8):
    """The largest magnitude M (for ``band_lane_lmax``: the largest lmax at scoring (10, -1, -2)) that the rule
    accepts at read length ``L``, from the inequality itself; ``edge + 1`` is the smallest it rejects.  Written out
    here and never read back from the library: tests/c/score_range_check.cpp finds the same edges by bisecting the
    library's predicates, and tests/test_score_range_cpu.py compares the two."""
    return {
        "wide": lambda: largest_below(2 ** 31, 2 * L + 1),            # (2L + 1) M < 2^31: int32 DP cells
        "lane_int32": lambda: largest_below(2 ** 30, 4 * L + 4),      # (4L + 4) M < 2^30: the lane kernel's G
        "ho1": lambda: largest_below(2 ** 15, 4 * L + 4),             # (4L + 4) M < 2^15: int16 hand-off column
        "band_neg": lambda: largest_below(2 ** 29, 4 * L + 2),        # (4L + 2) M < 2^29: kBandNeg as -inf
        "ungapped_int32": lambda: largest_below(2 ** 31, L),          # amax L < 2^31: the closed form's stores
        "key32": lambda: largest_below(2 ** 15, 2 * L + 32),          # amax (2L + 32) < 2^15: 32-bit folded keys
        "local_key": lambda: largest_below(2 ** 24, L),               # match min(n, m) < 2^24: the best-cell key
        "local_int32": lambda: min(largest_below(2 ** 31, L + 1), 2 ** 30 - 1),  # match min(n, m) + M < 2^31
        "band_lane_lmax": lambda: (largest_below(2 ** 30, 10) - 2 * band - 8) // 6,  # (6L + 2 band + 8) 10 < 2^30
    }[rule]()


def h2_byte(v):
    """A cell step whose f16 encoding has a zero low byte: at most three significant bits, |v| <= 2048."""
    odd = abs(v)
    while odd and odd % 2 == 0:
        odd //= 2
    return odd <= 7 and abs(v) <= 2048


def lane_form(match, mismatch, indel, L, planes=True, prof_on=True, sfx_on=True, h2_on=True):
    """What the lane-per-pair full DP is expected to report for a scoring on reads of at most ``L`` bases, restated
    from the rules: {prof, sfx, ho, h2}.  ``planes``: the read set has a 2-bit bit-plane layout (ACGT, L <= 256);
    the three switches are OVL_LANE_FORM's bits."""
    sma, smm, top = match - 2 * indel, mismatch - 2 * indel, max(match, mismatch)
    M = max(abs(match), abs(mismatch), abs(indel))
    prof = prof_on and planes and indel <= 0 and -128 <= sma <= 127 and -128 <= smm <= 127
    sfx = prof and sfx_on
    ho = 1 if (4 * L + 4) * M < 2 ** 15 else 0
    if sfx and indel <= 0 and top >= indel and top - 2 * indel <= 15 and L <= 256:
        ho = 2
    h2 = ho == 2 and h2_on and h2_byte(sma) and h2_byte(smm)
    return {"prof": int(prof), "sfx": int(sfx), "ho": ho, "h2": int(h2)}


def step_range(reads, a, b, match, mismatch, indel):
    """The reference recurrence (aligners.py:33-48: diag >= up and diag >= left, else up >= left) over every pair at
    once, an anti-diagonal per step, in int64: (score, end, lo, hi) with [lo, hi] the range of all vertical and
    horizontal steps of G = dp - indel * (i + j) inside the pairs' own matrices."""
    n_reads = len(reads)
    lens = np.array([len(s) for s in reads], dtype=np.int64)
    L = int(lens.max())
    codes = np.full((n_reads, L + 1), 255, dtype=np.uint8)
    for k, s in enumerate(reads):
        codes[k, 1:len(s) + 1] = np.frombuffer(s.encode("ascii"), dtype=np.uint8)
    S, T = codes[a].astype(np.int16), codes[b].astype(np.int16)  # S[p, i], T[p, j], 1-based
    n, m = lens[a], lens[b]
    P = a.shape[0]
    ii = np.arange(L + 1, dtype=np.int64)[None, :]
    # diagonal d holds dp[i][d - i] at [p, i]; cells off the (L + 1) x (L + 1) square are never read
    prev2 = np.zeros((P, L + 1), dtype=np.int64)
    prev1 = np.zeros((P, L + 1), dtype=np.int64)
    last = np.zeros((P, L + 1), dtype=np.int64)  # last[p, j] = dp[n][j]
    lo, hi = np.int64(0), np.int64(0)
    seen = False
    for d in range(1, 2 * L + 1):
        jj = d - ii
        cur = np.zeros((P, L + 1), dtype=np.int64)
        inner = (ii >= 1) & (jj >= 1) & (jj <= L)
        i1 = np.nonzero(inner[0])[0]
        if i1.size:
            j1 = d - i1
            sub = np.where(S[:, i1] == T[:, j1], match, mismatch)
            diag = prev2[:, i1 - 1] + sub
            up = prev1[:, i1 - 1] + indel    # dp[i-1][j] lies on diagonal d - 1 at row i - 1
            left = prev1[:, i1] + indel      # dp[i][j-1] lies on diagonal d - 1 at row i
            cur[:, i1] = np.where((diag >= up) & (diag >= left), diag, np.where(up >= left, up, left))
        # steps of G into the cells of this diagonal (boundary cells i = 0 or j = 0 included), inside (n, m)
        jn = np.broadcast_to(jj, (P, L + 1))
        own = (ii <= n[:, None]) & (jn >= 0) & (jn <= m[:, None])
        vert = own & (ii >= 1)
        horz = own & (jn >= 1)
        for mask, before in ((vert, np.concatenate([np.zeros((P, 1), np.int64), prev1[:, :-1]], axis=1)),
                             (horz, prev1)):
            if mask.any():
                st = (cur - before - indel)[mask]
                lo = st.min() if not seen else min(lo, st.min())
                hi = st.max() if not seen else max(hi, st.max())
                seen = True
        rows = np.nonzero((d - n >= 0) & (d - n <= L))[0]
        last[rows, (d - n)[rows]] = cur[rows, n[rows]]
        prev2, prev1 = prev1, cur
    jcol = np.arange(L + 1)[None, :]
    vals = np.where(jcol <= m[:, None], last, np.iinfo(np.int64).min)
    end = vals.argmax(axis=1)  # the first maximum: the reference's strict '>' over ascending j
    score = vals[np.arange(P), end]
    return score.astype(np.int64), end.astype(np.int64), int(lo), int(hi)
