"""The named cases of placed consensus that tests/test_consensus_placed_cpu.py (host form against the loop form) and
tests/test_gpu_consensus_placed.py (device form against the host form) share.  Every case is small enough for the loop
form, ``ovlgraph.consensus.pileup_placed_loop``, to take about a second; ``want(case)`` computes it once per session.

A case is what the rule takes: contigs, reads, the placement (contig, offset), slack, weights, rounds, min_depth,
min_vote_score and the scoring.  ``full`` says that the case's offsets are small enough for a slack that covers every
cell (the comparison with ovl_consensus)."""
import random
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

KEYS = ("counts", "called", "n_changed", "n_other", "aln", "total_changed", "rounds")


@dataclass
class Case:
    name: str
    contigs: List[str]
    reads: List[str]
    contig: List[int]
    offset: List[int]
    slack: int = 8
    weights: Optional[List[int]] = None
    rounds: int = 1
    min_depth: int = 3
    min_vote_score: int = 1
    scoring: Tuple[int, int, int] = (10, -1, -1)
    full: bool = True


def native_args(c: Case, **over):
    """Positional and keyword arguments of ``engine.consensus_placed`` / ``consensus_placed_host``."""
    kw = dict(slack=c.slack, weights=c.weights, rounds=c.rounds, min_depth=c.min_depth,
              min_vote_score=c.min_vote_score, match=c.scoring[0], mismatch=c.scoring[1], indel=c.scoring[2])
    kw.update(over)
    return (c.reads, c.contigs, c.contig, c.offset), kw


def loop_args(c: Case, **over):
    kw = dict(slack=c.slack, weights=c.weights, rounds=c.rounds, min_depth=c.min_depth,
              min_vote_score=c.min_vote_score, match_score=c.scoring[0], mismatch=c.scoring[1], indel=c.scoring[2])
    kw.update(over)
    return (c.contigs, c.reads, c.contig, c.offset), kw


_WANT = {}


def want(c: Case):
    """The loop form's result for the case, computed once and never changed."""
    if c.name not in _WANT:
        from ovlgraph.consensus import pileup_placed_loop
        a, kw = loop_args(c)
        res = pileup_placed_loop(*a, **kw)
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
        _WANT[c.name] = res
    return _WANT[c.name]


def assert_same(got, ref, what):
    for k in KEYS:
        assert np.array_equal(got[k], ref[k]), f"{what}: {k}"


def _seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _mutate(rng, s, rate):
    return "".join(rng.choice([b for b in "ACGT" if b != ch]) if rng.random() < rate else ch for ch in s)


def _sampled(name, seed, m, L, n, slack=8, err=0.05, contig_err=0.03, jitter=0, **kw):
    """n reads of length L sampled from a genome of m bases with substitution errors, placed where they came from
    (plus a jitter of up to ``jitter`` bases) on a contig that is the genome with errors of its own."""
    rng = random.Random(seed)
    genome = _seq(rng, m)
    reads, offset = [], []
    for _ in range(n):
        at = rng.randrange(0, max(1, m - L + 1))
        reads.append(_mutate(rng, genome[at:at + L], err))
        offset.append(at + rng.randint(-jitter, jitter))
    return Case(name, [_mutate(rng, genome, contig_err)], reads, [0] * n, offset, slack, **kw)


def _gapped(name, seed, slack, scoring=(10, -1, -1), m=120, L=40):
    """Reads with a deletion and with an insertion of g bases in their middle, for g = 1, slack and slack + 1 (the
    first two stay inside the band, the last leaves it), each at its true offset, among plain reads."""
    rng = random.Random(seed)
    genome = _seq(rng, m)
    reads, offset = [], []
    for g in sorted({1, max(1, slack), slack + 1}):
        for _ in range(2):
            at = rng.randrange(0, m - L - g)
            half = L // 2
            reads.append(genome[at:at + half] + genome[at + half + g:at + L + g])      # g contig bases missing
            offset.append(at)
            reads.append(genome[at:at + half] + _seq(rng, g) + genome[at + half:at + L - g])  # g bases inserted
            offset.append(at)
    for _ in range(6):
        at = rng.randrange(0, m - L)
        reads.append(_mutate(rng, genome[at:at + L], 0.05))
        offset.append(at)
    return Case(name, [_mutate(rng, genome, 0.03)], reads, [0] * len(reads), offset, slack, scoring=scoring,
                min_depth=2)


def _rounds(name, rounds):
    """A contig with two planted errors 10 bases apart.  Four reads cover only the first and fix it in round 1; four
    reads cover both, score 178 with two mismatches -- below min_vote_score 185 -- and vote only in round 2, with
    one mismatch left (189), which fixes the second.  Round 3 changes nothing."""
    rng = random.Random(77)
    genome = _seq(rng, 60)
    contig = list(genome)
    for e in (25, 35):
        contig[e] = "A" if genome[e] != "A" else "C"
    offs = [8, 10, 12, 14, 18, 19, 20, 21]
    reads = [genome[o:o + 20] for o in offs]
    return Case(name, ["".join(contig)], reads, [0] * 8, offs, slack=2, rounds=rounds, min_vote_score=185)


def _build() -> List[Case]:
    cases: List[Case] = []
    # read lengths around the 32- and 64-row marks, and the shortest
    for L in (1, 2, 31, 32, 33, 63, 64, 65, 100, 129):
        cases.append(_sampled(f"len_{L}", 100 + L, 160, L, 6, slack=8, jitter=2, min_depth=1))
    cases.append(Case("len_mixed", *_mixed_lengths()))
    # read counts around the lane-per-read wavefront boundary
    for n in (1, 63, 64, 65, 130):
        cases.append(_sampled(f"count_{n}", 200 + n, 80, 20, n, slack=4, jitter=1))
    # slack on both sides of each template width, with gaps inside and outside the band
    for s in (0, 1, 4, 5, 8, 9, 15):
        cases.append(_gapped(f"slack_{s}", 300 + s, s))
    # the scorings
    cases.append(_gapped("scoring_2_-3_-5", 401, 4, (2, -3, -5)))
    cases.append(_gapped("scoring_1_-1_-1", 402, 8, (1, -1, -1)))
    cases.append(_gapped("scoring_positive_indel", 403, 3, (3, -2, 1), m=60, L=20))
    cases.append(_gapped("scoring_never_taken", 404, 5, (10, -(2 ** 31), -(2 ** 62)), m=60, L=20))
    # placement: windows clipped at the contig's start and end, and no window at all
    rng = random.Random(500)
    g = _seq(rng, 50)
    L, s = 12, 3
    cases.append(Case("clip_start", [g], [g[0:L], "TTT" + g[0:L - 3], _seq(rng, L - 1) + g[0:1], g[0:L],
                                          g[0:1] + g[0:L - 1]],
                      [0] * 5, [0, -3, -L + 1, -L - s + 1, -1], s, min_depth=1))
    cases.append(Case("clip_end", [g], [g[50 - L:], g[45:] + "ACGTACG", g[49:] + g[:L - 1], g[40:] + "TT", "ACGTACGTACGT"],
                      [0] * 5, [50 - L, 45, 49, 40, 50 + s - 1], s, min_depth=1))
    cases.append(Case("no_window", [g], [g[:L]] * 7, [0] * 7,
                      [-L - s, -L - s - 5, 50 + s, 50 + s + 7, 2 ** 31 - 1, -2 ** 31, 0], s, min_depth=1, full=False))
    # contigs: an empty one, one of one base, a repeated one, an unplaced read, an empty read
    cases.append(Case("contigs_edge", ["", "G", g, g, "T"],
                      [g[:L], "G", "GG", g[5:5 + L], _mutate(rng, g[5:5 + L], 0.2), "", g[:L], "A", g[30:42]],
                      [0, 1, 1, 2, 3, 2, -1, 4, 3], [0, 0, -1, 5, 5, 0, 0, 0, 30], s, min_depth=1))
    # weights 0, 1 and 7
    w = _sampled("weights", 600, 90, 25, 30, slack=4, jitter=1)
    w.weights = [(0, 1, 7)[i % 3] for i in range(30)]
    cases.append(w)
    # 200 copies' worth of votes on the same columns: 20 reads at one place, 10 votes each, two of them outvoted
    g2 = _seq(rng, 40)
    same = [g2[5:35]] * 18 + [_mutate(rng, g2[5:35], 0.3)] * 2
    cases.append(Case("pile_200", [_mutate(rng, g2, 0.1)], same, [0] * 20, [5] * 20, 4, [10] * 20))
    # read content: N and lower-case bytes, in the reads and in the contig
    rd = [g[3:3 + L], g[3:6] + "N" + g[7:3 + L], g[3:8].lower() + g[8:3 + L], "NNNNNNNNNNNN", g[20:26] + "n" + g[27:32]]
    cases.append(Case("other_bytes", [g[:24] + "N" + g[25:30] + "a" + g[31:]], rd, [0] * 5, [3, 3, 3, 10, 20], s,
                      min_depth=1))
    # a read whose best score equals min_vote_score (five matches: 50) and one a point below it (3 + 2 matches
    # around one mismatch: 49)
    five = g[10:15]
    six = g[20:23] + ("A" if g[23] != "A" else "C") + g[24:26]
    cases.append(Case("vote_edge", [g], [five, six], [0, 0], [10, 20], 2, min_depth=1, min_vote_score=50))
    # rounds: the planted input needs two rounds, and a third that changes nothing ends the loop
    for r in (1, 2, 3, 5):
        cases.append(_rounds(f"rounds_{r}", r))
    return cases


def _mixed_lengths():
    rng = random.Random(42)
    genome = _seq(rng, 200)
    reads, offset = [], []
    for L in (1, 2, 31, 32, 33, 63, 64, 65, 100, 129) * 7:  # 70 reads: two wavefronts of uneven lanes
        at = rng.randrange(0, 200 - L + 1)
        reads.append(_mutate(rng, genome[at:at + L], 0.04))
        offset.append(at + rng.randint(-3, 3))
    return [_mutate(rng, genome, 0.03)], reads, [0] * len(reads), offset, 5


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def permuted(c: Case, seed: int = 9):
    """The case with its reads in another order, and the permutation (new position -> old position)."""
    order = list(range(len(c.reads)))
    random.Random(seed).shuffle(order)
    pick = lambda x: [x[i] for i in order]  # noqa: E731
    return Case(c.name + "_permuted", c.contigs, pick(c.reads), pick(c.contig), pick(c.offset), c.slack,
                pick(c.weights) if c.weights is not None else None, c.rounds, c.min_depth, c.min_vote_score,
                c.scoring, c.full), order


def full_slack(c: Case) -> int:
    """A slack under which every cell of every read's table is in the band and the window is the whole contig."""
    m = max([len(x) for x in c.contigs] + [1])
    n = max([len(x) for x in c.reads] + [1])
    return max(n, m) + max([abs(o) for o in c.offset] + [0])


class RawCall:
    """The C arguments of ovl_consensus_placed_host for a case, with guard values in every output."""

    def __init__(self, c: Case):
        import ctypes
        from ovlgraph.engine import encode_reads
        self.R, self.C = len(c.reads), len(c.contigs)
        self.buf, offs = encode_reads(list(c.reads) + list(c.contigs))
        self.r_off = np.ascontiguousarray(offs[: self.R + 1])
        self.c_off = np.ascontiguousarray(offs[self.R:])
        self.total = int(self.c_off[-1] - self.c_off[0])
        self.contig = np.asarray(c.contig, np.int32)
        self.offset = np.asarray(c.offset, np.int32)
        self.weight = np.asarray(c.weights if c.weights is not None else [1] * self.R, np.int32)
        self.counts = np.full((self.total, 6), 77, np.int32)
        self.called = np.full(self.total, 77, np.uint8)
        self.aln = np.full((self.R, 3), 77, np.int32)
        self.i64 = [ctypes.c_int64(77) for _ in range(3)]
        self.done = ctypes.c_int32(77)
        self.scalars = dict(n_reads=self.R, n_contigs=self.C, slack=c.slack, match=c.scoring[0],
                            mismatch=c.scoring[1], indel=c.scoring[2], min_vote_score=c.min_vote_score,
                            min_depth=c.min_depth, rounds=c.rounds)

    def untouched(self) -> bool:
        return bool((self.counts == 77).all() and (self.called == 77).all() and (self.aln == 77).all()
                    and all(v.value == 77 for v in self.i64) and self.done.value == 77)

    def args(self, head: Sequence = (), **over):
        """The argument list; ``over`` replaces arguments by name (a pointer argument by None or another array)."""
        import ctypes
        p = lambda x: None if x is None else ctypes.c_void_p(x.ctypes.data)  # noqa: E731
        v = dict(reads=self.buf, r_off=self.r_off, weight=self.weight, contigs=self.buf, c_off=self.c_off,
                 contig=self.contig, offset=self.offset, counts=self.counts, called=self.called, aln=self.aln,
                 n_changed=self.i64[0], n_other=self.i64[1], total_changed=self.i64[2], rounds_done=self.done)
        v.update(self.scalars)
        v.update(over)
        ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
        return list(head) + [p(v["reads"]), p(v["r_off"]), v["n_reads"], p(v["weight"]), p(v["contigs"]),
                             p(v["c_off"]), v["n_contigs"], p(v["contig"]), p(v["offset"]), v["slack"], v["match"],
                             v["mismatch"], v["indel"], v["min_vote_score"], v["min_depth"], v["rounds"],
                             p(v["counts"]), p(v["called"]), ref(v["n_changed"]), ref(v["n_other"]),
                             ref(v["total_changed"]), ref(v["rounds_done"]), p(v["aln"])]


def bad_calls(c: Case):
    """(name, replaced arguments, expected code) for every argument check of the host form."""
    raw = RawCall(c)
    dec = raw.r_off.copy()
    dec[1] = dec[0] - 1 if raw.R else 0
    cdec = raw.c_off.copy()
    cdec[-1] = cdec[0] - 1
    neg_w = raw.weight.copy()
    neg_w[0] = -1
    hi, lo = raw.contig.copy(), raw.contig.copy()
    hi[0], lo[0] = raw.C, -2
    heavy = np.full(raw.R, 2 ** 31 - 1, np.int32)
    long_r = raw.r_off.copy()
    long_r[1:] += 2 ** 20
    huge_c = raw.c_off.copy()
    huge_c[-1] = huge_c[0] + 2 ** 31
    ARG, INDEX, UNSUPPORTED = -1, -7, -4
    return [
        ("negative n_reads", dict(n_reads=-1), ARG), ("negative n_contigs", dict(n_contigs=-1), ARG),
        ("negative slack", dict(slack=-1), ARG), ("min_vote_score 0", dict(min_vote_score=0), ARG),
        ("min_depth 0", dict(min_depth=0), ARG), ("rounds 0", dict(rounds=0), ARG),
        ("NULL r_off", dict(r_off=None), ARG), ("NULL c_off", dict(c_off=None), ARG),
        ("NULL contig", dict(contig=None), ARG), ("NULL offset", dict(offset=None), ARG),
        ("NULL reads", dict(reads=None), ARG), ("NULL contigs", dict(contigs=None), ARG),
        ("NULL called", dict(called=None), ARG), ("NULL n_changed", dict(n_changed=None), ARG),
        ("NULL n_other", dict(n_other=None), ARG), ("NULL total_changed", dict(total_changed=None), ARG),
        ("NULL rounds_done", dict(rounds_done=None), ARG),
        ("read offsets decrease", dict(r_off=dec), ARG), ("contig offsets decrease", dict(c_off=cdec), ARG),
        ("negative weight", dict(weight=neg_w), ARG),
        ("contig index too high", dict(contig=hi), INDEX), ("contig index below -1", dict(contig=lo), INDEX),
        ("weight * length reaches 2^31", dict(weight=heavy), UNSUPPORTED),
        ("a read of 2^20 bases", dict(r_off=long_r), UNSUPPORTED),
        ("contigs of 2^31 bases", dict(c_off=huge_c), UNSUPPORTED),
        ("match beyond the key", dict(match=1 << 24), UNSUPPORTED),
    ]
