"""The named small inputs that tests/test_correct_cpu.py and tests/test_gpu_correct.py share: each the smallest shape at
which the k-mer spectrum kernels (csrc/ovl_spectrum.hip) can go wrong.  A case is (name, reads, k, min_count); what a
case is named for is asserted by test_correct_cpu.py::test_the_cases_reach_what_they_are_named_for."""
import ctypes
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name reads k min_count")

STATS = ("kmers", "distinct", "solid", "untrusted", "changed", "ties", "threshold", "windows")
_OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def genome(length, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=length))


def with_errors(read, positions):
    out = list(read)
    for p in positions:
        out[p] = _OTHER[out[p]]
    return "".join(out)


def family(text, copies, *error_sets):
    """`copies` clean copies of `text`, then one copy per error set with those positions substituted."""
    return [text] * copies + [with_errors(text, e) for e in error_sets]


def _phix(n, p, seed=0):
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads
    return simulate_reads(read_genome_from_fasta(), 100, n, p, seed=seed)


def _cases():
    from ovlgraph.reads import random_genome, simulate_reads
    g = genome(400, 11)
    out = [
        Case("no_reads", [], 4, "auto"),
        Case("empty_reads", ["", g[:30], "", g[:30], g[:30], with_errors(g[:30], [9]), ""], 6, 2),
        # reads of k - 1, k and k + 1 bases beside the reads that make the spectrum
        Case("lengths_around_k", family(g[:40], 4, [20]) + [g[3:8], g[3:9], g[3:10], with_errors(g[3:10], [3]),
                                                            with_errors(g[3:9], [0])], 6, 3),
    ]
    # 63, 64, 65 and 129 windows: the wavefront's step edges
    for n_win in (63, 64, 65, 129):
        L = n_win + 12 - 1
        out.append(Case(f"windows_{n_win}", family(g[:L], 4, [0], [L - 1], [L // 2], [5, L - 30]), 12, 3))
    # the 32-bit boundary of the key and its top field
    out.append(Case("k_1", family(g[:50], 3, [7]) + ["TTTT", "N", "A"], 1, "auto"))
    out.append(Case("k_16", family(g[:80], 4, [0], [40], [79], [30, 36]), 16, 3))
    out.append(Case("k_31", family(g[:100], 4, [0], [50], [99], [40, 60]) + family("T" * 40 + g[:30], 3, [35]), 31, 3))
    out.append(Case("error_at_0_and_last", family(g[100:160], 5, [0], [59], [0, 59]), 12, 3))
    out.append(Case("two_errors_closer_than_k", family(g[100:180], 5, [30, 35], [40, 51], [20, 21]), 12, 3))
    # every fifth base wrong: all 150 positions untrusted, 150 * 3 * 12 work items
    out.append(Case("damaged_read", family(g[:150], 5, list(range(2, 150, 5))) +
                    family(g[200:350], 4, list(range(0, 150, 13))), 12, 3))
    # two variants of one locus with equal support, and a third that could become either: it stays
    locus = g[200:240]
    va, vb, vc = (locus[:20] + x + locus[21:] for x in "ACG")
    out.append(Case("tie_stays", [va] * 3 + [vb] * 3 + [vc], 8, 2))
    out.append(Case("n_and_lower_case", family(g[:60], 4, [30]) + [g[:25] + "N" + g[26:60], g[:60].lower(),
                                                                    g[:10] + "acg" + g[13:60], "NNNNNNNNNNNNNN",
                                                                    with_errors(g[:20], [15]) + "N" + g[21:60]], 8, 3))
    # ~0 marks a window without a key; the key of k T's has every bit below 2k set
    out.append(Case("all_t_beside_keyless", ["TTTTTTTTTTNTTTTTTTTT", "TTTTTTTTGTTTTTTTT", "TTTTTTTTTTTT", "NNNNNN",
                                             "TTTTTTTTTTTTTTTT"], 4, 3))
    out.append(Case("min_count_1", family(g[:60], 3, [10], [50]), 10, 1))
    out.append(Case("min_count_above_all", family(g[:60], 3, [10], [50]), 10, 1000))
    out.append(Case("duplicated_reads", [with_errors(g[50:110], [25])] + [g[50:110]] * 4 +
                    [with_errors(g[50:110], [25])], 12, 3))
    out.append(Case("many_short_reads", simulate_reads(random_genome(500, 3), 40, 2100, 0.02, seed=1), 8, "auto"))
    out.append(Case("phix_300", _phix(300, 0.01), 12, "auto"))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def assert_same(got, want, what=""):
    """(reads, stats) of two forms, element for element."""
    assert got[0] == want[0], what
    for key in STATS:
        assert got[1][key] == want[1][key], (what, key, got[1][key], want[1][key])
    assert got[1]["changed_per_read"].dtype == np.int32
    assert np.array_equal(got[1]["changed_per_read"], want[1]["changed_per_read"]), what


def assert_same_spectrum(got, want, what=""):
    assert got[0].dtype == np.uint64 and got[1].dtype == np.int32, what
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what


def quality(noisy, corrected, clean):
    """(errors before, errors after, correct bases changed by mistake, all changes) against the error-free reads."""
    before = after = wrong = changes = 0
    for n, c, t in zip(noisy, corrected, clean):
        assert len(n) == len(c) == len(t)
        for x, y, z in zip(n, c, t):
            before += x != z
            after += y != z
            wrong += x != y and x == z
            changes += x != y
    return before, after, wrong, changes


SMALL_QUALITY = dict(genome_len=300, genome_seed=7, l=40, N=400, p=0.02, seed=0, k=8)


def small_quality_reads():
    from ovlgraph.reads import random_genome, simulate_reads
    q = SMALL_QUALITY
    g = random_genome(q["genome_len"], q["genome_seed"])
    return simulate_reads(g, q["l"], q["N"], q["p"], seed=q["seed"]), simulate_reads(g, q["l"], q["N"], 0.0,
                                                                                     seed=q["seed"])


class RawCorrect:
    """One raw call of ovl_correct_reads / ovl_correct_reads_host with sentinel-filled outputs."""

    def __init__(self, reads):
        from ovlgraph.engine import encode_reads
        self.buf, self.offs = encode_reads(reads)
        self.n = len(reads)
        self.out = np.full(self.buf.shape[0] + 8, 0x5A, dtype=np.uint8)
        self.changed = np.full(self.n + 2, -77, dtype=np.int32)
        self.stats = np.full(8, -77, dtype=np.int64)

    def __call__(self, L, ctx=None, k=4, min_count=0, **null):
        p = lambda name, x: None if null.get(name) else ctypes.c_void_p(x.ctypes.data)  # noqa: E731
        args = (p("seqs", self.buf), p("offsets", self.offs), null.get("n_reads", self.n), k, min_count,
                p("out_seqs", self.out), p("out_changed", self.changed), p("out_stats", self.stats))
        return L.ovl_correct_reads(ctx, *args) if ctx is not None else L.ovl_correct_reads_host(*args)

    def untouched(self):
        return bool((self.out == 0x5A).all() and (self.changed == -77).all() and (self.stats == -77).all())


class RawSpectrum:
    """One raw call of ovl_kmer_spectrum / ovl_kmer_spectrum_host with sentinel-filled outputs."""

    def __init__(self, reads, capacity):
        from ovlgraph.engine import encode_reads
        self.buf, self.offs = encode_reads(reads)
        self.n = len(reads)
        self.capacity = capacity
        self.keys = np.full(capacity + 2, 0x5A5A, dtype=np.uint64)
        self.counts = np.full(capacity + 2, -77, dtype=np.int32)
        self.nd = ctypes.c_int64(-77)

    def __call__(self, L, ctx=None, k=4, **null):
        p = lambda name, x: None if null.get(name) else ctypes.c_void_p(x.ctypes.data)  # noqa: E731
        args = (p("seqs", self.buf), p("offsets", self.offs), null.get("n_reads", self.n), k, p("out_keys", self.keys),
                p("out_counts", self.counts), null.get("capacity", self.capacity),
                None if null.get("out_n_distinct") else ctypes.byref(self.nd))
        return L.ovl_kmer_spectrum(ctx, *args) if ctx is not None else L.ovl_kmer_spectrum_host(*args)

    def arrays_untouched(self):
        return bool((self.keys == 0x5A5A).all() and (self.counts == -77).all())


def bad_correct_calls():
    """(what, keyword arguments of RawCorrect.__call__, the code)."""
    return [("k 0", dict(k=0), -1), ("k 32", dict(k=32), -1), ("n_reads < 0", dict(n_reads=-1), -1),
            ("min_count < 0", dict(min_count=-1), -1), ("seqs NULL", dict(seqs=True), -1),
            ("offsets NULL", dict(offsets=True), -1), ("out_seqs NULL", dict(out_seqs=True), -1),
            ("out_changed NULL", dict(out_changed=True), -1), ("out_stats NULL", dict(out_stats=True), -1)]


def bad_spectrum_calls():
    return [("k 0", dict(k=0), -1), ("k 32", dict(k=32), -1), ("n_reads < 0", dict(n_reads=-1), -1),
            ("seqs NULL", dict(seqs=True), -1), ("offsets NULL", dict(offsets=True), -1),
            ("out_keys NULL", dict(out_keys=True), -1), ("out_counts NULL", dict(out_counts=True), -1),
            ("capacity < 0", dict(capacity=-1), -1), ("out_n_distinct NULL", dict(out_n_distinct=True), -1)]
