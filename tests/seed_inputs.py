"""Input sets shared by the seed-candidate tests (tests/test_seed_candidates_cpu.py, tests/test_gpu_seed_candidates.py):
name -> (distinct reads, k).  Every set is built from a fixed seed."""
import random


def _random_reads(rng, alphabet, n, lo, hi):
    return ["".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


def _distinct(reads):
    from ovlgraph.candidates import dedup_reads
    return dedup_reads(reads)[0]


def phix_reads(n, seed=0):
    from ovlgraph.reads import read_genome_from_fasta, simulate_reads
    return simulate_reads(read_genome_from_fasta(), 100, n, 0.01, seed=seed)


def input_sets():
    sets = {}
    sets["phix200"] = (_distinct(phix_reads(200)), 12)
    # lengths 3-70 at k = 5: some reads are shorter than k and must appear in no pair
    sets["acgt"] = (_distinct(_random_reads(random.Random(11), "ACGT", 120, 3, 70)), 5)
    # the 4- and 8-bit code paths
    sets["six_letters"] = (_distinct(_random_reads(random.Random(12), "ACGTNX", 120, 3, 70)), 5)
    sets["forty_bytes"] = (_distinct(_random_reads(random.Random(13), "".join(chr(48 + i) for i in range(40)), 120, 3,
                                                   70)), 5)
    # 40 symbols with planted overlaps: k-mers that do find a group on the 8-bit path (k = 3: chance hits are rare)
    rng = random.Random(14)
    text = "".join(rng.choice("".join(chr(48 + i) for i in range(40))) for _ in range(400))
    sets["forty_bytes_overlaps"] = (_distinct([text[p:p + rng.randint(20, 60)] for p in range(0, 380, 7)]), 7)
    # repeats inside a read: the first-offset rule
    rng = random.Random(15)
    sets["repeats"] = (_distinct(["AC" * 20, "A" * 30, "ACGT" * 8] + _random_reads(rng, "ACGT", 60, 3, 40)), 4)
    # a read whose own prefix recurs inside it (a is in its own group: the b == a drop), among reads sharing the prefix
    rng = random.Random(16)
    own = "ACGTTGCA"
    sharing = [own + "GGA" + own + "TTC" + own[:6], own + "CCCCC", "TT" + own + "A", own + "GATTACA"]
    sets["own_prefix"] = (_distinct(sharing + _random_reads(rng, "ACGT", 30, 10, 40) + [own + "TCTCTC"]), 8)
    sets["empty"] = ([], 3)
    sets["single"] = (["ACGTACGTAC"], 3)
    return sets


def gpu_only_sets():
    sets = {}
    # 200 reads sharing one 12-base prefix behind a common read: a group longer than 64
    rng = random.Random(21)
    prefix = "ACGTTGCATGCA"
    common = "".join(rng.choice("ACGT") for _ in range(30)) + prefix + "GGTT"
    sets["long_group"] = (_distinct([common] + [prefix + "".join(rng.choice("ACGT") for _ in range(rng.randint(5, 40)))
                                                for _ in range(200)]), 12)
    # 2,100 reads: the per-read grid is many blocks
    sets["many_reads"] = (_distinct(_random_reads(random.Random(22), "ACGT", 2100, 20, 50)), 6)
    # reads of 2,500 bases among pieces of them: more offsets than a four-wavefront block holds keys for, many
    # 64-offset chunks per read, and k-mers that recur far apart inside a read (a low-complexity stretch)
    rng = random.Random(23)
    long_reads = []
    for _ in range(3):
        body = "".join(rng.choice("ACGT") for _ in range(2200))
        long_reads.append(body[:900] + "ACGTACGTAC" * 30 + body[900:])
    pieces = [r[p:p + rng.randint(30, 80)] for r in long_reads for p in range(5, 2400, 97)]
    sets["long_reads"] = (_distinct(long_reads + pieces), 10)
    return sets
