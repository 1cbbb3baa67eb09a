"""Graph builders and reference forms shared by the unitig pipeline's tests (test_unitigs_cpu.py,
test_gpu_unitigs.py): the golden hand graphs as DiGraphs, the random graph families as CSR, a dense numpy closure
with the positional sweep, and the reference's literal has_path loop."""
from itertools import combinations

import networkx as nx
import numpy as np


def hand_graph(rec):
    G = nx.DiGraph()
    G.add_nodes_from(f"n{i}" for i in range(rec["n_nodes"]))
    for u, v in rec["edges"]:
        G.add_edge(f"n{u}", f"n{v}")
    return G


def assert_hand_graph_matches(R, rec):
    assert list(R.nodes()) == [f"n{i}" for i in rec["nodes"]]
    assert list(R.edges()) == [(f"n{u}", f"n{v}") for u, v in rec["reduced_edges"]]
    for node, preds in zip(R.nodes(), rec["pred"]):
        assert list(R.pred[node]) == [f"n{p}" for p in preds]


# ------------------------------------------------------------------ graph families
def csr_from_lists(rng, succ):
    """CSR of the successor lists, every list in shuffled order."""
    off = np.zeros(len(succ) + 1, np.int64)
    np.cumsum([len(s) for s in succ], out=off[1:])
    heads = [rng.permutation(np.asarray(s, np.int64)) for s in succ if len(s)]
    return off, (np.concatenate(heads) if heads else np.zeros(0, np.int64)).astype(np.int32)


def random_digraph(rng, n, c):
    """Each ordered pair (self-loops included) is an edge with probability c / n."""
    m = rng.random((n, n)) < c / n
    return csr_from_lists(rng, [np.flatnonzero(row) for row in m])


def random_dag(rng, n, density):
    """A random DAG (edges from lower to higher rank) under a random relabelling."""
    m = np.triu(rng.random((n, n)) < density, k=1)
    label = rng.permutation(n)
    succ = [None] * n
    for u in range(n):
        succ[label[u]] = label[np.flatnonzero(m[u])]
    return csr_from_lists(rng, succ)


def relabelled_chain(rng, n):
    """A chain through all n nodes plus n / 2 forward shortcuts, randomly relabelled: diameter n, and the path
    crosses the closure's pivot blocks in random order."""
    label = rng.permutation(n)
    succ = [set() for _ in range(n)]
    for i in range(n - 1):
        succ[label[i]].add(int(label[i + 1]))
    for _ in range(n // 2):
        i = int(rng.integers(0, max(n - 2, 1)))
        j = int(rng.integers(min(i + 2, n - 1), n))
        if j > i:
            succ[label[i]].add(int(label[j]))
    return csr_from_lists(rng, [sorted(s) for s in succ])


def complete_graph(rng, n):
    return csr_from_lists(rng, [np.arange(n)] * n)


def families(n, seed):
    """(name, off, heads, mix_from) of every family at size n.  mix_from is the smallest of the tests' sizes (1, 2,
    3, 8, 63, ...) from which the family holds both an edge the rule removes and one it keeps, or None where that is
    not asserted.  A removable edge needs a node with two successors of which the earlier reaches the later: the
    digraphs at c >= 1.5 have one from two nodes (self-loops count), the chain from three (its one shortcut), the
    DAG at density 0.5 from eight (28 pairs) and the DAG at 0.05 from 63 (at eight nodes it has 1.4 edges on
    average).  The c = 0.7 digraph may remove nothing, and the complete graph keeps only first successors."""
    rng = np.random.default_rng(seed * 1000 + n)
    out = [(f"digraph_c{c}_n{n}", *random_digraph(rng, n, c), 2 if c >= 1.5 else None) for c in (0.7, 1.5, 3)]
    out += [(f"dag_d{d}_n{n}", *random_dag(rng, n, d), mix_from) for d, mix_from in ((0.05, 63), (0.5, 8))]
    out.append((f"chain_n{n}", *relabelled_chain(rng, n), 3))
    out.append((f"complete_n{n}", *complete_graph(rng, n), None))
    return out


def dense_reference(off, heads):
    """(mask, closure words) from a dense numpy closure (repeated squaring of the boolean adjacency matrix) and the
    positional sweep, the rule as the issue states it."""
    n = off.shape[0] - 1
    words = (n + 63) // 64
    A = np.zeros((n, n), bool)
    tails = np.repeat(np.arange(n), np.diff(off))
    A[tails, heads] = True
    R = A.copy()
    while True:  # R <- R | R.R until it stops growing: paths of at least one edge
        R2 = R | ((R.astype(np.float32) @ R.astype(np.float32)) > 0)
        if np.array_equal(R2, R):
            break
        R = R2
    mask = np.zeros(heads.shape[0], np.uint8)
    for v in range(n):
        acc = np.zeros(n, bool)
        for e in range(int(off[v]), int(off[v + 1])):
            w = int(heads[e])
            mask[e] = acc[w]
            acc |= R[w]
    padded = np.zeros((n, words * 64), np.uint8)
    padded[:, :n] = R
    closure = np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(n, words) if n else \
        np.zeros((0, 0), np.uint64)
    return mask, closure


def literal_loop(off, heads):
    """The reference's loop in networkx: combinations over successors(v) and nx.has_path on the input graph."""
    n = off.shape[0] - 1
    G = nx.DiGraph()
    G.add_nodes_from(range(n))
    for v in range(n):
        G.add_edges_from((v, int(w)) for w in heads[off[v]:off[v + 1]])
    removed = set()
    for v in G.nodes():
        for u, w in combinations(G.successors(v), 2):
            if nx.has_path(G, u, w):
                removed.add((v, w))
    tails = np.repeat(np.arange(n), np.diff(off))
    return np.array([(int(t), int(h)) in removed for t, h in zip(tails, heads)], np.uint8)
