// ovl_unitigs_api.cpp — the unitig pipeline (overlapGraphs.py:332-412: construct_string_graph, transitive_reduction2,
// find_unitigs) from the score columns, without a graph object (the rule: include/ovl.h and ovl_unitigs.hip carry its
// statement).  The host form (ovl_unitigs_host: one thread) and the device calls (ovl_unitigs over uploaded columns,
// ovl_unitigs_candidates over the resident k = 0 candidate list scored into device columns), which share one routine
// from the degree kernel on.  The walk over the node facts and the spelling are sequential by definition: one host
// routine serves every form.
#include "ovl_ctx.h"
#include "ovl_graph_check.h"
#include "ovl_reach_host.h"
#include "ovl_unitigs.h"

// The device blocks of a call.  (Not in the namespace below: tests/c/stage_block_check.cpp carves them without a
// device.)  The input block: the raw list's tables, then the reads with a second copy (n_sx of them: the candidate
// form scores their self pairs; returned), the self columns (n_self entries each) and the score columns.
int32_t* lay_unitigs_in(Carve& b, OvlUnitigArgs& g, int32_t n, int32_t n_raw, size_t n_sx, size_t n_self) {
    const size_t N = (size_t)n, P = N > 0 ? N * (N - 1) : 0;
    g.ids = b.take<int32_t>((size_t)n_raw);
    g.prev = b.take<int32_t>((size_t)n_raw);
    g.first = b.take<int32_t>(N);
    g.self_ix = b.take<int32_t>(N);
    int32_t* sx = b.take<int32_t>(n_sx);
    g.self_score = b.take<int32_t>(n_self);
    g.self_end = b.take<int32_t>(n_self);
    g.score = b.take<int32_t>(P);
    g.end = b.take<int32_t>(P);
    return sx;
}

// The per-node block: degrees, offsets, the marking's order (returned), the node facts
int32_t* lay_unitigs_node(Carve& b, OvlUnitigArgs& g, int32_t n) {
    const size_t N = (size_t)n;
    g.deg = b.take<int64_t>(N + 1);
    g.off = b.take<int64_t>(N + 1);
    int32_t* order = b.take<int32_t>(N);
    g.outdeg = b.take<int32_t>(N);
    g.indeg = b.take<int32_t>(N);
    g.nxt = b.take<int32_t>(N);
    g.nend = b.take<int32_t>(N);
    return order;
}

// The per-edge block: the CSR's columns, the mask, the kept flags and their scan, the kept edges' columns
void lay_unitigs_edge(Carve& b, OvlUnitigArgs& g, int64_t n_edges) {
    const size_t E = (size_t)n_edges;
    g.tail = b.take<int32_t>(E);
    g.head = b.take<int32_t>(E);
    g.weight = b.take<int32_t>(E);
    g.eend = b.take<int32_t>(E);
    g.reduced = b.take<uint8_t>(E);
    g.keep = b.take<int32_t>(E + 1);
    g.pos = b.take<int32_t>(E + 1);
    g.k_tail = b.take<int32_t>(E);
    g.k_head = b.take<int32_t>(E);
    g.k_weight = b.take<int32_t>(E);
    g.k_end = b.take<int32_t>(E);
}

namespace {

constexpr int64_t kUnitigsMax = int64_t(1) << 31;

// what ovl_last_unitigs(NULL) and ovl_unitigs_edges_copy(NULL) report: this thread's last ovl_unitigs_host
struct HostLast {
    UnitigsState::Last last;
    std::vector<int32_t> tail, head, weight, end;
};
thread_local HostLast g_host;

struct Outputs {
    int64_t* path_off;
    int32_t* path_nodes;
    uint8_t* bases;
    int64_t* c_off;
    int32_t* n_contigs;
    int64_t *n_edges, *n_kept;
    int32_t* cycle_node;
};

// The raw list's facts, made by the checks: first[x], prev[j], and the reads with at least two copies.
struct RawFacts {
    std::vector<int32_t> first, prev, self;  // self: the distinct reads with a second copy, ascending
    int64_t total = 0;                       // sum len
    int64_t max_edges = 0;                   // sum over x of min(N - 1 - first[x], n): no row holds more
};

// The checks every form shares.  host_cols: score / end (and the self columns) are host arrays of this call.
template <typename C>
int check_unitigs(const C* c, const uint8_t* seqs, const int64_t* offsets, int32_t n, const int32_t* ids, int32_t n_raw,
                  const int32_t* score, const int32_t* end, const int32_t* self_score, const int32_t* self_end,
                  bool host_cols, const Outputs& o, RawFacts* f) {
    if (!o.n_contigs) return fail(c, OVL_E_ARG, "unitigs: n_contigs is NULL");
    if (n < 0 || n_raw < 0) return fail(c, OVL_E_ARG, "unitigs: negative count");
    if (n > 0 && !offsets) return fail(c, OVL_E_ARG, "unitigs: offsets is NULL");
    if (n_raw > 0 && !ids) return fail(c, OVL_E_ARG, "unitigs: ids is NULL");
    if (n_raw < n) return fail(c, OVL_E_ARG, "unitigs: %d raw reads cannot hold %d distinct reads", n_raw, n);
    for (int32_t r = 0; r < n; ++r)
        if (offsets[r + 1] < offsets[r]) return fail(c, OVL_E_ARG, "unitigs: offsets decrease at read %d", r);
    f->total = n > 0 ? offsets[n] - offsets[0] : 0;
    if (o.bases && f->total > 0 && !seqs) return fail(c, OVL_E_ARG, "unitigs: seqs is NULL");
    if (f->total >= kUnitigsMax)
        return fail(c, OVL_E_UNSUPPORTED, "unitigs: the reads together must stay below 2^31 bases");
    if ((int64_t)n * n >= kUnitigsMax) return fail(c, OVL_E_UNSUPPORTED, "unitigs: n^2 must stay below 2^31");
    if (host_cols && n > 1 && (!score || !end)) return fail(c, OVL_E_ARG, "unitigs: a score column is NULL");
    try {
        f->first.assign((size_t)n, -1);
        f->prev.assign((size_t)n_raw, -1);
        std::vector<int32_t> last((size_t)n, -1);
        std::vector<uint8_t> twice((size_t)n, 0);
        int32_t seen = 0;
        for (int32_t j = 0; j < n_raw; ++j) {
            const int32_t x = ids[j];
            if (x < 0 || x >= n)
                return fail(c, OVL_E_INDEX, "unitigs: ids[%d] = %d outside [0, %d)", j, x, n);
            if (x > seen)
                return fail(c, OVL_E_ARG, "unitigs: ids[%d] = %d, but the distinct reads are numbered by first "
                                          "occurrence and %d is the next", j, x, seen);
            if (x == seen) f->first[(size_t)seen++] = j;
            f->prev[(size_t)j] = last[(size_t)x];
            if (last[(size_t)x] >= 0) twice[(size_t)x] = 1;
            last[(size_t)x] = j;
        }
        if (seen != n) return fail(c, OVL_E_ARG, "unitigs: ids name %d of the %d distinct reads", seen, n);
        f->self.clear();
        f->max_edges = 0;
        for (int32_t x = 0; x < n; ++x) {
            if (twice[(size_t)x]) f->self.push_back(x);
            f->max_edges += std::min<int64_t>(n_raw - 1 - f->first[(size_t)x], n);
        }
    } catch (const std::bad_alloc&) {
        return fail(c, OVL_E_OOM, "unitigs: no memory for the raw list's tables");
    }
    if (host_cols && !f->self.empty() && (!self_score || !self_end))
        return fail(c, OVL_E_ARG, "unitigs: a read has two copies and a self column is NULL");
    return OVL_OK;
}

// find_unitigs over the node facts of the reduced graph: from every node not yet on a path, in node order, the path
// goes on while its last node has one successor and one predecessor and that successor is on no earlier path.
// Returns -1, or the node at which a walk came back to its own path (the paths are then incomplete).  ends[k]: the
// end_position of the edge that brought path_nodes[k] onto its path (0 for a path's first node).
int32_t walk_unitigs(int32_t n, const int32_t* outdeg, const int32_t* indeg, const int32_t* nxt, const int32_t* nend,
                     std::vector<int64_t>& path_off, std::vector<int32_t>& path_nodes, std::vector<int32_t>* ends) {
    std::vector<int32_t> stamp((size_t)n, -1);  // the path a node is on
    path_off.assign(1, 0);
    path_nodes.clear();
    if (ends) ends->clear();
    for (int32_t v = 0; v < n; ++v) {
        if (stamp[(size_t)v] >= 0) continue;
        const int32_t id = (int32_t)path_off.size() - 1;
        stamp[(size_t)v] = id;
        path_nodes.push_back(v);
        if (ends) ends->push_back(0);
        int32_t last = v;
        while (outdeg[last] == 1 && indeg[last] == 1) {
            const int32_t nx = nxt[last];
            if (nx < 0 || nx >= n) break;  // (never: a node with one kept out-edge had its head stored)
            if (stamp[(size_t)nx] == id) return nx;
            if (stamp[(size_t)nx] >= 0) break;
            stamp[(size_t)nx] = id;
            path_nodes.push_back(nx);
            if (ends) ends->push_back(nend[last]);
            last = nx;
        }
        path_off.push_back((int64_t)path_nodes.size());
    }
    return -1;
}

// From the node facts to the caller's outputs: the walk, the spelling, the counts.  OVL_OK, or OVL_UNITIGS_CYCLE with
// only *cycle_node, *n_edges and *n_kept written.
int finish_unitigs(const uint8_t* seqs, const int64_t* offsets, int32_t n, const int32_t* outdeg, const int32_t* indeg,
                   const int32_t* nxt, const int32_t* nend, int64_t n_edges, int64_t n_kept, const Outputs& o,
                   UnitigsState::Last* last) {
    std::vector<int64_t> path_off;
    std::vector<int32_t> path_nodes, ends;
    const int32_t cyc = walk_unitigs(n, outdeg, indeg, nxt, nend, path_off, path_nodes, &ends);
    if (o.n_edges) *o.n_edges = n_edges;
    if (o.n_kept) *o.n_kept = n_kept;
    last->edges = n_edges;
    last->kept = n_kept;
    if (cyc >= 0) {
        if (o.cycle_node) *o.cycle_node = cyc;
        return OVL_UNITIGS_CYCLE;
    }
    const int32_t np = (int32_t)path_off.size() - 1;
    last->paths = np;
    if (o.cycle_node) *o.cycle_node = -1;
    if (o.path_off) std::copy(path_off.begin(), path_off.end(), o.path_off);
    if (o.path_nodes) std::copy(path_nodes.begin(), path_nodes.end(), o.path_nodes);
    int64_t at = 0;
    if (o.c_off) o.c_off[0] = 0;
    for (int32_t p = 0; p < np; ++p) {
        for (int64_t k = path_off[(size_t)p]; k < path_off[(size_t)p + 1]; ++k) {
            const int32_t v = path_nodes[(size_t)k];
            const int64_t len = offsets[v + 1] - offsets[v];
            const int64_t e = std::min<int64_t>(std::max<int32_t>(ends[(size_t)k], 0), len);  // read[e:], as a slice
            if (o.bases && len > e) memcpy(o.bases + at, seqs + offsets[v] + e, (size_t)(len - e));
            at += len - e;
        }
        if (o.c_off) o.c_off[p + 1] = at;
    }
    *o.n_contigs = np;
    return OVL_OK;
}

// The fits check of a call with n nodes, in_bytes of inputs and at most max_edges edges: the per-node block, the
// per-edge block and the scans' scratch at that many edges, the matrix and the pivot rows
int unitigs_fits(Dev* c, size_t in_bytes, int32_t n, int64_t max_edges) {
    Carve nb, eb;
    OvlUnitigArgs g{};
    lay_unitigs_node(nb, g, n);
    lay_unitigs_edge(eb, g, max_edges);
    size_t temp = 0;
    HIPCHK(c, ovl_unitigs_scan_bytes(max_edges + 1, &temp));
    const size_t N = (size_t)std::max(n, 1), words = (N + 63) / 64;
    return check_fits(c, "unitigs", "columns, CSR and matrix",
                      in_bytes + nb.at + eb.at + temp + 8 * N * words + 8 * 64 * words,
                      {&c->ug.in, &c->ug.node, &c->ug.edge, &c->ug.temp, &c->rc.matrix, &c->rc.pivot});
}

// From the degree kernel to the outputs, on c->stream.  g holds the inputs' device addresses; the timer is armed and
// marks 0 and 1 are recorded.  On return the stream is drained, whichever way the routine leaves.
int run_unitigs(Dev* c, OvlUnitigArgs g, const uint8_t* seqs, const int64_t* offsets, const Outputs& o) {
    hipStream_t s = c->stream;
    const int32_t n = g.n;
    const size_t N = (size_t)n;
    UnitigsState& st = c->ug;
    st.kept = -1;
    std::vector<int64_t> h_off(N + 1, 0);
    std::vector<int32_t> order, facts(4 * N, 0);
    int32_t n_kept32 = 0;
    StreamDrain drain(s);
    Carve node_size;
    lay_unitigs_node(node_size, g, n);
    HIPCHK(c, ensure(st.node, node_size.at));
    Carve nb(st.node.p);
    int32_t* d_order = lay_unitigs_node(nb, g, n);
    size_t temp = 0;
    HIPCHK(c, ovl_unitigs_scan_bytes((int64_t)n + 1, &temp));
    HIPCHK(c, ensure(st.temp, temp));
    HIPCHK(c, hipMemsetAsync(g.deg, 0, 8 * (N + 1), s));
    HIPCHK(c, ovl_launch_unitigs_degree(&g, s));
    HIPCHK(c, ovl_launch_unitigs_offsets(&g, st.temp.p, st.temp.bytes, s));
    HIPCHK(c, hipMemcpyAsync(h_off.data(), g.off, 8 * (N + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const int64_t E = h_off[N];
    if (E < 0 || E >= kUnitigsMax || E > (int64_t)n * n)
        return fail(c, OVL_E_INTERNAL, "unitigs: %lld edges from %d nodes", (long long)E, n);
    g.n_edges = E;
    Carve edge_size;
    lay_unitigs_edge(edge_size, g, E);
    HIPCHK(c, ensure(st.edge, edge_size.at));
    HIPCHK(c, ovl_unitigs_scan_bytes(E + 1, &temp));
    HIPCHK(c, ensure(st.temp, temp));
    Carve eb(st.edge.p);
    lay_unitigs_edge(eb, g, E);
    HIPCHK(c, ovl_launch_unitigs_fill(&g, s));
    HIPCHK(c, st.timer.mark(2, s));
    const int32_t words = (int32_t)((N + 63) / 64);
    st.last.words = words;
    if (E > 0) {
        // the marking's order from the downloaded offsets: 8 bytes per node, the one synchronisation above
        reach_mark_order(h_off.data(), n, order);
        if (!order.empty())
            HIPCHK(c, hipMemcpyAsync(d_order, order.data(), 4 * order.size(), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(g.reduced, 0, (size_t)E, s));  // (nodes with one out-edge keep it)
        OvlReachArgs a{};
        a.off = g.off;
        a.head = g.head;
        a.order = d_order;
        a.n_nodes = n;
        a.n_order = (int32_t)order.size();
        a.words = words;
        a.reduced = g.reduced;
        const int rc = reach_launches(c, &a, false, s);
        if (rc != OVL_OK) return rc;
    }
    HIPCHK(c, st.timer.mark(3, s));
    // the node facts start as {outdeg, indeg} = 0 and {nxt, nend} = -1, each pair with its padding in one fill
    HIPCHK(c, hipMemsetAsync(g.outdeg, 0, nb.offset_of(g.nxt) - nb.offset_of(g.outdeg), s));
    HIPCHK(c, hipMemsetAsync(g.nxt, 0xFF, nb.at - nb.offset_of(g.nxt), s));
    HIPCHK(c, ovl_launch_unitigs_facts(&g, s));
    HIPCHK(c, ovl_launch_unitigs_kept(&g, st.temp.p, st.temp.bytes, s));
    HIPCHK(c, st.timer.mark(4, s));
    const int32_t* d_fact[4] = {g.outdeg, g.indeg, g.nxt, g.nend};
    for (int i = 0; i < 4 && n > 0; ++i)
        HIPCHK(c, hipMemcpyAsync(facts.data() + (size_t)i * N, d_fact[i], 4 * N, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&n_kept32, g.pos + E, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    drain.armed = false;
    if (n_kept32 < 0 || n_kept32 > E)
        return fail(c, OVL_E_INTERNAL, "unitigs: %d kept edges of %lld", n_kept32, (long long)E);
    st.kept = n_kept32;
    const int32_t* kept_at[4] = {g.k_tail, g.k_head, g.k_weight, g.k_end};
    std::copy(kept_at, kept_at + 4, st.kept_at);
    for (int i = 0; i < 4; ++i) st.last.ms[i] = st.timer.ms(i, i + 1);
    return finish_unitigs(seqs, offsets, n, facts.data(), facts.data() + N, facts.data() + 2 * N, facts.data() + 3 * N, E,
                          n_kept32, o, &st.last);
}

// the raw list's tables into the placed input block
int upload_raw(Dev* c, const OvlUnitigArgs& g, const int32_t* ids, const RawFacts& f,
               const std::vector<int32_t>& self_ix, hipStream_t s) {
    const size_t n = (size_t)g.n, n_raw = (size_t)g.n_raw;
    if (n_raw > 0) {
        HIPCHK(c, hipMemcpyAsync(writable(g.ids), ids, 4 * n_raw, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(writable(g.prev), f.prev.data(), 4 * n_raw, hipMemcpyHostToDevice, s));
    }
    if (n > 0) {
        HIPCHK(c, hipMemcpyAsync(writable(g.first), f.first.data(), 4 * n, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(writable(g.self_ix), self_ix.data(), 4 * n, hipMemcpyHostToDevice, s));
    }
    return OVL_OK;
}

// an empty read set: no node, no path, no contig
int empty_result(const Outputs& o, UnitigsState::Last* last) {
    *last = {};
    if (o.path_off) o.path_off[0] = 0;
    if (o.c_off) o.c_off[0] = 0;
    if (o.n_edges) *o.n_edges = 0;
    if (o.n_kept) *o.n_kept = 0;
    if (o.cycle_node) *o.cycle_node = -1;
    *o.n_contigs = 0;
    return OVL_OK;
}

int finish(StageCall& call, int rc) {
    const double* ms = call.dev->ug.last.ms;
    call.done(ms[0] + ms[1] + ms[2] + ms[3]);
    return rc;
}

}  // namespace

OVL_API int ovl_unitigs_host(const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, const int32_t* ids,
                             int32_t n_raw, const int32_t* score, const int32_t* end, const int32_t* self_score,
                             const int32_t* self_end, int64_t* path_off, int32_t* path_nodes, uint8_t* bases,
                             int64_t* c_off, int32_t* n_contigs, int64_t* n_edges, int64_t* n_kept,
                             int32_t* cycle_node) {
    const ovl_ctx* none = nullptr;
    const Outputs o{path_off, path_nodes, bases, c_off, n_contigs, n_edges, n_kept, cycle_node};
    RawFacts f;
    const int rc = check_unitigs(none, seqs, offsets, n_reads, ids, n_raw, score, end, self_score, self_end, true, o, &f);
    if (rc != OVL_OK) return rc;
    g_host.tail.clear();
    g_host.head.clear();
    g_host.weight.clear();
    g_host.end.clear();
    if (n_reads == 0) return empty_result(o, &g_host.last);
    g_host.last = {};
    const int32_t n = n_reads;
    const size_t N = (size_t)n;
    const int64_t words = ((int64_t)n + 63) / 64;
    g_host.last.words = (int32_t)words;
    try {
        // 1: the string graph's CSR, rows in node order, a row in ascending raw position
        std::vector<int64_t> off(N + 1, 0);
        std::vector<int32_t> head, weight, eend;
        for (int32_t x = 0; x < n; ++x) {
            const int32_t fx = f.first[(size_t)x];
            for (int32_t j = fx + 1; j < n_raw; ++j) {
                if (f.prev[(size_t)j] > fx) continue;
                const int32_t y = ids[j];
                const int64_t col = y == x ? x : ovl_unitigs_col(x, y, n);
                const int32_t sc = y == x ? self_score[col] : score[col];
                if (sc <= 0) continue;
                head.push_back(y);
                weight.push_back(sc);
                eend.push_back(y == x ? self_end[col] : end[col]);
            }
            off[(size_t)x + 1] = (int64_t)head.size();
        }
        const int64_t E = (int64_t)head.size();
        // 2: the reduction
        std::vector<uint8_t> reduced((size_t)E, 0);
        if (E > 0) {
            std::vector<uint64_t> R;
            if (!reach_alloc_matrix(R, n, words))
                return fail(none, OVL_E_OOM, "no memory for the %d x %d-bit reachability matrix", n, n);
            reach_closure_host(off.data(), head.data(), n, words, R.data());
            reach_mark_host(off.data(), head.data(), n, words, R.data(), reduced.data());
        }
        // 3: the kept edges in CSR order and the node facts
        std::vector<int32_t> facts(4 * N, 0);
        int32_t *outdeg = facts.data(), *indeg = outdeg + N, *nxt = indeg + N, *nend = nxt + N;
        std::fill(nxt, nxt + 2 * N, -1);
        for (int32_t x = 0; x < n; ++x)
            for (int64_t e = off[(size_t)x]; e < off[(size_t)x + 1]; ++e) {
                if (reduced[(size_t)e]) continue;
                g_host.tail.push_back(x);
                g_host.head.push_back(head[(size_t)e]);
                g_host.weight.push_back(weight[(size_t)e]);
                g_host.end.push_back(eend[(size_t)e]);
                ++outdeg[x];
                ++indeg[head[(size_t)e]];
                nxt[x] = head[(size_t)e];
                nend[x] = eend[(size_t)e];
            }
        return finish_unitigs(seqs, offsets, n, outdeg, indeg, nxt, nend, E, (int64_t)g_host.tail.size(), o,
                              &g_host.last);
    } catch (const std::bad_alloc&) {
        return fail(none, OVL_E_OOM, "unitigs: no memory for the graph's tables");
    }
}

OVL_API int ovl_unitigs_walk_host(const int64_t* off, const int32_t* head, int32_t n_nodes, int64_t* path_off,
                                  int32_t* path_nodes, int32_t* n_paths, int32_t* cycle_node) {
    const ovl_ctx* none = nullptr;
    if (!n_paths) return fail(none, OVL_E_ARG, "unitigs walk: n_paths is NULL");
    const uint8_t some = 0;
    const int64_t count = 0;
    const int rc = check_graph(none, off, head, nullptr, false, n_nodes, &some, &count, nullptr, nullptr);
    if (rc != OVL_OK) return rc;
    try {
        const size_t N = (size_t)n_nodes;
        std::vector<int32_t> facts(3 * N, 0);
        int32_t *outdeg = facts.data(), *indeg = outdeg + N, *nxt = indeg + N;
        for (int32_t v = 0; v < n_nodes; ++v)
            for (int64_t e = off[v]; e < off[v + 1]; ++e) {
                ++outdeg[v];
                ++indeg[head[e]];
                nxt[v] = head[e];
            }
        std::vector<int64_t> p_off;
        std::vector<int32_t> p_nodes;
        const int32_t cyc = walk_unitigs(n_nodes, outdeg, indeg, nxt, nullptr, p_off, p_nodes, nullptr);
        if (cyc >= 0) {
            if (cycle_node) *cycle_node = cyc;
            return OVL_UNITIGS_CYCLE;
        }
        if (cycle_node) *cycle_node = -1;
        if (path_off) std::copy(p_off.begin(), p_off.end(), path_off);
        if (path_nodes) std::copy(p_nodes.begin(), p_nodes.end(), path_nodes);
        *n_paths = (int32_t)p_off.size() - 1;
    } catch (const std::bad_alloc&) {
        return fail(none, OVL_E_OOM, "unitigs walk: no memory for the node facts");
    }
    return OVL_OK;
}

OVL_API int ovl_unitigs(ovl_ctx* ctx, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, const int32_t* ids,
                        int32_t n_raw, const int32_t* score, const int32_t* end, const int32_t* self_score,
                        const int32_t* self_end, int64_t* path_off, int32_t* path_nodes, uint8_t* bases, int64_t* c_off,
                        int32_t* n_contigs, int64_t* n_edges, int64_t* n_kept, int32_t* cycle_node) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    StageCall call(ctx);
    Dev* c = call.dev;
    const Outputs o{path_off, path_nodes, bases, c_off, n_contigs, n_edges, n_kept, cycle_node};
    RawFacts f;
    int rc = check_unitigs(c, seqs, offsets, n_reads, ids, n_raw, score, end, self_score, self_end, true, o, &f);
    if (rc != OVL_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N = (size_t)n_reads, P = N > 0 ? N * (N - 1) : 0;
    const bool self = !f.self.empty();
    OvlUnitigArgs g{};
    g.n = n_reads;
    g.n_raw = n_raw;
    Carve size;
    lay_unitigs_in(size, g, n_reads, n_raw, 0, self ? N : 0);
    if ((rc = unitigs_fits(c, size.at, n_reads, f.max_edges)) != OVL_OK) return rc;
    call.begin();
    c->ug.last = {};
    c->ug.kept = -1;
    if (n_reads == 0) return empty_result(o, &c->ug.last);
    std::vector<int32_t> self_ix(N, -1);
    for (int32_t x : f.self) self_ix[(size_t)x] = x;
    hipStream_t s = c->stream;
    HIPCHK(c, ensure(c->ug.in, size.at));
    HIPCHK(c, c->ug.timer.arm(ctx->timing));
    Carve in(c->ug.in.p);
    lay_unitigs_in(in, g, n_reads, n_raw, 0, self ? N : 0);
    StreamDrain drain(s);
    if ((rc = upload_raw(c, g, ids, f, self_ix, s)) != OVL_OK) return rc;
    if (self) {
        HIPCHK(c, hipMemcpyAsync(writable(g.self_score), self_score, 4 * N, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(writable(g.self_end), self_end, 4 * N, hipMemcpyHostToDevice, s));
    }
    if (P > 0) {
        HIPCHK(c, hipMemcpyAsync(writable(g.score), score, 4 * P, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(writable(g.end), end, 4 * P, hipMemcpyHostToDevice, s));
    }
    HIPCHK(c, c->ug.timer.mark(0, s));  // after the uploads; nothing is scored here
    HIPCHK(c, c->ug.timer.mark(1, s));
    rc = run_unitigs(c, g, seqs, offsets, o);
    drain.armed = false;     // (run_unitigs drains the stream whichever way it leaves)
    c->ug.last.ms[0] = 0.0;  // (two marks with nothing between them)
    return finish(call, rc);
}

OVL_API int ovl_unitigs_candidates(ovl_ctx* ctx, const uint8_t* seqs, const int32_t* ids, int32_t n_raw, int32_t match,
                                   int32_t mismatch, int64_t indel, int32_t band, int64_t* path_off,
                                   int32_t* path_nodes, uint8_t* bases, int64_t* c_off, int32_t* n_contigs,
                                   int64_t* n_edges, int64_t* n_kept, int32_t* cycle_node) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    StageCall call(ctx);
    Dev* c = call.dev;
    if (c->n_reads < 0 || !ctx->res_valid) return fail(c, OVL_E_STATE, "no resident reads: call ovl_set_reads first");
    if (c->cand_n < 0) return fail(c, OVL_E_STATE, "no candidate list: call ovl_candidates(k = 0) first");
    const int32_t n_reads = c->n_reads;
    const size_t N = (size_t)n_reads, P = N > 0 ? N * (N - 1) : 0;
    if (c->cand_seed || c->cand_n != (int64_t)P)
        return fail(c, OVL_E_ARG, "unitigs: the candidate list holds %lld pairs, not the %lld of ovl_candidates(k = 0) "
                                  "over %d reads", (long long)c->cand_n, (long long)P, n_reads);
    const Outputs o{path_off, path_nodes, bases, c_off, n_contigs, n_edges, n_kept, cycle_node};
    RawFacts f;
    const int64_t* offsets = ctx->res_off.data();
    int rc = check_unitigs(c, seqs, offsets, n_reads, ids, n_raw, nullptr, nullptr, nullptr, nullptr, false, o, &f);
    if (rc != OVL_OK) return rc;
    Plan p;
    if ((rc = check_scoring_args(ctx, match, mismatch, indel, band, &p)) != OVL_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t M = f.self.size();
    OvlUnitigArgs g{};
    g.n = n_reads;
    g.n_raw = n_raw;
    Carve size;
    lay_unitigs_in(size, g, n_reads, n_raw, M, M);
    if ((rc = unitigs_fits(c, size.at, n_reads, f.max_edges)) != OVL_OK) return rc;
    call.begin();
    c->ug.last = {};
    c->ug.kept = -1;
    if (n_reads == 0) return empty_result(o, &c->ug.last);
    std::vector<int32_t> self_ix(N, -1);
    for (size_t k = 0; k < M; ++k) self_ix[(size_t)f.self[k]] = (int32_t)k;
    hipStream_t s = c->stream;
    HIPCHK(c, ensure(c->ug.in, size.at));
    HIPCHK(c, c->ug.timer.arm(ctx->timing));
    Carve in(c->ug.in.p);
    int32_t* d_sx = lay_unitigs_in(in, g, n_reads, n_raw, M, M);
    StreamDrain drain(s);
    if ((rc = upload_raw(c, g, ids, f, self_ix, s)) != OVL_OK) return rc;
    if (M > 0) HIPCHK(c, hipMemcpyAsync(d_sx, f.self.data(), 4 * M, hipMemcpyHostToDevice, s));
    HIPCHK(c, c->ug.timer.mark(0, s));
    LaunchIo io;
    if (P > 0) {
        rc = launch_score(c, p, {as<int32_t>(c->cand_a), as<int32_t>(c->cand_b), (int64_t)P}, {match, mismatch, indel},
                          {writable(g.score), writable(g.end)}, io, s);
        if (rc != OVL_OK) return rc;
    }
    if (M > 0) {  // the self pairs of the reads with a second copy, by the same scorer
        rc = launch_score(c, p, {d_sx, d_sx, (int64_t)M}, {match, mismatch, indel},
                          {writable(g.self_score), writable(g.self_end)}, io, s);
        if (rc != OVL_OK) return rc;
    }
    HIPCHK(c, c->ug.timer.mark(1, s));
    rc = run_unitigs(c, g, seqs, offsets, o);
    drain.armed = false;  // (run_unitigs drains the stream whichever way it leaves)
    return finish(call, rc);
}

OVL_API int ovl_unitigs_edges_copy(const ovl_ctx* ctx, int32_t* tail, int32_t* head, int32_t* weight, int32_t* end) {
    int32_t* out[4] = {tail, head, weight, end};
    if (!ctx) {
        const std::vector<int32_t>* col[4] = {&g_host.tail, &g_host.head, &g_host.weight, &g_host.end};
        for (int i = 0; i < 4; ++i)
            if (out[i]) std::copy(col[i]->begin(), col[i]->end(), out[i]);
        return OVL_OK;
    }
    Dev* c = ctx->devs[0];
    if (c->ug.kept < 0) return fail(c, OVL_E_STATE, "no kept edges: call ovl_unitigs or ovl_unitigs_candidates first");
    if (c->ug.kept == 0) return OVL_OK;
    DeviceGuard guard;
    HIPCHK(c, hipSetDevice(c->device));
    StreamDrain drain(c->stream);
    for (int i = 0; i < 4; ++i)
        if (out[i])
            HIPCHK(c, hipMemcpyAsync(out[i], c->ug.kept_at[i], 4 * (size_t)c->ug.kept, hipMemcpyDeviceToHost,
                                     c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    drain.armed = false;
    return OVL_OK;
}

OVL_API int ovl_last_unitigs(const ovl_ctx* ctx, int64_t* edges, int64_t* kept, int32_t* paths, int32_t* words_per_row) {
    const UnitigsState::Last& st = ctx ? ctx->devs[0]->ug.last : g_host.last;
    if (edges) *edges = st.edges;
    if (kept) *kept = st.kept;
    if (paths) *paths = st.paths;
    if (words_per_row) *words_per_row = st.words;
    return OVL_OK;
}

OVL_API int ovl_last_unitigs_timing(const ovl_ctx* ctx, double* score_ms, double* build_ms, double* reduce_ms,
                                    double* facts_ms) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    const double* ms = ctx->devs[0]->ug.last.ms;
    if (score_ms) *score_ms = ms[0];
    if (build_ms) *build_ms = ms[1];
    if (reduce_ms) *reduce_ms = ms[2];
    if (facts_ms) *facts_ms = ms[3];
    return OVL_OK;
}
