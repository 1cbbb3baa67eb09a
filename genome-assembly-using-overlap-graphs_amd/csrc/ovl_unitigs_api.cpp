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

inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

// A block of device tables laid out one after the other, each 256-byte aligned.
struct Block {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t o = at;
        at = al256(at + bytes);
        return o;
    }
};

// From the first copy enqueued to the return: whichever way a device call leaves, the stream is drained before the
// host memory its copies read or write can go away.  Declared after the vectors, so it goes first.
struct StreamDrain {
    hipStream_t s;
    explicit StreamDrain(hipStream_t stream) : s(stream) {}
    ~StreamDrain() { (void)hipStreamSynchronize(s); }
};

// Device bytes of a call with n nodes, `cols` bytes of inputs and at most max_edges edges: the per-node block, the
// per-edge block (41 bytes per edge), the matrix and the pivot rows
size_t device_bytes(int32_t n, size_t cols, int64_t max_edges) {
    const size_t N = (size_t)std::max(n, 1), words = (N + 63) / 64;
    return cols + 44 * N + 4096 + 41 * (size_t)max_edges + 8 * N * words + 8 * 64 * words;
}

int check_fits(Dev* c, size_t need) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    const size_t held = c->ug.in.bytes + c->ug.node.bytes + c->ug.edge.bytes + c->ug.temp.bytes + c->rc.matrix.bytes +
                        c->rc.pivot.bytes;
    if (need > free_b + held)
        return fail(c, OVL_E_UNSUPPORTED, "unitigs: %zu bytes of columns, CSR and matrix do not fit the device (%zu free)",
                    need, free_b + held);
    return OVL_OK;
}

// From the degree kernel to the outputs, on c->stream.  g holds the inputs' device addresses; the timer is armed and
// marks 0 and 1 are recorded.  On return the stream is synchronised.
int run_unitigs(Dev* c, OvlUnitigArgs g, const uint8_t* seqs, const int64_t* offsets, const Outputs& o) {
    hipStream_t s = c->stream;
    const int32_t n = g.n;
    const size_t N = (size_t)n;
    UnitigsState& st = c->ug;
    st.kept = -1;
    Block nb;
    const size_t o_deg = nb.take(8 * (N + 1)), o_off = nb.take(8 * (N + 1)), o_order = nb.take(4 * N),
                 o_outdeg = nb.take(4 * N), o_indeg = nb.take(4 * N), o_nxt = nb.take(4 * N), o_nend = nb.take(4 * N);
    HIPCHK(c, ensure(st.node, nb.at));
    char* node = as<char>(st.node);
    g.deg = reinterpret_cast<int64_t*>(node + o_deg);
    g.off = reinterpret_cast<int64_t*>(node + o_off);
    g.outdeg = reinterpret_cast<int32_t*>(node + o_outdeg);
    g.indeg = reinterpret_cast<int32_t*>(node + o_indeg);
    g.nxt = reinterpret_cast<int32_t*>(node + o_nxt);
    g.nend = reinterpret_cast<int32_t*>(node + o_nend);
    size_t temp = 0;
    HIPCHK(c, ovl_unitigs_scan_bytes((int64_t)n + 1, &temp));
    HIPCHK(c, ensure(st.temp, temp));
    std::vector<int64_t> h_off(N + 1, 0);
    std::vector<int32_t> order, facts(4 * N, 0);
    int32_t n_kept32 = 0;
    StreamDrain drain(s);
    HIPCHK(c, hipMemsetAsync(g.deg, 0, 8 * (N + 1), s));
    HIPCHK(c, ovl_launch_unitigs_degree(&g, s));
    HIPCHK(c, ovl_launch_unitigs_offsets(&g, st.temp.p, st.temp.bytes, s));
    HIPCHK(c, hipMemcpyAsync(h_off.data(), g.off, 8 * (N + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const int64_t E = h_off[N];
    if (E < 0 || E >= kUnitigsMax || E > (int64_t)n * n)
        return fail(c, OVL_E_INTERNAL, "unitigs: %lld edges from %d nodes", (long long)E, n);
    g.n_edges = E;
    const size_t Ez = (size_t)E;
    Block eb;
    const size_t o_tail = eb.take(4 * Ez), o_head = eb.take(4 * Ez), o_w = eb.take(4 * Ez), o_e = eb.take(4 * Ez),
                 o_red = eb.take(Ez), o_keep = eb.take(4 * (Ez + 1)), o_pos = eb.take(4 * (Ez + 1)),
                 o_kt = eb.take(4 * Ez), o_kh = eb.take(4 * Ez), o_kw = eb.take(4 * Ez), o_ke = eb.take(4 * Ez);
    HIPCHK(c, ensure(st.edge, eb.at));
    HIPCHK(c, ovl_unitigs_scan_bytes(E + 1, &temp));
    HIPCHK(c, ensure(st.temp, temp));
    char* edge = as<char>(st.edge);
    g.tail = reinterpret_cast<int32_t*>(edge + o_tail);
    g.head = reinterpret_cast<int32_t*>(edge + o_head);
    g.weight = reinterpret_cast<int32_t*>(edge + o_w);
    g.eend = reinterpret_cast<int32_t*>(edge + o_e);
    g.reduced = reinterpret_cast<uint8_t*>(edge + o_red);
    g.keep = reinterpret_cast<int32_t*>(edge + o_keep);
    g.pos = reinterpret_cast<int32_t*>(edge + o_pos);
    g.k_tail = reinterpret_cast<int32_t*>(edge + o_kt);
    g.k_head = reinterpret_cast<int32_t*>(edge + o_kh);
    g.k_weight = reinterpret_cast<int32_t*>(edge + o_kw);
    g.k_end = reinterpret_cast<int32_t*>(edge + o_ke);
    HIPCHK(c, ovl_launch_unitigs_fill(&g, s));
    HIPCHK(c, st.timer.mark(2, s));
    const int32_t words = (int32_t)((N + 63) / 64);
    st.last.words = words;
    if (E > 0) {
        // the marking's order from the downloaded offsets: 8 bytes per node, the one synchronisation above
        reach_mark_order(h_off.data(), n, order);
        if (!order.empty())
            HIPCHK(c, hipMemcpyAsync(node + o_order, order.data(), 4 * order.size(), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(g.reduced, 0, Ez, s));  // (nodes with one out-edge keep it)
        OvlReachArgs a{};
        a.off = g.off;
        a.head = g.head;
        a.order = reinterpret_cast<const int32_t*>(node + o_order);
        a.n_nodes = n;
        a.n_order = (int32_t)order.size();
        a.words = words;
        a.reduced = g.reduced;
        const int rc = reach_launches(c, &a, false, s);
        if (rc != OVL_OK) return rc;
    }
    HIPCHK(c, st.timer.mark(3, s));
    HIPCHK(c, hipMemsetAsync(g.outdeg, 0, o_nxt - o_outdeg, s));
    HIPCHK(c, hipMemsetAsync(g.nxt, 0xFF, nb.at - o_nxt, s));
    HIPCHK(c, ovl_launch_unitigs_facts(&g, s));
    HIPCHK(c, ovl_launch_unitigs_kept(&g, st.temp.p, st.temp.bytes, s));
    HIPCHK(c, st.timer.mark(4, s));
    const int32_t* d_fact[4] = {g.outdeg, g.indeg, g.nxt, g.nend};
    for (int i = 0; i < 4 && n > 0; ++i)
        HIPCHK(c, hipMemcpyAsync(facts.data() + (size_t)i * N, d_fact[i], 4 * N, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&n_kept32, g.pos + E, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (n_kept32 < 0 || n_kept32 > E)
        return fail(c, OVL_E_INTERNAL, "unitigs: %d kept edges of %lld", n_kept32, (long long)E);
    st.kept = n_kept32;
    st.kept_at[0] = o_kt;
    st.kept_at[1] = o_kh;
    st.kept_at[2] = o_kw;
    st.kept_at[3] = o_ke;
    for (int i = 0; i < 4; ++i) st.last.ms[i] = st.timer.ms(i, i + 1);
    return finish_unitigs(seqs, offsets, n, facts.data(), facts.data() + N, facts.data() + 2 * N, facts.data() + 3 * N, E,
                          n_kept32, o, &st.last);
}

// the raw list's tables at the head of the input block: ids, prev, first, self_ix
struct RawPlan {
    size_t ids, prev, first, self_ix;
    RawPlan(Block& b, int32_t n, int32_t n_raw) {
        ids = b.take(4 * (size_t)n_raw);
        prev = b.take(4 * (size_t)n_raw);
        first = b.take(4 * (size_t)n);
        self_ix = b.take(4 * (size_t)n);
    }
};

int upload_raw(Dev* c, char* in, const RawPlan& r, const int32_t* ids, int32_t n_raw, const RawFacts& f,
               const std::vector<int32_t>& self_ix, OvlUnitigArgs* g, hipStream_t s) {
    const size_t n = f.first.size();
    if (n_raw > 0) {
        HIPCHK(c, hipMemcpyAsync(in + r.ids, ids, 4 * (size_t)n_raw, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(in + r.prev, f.prev.data(), 4 * (size_t)n_raw, hipMemcpyHostToDevice, s));
    }
    if (n > 0) {
        HIPCHK(c, hipMemcpyAsync(in + r.first, f.first.data(), 4 * n, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(in + r.self_ix, self_ix.data(), 4 * n, hipMemcpyHostToDevice, s));
    }
    g->n = (int32_t)n;
    g->n_raw = n_raw;
    g->ids = reinterpret_cast<const int32_t*>(in + r.ids);
    g->prev = reinterpret_cast<const int32_t*>(in + r.prev);
    g->first = reinterpret_cast<const int32_t*>(in + r.first);
    g->self_ix = reinterpret_cast<const int32_t*>(in + r.self_ix);
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
    Block b;
    const RawPlan raw(b, n_reads, n_raw);
    const size_t o_ss = b.take(self ? 4 * N : 0), o_se = b.take(self ? 4 * N : 0), o_s = b.take(4 * P),
                 o_e = b.take(4 * P);
    if ((rc = check_fits(c, device_bytes(n_reads, b.at, f.max_edges))) != OVL_OK) return rc;
    call.begin();
    c->ug.last = {};
    c->ug.kept = -1;
    if (n_reads == 0) return empty_result(o, &c->ug.last);
    std::vector<int32_t> self_ix(N, -1);
    for (int32_t x : f.self) self_ix[(size_t)x] = x;
    hipStream_t s = c->stream;
    HIPCHK(c, ensure(c->ug.in, b.at));
    HIPCHK(c, c->ug.timer.arm(ctx->timing));
    char* in = as<char>(c->ug.in);
    OvlUnitigArgs g{};
    StreamDrain drain(s);
    if ((rc = upload_raw(c, in, raw, ids, n_raw, f, self_ix, &g, s)) != OVL_OK) return rc;
    if (self) {
        HIPCHK(c, hipMemcpyAsync(in + o_ss, self_score, 4 * N, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(in + o_se, self_end, 4 * N, hipMemcpyHostToDevice, s));
    }
    if (P > 0) {
        HIPCHK(c, hipMemcpyAsync(in + o_s, score, 4 * P, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(in + o_e, end, 4 * P, hipMemcpyHostToDevice, s));
    }
    HIPCHK(c, c->ug.timer.mark(0, s));  // after the uploads; nothing is scored here
    HIPCHK(c, c->ug.timer.mark(1, s));
    g.self_score = reinterpret_cast<const int32_t*>(in + o_ss);
    g.self_end = reinterpret_cast<const int32_t*>(in + o_se);
    g.score = reinterpret_cast<const int32_t*>(in + o_s);
    g.end = reinterpret_cast<const int32_t*>(in + o_e);
    rc = run_unitigs(c, g, seqs, offsets, o);
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
    Block b;
    const RawPlan raw(b, n_reads, n_raw);
    const size_t o_sx = b.take(4 * M), o_ss = b.take(4 * M), o_se = b.take(4 * M), o_s = b.take(4 * P),
                 o_e = b.take(4 * P);
    if ((rc = check_fits(c, device_bytes(n_reads, b.at, f.max_edges))) != OVL_OK) return rc;
    call.begin();
    c->ug.last = {};
    c->ug.kept = -1;
    if (n_reads == 0) return empty_result(o, &c->ug.last);
    std::vector<int32_t> self_ix(N, -1);
    for (size_t k = 0; k < M; ++k) self_ix[(size_t)f.self[k]] = (int32_t)k;
    hipStream_t s = c->stream;
    HIPCHK(c, ensure(c->ug.in, b.at));
    HIPCHK(c, c->ug.timer.arm(ctx->timing));
    char* in = as<char>(c->ug.in);
    OvlUnitigArgs g{};
    StreamDrain drain(s);
    if ((rc = upload_raw(c, in, raw, ids, n_raw, f, self_ix, &g, s)) != OVL_OK) return rc;
    if (M > 0) HIPCHK(c, hipMemcpyAsync(in + o_sx, f.self.data(), 4 * M, hipMemcpyHostToDevice, s));
    HIPCHK(c, c->ug.timer.mark(0, s));
    int32_t* d_sx = reinterpret_cast<int32_t*>(in + o_sx);
    if (P > 0) {
        rc = launch_score(c, p, as<int32_t>(c->cand_a), as<int32_t>(c->cand_b), (int64_t)P, match, mismatch, indel,
                          reinterpret_cast<int32_t*>(in + o_s), reinterpret_cast<int32_t*>(in + o_e), s);
        if (rc != OVL_OK) return rc;
    }
    if (M > 0) {  // the self pairs of the reads with a second copy, by the same scorer
        rc = launch_score(c, p, d_sx, d_sx, (int64_t)M, match, mismatch, indel, reinterpret_cast<int32_t*>(in + o_ss),
                          reinterpret_cast<int32_t*>(in + o_se), s);
        if (rc != OVL_OK) return rc;
    }
    HIPCHK(c, c->ug.timer.mark(1, s));
    g.self_score = reinterpret_cast<const int32_t*>(in + o_ss);
    g.self_end = reinterpret_cast<const int32_t*>(in + o_se);
    g.score = reinterpret_cast<const int32_t*>(in + o_s);
    g.end = reinterpret_cast<const int32_t*>(in + o_e);
    return finish(call, run_unitigs(c, g, seqs, offsets, o));
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
    for (int i = 0; i < 4; ++i)
        if (out[i])
            HIPCHK(c, hipMemcpyAsync(out[i], as<char>(c->ug.edge) + c->ug.kept_at[i], 4 * (size_t)c->ug.kept,
                                     hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
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
