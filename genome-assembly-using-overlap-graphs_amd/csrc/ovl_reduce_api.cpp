// ovl_reduce_api.cpp — transitive reduction of an overlap graph (overlapGraphs.py:235-303): the argument checks,
// the host form (ovl_transitive_reduce_host) and the device call (ovl_transitive_reduce, ovl_reduce.hip).
#include "ovl_ctx.h"
#include "ovl_graph_check.h"

namespace {

constexpr int32_t kReduceWindow = 20224;   // out-row entries in LDS per pass (79 KiB: two workgroups per CU)
constexpr int32_t kReduceBlocksPerCu = 2;

// A mark array per source node, reset by re-walking the node's successors.
void reduce_host(const int64_t* off, const int32_t* head, const int64_t* weight, int32_t n_nodes, uint8_t* reduced,
                 int64_t* n_reduced) {
    std::vector<int64_t> row((size_t)n_nodes, 0);
    std::vector<uint8_t> mark((size_t)n_nodes, 0);  // 0 no edge (v, x), 1 edge, 2 eliminated
    int64_t count = 0;
    for (int32_t v = 0; v < n_nodes; ++v) {
        const int64_t e0 = off[v], e1 = off[v + 1];
        for (int64_t e = e0; e < e1; ++e) {
            row[(size_t)head[e]] = weight[e];
            mark[(size_t)head[e]] = 1;
        }
        for (int64_t e = e0; e < e1; ++e) {
            const int32_t w = head[e];
            const int64_t vw = weight[e];
            for (int64_t f = off[w]; f < off[w + 1]; ++f) {
                const size_t x = (size_t)head[f];
                if (mark[x] == 1 && vw + weight[f] >= row[x]) mark[x] = 2;
            }
        }
        for (int64_t e = e0; e < e1; ++e) {
            const size_t x = (size_t)head[e];
            reduced[e] = mark[x] == 2;
            count += mark[x] == 2;
            mark[x] = 0;
        }
    }
    *n_reduced = count;
}

}  // namespace

OVL_API int ovl_transitive_reduce_host(const int64_t* off, const int32_t* head, const int64_t* weight,
                                       int32_t n_nodes, uint8_t* reduced, int64_t* n_reduced) {
    const int rc = check_graph((const ovl_ctx*)nullptr, off, head, weight, true, n_nodes, reduced, n_reduced,
                               nullptr, nullptr);
    if (rc != OVL_OK) return rc;
    reduce_host(off, head, weight, n_nodes, reduced, n_reduced);
    return OVL_OK;
}

OVL_API int ovl_transitive_reduce(ovl_ctx* ctx, const int64_t* off, const int32_t* head, const int64_t* weight,
                                  int32_t n_nodes, uint8_t* reduced, int64_t* n_reduced) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    StageCall call(ctx);
    Dev* c = call.dev;
    std::vector<int64_t> work;
    int64_t steps = 0;
    const int rc = check_graph(c, off, head, weight, true, n_nodes, reduced, n_reduced, &work, &steps);
    if (rc != OVL_OK) return rc;
    const int64_t n_edges = n_nodes > 0 ? off[n_nodes] : 0;
    const int32_t window = std::min(kReduceWindow, c->k.tr_window > 0 ? c->k.tr_window : kReduceWindow);
    call.begin();
    c->tr.last = {window, (int32_t)(((int64_t)n_nodes + window - 1) / window), steps};
    *n_reduced = 0;
    if (n_edges == 0) return OVL_OK;
    // nodes with out-edges, heaviest first (ties in node order)
    std::vector<int32_t> order;
    order.reserve((size_t)n_nodes);
    for (int32_t v = 0; v < n_nodes; ++v)
        if (off[v + 1] > off[v]) order.push_back(v);
    std::stable_sort(order.begin(), order.end(),
                     [&](int32_t x, int32_t y) { return work[(size_t)x] > work[(size_t)y]; });
    std::vector<int2> edge((size_t)n_edges);
    for (int64_t e = 0; e < n_edges; ++e) edge[(size_t)e] = make_int2(head[e], (int32_t)weight[e]);
    // lanes per successor list: the power of two in [8, 64] that covers the mean list walked in one trip
    const int64_t mean = steps / n_edges;
    int32_t group = 8;
    while (group < 64 && group * kReduceLoads < mean) group *= 2;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    StreamDrain drain(s);
    HIPCHK(c, ensure(c->tr.off, sizeof(int64_t) * ((size_t)n_nodes + 1)));
    HIPCHK(c, ensure(c->tr.edge, sizeof(int2) * (size_t)n_edges));
    HIPCHK(c, ensure(c->tr.order, sizeof(int32_t) * order.size()));
    HIPCHK(c, ensure(c->tr.ctr, 16));
    HIPCHK(c, ensure(c->tr.out, (size_t)n_edges));
    HIPCHK(c, hipMemcpyAsync(c->tr.off.p, off, sizeof(int64_t) * ((size_t)n_nodes + 1), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->tr.edge.p, edge.data(), sizeof(int2) * (size_t)n_edges, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->tr.order.p, order.data(), sizeof(int32_t) * order.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(c->tr.ctr.p, 0, 16, s));
    HIPCHK(c, hipMemsetAsync(c->tr.out.p, 0, (size_t)n_edges, s));
    OvlReduceArgs a{};
    a.off = as<int64_t>(c->tr.off);
    a.edge = as<int2>(c->tr.edge);
    a.order = as<int32_t>(c->tr.order);
    a.n_nodes = n_nodes;
    a.n_order = (int32_t)order.size();
    a.window = window;
    a.group = group;
    a.counter = as<uint32_t>(c->tr.ctr);
    a.reduced = as<uint8_t>(c->tr.out);
    const int32_t blocks = (int32_t)std::min<int64_t>((int64_t)order.size(), (int64_t)c->cu_count * kReduceBlocksPerCu);
    HIPCHK(c, c->tr.timer.arm(ctx->timing));
    HIPCHK(c, c->tr.timer.mark(0, s));
    HIPCHK(c, ovl_launch_reduce(&a, blocks, s));
    HIPCHK(c, c->tr.timer.mark(1, s));
    HIPCHK(c, hipMemcpyAsync(reduced, c->tr.out.p, (size_t)n_edges, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    drain.armed = false;
    int64_t count = 0;
    for (int64_t e = 0; e < n_edges; ++e) count += reduced[e];
    *n_reduced = count;
    return call.done(c->tr.timer.ms(0, 1));
}

OVL_API int ovl_last_transitive(const ovl_ctx* ctx, int32_t* window_nodes, int32_t* passes, int64_t* two_hop_steps) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    const TransitiveState::Last& t = ctx->devs[0]->tr.last;
    if (window_nodes) *window_nodes = t.window;
    if (passes) *passes = t.passes;
    if (two_hop_steps) *two_hop_steps = t.steps;
    return OVL_OK;
}
