// ovl_reach_api.cpp — reachability reduction of a string graph (overlapGraphs.py:354-367, transitive_reduction2):
// the host form (ovl_reach_reduce_host) and the device call (ovl_reach_reduce, ovl_reach.hip).  The argument checks
// are ovl_graph_check.h's, shared with ovl_reduce_api.cpp.
#include "ovl_ctx.h"
#include "ovl_graph_check.h"
#include "ovl_reach_host.h"

namespace {

constexpr int32_t kReachWindowWords = 64 * kReachAccWords;  // a wavefront's acc: 16,384 columns per window

int32_t pow2_at_least(int32_t x, int32_t cap) {
    int32_t g = 1;
    while (g < x && g < cap) g *= 2;
    return g;
}

}  // namespace

int32_t reach_window_words(const Dev* c) {
    return c->k.reach_window > 0 ? std::min(kReachWindowWords, (c->k.reach_window + 63) / 64) : kReachWindowWords;
}

int reach_launches(Dev* c, OvlReachArgs* a, bool closure, hipStream_t s) {
    const int32_t words = a->words;
    HIPCHK(c, ensure(c->rc.matrix, sizeof(uint64_t) * (size_t)a->n_nodes * (size_t)words));
    HIPCHK(c, ensure(c->rc.pivot, sizeof(uint64_t) * 64 * (size_t)words));
    a->matrix = as<uint64_t>(c->rc.matrix);
    a->pivot = as<uint64_t>(c->rc.pivot);
    const int32_t row_group = pow2_at_least(words, 64);
    // the window the marking walks with: never wider than a row, so that rows of up to 64 words take the
    // one-word-per-lane form (ovl_launch_reach_mark) at the default window too
    const int32_t mark_window = std::min(words, reach_window_words(c));
    const int32_t mark_group = pow2_at_least(mark_window, 64);
    HIPCHK(c, ovl_launch_reach_fill(a, s));
    if (closure || a->n_order > 0) {
        for (int32_t K = 0; K < words; ++K) {
            HIPCHK(c, ovl_launch_reach_pivot(a, K, s));
            HIPCHK(c, ovl_launch_reach_update(a, K, row_group, s));
        }
    }
    HIPCHK(c, ovl_launch_reach_mark(a, mark_group, mark_window, s));
    return OVL_OK;
}

OVL_API int ovl_reach_reduce_host(const int64_t* off, const int32_t* head, int32_t n_nodes, uint8_t* reduced,
                                  int64_t* n_reduced, uint64_t* closure) {
    const ovl_ctx* none = nullptr;
    const int rc = check_graph(none, off, head, nullptr, false, n_nodes, reduced, n_reduced, nullptr, nullptr);
    if (rc != OVL_OK) return rc;
    const int64_t words = ((int64_t)n_nodes + 63) / 64;
    std::vector<uint64_t> own;
    uint64_t* R = closure;
    if (!R) {
        if (!reach_alloc_matrix(own, n_nodes, words))
            return fail(none, OVL_E_OOM, "no memory for the %d x %d-bit reachability matrix", n_nodes, n_nodes);
        R = own.data();
    } else {
        std::fill(R, R + (int64_t)n_nodes * words, uint64_t(0));
    }
    reach_closure_host(off, head, n_nodes, words, R);
    *n_reduced = reach_mark_host(off, head, n_nodes, words, R, reduced);
    return OVL_OK;
}

OVL_API int ovl_reach_reduce(ovl_ctx* ctx, const int64_t* off, const int32_t* head, int32_t n_nodes, uint8_t* reduced,
                             int64_t* n_reduced, uint64_t* closure) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    StageCall call(ctx);
    Dev* c = call.dev;
    const int rc = check_graph(c, off, head, nullptr, false, n_nodes, reduced, n_reduced, nullptr, nullptr);
    if (rc != OVL_OK) return rc;
    const int64_t n_edges = n_nodes > 0 ? off[n_nodes] : 0;
    const int32_t words = (int32_t)(((int64_t)n_nodes + 63) / 64);
    const int32_t window_words = reach_window_words(c);
    call.begin();
    c->rc.last = {words, words, window_words * 64};  // (ceil(n_nodes / 64) pivot blocks: one per word column)
    const size_t matrix_bytes = sizeof(uint64_t) * (size_t)n_nodes * (size_t)words;
    if (n_edges == 0) {  // nothing reaches anything
        if (closure && matrix_bytes) memset(closure, 0, matrix_bytes);
        *n_reduced = 0;
        return OVL_OK;
    }
    std::vector<int32_t> order;
    reach_mark_order(off, n_nodes, order);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    StreamDrain drain(s);
    HIPCHK(c, ensure(c->rc.matrix, matrix_bytes));  // (ahead of the timed launches; reach_launches finds them made)
    HIPCHK(c, ensure(c->rc.pivot, sizeof(uint64_t) * 64 * (size_t)words));
    HIPCHK(c, ensure(c->rc.off, sizeof(int64_t) * ((size_t)n_nodes + 1)));
    HIPCHK(c, ensure(c->rc.head, sizeof(int32_t) * (size_t)n_edges));
    HIPCHK(c, ensure(c->rc.order, sizeof(int32_t) * order.size()));
    HIPCHK(c, ensure(c->rc.out, (size_t)n_edges));
    HIPCHK(c, hipMemcpyAsync(c->rc.off.p, off, sizeof(int64_t) * ((size_t)n_nodes + 1), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->rc.head.p, head, sizeof(int32_t) * (size_t)n_edges, hipMemcpyHostToDevice, s));
    if (!order.empty())
        HIPCHK(c, hipMemcpyAsync(c->rc.order.p, order.data(), sizeof(int32_t) * order.size(), hipMemcpyHostToDevice,
                                 s));
    HIPCHK(c, hipMemsetAsync(c->rc.out.p, 0, (size_t)n_edges, s));  // (nodes with one out-edge keep it)
    OvlReachArgs a{};
    a.off = as<int64_t>(c->rc.off);
    a.head = as<int32_t>(c->rc.head);
    a.order = as<int32_t>(c->rc.order);
    a.n_nodes = n_nodes;
    a.n_order = (int32_t)order.size();
    a.words = words;
    a.reduced = as<uint8_t>(c->rc.out);
    HIPCHK(c, c->rc.timer.arm(ctx->timing));
    HIPCHK(c, c->rc.timer.mark(0, s));
    const int lrc = reach_launches(c, &a, closure != nullptr, s);
    if (lrc != OVL_OK) return lrc;
    HIPCHK(c, c->rc.timer.mark(1, s));
    HIPCHK(c, hipMemcpyAsync(reduced, c->rc.out.p, (size_t)n_edges, hipMemcpyDeviceToHost, s));
    if (closure) HIPCHK(c, hipMemcpyAsync(closure, c->rc.matrix.p, matrix_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    drain.armed = false;
    int64_t count = 0;
    for (int64_t e = 0; e < n_edges; ++e) count += reduced[e];
    *n_reduced = count;
    return call.done(c->rc.timer.ms(0, 1));
}

OVL_API int ovl_last_reach(const ovl_ctx* ctx, int32_t* words_per_row, int32_t* pivot_blocks, int32_t* window_bits) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    const ReachState::Last& r = ctx->devs[0]->rc.last;
    if (words_per_row) *words_per_row = r.words;
    if (pivot_blocks) *pivot_blocks = r.blocks;
    if (window_bits) *window_bits = r.window;
    return OVL_OK;
}
