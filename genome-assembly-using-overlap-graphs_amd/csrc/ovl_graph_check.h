// ovl_graph_check.h — the argument checks of the graph stages that take a CSR (ovl_reduce_api.cpp,
// ovl_reach_api.cpp): one copy for both, for their host forms and their device calls.
#pragma once
#include "ovl_ctx.h"

constexpr int64_t kReduceWeightLimit = int64_t(1) << 30;  // the device forms int32 sums of two weights

// Every check of an entry point, before anything is launched or written.  `weight` may be null for a stage that
// reads no weights (`weighted` false).  `work` and `steps`, when given (both or neither), receive each node's
// two-hop work sum over w in succ(v) of deg(w) and their total.
template <typename C>
int check_graph(const C* c, const int64_t* off, const int32_t* head, const int64_t* weight, bool weighted,
                int32_t n_nodes, const uint8_t* reduced, const int64_t* n_reduced, std::vector<int64_t>* work,
                int64_t* steps) {
    if (n_nodes < 0) return fail(c, OVL_E_ARG, "negative node count");
    if (!off || !n_reduced) return fail(c, OVL_E_ARG, "NULL off or n_reduced");
    if (off[0] != 0) return fail(c, OVL_E_ARG, "off[0] = %lld, not 0", (long long)off[0]);
    for (int32_t v = 0; v < n_nodes; ++v)
        if (off[v + 1] < off[v]) return fail(c, OVL_E_ARG, "off decreases at node %d", v);
    const int64_t n_edges = off[n_nodes];
    if (n_edges > 0 && (!head || (weighted && !weight) || !reduced))
        return fail(c, OVL_E_ARG, weighted ? "NULL head, weight or reduced" : "NULL head or reduced");
    for (int64_t e = 0; e < n_edges; ++e)
        if (head[e] < 0 || head[e] >= n_nodes)
            return fail(c, OVL_E_INDEX, "edge %lld: head %d outside [0, %d)", (long long)e, head[e], n_nodes);
    if (weighted)
        for (int64_t e = 0; e < n_edges; ++e)
            if (weight[e] >= kReduceWeightLimit || weight[e] <= -kReduceWeightLimit)
                return fail(c, OVL_E_RANGE, "edge %lld: |weight| = |%lld| >= 2^30", (long long)e,
                            (long long)weight[e]);
    if (!work) return OVL_OK;  // the host forms need no step counts
    int64_t total = 0;
    work->assign((size_t)n_nodes, 0);
    for (int32_t v = 0; v < n_nodes; ++v) {
        int64_t w = 0;
        for (int64_t e = off[v]; e < off[v + 1]; ++e) w += off[head[e] + 1] - off[head[e]];
        (*work)[(size_t)v] = w;
        total += w;
    }
    *steps = total;
    return OVL_OK;
}
