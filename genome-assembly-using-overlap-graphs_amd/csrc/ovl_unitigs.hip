// The unitig pipeline's string graph and node facts from the score columns (ovl_unitigs, ovl_unitigs_candidates).
//
// The raw reads R[0 .. N) hold the distinct reads d[0 .. n) in first-occurrence order; ids[j] is R[j]'s distinct read,
// first[x] the first raw position of x, prev[j] the previous raw position holding ids[j] or -1.  The reference's
// construct_string_graph scores combinations(R, 2) and adds an edge where the score is positive, so the successor
// list of node x, in insertion order, is: for j = first[x] + 1 .. N - 1 ascending, ids[j] iff prev[j] <= first[x]
// (j is that read's first occurrence after first[x]) and score(x, ids[j]) > 0.  The self pair (x, x), reached when x
// has a second copy, takes its (score, end) from the self columns; every other pair from the n (n - 1) columns in
// ovl_candidates(k = 0) order.  No sort: the CSR is a stream compaction of the n x N grid.
//
//   degree   a wavefront per row x, lanes over j; the flag is counted by ballot and popcount, lane 0 stores deg[x]
//   offsets  hipcub's exclusive scan of deg over n + 1 entries
//   fill     the same walk; an edge's place is off[x] + the running base + the ballot's prefix below its lane, so a
//            row's edges stand in ascending j.  tail, head, weight and end_position per edge
//   facts    (after ovl_reach.hip's marking) a lane per edge: keep[e] = !reduced[e]; a kept edge adds one to
//            outdeg[tail] and indeg[head] (int32 atomics) and stores head and end_position into nxt[tail], nend[tail]
//            -- the host reads those only where outdeg[tail] == 1, where exactly one lane stored them
//   kept     hipcub's exclusive scan of keep, then a lane per kept edge copies its four columns to pos[e]: the
//            reduced graph's edges in CSR order
// Every launch is bounded by its grid; no workgroup waits on another; every store is a vector store.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>

#include "ovl_unitigs.h"

namespace ovl_unitigs {

constexpr int kThreads = 256;
constexpr int kRowsPerBlock = kThreads / 64;

// whether raw position j > first[x] yields an edge of row x, and the edge
__device__ __forceinline__ bool edge_at(const OvlUnitigArgs& g, int32_t x, int32_t fx, int32_t j, int32_t& y,
                                        int32_t& sc, int32_t& en) {
    y = g.ids[j];
    sc = en = 0;
    if (g.prev[j] > fx || (uint32_t)y >= (uint32_t)g.n) return false;
    if (y == x) {
        const int32_t ix = g.self_ix[x];
        if (ix < 0) return false;  // (a read with one copy has no second occurrence: never reached)
        sc = g.self_score[ix];
        en = g.self_end[ix];
    } else {
        const int64_t col = ovl_unitigs_col(x, y, g.n);
        sc = g.score[col];
        en = g.end[col];
    }
    return sc > 0;
}

template <bool FILL>
__global__ __launch_bounds__(kThreads) void row_kernel(OvlUnitigArgs g) {
    const int lane = threadIdx.x & 63;
    const int32_t x = (int32_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);  // (the same for a wavefront's lanes)
    if (x >= g.n) return;
    const int32_t fx = g.first[x];
    int64_t base = FILL ? g.off[x] : 0;
    const int64_t cap = FILL ? g.off[x + 1] : 0;
    for (int32_t j0 = fx + 1; j0 < g.n_raw; j0 += 64) {  // (j0 is wave-uniform: every lane takes every ballot)
        const int32_t j = j0 + lane;
        int32_t y = 0, sc = 0, en = 0;
        const bool flag = j < g.n_raw && edge_at(g, x, fx, j, y, sc, en);
        const unsigned long long m = __ballot(flag);
        if (FILL && flag) {
            const int64_t e = base + __popcll(m & ((1ull << lane) - 1ull));
            if (e < cap) {  // (the degree pass counted the same flags)
                g.tail[e] = x;
                g.head[e] = y;
                g.weight[e] = sc;
                g.eend[e] = en;
            }
        }
        base += __popcll(m);
    }
    if (!FILL && lane == 0) g.deg[x] = base;
}

__global__ __launch_bounds__(kThreads) void facts_kernel(OvlUnitigArgs g) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e <= g.n_edges; e += stride) {
        if (e == g.n_edges) {
            g.keep[e] = 0;
            continue;
        }
        const int32_t k = g.reduced[e] == 0;
        g.keep[e] = k;
        if (!k) continue;
        const int32_t t = g.tail[e], h = g.head[e];
        if ((uint32_t)t >= (uint32_t)g.n || (uint32_t)h >= (uint32_t)g.n) continue;
        atomicAdd(g.outdeg + t, 1);
        atomicAdd(g.indeg + h, 1);
        g.nxt[t] = h;
        g.nend[t] = g.eend[e];
    }
}

__global__ __launch_bounds__(kThreads) void kept_kernel(OvlUnitigArgs g) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < g.n_edges; e += stride) {
        if (!g.keep[e]) continue;
        const int64_t k = g.pos[e];
        if (k < 0 || k >= g.n_edges) continue;
        g.k_tail[k] = g.tail[e];
        g.k_head[k] = g.head[e];
        g.k_weight[k] = g.weight[e];
        g.k_end[k] = g.eend[e];
    }
}

inline unsigned edge_blocks(int64_t count) {
    return (unsigned)std::min<int64_t>((count + kThreads - 1) / kThreads, 2048);
}

}  // namespace ovl_unitigs

extern "C" hipError_t ovl_launch_unitigs_degree(const OvlUnitigArgs* g, hipStream_t stream) {
    if (g->n <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((g->n + ovl_unitigs::kRowsPerBlock - 1) / ovl_unitigs::kRowsPerBlock);
    ovl_unitigs::row_kernel<false><<<blocks, ovl_unitigs::kThreads, 0, stream>>>(*g);
    return hipGetLastError();
}

extern "C" hipError_t ovl_unitigs_scan_bytes(int64_t count, size_t* bytes) {
    size_t b64 = 0, b32 = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, b64, (const int64_t*)nullptr, (int64_t*)nullptr,
                                                    (int)count);
    if (e != hipSuccess) return e;
    e = hipcub::DeviceScan::ExclusiveSum(nullptr, b32, (const int32_t*)nullptr, (int32_t*)nullptr, (int)count);
    *bytes = std::max(b64, b32);
    return e;
}

extern "C" hipError_t ovl_launch_unitigs_offsets(const OvlUnitigArgs* g, void* temp, size_t temp_bytes,
                                                 hipStream_t stream) {
    return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, (const int64_t*)g->deg, g->off, g->n + 1, stream);
}

extern "C" hipError_t ovl_launch_unitigs_fill(const OvlUnitigArgs* g, hipStream_t stream) {
    if (g->n <= 0 || g->n_edges <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((g->n + ovl_unitigs::kRowsPerBlock - 1) / ovl_unitigs::kRowsPerBlock);
    ovl_unitigs::row_kernel<true><<<blocks, ovl_unitigs::kThreads, 0, stream>>>(*g);
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_unitigs_facts(const OvlUnitigArgs* g, hipStream_t stream) {
    ovl_unitigs::facts_kernel<<<ovl_unitigs::edge_blocks(g->n_edges + 1), ovl_unitigs::kThreads, 0, stream>>>(*g);
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_unitigs_kept(const OvlUnitigArgs* g, void* temp, size_t temp_bytes,
                                              hipStream_t stream) {
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, (const int32_t*)g->keep, g->pos,
                                                    (int)(g->n_edges + 1), stream);
    if (e != hipSuccess || g->n_edges <= 0) return e;
    ovl_unitigs::kept_kernel<<<ovl_unitigs::edge_blocks(g->n_edges), ovl_unitigs::kThreads, 0, stream>>>(*g);
    return hipGetLastError();
}
