// ovl_unitigs.h — the launches of ovl_unitigs.hip as ovl_unitigs_api.cpp drives them, and the one statement both
// sides share of where pair (x, y) stands in the score columns.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// The index of the ordered pair (x, y), x != y, in the ovl_candidates(k = 0) list over n distinct reads: row x holds
// every other read in ascending order.
__host__ __device__ inline int64_t ovl_unitigs_col(int32_t x, int32_t y, int32_t n) {
    return (int64_t)x * (n - 1) + y - (y > x ? 1 : 0);
}

// Everything lives in device memory.  Per raw read j: ids[j], its distinct read, and prev[j], the previous raw position
// that holds ids[j] or -1.  Per distinct read x: first[x], its first raw position; self_ix[x], where the self pair's
// (score, end) stands in the self columns, or -1 for a read with one copy.  score / end: the n (n - 1) columns in
// ovl_unitigs_col order.  deg / off: n + 1 int64 (deg[n] zeroed by the caller; off its exclusive scan).  Per edge:
// tail, head, weight, eend, reduced (the marking's mask), keep (n_edges + 1 int32, the last one 0) and pos, keep's
// exclusive scan; k_*: the kept edges' columns.  Per node: outdeg, indeg (zeroed by the caller), nxt, nend.
struct OvlUnitigArgs {
    int32_t n, n_raw;
    const int32_t* ids;
    const int32_t* prev;
    const int32_t* first;
    const int32_t* self_ix;
    const int32_t* score;
    const int32_t* end;
    const int32_t* self_score;
    const int32_t* self_end;
    int64_t* deg;
    int64_t* off;
    int64_t n_edges;
    int32_t* tail;
    int32_t* head;
    int32_t* weight;
    int32_t* eend;
    uint8_t* reduced;
    int32_t* keep;
    int32_t* pos;
    int32_t* k_tail;
    int32_t* k_head;
    int32_t* k_weight;
    int32_t* k_end;
    int32_t* outdeg;
    int32_t* indeg;
    int32_t* nxt;
    int32_t* nend;
};

// deg[x] = the edges of row x: a wavefront per row, lanes over the raw positions after first[x]
extern "C" hipError_t ovl_launch_unitigs_degree(const OvlUnitigArgs* g, hipStream_t stream);
// off = exclusive scan of deg over n + 1 entries (off[n] = the edges), through `temp` (ovl_unitigs_scan_bytes(n + 1))
extern "C" hipError_t ovl_unitigs_scan_bytes(int64_t count, size_t* bytes);
extern "C" hipError_t ovl_launch_unitigs_offsets(const OvlUnitigArgs* g, void* temp, size_t temp_bytes,
                                                 hipStream_t stream);
// tail, head, weight, eend of every edge at off[x] + its rank in row x, ascending raw position
extern "C" hipError_t ovl_launch_unitigs_fill(const OvlUnitigArgs* g, hipStream_t stream);
// keep[e] = !reduced[e]; outdeg, indeg by int32 atomics over the kept edges; nxt[tail], nend[tail] stored by every
// kept edge (meaningful where outdeg[tail] == 1: one lane stored it)
extern "C" hipError_t ovl_launch_unitigs_facts(const OvlUnitigArgs* g, hipStream_t stream);
// pos = exclusive scan of keep over n_edges + 1 entries (pos[n_edges] = the kept edges), then the kept edges' columns
// in CSR order
extern "C" hipError_t ovl_launch_unitigs_kept(const OvlUnitigArgs* g, void* temp, size_t temp_bytes,
                                              hipStream_t stream);
