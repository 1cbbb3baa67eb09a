// Transitive reduction of an overlap graph (overlapGraphs.py:235-303) on the GPU (ovl_transitive_reduce).
//
// The reference's marking loops reduce to one rule: edge (v, x) is removed iff some w in succ(v)
// has an edge (w, x) with weight(v, w) + weight(w, x) >= weight(v, x).  The work is one step per two-hop path
// v -> w -> x: sum over v, over w in succ(v), of deg(w).
//
// Persistent workgroups of kReduceThreads take source nodes from one atomic counter; the host lists the nodes
// with out-edges by descending two-hop work, so the heavy ones start first.  For its node v a workgroup
//   fill   scatters weight(v, x) into a window row[x - t0] of LDS for v's heads x in [t0, t0 + window);
//          every other entry holds kNoEdge;
//   mark   splits succ(v) over groups of `group` lanes; a group's lanes stride over succ(w), read row[x] and
//          store kGone into it when it holds a weight <= weight(v, w) + weight(w, x);
//   write  stores reduced[e] = (row[head[e]] == kGone) for v's edges in the window and puts kNoEdge back into
//          exactly those entries, so a node's cost is its own degree and two-hop work, never the window's size.
// A graph with more nodes than the window takes ceil(n_nodes / window) passes per node; a pass whose window holds
// none of v's heads ends after the fill.
//
// The eliminated flag shares the entry's word with the weight: weights are in (-2^30, 2^30), kNoEdge and kGone lie
// below every sum of two.  A marker overwrites the whole word with kGone and nothing else is ever stored during
// the mark phase, so concurrent markers of one entry all store the same value and no read-modify-write can lose a
// flag; a marker that reads kGone (or the weight just before another marker's store) decides the same either way.
// Heads are distinct within a node's list, so in the write phase each entry is read and reset by one thread only.
//
// Taking a node: every lane of the block's first wavefront issues the counter add (lanes 1..63 add 0) and every
// one of them stores lane 0's result to LDS -- straight-line code with no lane-0-only region around the atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ovl_kernels.h"

namespace ovl_reduce {

constexpr int32_t kNoEdge = INT32_MIN;
constexpr int32_t kGone = INT32_MIN + 1;

__global__ __launch_bounds__(kReduceThreads) void reduce_kernel(OvlReduceArgs a) {
    extern __shared__ int32_t row[];
    __shared__ uint32_t s_take;
    const int32_t tid = threadIdx.x;
    const int32_t T = a.window;
    for (int32_t i = tid; i < T; i += kReduceThreads) row[i] = kNoEdge;
    const int32_t G = a.group;
    const int32_t grp = tid / G, gl = tid % G, n_grp = kReduceThreads / G;
    for (;;) {
        if (tid < 64) {
            const uint32_t old = atomicAdd(a.counter, tid == 0 ? 1u : 0u);
            s_take = (uint32_t)__builtin_amdgcn_readlane((int32_t)old, 0);
        }
        __syncthreads();  // also: the previous node's resets are done before this node's fill
        const uint32_t k = s_take;
        if (k >= (uint32_t)a.n_order) break;
        const int32_t v = a.order[k];
        const int64_t e0 = a.off[v];
        const int32_t deg = (int32_t)(a.off[v + 1] - e0);
        for (int64_t t64 = 0; t64 < a.n_nodes; t64 += T) {  // (64-bit: the last step may pass INT32_MAX)
            const int32_t t0 = (int32_t)t64;
            int32_t mine = 0;
            for (int32_t i = tid; i < deg; i += kReduceThreads) {
                const int2 ed = a.edge[e0 + i];
                const uint32_t x = (uint32_t)(ed.x - t0);
                if (x < (uint32_t)T) {
                    row[x] = ed.y;
                    mine = 1;
                }
            }
            // the fill is visible to the markers (and s_take has been read by every thread)
            if (__syncthreads_or(mine) == 0) continue;
            for (int32_t i = grp; i < deg; i += n_grp) {
                const int2 vw = a.edge[e0 + i];
                const int64_t f0 = a.off[vw.x];
                const int32_t dw = (int32_t)(a.off[vw.x + 1] - f0);
                // kReduceLoads loads of succ(w) in flight per lane before the first is used: the lists come from
                // L2, and one load per trip left the marking waiting on its latency
                for (int32_t j = gl; j < dw; j += kReduceLoads * G) {
                    int2 wx[kReduceLoads];
#pragma unroll
                    for (int u = 0; u < kReduceLoads; ++u)
                        wx[u] = j + u * G < dw ? a.edge[f0 + j + u * G] : make_int2(-1, 0);
#pragma unroll
                    for (int u = 0; u < kReduceLoads; ++u) {
                        const uint32_t x = (uint32_t)(wx[u].x - t0);  // (past the list: head -1, outside any window)
                        if (x < (uint32_t)T) {
                            const int32_t r = row[x];
                            if (r > kGone && vw.y + wx[u].y >= r) row[x] = kGone;
                        }
                    }
                }
            }
            __syncthreads();
            for (int32_t i = tid; i < deg; i += kReduceThreads) {
                const uint32_t x = (uint32_t)(a.edge[e0 + i].x - t0);
                if (x < (uint32_t)T) {
                    a.reduced[e0 + i] = row[x] == kGone ? 1 : 0;
                    row[x] = kNoEdge;
                }
            }
            __syncthreads();  // the resets are done before the next window's fill
        }
    }
}

}  // namespace ovl_reduce

extern "C" hipError_t ovl_launch_reduce(const OvlReduceArgs* a, int32_t blocks, hipStream_t stream) {
    if (a->n_order <= 0 || blocks <= 0) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ovl_reduce::reduce_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(sizeof(int32_t) * (size_t)a->window));
    if (e != hipSuccess) return e;
    ovl_reduce::reduce_kernel<<<(unsigned)blocks, kReduceThreads, sizeof(int32_t) * (size_t)a->window, stream>>>(*a);
    return hipGetLastError();
}
