// Batched local_alignment (aligners.py:85-167): many short queries against windows of one reference in one
// launch (ovl_local_align_batch).  The arithmetic, tie order, best-cell rule and traceback codes are sw_kernel's
// (ovl_local.hip); what differs is who owns what.
//
// One wavefront (one 64-thread block) owns one query from its first strip to its last op: it sweeps the query's
// 64-row strips in sequence with sw_kernel's anti-diagonal step (lane L on row 64s+1+L, column j = tau - L + 1,
// 64 branch-free unrolled steps per chunk), keeps a strip's last row for the next strip in a row of its own
// (n_chunks x 64 int32: in LDS when the launch's longest window fits, else a private global row), writes the
// traceback codes into a slab of its own in HBM ([strip][tau][lane], one byte per cell, code | 4 when the cell is
// > 0, non-cells 0), then walks that table itself (aligners.py:133-153) and stores the ops, their count and the
// cell where the walk stopped.  No wavefront ever waits on another: there are no epoch words and no polls, and
// the launch's wavefronts take query indices from one atomic counter until it runs out (the host lists the
// queries by descending n * m, so the long ones start first).
//
// The row is updated in place: chunk c of the previous strip's row is read when chunk c starts, chunk c-1 of this
// strip's row is written when chunk c ends, so a word is always read before it is overwritten.
//
// The slab is sized for the largest query of the launch and reused for every query the wavefront takes.  A query's
// fill stores every byte of its own [strip][tau][lane] extent, and the walk reads only inside that extent, so a
// short query never sees the codes a longer one left behind and nothing is cleared in between.
//
// Same-wavefront visibility: the slab, the global row and the op scratch are stored by one lane and read by
// another lane of the same wavefront.  Between the two sides stands drain(): s_waitcnt vmcnt(0), which retires the
// wavefront's own stores, and a workgroup-scope fence.  That is enough because both sides run on one CU: its
// vector L1 is write-through and shared by the (single) wavefront of the block, so once the stores have retired a
// load from the same CU returns them; an agent-scope fence would only add an L2 write-back and an L1
// invalidate that serve readers on other CUs, and there are none -- each slab, row and scratch belongs to one
// wavefront for the whole launch, and a kernel's start already invalidates what an earlier launch left in L1.
//
// The ops of all queries are packed: a wavefront walks into a scratch of its own, then reserves [base, base +
// count) of one output buffer with an atomic add and copies the ops there with all lanes, so only the ops that
// exist and one OvlLocalBatchRecord per query cross the link.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "ovl_kernels.h"
#include "ovl_wave.h"

namespace ovl_local_batch {

using namespace ovl_wave;

// this wavefront's stores become visible to its own other lanes (see the file comment)
__device__ __forceinline__ void drain() {
    vm_drain();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}

// the next query index of this wavefront
__device__ __forceinline__ uint32_t take(uint32_t* counter, int lane) {
    const uint32_t old = atomicAdd(counter, lane == 0 ? 1u : 0u);
    return (uint32_t)__builtin_amdgcn_readlane((int32_t)old, 0);
}

template <bool TB>
__global__ __launch_bounds__(64) void sw_batch_kernel(OvlLocalBatchArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t tbs[64 * 64];  // one chunk of codes: [step][lane]
    extern __shared__ __attribute__((aligned(16))) int32_t lrow[];  // the carried row (a.row_pitch == 0)
    const int32_t match = a.match, mismatch = a.mismatch, indel = a.indel;
    const int lane = threadIdx.x;
    const bool row_lds = a.row_pitch == 0;
    int32_t* grow = row_lds ? nullptr : a.rows + (int64_t)blockIdx.x * a.row_pitch;
    int8_t* slab = TB ? a.slabs + (int64_t)blockIdx.x * a.slab_pitch : nullptr;
    int8_t* wops = TB ? a.wave_ops + (int64_t)blockIdx.x * a.wave_ops_pitch : nullptr;
    // every lane issues the add (lanes 1..63 add 0), so taking an index is straight-line code with no
    // divergent region around the atomic; lane 0's return value is the wavefront's index
    for (uint32_t k = take(a.counter, lane); k < (uint32_t)a.n_items; k = take(a.counter, lane)) {
        const OvlLocalBatchItem it = a.items[k];
        const uint8_t* q = a.q + it.q_off;
        const uint8_t* r = a.ref + it.win_lo;
        const int32_t n = it.n, m = it.m;
        const int32_t n_strips = (n + 63) / 64;
        const int32_t n_chunks = (m + 62 + 64) / 64;   // steps tau = 0 .. m + 62
        const int64_t steps = (int64_t)n_chunks * 64;  // traceback row pitch
        unsigned long long qbest = 0;
        for (int32_t s = 0; s < n_strips; ++s) {
            const int32_t i = 64 * s + 1 + lane;
            const bool row_ok = i <= n;
            const uint32_t sc = row_ok ? (uint32_t)q[i - 1] : 0xFFFFFFFFu;
            const bool produce = s + 1 < n_strips;  // strip s+1 reads our last row (row 64s+64 <= n)
            int32_t cur = 0;    // dp[i][j-1]
            int32_t uprev = 0;  // dp[i-1][j-1]
            int32_t tch = 0;
            int32_t bval = 0, bj = 0;      // this row's first strict maximum (from 0)
            int32_t out_a = 0, out_b = 0;  // row staging: chunk c-1 (lanes 1..63) / chunk c (lane 0)
            int8_t* tbrow = TB ? slab + (int64_t)s * steps * 64 : nullptr;
            int32_t pend = -1;             // chunk whose codes sit in LDS, still to be written out
            if (s > 0) {
                // the previous strip's row stores, read below by other lanes
                if (row_lds) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                else drain();
            }
            for (int32_t c = 0; c < n_chunks; ++c) {
                // inputs of chunk c: lane u holds dp[64s][64c+1+u] (lane 0's "up" at step u) and t[64c+u]
                const int32_t tcol = 64 * c + lane;
                const int32_t v_t = tcol < m ? (int32_t)r[tcol] : 0;
                int32_t v_rin = 0;
                if (s > 0 && tcol + 1 <= m) v_rin = row_lds ? lrow[tcol] : grow[tcol];
                unroll<0, 64>([&](auto uc) {
                    constexpr int u = decltype(uc)::value;
                    const int32_t tau = 64 * c + u;
                    const int32_t j = tau - lane + 1;
                    const int32_t lds_up = __builtin_amdgcn_readlane(v_rin, u);
                    const int32_t lds_t = __builtin_amdgcn_readlane(v_t, u);
                    if (TB && u == 0 && pend >= 0) {  // (u is a compile-time step index)
                        // the previous chunk's codes leave LDS once this chunk's inputs are in registers
                        flush_codes(tbs, tbrow + (int64_t)pend * 64 * 64, lane);
                        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    }
                    int32_t upin = shr1(cur);
                    int32_t tin = shr1(tch);
                    upin = lane == 0 ? lds_up : upin;
                    tin = lane == 0 ? lds_t : tin;
                    const bool cell = row_ok && j >= 1 && j <= m;
                    const int32_t diag = uprev + ((uint32_t)tin == sc ? match : mismatch);
                    const int32_t up = upin + indel;
                    const int32_t left = cur + indel;
                    const int32_t mx = diag > up ? diag : up;
                    int32_t v = mx > left ? mx : left;
                    v = v > 0 ? v : 0;
                    if constexpr (TB) {
                        int32_t code = (diag >= up && diag >= left && diag >= 0) ? 1
                                     : ((up >= left && up >= 0) ? 2 : (left >= 0 ? 3 : 0));
                        code |= v > 0 ? 4 : 0;
                        tbs[u * 64 + lane] = (uint8_t)(cell ? code : 0);
                    }
                    cur = cell ? v : cur;
                    const bool better = cell && v > bval;
                    bval = better ? v : bval;
                    bj = better ? j : bj;
                    if (produce) {
                        // lane 63 finished column j63 = tau - 62 of row 64s+64
                        const int32_t v63 = __builtin_amdgcn_readlane(cur, 63);
                        if constexpr (u <= 62) out_a = writelane<u + 1>(out_a, v63);  // row chunk c-1, lane u+1
                        else out_b = writelane<0>(out_b, v63);                        // row chunk c, lane 0
                    }
                    uprev = upin;
                    tch = tin;
                });
                // row chunk c-1 (columns 64(c-1)+1 .. 64c) is complete; this strip read it a chunk ago
                if (produce && c >= 1) {
                    const int32_t w = 64 * (c - 1) + lane;
                    if (w + 1 <= m) {
                        if (row_lds) lrow[w] = out_a;
                        else grow[w] = out_a;
                    }
                }
                out_a = out_b;
                pend = c;
            }
            // the last row chunk and the last chunk of codes
            if (produce) {
                const int32_t w = 64 * (n_chunks - 1) + lane;
                if (w + 1 <= m) {
                    if (row_lds) lrow[w] = out_a;
                    else grow[w] = out_a;
                }
            }
            if (TB && pend >= 0) {
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                flush_codes(tbs, tbrow + (int64_t)pend * 64 * 64, lane);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            }
            // strip's best: max value, then smallest row i, then smallest column j (fill order)
            unsigned long long key = 0;
            if (row_ok && bval > 0)
                key = ((unsigned long long)(uint32_t)bval << 40) |
                      ((unsigned long long)(0xFFFFFu - (uint32_t)i) << 20) |
                      (unsigned long long)(0xFFFFFu - (uint32_t)bj);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const unsigned long long o = __shfl_xor(key, off, 64);
                key = o > key ? o : key;
            }
            qbest = key > qbest ? key : qbest;
        }
        int32_t score = 0, bi = 0, bjq = 0;
        if (qbest) {
            score = (int32_t)(qbest >> 40);
            bi = (int32_t)(0xFFFFFu - (uint32_t)((qbest >> 20) & 0xFFFFF));
            bjq = (int32_t)(0xFFFFFu - (uint32_t)(qbest & 0xFFFFF));
        }
        // aligners.py:133-153: walk while i > 0, j > 0 and dp[i][j] > 0 (every lane walks the same cells)
        int32_t wi = bi, wj = bjq, cnt = 0;
        unsigned long long base = 0;
        if (TB && bi > 0 && bjq > 0) {
            drain();  // the fill's code stores, read below by whichever lane's cell the walk visits
            while (wi > 0 && wj > 0) {
                const int32_t st = (wi - 1) >> 6, L = (wi - 1) & 63;
                const int8_t code = slab[((int64_t)st * steps + (wj + L - 1)) * 64 + L];
                if (!(code & 4)) break;
                const int8_t op = code & 3;
                if (op == 1) { --wi; --wj; }
                else if (op == 2) { --wi; }
                else if (op == 3) { --wj; }
                else break;
                if (lane == 0) wops[cnt] = op;
                ++cnt;
            }
            if (cnt > 0) {
                base = atomicAdd(a.ops_total, lane == 0 ? (unsigned long long)cnt : 0ull);
                base = __shfl(base, 0, 64);
                drain();  // lane 0's scratch stores, read below by every lane
                for (int32_t t = lane; t < cnt; t += 64) a.ops[base + (unsigned long long)t] = wops[t];
            }
        }
        if (lane == 0) {
            OvlLocalBatchRecord* o = a.out + it.out;
            o->score = score; o->end_i = bi; o->end_j = bjq; o->start_i = wi; o->start_j = wj; o->n_ops = cnt;
            o->ops_lo = (uint32_t)base; o->ops_hi = (uint32_t)(base >> 32);
        }
        // the next query's stores to the row, the slab and the scratch follow this query's loads of them in
        // program order, and those loads' values have been used
    }
}

}  // namespace ovl_local_batch

extern "C" hipError_t ovl_launch_local_batch(const OvlLocalBatchArgs* a, int32_t waves, uint32_t lds_row_bytes,
                                             hipStream_t stream) {
    if (a->n_items <= 0 || waves <= 0) return hipSuccess;
    if (a->slabs)
        ovl_local_batch::sw_batch_kernel<true><<<(unsigned)waves, 64, lds_row_bytes, stream>>>(*a);
    else
        ovl_local_batch::sw_batch_kernel<false><<<(unsigned)waves, 64, lds_row_bytes, stream>>>(*a);
    return hipGetLastError();
}
