// Consensus (ovl_consensus, ovl_consensus_api.cpp): the read pileup over the walks that the batch kernel
// (ovl_local_batch.hip) left in device memory, and the per-base vote.
//
// consensus_pileup_kernel: one wavefront per read, reads taken from one atomic counter as sw_batch_kernel takes
// its queries.  A read's walk is ops[base .. base + cnt), op t taken at the cell the walk had reached after ops
// 0 .. t-1 from (bi, bj): diag (1) moves up and left, up (2) moves up, left (3) moves left.  The wavefront consumes
// the ops 64 at a time, lane t on op t: the cell's column is bj minus the number of earlier ops in {1, 3}, its row bi
// minus the number of earlier ops in {1, 2} -- two ballots and a popcount of the bits below the lane, with the two
// totals carried from chunk to chunk.  Every op then casts one vote, an int32 atomicAdd, into the column's six
// channels (DP column j is contig base j - 1 of the window): A, C, G, T by the read's byte for a diag, gap for a
// left, ins for an up -- the column at the left of an inserted base.  No LDS, no barrier, no scratch.  Integer
// adds: the counts do not depend on the order in which reads or ops arrive.
//
// The counts are base-major, six int32 per contig base, the layout of the C ABI: a diag-only walk (the common one)
// puts lane t on base (column - t), so a wavefront's adds fall on 64 neighbouring 24-byte rows.
//
// consensus_vote_kernel: one thread per contig base; the changed bases are counted by a ballot per wavefront and one
// atomic add.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ovl_kernels.h"

namespace ovl_consensus {

// the channel of a read byte: upper-case A, C, G, T only
__device__ __forceinline__ int32_t channel(uint32_t byte) {
    return byte == 'A' ? 0 : (byte == 'C' ? 1 : (byte == 'G' ? 2 : (byte == 'T' ? 3 : -1)));
}

__global__ __launch_bounds__(64) void consensus_pileup_kernel(OvlPileupArgs a) {
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (;;) {
        // every lane issues the add (lanes 1..63 add 0), as in sw_batch_kernel
        const uint32_t old = atomicAdd(a.counter, lane == 0 ? 1u : 0u);
        const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int32_t)old, 0);
        if (k >= (uint32_t)a.n_items) break;
        const OvlLocalBatchItem it = a.items[k];
        const OvlLocalBatchRecord* rec = a.out + it.out;
        const int32_t bi = rec->end_i, bj = rec->end_j, cnt = rec->n_ops;
        const unsigned long long hi = rec->ops_hi;
        const unsigned long long base = rec->ops_lo | (hi << 32);  // ops_base()
        const uint8_t* q = a.q + it.q_off;
        int32_t cols = 0, rows = 0;  // ops before this chunk that consumed a column / a row
        uint32_t other = 0, bad = 0;
        for (int32_t t0 = 0; t0 < cnt; t0 += 64) {
            const int32_t t = t0 + lane;
            const bool live = t < cnt;
            const int32_t op = live ? (int32_t)a.ops[base + (unsigned long long)t] : 0;
            const unsigned long long mc = __ballot(op == 1 || op == 3), mr = __ballot(op == 1 || op == 2);
            const int32_t wj = bj - cols - __popcll(mc & below);  // the cell this op was taken at
            const int32_t wi = bi - rows - __popcll(mr & below);
            const bool inside = wj >= 1 && wj <= it.m && wi >= 1 && wi <= it.n && op >= 1 && op <= 3;
            int32_t ch = -1;
            if (live && inside) ch = op == 3 ? 4 : (op == 2 ? 5 : channel(q[wi - 1]));
            if (ch >= 0) atomicAdd(a.counts + ((int64_t)it.win_lo + (wj - 1)) * 6 + ch, 1);
            other += (uint32_t)__popcll(__ballot(live && inside && op == 1 && ch < 0));
            bad += (uint32_t)__popcll(__ballot(live && !inside));
            cols += __popcll(mc);
            rows += __popcll(mr);
        }
        if (lane == 0 && other) atomicAdd(a.ctr + 0, (unsigned long long)other);
        if (lane == 0 && bad) atomicAdd(a.ctr + 2, (unsigned long long)bad);
    }
}

__global__ __launch_bounds__(256) void consensus_add_kernel(const int64_t* hits, int64_t n_hits, int32_t* counts) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_hits; i += (int64_t)gridDim.x * 256)
        atomicAdd(counts + hits[i], 1);
}

__global__ __launch_bounds__(256) void consensus_vote_kernel(const uint8_t* ref, const int32_t* counts,
                                                             int64_t n_bases, int32_t min_depth, uint8_t* called,
                                                             unsigned long long* ctr) {
    for (int64_t b0 = (int64_t)blockIdx.x * 256; b0 < n_bases; b0 += (int64_t)gridDim.x * 256) {
        const int64_t b = b0 + threadIdx.x;
        bool changed = false;
        if (b < n_bases) {
            const int32_t* c = counts + b * 6;
            const int32_t v[4] = {c[0], c[1], c[2], c[3]};
            const uint32_t own = ref[b];
            uint32_t call = own;
            if ((int64_t)v[0] + v[1] + v[2] + v[3] >= min_depth) {
                const int32_t top = max(max(v[0], v[1]), max(v[2], v[3]));
                const int32_t oc = channel(own);
                const bool keep = oc >= 0 && (oc == 0 ? v[0] : (oc == 1 ? v[1] : (oc == 2 ? v[2] : v[3]))) == top;
                if (!keep) call = v[0] == top ? 'A' : (v[1] == top ? 'C' : (v[2] == top ? 'G' : 'T'));
            }
            called[b] = (uint8_t)call;
            changed = call != own;
        }
        const unsigned long long m = __ballot(changed);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(ctr + 1, (unsigned long long)__popcll(m));
    }
}

}  // namespace ovl_consensus

extern "C" hipError_t ovl_launch_consensus_pileup(const OvlPileupArgs* a, int32_t waves, hipStream_t stream) {
    if (a->n_items <= 0 || waves <= 0) return hipSuccess;
    ovl_consensus::consensus_pileup_kernel<<<(unsigned)waves, 64, 0, stream>>>(*a);
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_consensus_add(const int64_t* hits, int64_t n_hits, int32_t* counts,
                                               hipStream_t stream) {
    if (n_hits <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((n_hits + 255) / 256, 2048);
    ovl_consensus::consensus_add_kernel<<<(unsigned)blocks, 256, 0, stream>>>(hits, n_hits, counts);
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_consensus_vote(const uint8_t* ref, const int32_t* counts, int64_t n_bases,
                                                int32_t min_depth, uint8_t* called, unsigned long long* ctr,
                                                hipStream_t stream) {
    if (n_bases <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((n_bases + 255) / 256, 2048);
    ovl_consensus::consensus_vote_kernel<<<(unsigned)blocks, 256, 0, stream>>>(ref, counts, n_bases, min_depth,
                                                                                called, ctr);
    return hipGetLastError();
}
