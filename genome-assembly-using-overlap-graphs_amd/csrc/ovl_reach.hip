// Reachability reduction of a string graph (overlapGraphs.py:354-367, transitive_reduction2) on the GPU
// (ovl_reach_reduce).
//
// The reference's has_path loop reduces to one rule: with R[u][x] true iff the input graph has a
// path of at least one edge from u to x, edge (v, w) is removed iff some u that stands before w in v's successor
// order has R[u][w].
//
// R is a bit matrix in HBM: n rows of `words` = ceil(n / 64) uint64, bit x of row u is bit x & 63 of word x >> 6,
// bits at and above n are zero.  Four kernels, every phase its own launch on one stream; no workgroup ever waits
// on another, and no lane reads within a launch what another lane of its wavefront stored there:
//   fill     a workgroup per node builds the node's row in LDS (ds_or of one bit per edge) and stores it; rows
//            wider than the LDS window take several column windows.  No global atomics.
//   pivot    (block K of 64 nodes)  every workgroup closes the 64 x 64 diagonal tile in its first wavefront --
//            lane i holds row 64K+i's word K, step k broadcasts lane k's word by readlane and the lanes whose bit k
//            is set OR it in -- then writes, for its chunk of 64 word columns, P*[i] = P[i] | OR_{k in tile*[i]} P[k]
//            into the 64-row pivot buffer from the unmodified rows staged in LDS.  It writes nothing into R, so the
//            workgroups of one launch share no word that any of them stores.
//   update   every row i -- the pivot block's own rows included, for which the same formula yields P*[i] -- reads
//            c = R[i][word K] and ORs P*[k] in for each set bit k of c; a row with c == 0 does nothing.  A row is
//            one lane group (a power of two of lanes, a wavefront from 64 words), lanes across the words, the
//            group's lanes walking c's bits together, up to kReachLoads pivot rows in flight per lane.
//   mark     a lane group per node with at least two out-edges, heaviest (degree x words) first in dispatch order;
//            acc -- the OR of R[u] over the successors seen so far -- lives in registers, kReachAccWords words per
//            lane; succ(v) is walked in order, the lane that owns word w >> 6 tests bit w and stores reduced[e],
//            then every lane ORs its words of R[w] in.  kReachAhead successors' rows (sixteen where a lane holds
//            one word) are loaded before the first is used, and the next trip's heads with them: the loads do
//            not depend on acc.  Rows wider than the lanes hold are processed in column windows, succ(v)
//            re-walked per window.
// After ceil(n / 64) pivot / update pairs R is the transitive closure (blocked Warshall): correct for any digraph,
// cycles and self-loops included, and the phase count does not depend on the graph's diameter.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ovl_kernels.h"

namespace ovl_reach {

constexpr int kFillThreads = 256;
constexpr int kFillWords = 4096;  // LDS window of a row under construction: 32 KiB, 262,144 columns

__global__ __launch_bounds__(kFillThreads) void fill_kernel(OvlReachArgs a) {
    __shared__ unsigned long long row[kFillWords];
    const int32_t v = (int32_t)blockIdx.x;
    const int32_t tid = threadIdx.x;
    const int64_t e0 = a.off[v], e1 = a.off[v + 1];
    uint64_t* out = a.matrix + (int64_t)v * a.words;
    for (int32_t w0 = 0; w0 < a.words; w0 += kFillWords) {
        const int32_t nw = min(kFillWords, a.words - w0);
        for (int32_t j = tid; j < nw; j += kFillThreads) row[j] = 0;
        __syncthreads();
        for (int64_t e = e0 + tid; e < e1; e += kFillThreads) {
            const int32_t x = a.head[e];
            const uint32_t j = (uint32_t)((x >> 6) - w0);
            if (j < (uint32_t)nw) atomicOr(&row[j], 1ull << (x & 63));
        }
        __syncthreads();
        for (int32_t j = tid; j < nw; j += kFillThreads) out[w0 + j] = row[j];
        __syncthreads();  // the stores have read the window before the next one is zeroed
    }
}

constexpr int kPivotThreads = 1024;  // 16 wavefronts: four pivot rows each
constexpr int kPivotLoads = 8;       // LDS rows a lane reads per trip, all in flight before the first OR

// the lowest set bit's index, cleared from c; 0 .. 63.  With c == 0 the previous index again: OR-ing a pivot row
// in twice changes nothing, so a trip of several loads needs no tail case
template <typename T>
__device__ __forceinline__ int32_t next_bit(T& c, int32_t prev) {
    if (c == 0) return prev;
    const int32_t k = sizeof(T) == 8 ? __builtin_ctzll(c) : __builtin_ctz((uint32_t)c);
    c &= c - 1;
    return k;
}

__global__ __launch_bounds__(kPivotThreads) void pivot_kernel(OvlReachArgs a, int32_t K) {
    __shared__ uint64_t p[64][64];  // [pivot row][word column of this workgroup's chunk]
    __shared__ uint64_t tile[64];   // tile*[i]: the pivot rows reachable from pivot row i inside the block
    const int32_t tid = threadIdx.x;
    const int32_t lane = tid & 63, wave = tid >> 6;
    const int32_t r0 = K * 64;
    const int32_t j = (int32_t)blockIdx.x * 64 + lane;  // this lane's word column
    if (wave == 0) {
        const uint64_t t = r0 + lane < a.n_nodes ? a.matrix[(int64_t)(r0 + lane) * a.words + K] : 0;
        uint32_t lo = (uint32_t)t, hi = (uint32_t)(t >> 32);
        for (int k = 0; k < 64; ++k) {  // (k is wave-uniform)
            const uint32_t klo = (uint32_t)__builtin_amdgcn_readlane((int32_t)lo, k);
            const uint32_t khi = (uint32_t)__builtin_amdgcn_readlane((int32_t)hi, k);
            const bool via = k < 32 ? (lo >> k) & 1u : (hi >> (k - 32)) & 1u;
            if (via) {
                lo |= klo;
                hi |= khi;
            }
        }
        tile[lane] = ((uint64_t)hi << 32) | lo;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int32_t i = q * 16 + wave;
        p[i][lane] = (r0 + i < a.n_nodes && j < a.words) ? a.matrix[(int64_t)(r0 + i) * a.words + j] : 0;
    }
    __syncthreads();
    for (int32_t i = wave * 4; i < wave * 4 + 4; ++i) {
        uint64_t out = p[i][lane];
        const uint64_t c = tile[i];  // (one address for the wavefront: the walk below is wave-uniform)
        uint32_t half[2] = {(uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)c),
                            (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(uint32_t)(c >> 32))};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            uint32_t cc = half[h];
            int32_t k = 0;
            while (cc) {
                uint64_t pv[kPivotLoads];
#pragma unroll
                for (int u = 0; u < kPivotLoads; ++u) {
                    k = next_bit(cc, k);
                    pv[u] = p[32 * h + k][lane];
                }
#pragma unroll
                for (int u = 0; u < kPivotLoads; ++u) out |= pv[u];
            }
        }
        if (j < a.words) a.pivot[(int64_t)i * a.words + j] = out;
    }
}

constexpr int kUpdateThreads = 256;

// acc |= the pivot rows' word j for the next N set bits of c (fewer: the last one again), N loads in flight
template <int N>
__device__ __forceinline__ void or_pivots(const uint64_t* pivot_j, int64_t words, uint64_t& c, int32_t& k,
                                          uint64_t& acc) {
    uint64_t pv[N];
#pragma unroll
    for (int u = 0; u < N; ++u) {
        k = next_bit(c, k);
        pv[u] = pivot_j[(int64_t)k * words];
    }
#pragma unroll
    for (int u = 0; u < N; ++u) acc |= pv[u];
}

__global__ __launch_bounds__(kUpdateThreads) void update_kernel(OvlReachArgs a, int32_t K, int32_t group_log2) {
    const int32_t group = 1 << group_log2;
    const int64_t t = (int64_t)blockIdx.x * kUpdateThreads + threadIdx.x;
    const int64_t i = t >> group_log2;
    const int32_t gl = (int32_t)t & (group - 1);
    if (i >= a.n_nodes) return;
    uint64_t* row = a.matrix + i * a.words;
    const uint64_t c = row[K];  // read by every lane of the row before any of them stores
    if (c == 0) return;
    for (int32_t j = gl; j < a.words; j += group) {
        uint64_t acc = row[j];
        uint64_t cc = c;
        int32_t k = 0;
        // dense pivot words kReachLoads rows per trip, the rest (and sparse words) four
        while (__popcll(cc) > 4) or_pivots<kReachLoads>(a.pivot + j, a.words, cc, k, acc);
        while (cc) or_pivots<4>(a.pivot + j, a.words, cc, k, acc);
        row[j] = acc;
    }
}

constexpr int kMarkThreads = 256;

// U words of acc per lane, AHEAD successors' rows loaded before the first is used; the next trip's heads are
// loaded before this trip's rows are consumed
template <int U, int AHEAD>
__global__ __launch_bounds__(kMarkThreads) void mark_kernel(OvlReachArgs a, int32_t group_log2, int32_t window_words) {
    const int32_t group = 1 << group_log2;
    const int64_t t = (int64_t)blockIdx.x * kMarkThreads + threadIdx.x;
    const int64_t slot = t >> group_log2;
    const int32_t gl = (int32_t)t & (group - 1);
    if (slot >= a.n_order) return;
    const int32_t v = a.order[slot];
    const int64_t e0 = a.off[v], e1 = a.off[v + 1];
    for (int32_t w0 = 0; w0 < a.words; w0 += window_words) {
        const int32_t nw = min(window_words, a.words - w0);  // <= group * U
        uint64_t acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = 0;
        int32_t w[AHEAD];
#pragma unroll
        for (int q = 0; q < AHEAD; ++q) w[q] = e0 + q < e1 ? a.head[e0 + q] : -1;
        for (int64_t e = e0; e < e1; e += AHEAD) {
            uint64_t r[AHEAD][U];
#pragma unroll
            for (int q = 0; q < AHEAD; ++q)
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int32_t j = gl + u * group;
                    r[q][u] = (w[q] >= 0 && j < nw) ? a.matrix[(int64_t)w[q] * a.words + w0 + j] : 0;
                }
            int32_t w_next[AHEAD];
#pragma unroll
            for (int q = 0; q < AHEAD; ++q) w_next[q] = e + AHEAD + q < e1 ? a.head[e + AHEAD + q] : -1;
#pragma unroll
            for (int q = 0; q < AHEAD; ++q) {
                if (w[q] < 0) continue;  // (past the list; its row reads as zeros)
                const uint32_t j = (uint32_t)((w[q] >> 6) - w0);  // the head's word, relative to the window
                if (j < (uint32_t)nw && (int32_t)(j & (uint32_t)(group - 1)) == gl) {
                    const uint32_t u_hit = j >> group_log2;
                    uint64_t word = 0;
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (u_hit == (uint32_t)u) word = acc[u];
                    a.reduced[e + q] = (uint8_t)((word >> (w[q] & 63)) & 1u);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) acc[u] |= r[q][u];
            }
#pragma unroll
            for (int q = 0; q < AHEAD; ++q) w[q] = w_next[q];
        }
    }
}

}  // namespace ovl_reach

extern "C" hipError_t ovl_launch_reach_fill(const OvlReachArgs* a, hipStream_t stream) {
    if (a->n_nodes <= 0) return hipSuccess;
    ovl_reach::fill_kernel<<<(unsigned)a->n_nodes, ovl_reach::kFillThreads, 0, stream>>>(*a);
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_reach_pivot(const OvlReachArgs* a, int32_t K, hipStream_t stream) {
    const unsigned blocks = (unsigned)((a->words + 63) / 64);
    ovl_reach::pivot_kernel<<<blocks, ovl_reach::kPivotThreads, 0, stream>>>(*a, K);
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_reach_update(const OvlReachArgs* a, int32_t K, int32_t group, hipStream_t stream) {
    const int64_t rows_per_block = ovl_reach::kUpdateThreads / group;
    const unsigned blocks = (unsigned)((a->n_nodes + rows_per_block - 1) / rows_per_block);
    ovl_reach::update_kernel<<<blocks, ovl_reach::kUpdateThreads, 0, stream>>>(*a, K, __builtin_ctz(group));
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_reach_mark(const OvlReachArgs* a, int32_t group, int32_t window_words,
                                            hipStream_t stream) {
    if (a->n_order <= 0) return hipSuccess;
    const int64_t per_block = ovl_reach::kMarkThreads / group;
    const unsigned blocks = (unsigned)((a->n_order + per_block - 1) / per_block);
    const int32_t group_log2 = __builtin_ctz(group);
    if (window_words <= group)  // one word per lane: the registers go to rows in flight instead
        ovl_reach::mark_kernel<1, kReachAhead * kReachAccWords>
            <<<blocks, ovl_reach::kMarkThreads, 0, stream>>>(*a, group_log2, window_words);
    else
        ovl_reach::mark_kernel<kReachAccWords, kReachAhead>
            <<<blocks, ovl_reach::kMarkThreads, 0, stream>>>(*a, group_log2, window_words);
    return hipGetLastError();
}
