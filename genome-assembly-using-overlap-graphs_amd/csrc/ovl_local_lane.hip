// Lane-per-read local alignment scores (aligners.py:85-137, the fill and its best cell): every read against every
// contig for ovl_read_best (ovl_depth_api.cpp).  The local-alignment counterpart of ovl_dp_lane.hip.
//
// One lane owns one read; the 64 reads of a wavefront sweep the same contig column by column, so the contig's
// symbol is wave-uniform: it comes through the scalar path, one dword per four columns (the host pads every
// contig's start to four bytes).  The read's DP column H[1..ROWS][j] lives in registers (ROWS is the launch's row
// capacity: 32, 64 or 128), its symbols in ROWS / 4 more, four to a register.  No cell waits on another lane, there
// is no LDS and no barrier, and the only stores are one {score, best cell} pair per (read, contig) into a tile
// [contig][read] that the reduction kernel below folds into the per-read results.
//
// Symbols are the host's renumbering of the bytes (0 .. 254); 255 pads a read up to ROWS and matches nothing.
// With mismatch <= 0 and indel <= 0 (the host sends other scorings elsewhere) a padding row's cell is at most a
// cell of the read's last row at the same or an earlier column, and its row index is larger, so it never wins the
// key below: rows beyond the read need no mask.
//
// Best cell: the reference keeps the first strict maximum in row-major fill order (smallest i, then smallest j).
// The sweep is column-major, so a column's cells are folded into key = value << 8 | (255 - i) by an unsigned max,
// and a column replaces the running best only when its key is strictly larger: a larger value, or the same value
// on a smaller row; the same value on the same row in a later column loses.  Values stay below 2^23 (host check).
//
// A read with 0 < len < read_length is aligned to the contig's last len columns (aligners.py:187-195): its lane
// clears its column and its best when the sweep reaches the window's first column; what it computed before is
// never looked at.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ovl_kernels.h"

namespace ovl_local_lane {

template <int ROWS>
__global__ __launch_bounds__(64) void sw_lane_kernel(OvlLocalLaneArgs a) {
    const int lane = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * 64 + lane;  // < a.pitch: the host pads the reads to whole wavefronts
    uint32_t q[ROWS / 4];
    {
        const uint4* qp = reinterpret_cast<const uint4*>(a.reads + r * ROWS);
#pragma unroll
        for (int w = 0; w < ROWS / 16; ++w) {
            const uint4 x = qp[w];
            q[4 * w] = x.x; q[4 * w + 1] = x.y; q[4 * w + 2] = x.z; q[4 * w + 3] = x.w;
        }
    }
    const int32_t n = a.r_len[r];
    const bool tail = n > 0 && n < a.read_length;
    const int32_t match = a.match, mismatch = a.mismatch, indel = a.indel;
    for (int32_t c = a.c_lo + (int32_t)blockIdx.y; c < a.c_hi; c += (int32_t)gridDim.y) {
        const int32_t m = a.c_len[c];
        const uint32_t* cw = reinterpret_cast<const uint32_t*>(a.contigs + a.c_off[c]);
        const int32_t wstart = (tail && m > n) ? m - n : 0;
        int32_t h[ROWS];
#pragma unroll
        for (int i = 0; i < ROWS; ++i) h[i] = 0;
        uint32_t bestkey = 0;
        int32_t bestj = 0;
        uint32_t word = 0;
        for (int32_t j = 0; j < m; ++j) {
            if ((j & 3) == 0) word = __builtin_amdgcn_readfirstlane(cw[j >> 2]);
            const uint32_t sym = word & 0xFFu;
            word >>= 8;
            if (wstart > 0 && j == wstart) {
#pragma unroll
                for (int i = 0; i < ROWS; ++i) h[i] = 0;
                bestkey = 0;
                bestj = 0;
            }
            int32_t diag = 0;  // H[i][j]   (H[0][.] = 0)
            int32_t up = 0;    // H[i][j+1], this column's cell one row up
            uint32_t colkey = 0;
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
                const int32_t left = h[i];
                const uint32_t qs = (q[i >> 2] >> (8 * (i & 3))) & 0xFFu;
                const int32_t d = diag + (qs == sym ? match : mismatch);
                const int32_t g = (up > left ? up : left) + indel;
                int32_t v = d > g ? d : g;
                v = v > 0 ? v : 0;
                h[i] = v;
                diag = left;
                up = v;
                const uint32_t key = ((uint32_t)v << 8) | (uint32_t)(254 - i);
                colkey = key > colkey ? key : colkey;
            }
            const bool better = colkey > bestkey;
            bestkey = better ? colkey : bestkey;
            bestj = better ? j + 1 : bestj;
        }
        const int32_t score = (int32_t)(bestkey >> 8);
        const uint32_t bi = 255u - (bestkey & 0xFFu);
        const int64_t o = (int64_t)(c - a.c_lo) * a.pitch + r;
        a.tile_score[o] = score;
        a.tile_end[o] = score > 0 ? ((bi << 20) | (uint32_t)bestj) : 0u;
    }
}

// One thread per read folds the tile's contigs, in contig order, into the read's running results: the best score,
// the first contig that attains it with its best cell, the count of contigs that attain it and their bits.  A
// strict improvement clears the row's earlier words.  Chunks start at multiples of 32 contigs, so a word of bits
// belongs to one launch.
__global__ __launch_bounds__(256) void read_best_fold_kernel(OvlLocalLaneArgs a, int32_t n_reads, int32_t words,
                                                             int32_t* best, int32_t* first, int32_t* n_best,
                                                             uint32_t* cell, uint32_t* tie_bits) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    int32_t bs = best[r], fb = first[r], nb = n_best[r];
    uint32_t ce = cell[r];
    uint32_t bits = 0;
    uint32_t* row = tie_bits ? tie_bits + r * words : nullptr;
    for (int32_t c = a.c_lo; c < a.c_hi; ++c) {
        const int64_t o = (int64_t)(c - a.c_lo) * a.pitch + r;
        const int32_t s = a.tile_score[o];
        if (fb < 0 || s > bs) {
            bs = s;
            fb = c;
            nb = 1;
            ce = a.tile_end[o];
            bits = 1u << (c & 31);
            if (row)
                for (int32_t w = 0; w < (c >> 5); ++w) row[w] = 0;
        } else if (s == bs) {
            ++nb;
            bits |= 1u << (c & 31);
        }
        if ((c & 31) == 31 || c + 1 == a.c_hi) {
            if (row) row[c >> 5] = bits;
            bits = 0;
        }
    }
    best[r] = bs;
    first[r] = fb;
    n_best[r] = nb;
    cell[r] = ce;
}

}  // namespace ovl_local_lane

extern "C" hipError_t ovl_launch_local_lane(const OvlLocalLaneArgs* a, int32_t rows, int32_t groups, int32_t split,
                                            hipStream_t stream) {
    if (groups <= 0 || split <= 0 || a->c_hi <= a->c_lo) return hipSuccess;
    const dim3 grid((unsigned)groups, (unsigned)split);
    if (rows == 32) ovl_local_lane::sw_lane_kernel<32><<<grid, 64, 0, stream>>>(*a);
    else if (rows == 64) ovl_local_lane::sw_lane_kernel<64><<<grid, 64, 0, stream>>>(*a);
    else if (rows == 128) ovl_local_lane::sw_lane_kernel<128><<<grid, 64, 0, stream>>>(*a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_read_best_fold(const OvlLocalLaneArgs* a, int32_t n_reads, int32_t words,
                                                int32_t* best, int32_t* first, int32_t* n_best, uint32_t* cell,
                                                uint32_t* tie_bits, hipStream_t stream) {
    if (n_reads <= 0 || a->c_hi <= a->c_lo) return hipSuccess;
    ovl_local_lane::read_best_fold_kernel<<<(unsigned)((n_reads + 255) / 256), 256, 0, stream>>>(
        *a, n_reads, words, best, first, n_best, cell, tie_bits);
    return hipGetLastError();
}
