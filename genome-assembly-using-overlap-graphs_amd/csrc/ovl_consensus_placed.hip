// Placed consensus (ovl_consensus_placed, ovl_consensus_placed_api.cpp): the banded alignment of every read at the
// place the layout gave it, and its votes.  The rule (include/ovl.h):
//
//   window  lo = max(0, offset - slack), hi = min(m, offset + L + slack); t = contig[lo:hi), w = hi - lo,
//           d = offset - lo
//   band    cell (i, j), 1 <= i <= L, 1 <= j <= w, is in the band iff |(j - i) - d| <= slack; row 0, column 0 and
//           every cell outside the band hold value 0 and code 0
//   fill    dg, u, l from the three neighbours; dg >= u && dg >= l && dg >= 0: diag (1); else u >= l && u >= 0: up
//           (2); else l >= 0: left (3); else 0.  The code is kept only where the value is > 0
//   best    the first strict maximum in row-major order; below min_vote_score the read casts no vote
//   walk    from the best cell along the codes until a code 0; every op votes with the read's weight
//
// placed_band_kernel<W>: one lane per read, W >= 2 * slack + 1 diagonals in registers.  Diagonal k of row i is
// column j = i + d - slack + k, so the diag neighbour is the same k of the row above, the up neighbour its k + 1 and
// the left neighbour this row's k - 1: the row is updated in place, k ascending.  A diagonal k > 2 * slack, or a
// column outside 1 .. w, is forced to 0, so both band edges and the window's edges read as 0 on every row.  The
// window's bytes slide through W registers, one new byte per row; the next row's two bytes are loaded before this
// row's cells are computed.  A row's codes are one 64-bit word, stored [row][lane] so that a wavefront's stores are
// one 512-byte run.  The lane then walks its own words back: at most L + w steps, each an int32 atomicAdd of its
// weight (integer sums: the counts do not depend on the order of reads or lanes).  No LDS, no barrier, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ovl_kernels.h"

namespace ovl_consensus_placed {

__device__ __forceinline__ int32_t channel(uint32_t byte) {
    return byte == 'A' ? 0 : (byte == 'C' ? 1 : (byte == 'G' ? 2 : (byte == 'T' ? 3 : -1)));
}

constexpr int32_t kNoByte = 256;  // a window register past the window's ends: equal to no read byte, and marks the
                                  // column as outside 1 .. w

template <int W>
__global__ __launch_bounds__(64) void placed_band_kernel(OvlPlacedArgs a) {
    const int32_t g = (int32_t)blockIdx.x * 64 + (int32_t)threadIdx.x;
    if (g >= a.n_items) return;
    const OvlPlacedItem it = a.items[g];
    const uint8_t* q = a.q + it.q_off;
    const uint8_t* t = a.ref + it.col0;
    const int32_t L = it.L, w = it.w;
    const int32_t nb = 2 * a.slack + 1;   // the live diagonals
    const int32_t j0 = it.d - a.slack;    // diagonal k of row i is column i + j0 + k
    const int32_t match = a.match, mismatch = a.mismatch, indel = a.indel;
    unsigned long long* slab = a.slab + g;
    const size_t pitch = (size_t)a.pitch;

    int32_t row[W], tw[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        row[k] = 0;
        const int32_t at = j0 + k;  // column 1 + j0 + k of row 1 is byte t[j0 + k]
        tw[k] = (at >= 0 && at < w) ? (int32_t)t[at] : kNoByte;
    }
    int32_t best = 0, bi = 0, bk = 0;
    int32_t qb = (int32_t)q[0];  // (L >= 1)
    for (int32_t i = 1; i <= L; ++i) {
        // the next row's bytes: the read's, and the window byte that enters at diagonal W - 1
        const int32_t at = i + j0 + W - 1;
        const int32_t qn = i < L ? (int32_t)q[i] : 0;
        const int32_t tn = (at >= 0 && at < w) ? (int32_t)t[at] : kNoByte;
        unsigned long long word = 0;
        int32_t left = 0;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const int32_t up = k + 1 < W ? row[k + 1] : 0;
            const int32_t dg = row[k] + (qb == tw[k] ? match : mismatch), u = up + indel, l = left + indel;
            int32_t v = 0;
            uint32_t op = 0;
            if (dg >= u && dg >= l && dg >= 0) { v = dg; op = 1; }
            else if (u >= l && u >= 0) { v = u; op = 2; }
            else if (l >= 0) { v = l; op = 3; }
            if (!(k < nb && tw[k] != kNoByte)) v = 0;
            if (v <= 0) op = 0;
            row[k] = left = v;
            word |= (unsigned long long)op << (2 * k);
            if (v > best) { best = v; bi = i; bk = k; }
        }
        slab[(size_t)(i - 1) * pitch] = word;
#pragma unroll
        for (int k = 0; k + 1 < W; ++k) tw[k] = tw[k + 1];
        tw[W - 1] = tn;
        qb = qn;
    }
    if (best < a.min_vote_score) return;

    int32_t i = bi, k = bk, j = bi + j0 + bk;
    const int32_t bj = j;
    const int32_t weight = it.weight;
    uint32_t ops = 0;
    unsigned long long other = 0;
    for (int32_t step = 0; step < L + w; ++step) {
        if (i < 1 || j < 1 || k < 0 || k >= W) break;
        const uint32_t code = (uint32_t)(slab[(size_t)(i - 1) * pitch] >> (2 * k)) & 3u;
        if (code == 0) break;
        int32_t* at = a.counts + ((int64_t)it.col0 + (j - 1)) * 6;
        if (code == 1) {
            const int32_t ch = channel(q[i - 1]);
            if (ch >= 0) atomicAdd(at + ch, weight);
            else other += (unsigned long long)weight;
            --i;
            --j;
        } else if (code == 2) {
            atomicAdd(at + 5, weight);
            --i;
            ++k;
        } else {
            atomicAdd(at + 4, weight);
            --j;
            --k;
        }
        ++ops;
    }
    int32_t* aln = a.aln + (int64_t)it.read * 3;
    aln[0] = best;
    aln[1] = it.lo + j;
    aln[2] = it.lo + bj;
    if (other) atomicAdd(a.ctr + 0, other);
    atomicAdd(a.ctr + 3, 1ull);
    atomicAdd(a.ctr + 4, (unsigned long long)ops);
}

}  // namespace ovl_consensus_placed

extern "C" hipError_t ovl_launch_consensus_placed(const OvlPlacedArgs* a, hipStream_t stream) {
    using namespace ovl_consensus_placed;
    if (a->n_items <= 0) return hipSuccess;
    if (a->slack < 0 || a->slack > kPlacedMaxSlack || a->pitch < a->n_items) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((a->n_items + 63) / 64);
    if (a->slack <= 4) placed_band_kernel<9><<<blocks, 64, 0, stream>>>(*a);
    else if (a->slack <= 8) placed_band_kernel<17><<<blocks, 64, 0, stream>>>(*a);
    else placed_band_kernel<31><<<blocks, 64, 0, stream>>>(*a);
    return hipGetLastError();
}
