// ovl_consensus_rule.h — what the two consensus entries (ovl_consensus_api.cpp, ovl_consensus_placed_api.cpp) share on
// the host: the channel of a read byte, the pileup of one walk and the call per contig base.  Standard headers only.
#pragma once

#include <algorithm>
#include <cstdint>

inline int32_t channel(uint8_t b) { return b == 'A' ? 0 : (b == 'C' ? 1 : (b == 'G' ? 2 : (b == 'T' ? 3 : -1))); }

// The pileup of one walk from cell (bi, bj): every op votes at the contig base of its cell's column (DP column j is
// base col0 + j - 1) -- a diag in the channel of the read's byte (none for a byte outside ACGT: counted and
// returned), a left in channel 4 (gap), an up in channel 5 (ins: the column at the left of the inserted base).
// vote(k) receives the flat index k = base * 6 + channel.
template <typename Vote>
int64_t pile_ops(const int8_t* ops, int64_t cnt, const uint8_t* q, int32_t bi, int32_t bj, int64_t col0, Vote&& vote) {
    int64_t other = 0;
    int32_t i = bi, j = bj;
    for (int64_t t = 0; t < cnt; ++t) {
        const int64_t at = (col0 + j - 1) * 6;
        if (ops[t] == 1) {
            const int32_t ch = channel(q[i - 1]);
            if (ch >= 0) vote(at + ch);
            else ++other;
            --i;
            --j;
        } else if (ops[t] == 2) {
            vote(at + 5);
            --i;
        } else {
            vote(at + 4);
            --j;
        }
    }
    return other;
}

// The call per contig base: with fewer than min_depth base votes it keeps its byte; else the largest of A, C, G, T
// wins, a tie going to the contig's own byte when it is among the tied and else to the first in that order.
inline uint8_t call_base(const int32_t* v, uint8_t own, int32_t min_depth) {
    if ((int64_t)v[0] + v[1] + v[2] + v[3] < min_depth) return own;
    const int32_t top = std::max(std::max(v[0], v[1]), std::max(v[2], v[3]));
    const int32_t oc = channel(own);
    if (oc >= 0 && v[oc] == top) return own;
    return v[0] == top ? 'A' : (v[1] == top ? 'C' : (v[2] == top ? 'G' : 'T'));
}
