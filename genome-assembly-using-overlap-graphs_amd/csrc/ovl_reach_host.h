// ovl_reach_host.h — the reachability reduction's rule on one host thread (closure by row-OR Warshall, the positional
// marking) and the marking's node order, shared by ovl_reach_api.cpp and ovl_unitigs_api.cpp.  Host only, header only.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <new>
#include <vector>

// rows * words uint64, or false when the size does not fit or cannot be allocated
inline bool reach_alloc_matrix(std::vector<uint64_t>& m, int64_t rows, int64_t words) {
    if (words > 0 && rows > (int64_t)(SIZE_MAX / sizeof(uint64_t)) / words) return false;
    try {
        m.assign((size_t)(rows * words), 0);
    } catch (const std::bad_alloc&) {
        return false;
    }
    return true;
}

// R[u] = the nodes reachable from u by at least one edge: the adjacency rows, then row-OR Warshall
inline void reach_closure_host(const int64_t* off, const int32_t* head, int32_t n, int64_t words, uint64_t* R) {
    for (int32_t v = 0; v < n; ++v)
        for (int64_t e = off[v]; e < off[v + 1]; ++e) R[v * words + (head[e] >> 6)] |= uint64_t(1) << (head[e] & 63);
    for (int32_t k = 0; k < n; ++k) {
        const uint64_t* rk = R + k * words;
        const int64_t kw = k >> 6;
        const uint64_t kb = uint64_t(1) << (k & 63);
        for (int32_t i = 0; i < n; ++i) {
            uint64_t* ri = R + i * words;
            if (!(ri[kw] & kb) || i == k) continue;
            for (int64_t j = 0; j < words; ++j) ri[j] |= rk[j];
        }
    }
}

// the positional rule over the closure: acc = OR of R[u] over the successors seen so far
inline int64_t reach_mark_host(const int64_t* off, const int32_t* head, int32_t n, int64_t words, const uint64_t* R,
                               uint8_t* reduced) {
    std::vector<uint64_t> acc((size_t)words);
    int64_t count = 0;
    for (int32_t v = 0; v < n; ++v) {
        const int64_t e0 = off[v], e1 = off[v + 1];
        if (e1 - e0 < 2) {
            if (e1 > e0) reduced[e0] = 0;  // a first successor is never removed
            continue;
        }
        std::fill(acc.begin(), acc.end(), 0);
        for (int64_t e = e0; e < e1; ++e) {
            const int32_t w = head[e];
            reduced[e] = (uint8_t)((acc[(size_t)(w >> 6)] >> (w & 63)) & 1u);
            count += reduced[e];
            const uint64_t* rw = R + w * words;
            for (int64_t j = 0; j < words; ++j) acc[(size_t)j] |= rw[j];
        }
    }
    return count;
}

// the marking's dispatch order: nodes with at least two out-edges, heaviest (degree x words) first, ties in node order
inline void reach_mark_order(const int64_t* off, int32_t n, std::vector<int32_t>& order) {
    order.clear();
    for (int32_t v = 0; v < n; ++v)
        if (off[v + 1] - off[v] >= 2) order.push_back(v);
    std::stable_sort(order.begin(), order.end(),
                     [&](int32_t x, int32_t y) { return off[x + 1] - off[x] > off[y + 1] - off[y]; });
}
