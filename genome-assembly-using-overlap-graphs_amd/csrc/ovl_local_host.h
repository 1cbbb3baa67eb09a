// ovl_local_host.h — the host side of local alignment (the reference's local_alignment, aligners.py:85-167, and
// align_read_or_contig_to_reference, aligners.py:170-202) that ovl_local_api.cpp (single and batched alignment),
// ovl_depth_api.cpp (read depth) and ovl_consensus_api.cpp (consensus) share: the window rule, the one host statement
// of the cell rule and the walk, the best-cell key limit, the argument checks of a read set against a contig set, and
// the rule that routes a query to the batch kernel or to sw_kernel.
#pragma once

#include "ovl_ctx.h"

// ovl_local_align_batch: a query stays on the batch kernel (one wavefront per query) up to this many 64-row
// strips and this large a traceback table of its own; all slabs of a launch together stay inside the budget,
// which caps the wavefront count; the carried row lives in LDS up to this many int32
constexpr int32_t kBatchMaxStrips = 16;
constexpr size_t kBatchSlabMax = size_t(64) << 20;
constexpr size_t kBatchSlabBudget = size_t(4) << 30;
constexpr int64_t kBatchLdsRow = 8192;
constexpr int32_t kBatchWavesPerCu = 8;

// The window of contig length m that a read of length L is aligned to, and what is added to window-relative
// positions (aligners.py:187-195): a read shorter than read_length takes the contig's last L bases -- the whole
// contig when L is 0 or above m, as the reference's slice [-L:] does -- and is shifted by m - L in every case.
struct Window {
    int32_t lo, len;
    int64_t shift;
};
inline Window window_of(int64_t L, int64_t m, int32_t read_length) {
    if (L >= read_length) return {0, (int32_t)m, 0};
    const int64_t wl = (L > 0 && L < m) ? L : m;
    return {(int32_t)(m - wl), (int32_t)wl, m - L};
}

// One launch of the batch kernel as its callers describe and receive it (local_batch_launch, ovl_local_api.cpp)
struct LocalBatchQuery {
    int32_t k, n, lo, m;  // caller's query index, its length, its window of the reference
    int64_t cost;
};
struct LocalBatchRun {
    std::vector<char> blob;  // the upload block: alive until the stream has been synchronised
    size_t o_q = 0;          // offset of the queries' bytes in it (and in Dev::lb.in)
    int32_t nb = 0, waves = 0;
    int64_t nm_sum = 0;      // capacity of Dev::lb.ops
};

// ovl_local_api.cpp: the batch kernel over `batch` (routed by the caller: every query fits the kernel), issued on
// the device's stream and not waited for.  It sorts `batch` by descending cost; query batch[b] becomes item b, whose
// OvlLocalBatchRecord is Dev::lb.out[b] and whose ops (with_ops) lie packed in Dev::lb.ops, their total at
// Dev::lb.ctr + 8.  The windows are of `reference` (host, uploaded behind the queries) or, when d_reference is not
// NULL, of that device copy of it.
int local_batch_launch(ovl_ctx* ctx, Dev* c, const uint8_t* queries, const int64_t* q_off,
                       std::vector<LocalBatchQuery>& batch, const uint8_t* reference, int32_t ref_len,
                       const uint8_t* d_reference, bool with_ops, int32_t match, int32_t mismatch, int32_t indel,
                       LocalBatchRun* run);

// scores at or below -2^40 all mean "never taken" for cells below 2^24, and keep int64 sums far from overflow
inline int64_t clamp_score(int64_t v) {
    const int64_t lim = int64_t(1) << 40;
    return v < -lim ? -lim : (v > lim ? lim : v);
}

struct Cell {
    int64_t score;
    int32_t bi, bj;
};

// aligners.py:106-137 over q[0..n) x t[0..m) with one carried row: the best score and the first strict maximum.
// TB: the traceback table too ((n + 1) x (m + 1) codes in `tb`: 1 diag, 2 up, 3 left, 0 where the cell is 0).
template <bool TB>
Cell sw_fill_host(const uint8_t* q, int32_t n, const uint8_t* t, int32_t m, int64_t match, int64_t mismatch,
                  int64_t indel, std::vector<int64_t>& row, std::vector<int8_t>* tb) {
    Cell best{0, 0, 0};
    const size_t pitch = (size_t)m + 1;
    if constexpr (TB) tb->assign(((size_t)n + 1) * pitch, 0);
    row.assign(pitch, 0);
    for (int32_t i = 1; i <= n; ++i) {
        int64_t diag = 0, left = 0;
        int8_t* codes = TB ? tb->data() + (size_t)i * pitch : nullptr;
        for (int32_t j = 1; j <= m; ++j) {
            const int64_t upv = row[(size_t)j];
            const int64_t d = diag + (q[i - 1] == t[j - 1] ? match : mismatch), u = upv + indel, l = left + indel;
            int64_t v = 0;
            int8_t op = 0;
            if (d >= u && d >= l && d >= 0) { v = d; op = 1; }
            else if (u >= l && u >= 0) { v = u; op = 2; }
            else if (l >= 0) { v = l; op = 3; }
            diag = upv;
            row[(size_t)j] = left = v;
            if constexpr (TB) codes[j] = v > 0 ? op : 0;
            if (v > best.score) best = {v, i, j};
        }
    }
    return best;
}

// aligners.py:139-161 over that table from (bi, bj): on_op(op) for every op in walk order; the column where the
// walk stops
template <typename OnOp>
int32_t sw_walk_host(const std::vector<int8_t>& tb, int32_t m, int32_t bi, int32_t bj, OnOp&& on_op) {
    const size_t pitch = (size_t)m + 1;
    int32_t i = bi, j = bj;
    while (i > 0 && j > 0) {
        const int8_t op = tb[(size_t)i * pitch + (size_t)j];
        if (op == 1) { --i; --j; }
        else if (op == 2) --i;
        else if (op == 3) --j;
        else break;
        on_op(op);
    }
    return j;
}

// (the best-cell key limit, local_limits_ok: ovl_score_range.h)

// The argument checks that every stage over a read set and a contig set shares, in the two places where they stand
// in each stage's order: the counts first, and, after the stage's own pointer checks, the offsets and the bytes.
struct SeqShape {
    int64_t max_n = 0, max_m = 0, c_total = 0;
};
template <typename C>
int check_seq_counts(const C* c, int32_t n_reads, int32_t n_contigs, int32_t read_length) {
    if (n_reads < 0 || n_contigs < 0 || read_length < 0) return fail(c, OVL_E_ARG, "negative count or read_length");
    return OVL_OK;
}
template <typename C>
int check_seq_sets(const C* c, const uint8_t* reads, const int64_t* r_off, int32_t n_reads, const uint8_t* contigs,
                   const int64_t* c_off, int32_t n_contigs, SeqShape* sh) {
    if (n_reads > 0 && r_off[0] < 0) return fail(c, OVL_E_ARG, "r_off[0] < 0");
    if (n_contigs > 0 && c_off[0] < 0) return fail(c, OVL_E_ARG, "c_off[0] < 0");
    for (int32_t r = 0; r < n_reads; ++r) {
        const int64_t n = r_off[r + 1] - r_off[r];
        if (n < 0) return fail(c, OVL_E_ARG, "read %d: offsets decrease", r);
        sh->max_n = std::max(sh->max_n, n);
    }
    for (int32_t k = 0; k < n_contigs; ++k) {
        const int64_t m = c_off[k + 1] - c_off[k];
        if (m < 0) return fail(c, OVL_E_ARG, "contig %d: offsets decrease", k);
        sh->max_m = std::max(sh->max_m, m);
    }
    if (n_contigs > 0) sh->c_total = c_off[n_contigs] - c_off[0];
    if ((sh->max_n > 0 && !reads) || (sh->max_m > 0 && !contigs)) return fail(c, OVL_E_ARG, "NULL sequence");
    return OVL_OK;
}

// The geometry of sw_kernel and sw_batch_kernel: 64-row strips of the query, 64-step chunks covering the steps
// tau = 0 .. m + 62 of a strip (the traceback pitch per strip), and the table's bytes, [strip][tau][lane]
inline int64_t local_strips(int64_t n) { return (n + 63) / 64; }
inline int64_t local_steps(int64_t m) { return (m + 126) / 64 * 64; }
inline size_t local_table_bytes(int64_t n, int64_t m) {
    return (size_t)local_strips(n) * (size_t)local_steps(m) * 64;
}
// (cells beyond int32, local_wide: ovl_score_range.h -- sw_kernel's wide form, and never the batch kernel)

// Where a query of n bases against a window of m goes: nowhere (Empty: every result is 0), through the batch kernel
// with the others, or alone through sw_kernel (ovl_local_align) -- wide scoring, more strips than one wavefront
// sweeps, or, where a traceback is wanted, a table beyond a slab.  local_batch_launch takes only Batch queries.
enum class LocalRoute { Empty, Batch, Single };
inline LocalRoute local_route(int64_t n, int64_t m, int64_t match, int64_t mismatch, int64_t indel, bool with_ops) {
    if (n == 0 || m == 0) return LocalRoute::Empty;
    if (local_wide(n, m, match, mismatch, indel) || local_strips(n) > kBatchMaxStrips ||
        (with_ops && local_table_bytes(n, m) > kBatchSlabMax))
        return LocalRoute::Single;
    return LocalRoute::Batch;
}
