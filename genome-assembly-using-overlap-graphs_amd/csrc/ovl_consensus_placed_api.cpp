// ovl_consensus_placed_api.cpp — placed consensus: every read votes on its contig where the layout placed it
// (include/ovl.h, ovl_consensus_placed: the rule).  The read is aligned only inside the band of 2 * slack + 1
// diagonals around the diagonal that offset[r] names, votes with weight[r], and the rounds run on the contigs as the
// round before called them.  The host form (ovl_consensus_placed_host: the band over ovl_local_host.h's cell statement
// and walk) and the device call (ovl_consensus_placed: ovl_consensus_placed.hip fills, walks and votes, one lane per
// read; ovl_consensus.hip's vote kernel calls the bases; between rounds only the counters cross the link).  The pileup
// and the vote rule are ovl_consensus_rule.h's, shared with ovl_consensus.
#include "ovl_consensus_rule.h"
#include "ovl_local_host.h"

namespace {

constexpr int64_t kSlabBudget = int64_t(256) << 20;  // a chunk's code words (bytes of Dev::pl.slab)

// The window of a placement (rule 1), in int64: no vote when it is empty
struct PlacedWindow {
    int64_t lo, w, d;
};
inline PlacedWindow placed_window(int64_t L, int64_t m, int64_t offset, int64_t slack) {
    const int64_t lo = std::max<int64_t>(0, offset - slack), hi = std::min<int64_t>(m, offset + L + slack);
    return {lo, hi > lo ? hi - lo : 0, offset - lo};
}

template <typename C>
int check_placed(const C* c, bool device, const uint8_t* reads, const int64_t* r_off, int32_t n_reads,
                 const int32_t* weight, const uint8_t* contigs, const int64_t* c_off, int32_t n_contigs,
                 const int32_t* contig, const int32_t* offset, int32_t slack, int32_t match, int32_t mismatch,
                 int64_t indel, int32_t min_vote_score, int32_t min_depth, int32_t rounds, const uint8_t* called,
                 const int64_t* n_changed, const int64_t* n_other, const int64_t* total_changed,
                 const int32_t* rounds_done, int64_t* total) {
    if (n_reads < 0 || n_contigs < 0 || slack < 0) return fail(c, OVL_E_ARG, "negative count or slack");
    if (min_vote_score < 1 || min_depth < 1 || rounds < 1)
        return fail(c, OVL_E_ARG, "min_vote_score %d, min_depth %d, rounds %d: each must be >= 1", min_vote_score,
                    min_depth, rounds);
    if ((n_reads > 0 && (!r_off || !contig || !offset)) || (n_contigs > 0 && !c_off))
        return fail(c, OVL_E_ARG, "NULL offsets or placement");
    if (!n_changed || !n_other || !total_changed || !rounds_done) return fail(c, OVL_E_ARG, "NULL output pointer");
    SeqShape sh;
    if (int rc = check_seq_sets(c, reads, r_off, n_reads, contigs, c_off, n_contigs, &sh)) return rc;
    *total = sh.c_total;
    if (*total > 0 && !called) return fail(c, OVL_E_ARG, "NULL output pointer");
    if (weight)
        for (int32_t r = 0; r < n_reads; ++r)
            if (weight[r] < 0) return fail(c, OVL_E_ARG, "read %d: weight %d < 0", r, weight[r]);
    for (int32_t r = 0; r < n_reads; ++r)
        if (contig[r] < -1 || contig[r] >= n_contigs)
            return fail(c, OVL_E_INDEX, "read %d placed on contig %d outside [-1, %d)", r, contig[r], n_contigs);
    if (*total >= (int64_t(1) << 31))
        return fail(c, OVL_E_UNSUPPORTED, "placed consensus: the contigs together must stay below 2^31 bases");
    if (device && slack > kPlacedMaxSlack)
        return fail(c, OVL_E_UNSUPPORTED, "placed consensus: slack %d > %d on the device (the host form takes any)",
                    slack, kPlacedMaxSlack);
    const int64_t top = std::max<int64_t>(0, std::max<int64_t>(std::max(match, mismatch), clamp_score(indel)));
    int64_t votes = 0;  // no channel can hold more than the sum of weight * length over the placed reads
    for (int32_t r = 0; r < n_reads; ++r) {
        if (contig[r] < 0) continue;
        const int64_t n = r_off[r + 1] - r_off[r], m = c_off[contig[r] + 1] - c_off[contig[r]];
        if (!local_limits_ok(n, m, match))
            return fail(c, OVL_E_UNSUPPORTED,
                        "placed consensus, read %d: lengths < 2^20 and match * min(n, m) < 2^24 required", r);
        votes += (int64_t)(weight ? weight[r] : 1) * n;
        if (votes >= (int64_t(1) << 31))
            return fail(c, OVL_E_UNSUPPORTED, "placed consensus: sum of weight * length reaches 2^31 at read %d", r);
        // the band kernel's int32 cells: a value is a sum over a path of at most n + w steps
        if (device && top * (n + placed_window(n, m, offset[r], slack).w) >= (int64_t(1) << 30))
            return fail(c, OVL_E_UNSUPPORTED,
                        "placed consensus, read %d: positive score * (n + window) must stay below 2^30 on the device",
                        r);
    }
    return OVL_OK;
}

// Rules 2 to 4 for one read on its window t[0 .. w): the codes of the whole (n + 1) x (w + 1) table in `tb` (0 outside
// the band) and the best cell.  The band's diagonals that have a cell, (j - i) - d in [klo, khi], are held as one row
// updated in place, k ascending: the diag neighbour is the row above's k, up its k + 1, left this row's k - 1.
Cell placed_fill_host(const uint8_t* q, int32_t n, const uint8_t* t, int32_t w, int64_t d, int64_t slack,
                      int64_t match, int64_t mismatch, int64_t indel, std::vector<int64_t>& row,
                      std::vector<int8_t>& tb) {
    Cell best{0, 0, 0};
    const size_t pitch = (size_t)w + 1;
    tb.assign(((size_t)n + 1) * pitch, 0);
    const int64_t klo = std::max<int64_t>(-slack, 1 - n - d), khi = std::min<int64_t>(slack, w - 1 - d);
    if (klo > khi) return best;
    const int64_t nk = khi - klo + 1;
    row.assign((size_t)nk + 1, 0);  // (the last entry stays 0: the up neighbour of the band's upper edge)
    for (int32_t i = 1; i <= n; ++i) {
        // column j = i + d + klo + k; the k whose column lies in 1 .. w
        const int64_t base = i + d + klo;
        const int64_t k0 = std::max<int64_t>(0, 1 - base), k1 = std::min<int64_t>(nk - 1, w - base);
        int64_t left = 0;
        int8_t* codes = tb.data() + (size_t)i * pitch;
        for (int64_t k = k0; k <= k1; ++k) {
            const int64_t j = base + k;
            const int64_t dg = row[(size_t)k] + (q[i - 1] == t[j - 1] ? match : mismatch);
            const int64_t u = row[(size_t)k + 1] + indel, l = left + indel;
            int64_t v = 0;
            int8_t op = 0;
            if (dg >= u && dg >= l && dg >= 0) { v = dg; op = 1; }
            else if (u >= l && u >= 0) { v = u; op = 2; }
            else if (l >= 0) { v = l; op = 3; }
            row[(size_t)k] = left = v;
            codes[j] = v > 0 ? op : 0;
            if (v > best.score) best = {v, i, (int32_t)j};
        }
        // (a k whose column has passed w keeps the value of its last cell, column w of the row above: what this
        // row's column w reads as its up neighbour, and no later cell reads again)
    }
    return best;
}

// One round on the host: counts (zeroed here), aln rows of the voting reads, n_other
void placed_round_host(const uint8_t* reads, const int64_t* r_off, int32_t n_reads, const int32_t* weight,
                       const uint8_t* ref, const int64_t* c_off, const int32_t* contig, const int32_t* offset,
                       int32_t slack, int32_t match, int32_t mismatch, int64_t ind, int32_t min_vote_score,
                       int64_t total, int32_t* counts, int32_t* aln, int64_t* n_other, std::vector<int8_t>& tb,
                       std::vector<int8_t>& ops, std::vector<int64_t>& row) {
    std::fill(counts, counts + total * 6, 0);
    if (aln) std::fill(aln, aln + (int64_t)n_reads * 3, 0);
    *n_other = 0;
    for (int32_t r = 0; r < n_reads; ++r) {
        const int32_t f = contig[r], wt = weight ? weight[r] : 1;
        const int32_t L = (int32_t)(r_off[r + 1] - r_off[r]);
        if (f < 0 || L == 0 || wt == 0) continue;
        const int64_t c0 = c_off[f] - c_off[0];
        const PlacedWindow pw = placed_window(L, c_off[f + 1] - c_off[f], offset[r], slack);
        if (pw.w == 0) continue;
        const uint8_t* q = reads + r_off[r];
        const Cell a = placed_fill_host(q, L, ref + c0 + pw.lo, (int32_t)pw.w, pw.d, slack, match, mismatch, ind,
                                        row, tb);
        if (a.score < min_vote_score) continue;
        ops.clear();
        const int32_t sj = sw_walk_host(tb, (int32_t)pw.w, a.bi, a.bj, [&](int8_t op) { ops.push_back(op); });
        *n_other += (int64_t)wt * pile_ops(ops.data(), (int64_t)ops.size(), q, a.bi, a.bj, c0 + pw.lo,
                                           [&](int64_t k) { counts[k] += wt; });
        if (aln) {
            aln[3 * (int64_t)r] = (int32_t)a.score;
            aln[3 * (int64_t)r + 1] = (int32_t)pw.lo + sj;
            aln[3 * (int64_t)r + 2] = (int32_t)pw.lo + a.bj;
        }
    }
}

int64_t count_differences(const uint8_t* a, const uint8_t* b, int64_t n) {
    int64_t d = 0;
    for (int64_t i = 0; i < n; ++i) d += a[i] != b[i];
    return d;
}

}  // namespace

OVL_API int ovl_consensus_placed_host(const uint8_t* reads, const int64_t* r_off, int32_t n_reads,
                                      const int32_t* weight, const uint8_t* contigs, const int64_t* c_off,
                                      int32_t n_contigs, const int32_t* contig, const int32_t* offset, int32_t slack,
                                      int32_t match, int32_t mismatch, int64_t indel, int32_t min_vote_score,
                                      int32_t min_depth, int32_t rounds, int32_t* counts, uint8_t* called,
                                      int64_t* n_changed, int64_t* n_other, int64_t* total_changed,
                                      int32_t* rounds_done, int32_t* aln) {
    const ovl_ctx* none = nullptr;
    int64_t total = 0;
    const int rc = check_placed(none, false, reads, r_off, n_reads, weight, contigs, c_off, n_contigs, contig, offset,
                                slack, match, mismatch, indel, min_vote_score, min_depth, rounds, called, n_changed,
                                n_other, total_changed, rounds_done, &total);
    if (rc != OVL_OK) return rc;
    try {
        std::vector<int32_t> own_counts;
        if (!counts) {
            own_counts.assign((size_t)total * 6, 0);
            counts = own_counts.data();
        }
        const uint8_t* first = total > 0 ? contigs + c_off[0] : nullptr;
        std::vector<uint8_t> ref(first, first + total);
        std::vector<int8_t> tb, ops;
        std::vector<int64_t> row;
        int32_t done = 0;
        do {
            placed_round_host(reads, r_off, n_reads, weight, ref.data(), c_off, contig, offset, slack, match,
                              mismatch, clamp_score(indel), min_vote_score, total, counts, aln, n_other, tb, ops, row);
            *n_changed = 0;
            for (int64_t b = 0; b < total; ++b) {
                called[b] = call_base(counts + b * 6, ref[(size_t)b], min_depth);
                *n_changed += called[b] != ref[(size_t)b];
            }
            std::copy(called, called + total, ref.begin());
            ++done;
        } while (*n_changed != 0 && done < rounds);
        *rounds_done = done;
        *total_changed = count_differences(called, first, total);
    } catch (const std::bad_alloc&) {
        return fail(none, OVL_E_OOM, "no memory for the counts or a traceback table");
    }
    return OVL_OK;
}

OVL_API int ovl_consensus_placed(ovl_ctx* ctx, const uint8_t* reads, const int64_t* r_off, int32_t n_reads,
                                 const int32_t* weight, const uint8_t* contigs, const int64_t* c_off,
                                 int32_t n_contigs, const int32_t* contig, const int32_t* offset, int32_t slack,
                                 int32_t match, int32_t mismatch, int64_t indel, int32_t min_vote_score,
                                 int32_t min_depth, int32_t rounds, int32_t* counts, uint8_t* called,
                                 int64_t* n_changed, int64_t* n_other, int64_t* total_changed, int32_t* rounds_done,
                                 int32_t* aln) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    StageCall call(ctx);
    Dev* c = call.dev;
    int64_t total = 0;
    const int rc = check_placed(c, true, reads, r_off, n_reads, weight, contigs, c_off, n_contigs, contig, offset,
                                slack, match, mismatch, indel, min_vote_score, min_depth, rounds, called, n_changed,
                                n_other, total_changed, rounds_done, &total);
    if (rc != OVL_OK) return rc;
    if (aln) std::fill(aln, aln + (int64_t)n_reads * 3, 0);
    *n_changed = *n_other = *total_changed = 0;
    *rounds_done = 1;
    call.begin();
    c->pl.last = {};
    PlacedState::Last& last = c->pl.last;
    last.rounds = 1;
    if (total == 0) return OVL_OK;  // no base to vote on, and every window is empty

    // the reads that have a window: one item each, in read order
    std::vector<OvlPlacedItem> items;
    try {
        for (int32_t r = 0; r < n_reads; ++r) {
            const int32_t f = contig[r], wt = weight ? weight[r] : 1;
            const int64_t L = r_off[r + 1] - r_off[r];
            if (f < 0 || L == 0 || wt == 0) continue;
            const PlacedWindow pw = placed_window(L, c_off[f + 1] - c_off[f], offset[r], slack);
            if (pw.w == 0) {
                ++last.windowless;
                continue;
            }
            items.push_back({r_off[r] - r_off[0], (int32_t)L, (int32_t)pw.w, (int32_t)pw.d,
                             (int32_t)(c_off[f] - c_off[0] + pw.lo), (int32_t)pw.lo, wt, r, 0});
        }
    } catch (const std::bad_alloc&) {
        return fail(c, OVL_E_OOM, "no memory for the items");
    }
    // chunks of items: what the slab budget holds (rows of the longest item x lanes), and no more reads than the
    // test knob allows
    std::vector<int32_t> cuts{0};
    size_t slab_words = 0;
    for (int32_t i0 = 0; i0 < (int32_t)items.size();) {
        int32_t i1 = i0;
        int64_t rows = 0;
        while (i1 < (int32_t)items.size()) {
            const int64_t rows1 = std::max<int64_t>(rows, items[(size_t)i1].L);
            const int64_t lanes1 = ((int64_t)(i1 - i0 + 1) + 63) / 64 * 64;
            if (i1 > i0 && rows1 * lanes1 * 8 > kSlabBudget) break;
            if (c->k.consensus_chunk > 0 && i1 - i0 >= c->k.consensus_chunk) break;
            rows = rows1;
            ++i1;
        }
        slab_words = std::max(slab_words, (size_t)rows * (size_t)(((int64_t)(i1 - i0) + 63) / 64 * 64));
        cuts.push_back(i1);
        i0 = i1;
    }

    const uint8_t* first = contigs + c_off[0];
    const int64_t r_bytes = n_reads > 0 ? r_off[n_reads] - r_off[0] : 0;
    const size_t o_q = items.size() * sizeof(OvlPlacedItem);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    unsigned long long ctr[5] = {0, 0, 0, 0, 0};
    StreamDrain drain(s);
    HIPCHK(c, ensure(c->cs.ref, (size_t)total));
    HIPCHK(c, ensure(c->cs.counts, sizeof(int32_t) * 6 * (size_t)total));
    HIPCHK(c, ensure(c->cs.called, (size_t)total));
    HIPCHK(c, ensure(c->cs.ctr, 64));
    HIPCHK(c, ensure(c->pl.in, o_q + (size_t)r_bytes));
    HIPCHK(c, ensure(c->pl.slab, slab_words * 8));
    HIPCHK(c, ensure(c->pl.aln, sizeof(int32_t) * 3 * (size_t)std::max(n_reads, 1)));
    HIPCHK(c, c->pl.timer.arm(ctx->timing));
    HIPCHK(c, hipMemcpyAsync(c->cs.ref.p, first, (size_t)total, hipMemcpyHostToDevice, s));
    if (!items.empty()) {
        HIPCHK(c, hipMemcpyAsync(c->pl.in.p, items.data(), o_q, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(as<char>(c->pl.in) + o_q, reads + r_off[0], (size_t)r_bytes, hipMemcpyHostToDevice,
                                 s));
    }
    unsigned long long* d_ctr = as<unsigned long long>(c->cs.ctr);  // {n_other, n_changed, -, voted, ops}

    OvlPlacedArgs p{};
    p.q = as<uint8_t>(c->pl.in) + o_q;
    p.ref = as<uint8_t>(c->cs.ref);
    p.slab = as<unsigned long long>(c->pl.slab);
    p.slack = slack;
    // scores at or below -2^30 are never taken: the cells stay below 2^30 (check_placed)
    const int64_t floor30 = -(int64_t(1) << 30);
    p.match = (int32_t)std::max<int64_t>(match, floor30);
    p.mismatch = (int32_t)std::max<int64_t>(mismatch, floor30);
    p.indel = (int32_t)std::max<int64_t>(clamp_score(indel), floor30);
    p.min_vote_score = min_vote_score;
    p.counts = as<int32_t>(c->cs.counts);
    p.aln = as<int32_t>(c->pl.aln);
    p.ctr = d_ctr;

    int32_t done = 0;
    for (;;) {
        HIPCHK(c, hipMemsetAsync(c->cs.counts.p, 0, sizeof(int32_t) * 6 * (size_t)total, s));
        HIPCHK(c, hipMemsetAsync(c->cs.ctr.p, 0, 64, s));
        HIPCHK(c, hipMemsetAsync(c->pl.aln.p, 0, sizeof(int32_t) * 3 * (size_t)std::max(n_reads, 1), s));
        HIPCHK(c, c->pl.timer.mark(0, s));
        for (size_t k = 0; k + 1 < cuts.size(); ++k) {
            p.items = as<OvlPlacedItem>(c->pl.in) + cuts[k];
            p.n_items = cuts[k + 1] - cuts[k];
            p.pitch = (p.n_items + 63) / 64 * 64;
            HIPCHK(c, ovl_launch_consensus_placed(&p, s));
            ++last.launches;
        }
        HIPCHK(c, c->pl.timer.mark(1, s));
        HIPCHK(c, ovl_launch_consensus_vote(as<uint8_t>(c->cs.ref), as<int32_t>(c->cs.counts), total, min_depth,
                                            as<uint8_t>(c->cs.called), d_ctr, s));
        HIPCHK(c, c->pl.timer.mark(2, s));
        // only the counters cross the link between rounds
        HIPCHK(c, hipMemcpyAsync(ctr, c->cs.ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        last.ms[0] += c->pl.timer.ms(0, 1);
        last.ms[1] += c->pl.timer.ms(1, 2);
        ++done;
        if (ctr[1] == 0 || done >= rounds) break;
        // the called bases are the next round's contigs
        HIPCHK(c, hipMemcpyAsync(c->cs.ref.p, c->cs.called.p, (size_t)total, hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(c, hipMemcpyAsync(called, c->cs.called.p, (size_t)total, hipMemcpyDeviceToHost, s));
    if (counts)
        HIPCHK(c, hipMemcpyAsync(counts, c->cs.counts.p, sizeof(int32_t) * 6 * (size_t)total, hipMemcpyDeviceToHost,
                                 s));
    if (aln && n_reads > 0)
        HIPCHK(c, hipMemcpyAsync(aln, c->pl.aln.p, sizeof(int32_t) * 3 * (size_t)n_reads, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    drain.armed = false;
    *n_other = (int64_t)ctr[0];
    *n_changed = (int64_t)ctr[1];
    *rounds_done = done;
    *total_changed = count_differences(called, first, total);
    last.voted = (int64_t)ctr[3];
    last.ops = (int64_t)ctr[4];
    last.rounds = done;
    return call.done(last.ms[0] + last.ms[1]);
}

OVL_API int ovl_last_consensus_placed(const ovl_ctx* ctx, int64_t* voted_reads, int64_t* windowless_reads,
                                      int64_t* ops, int32_t* launches, int32_t* rounds) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    const PlacedState::Last& l = ctx->devs[0]->pl.last;
    if (voted_reads) *voted_reads = l.voted;
    if (windowless_reads) *windowless_reads = l.windowless;
    if (ops) *ops = l.ops;
    if (launches) *launches = l.launches;
    if (rounds) *rounds = l.rounds;
    return OVL_OK;
}

OVL_API int ovl_last_consensus_placed_timing(const ovl_ctx* ctx, double* band_ms, double* vote_ms) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    if (band_ms) *band_ms = ctx->devs[0]->pl.last.ms[0];
    if (vote_ms) *vote_ms = ctx->devs[0]->pl.last.ms[1];
    return OVL_OK;
}
