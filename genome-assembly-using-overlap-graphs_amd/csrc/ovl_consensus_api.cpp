// ovl_consensus_api.cpp — consensus polishing: every placed read is aligned to its contig as
// align_read_or_contig_to_reference does it (aligners.py:170-202, the window rule of ovl_local_host.h), the walks are
// piled up into six vote channels per contig base, and every base with enough votes is called by majority.  The host
// form (ovl_consensus_host, over ovl_local_host.h's fill and walk) and the device call (ovl_consensus: the batch
// kernel's walks stay in device memory and ovl_consensus.hip piles them up and votes there).  The pileup routine and
// the vote rule (ovl_consensus_rule.h) are the one statement both forms share.
#include "ovl_consensus_rule.h"
#include "ovl_local_host.h"

namespace {

constexpr int64_t kOpsBudget = int64_t(256) << 20;  // the walks of one chunk of reads (bytes of Dev::lb.ops)

template <typename C>
int check_consensus(const C* c, const uint8_t* reads, const int64_t* r_off, int32_t n_reads, const uint8_t* contigs,
                    const int64_t* c_off, int32_t n_contigs, const int32_t* place, int32_t read_length, int32_t match,
                    int32_t min_depth, const uint8_t* called, const int64_t* n_changed, const int64_t* n_other,
                    int64_t* total) {
    if (int rc = check_seq_counts(c, n_reads, n_contigs, read_length)) return rc;
    if (min_depth < 1) return fail(c, OVL_E_ARG, "min_depth %d < 1", min_depth);
    if ((n_reads > 0 && (!r_off || !place)) || (n_contigs > 0 && !c_off))
        return fail(c, OVL_E_ARG, "NULL offsets or placement");
    if (!n_changed || !n_other) return fail(c, OVL_E_ARG, "NULL output pointer");
    SeqShape sh;
    if (int rc = check_seq_sets(c, reads, r_off, n_reads, contigs, c_off, n_contigs, &sh)) return rc;
    *total = sh.c_total;
    if (*total > 0 && !called) return fail(c, OVL_E_ARG, "NULL output pointer");
    for (int32_t r = 0; r < n_reads; ++r)
        if (place[r] < -1 || place[r] >= n_contigs)
            return fail(c, OVL_E_INDEX, "read %d placed on contig %d outside [-1, %d)", r, place[r], n_contigs);
    if (*total >= (int64_t(1) << 31))
        return fail(c, OVL_E_UNSUPPORTED, "consensus: the contigs together must stay below 2^31 bases");
    for (int32_t r = 0; r < n_reads; ++r) {
        if (place[r] < 0) continue;
        const int64_t n = r_off[r + 1] - r_off[r], m = c_off[place[r] + 1] - c_off[place[r]];
        // the lengths of the read and its whole contig, the product over its window
        if (!local_limits_ok(n, m, 0) || !local_limits_ok(n, window_of(n, m, read_length).len, match))
            return fail(c, OVL_E_UNSUPPORTED,
                        "consensus, read %d: lengths < 2^20 and match * min(n, m) < 2^24 required", r);
    }
    return OVL_OK;
}

void zero_aln(int32_t* aln, int32_t n_reads) {
    if (aln) std::fill(aln, aln + (int64_t)n_reads * 3, 0);
}

}  // namespace

OVL_API int ovl_consensus_host(const uint8_t* reads, const int64_t* r_off, int32_t n_reads, const uint8_t* contigs,
                               const int64_t* c_off, int32_t n_contigs, const int32_t* place, int32_t read_length,
                               int32_t match, int32_t mismatch, int64_t indel, int32_t min_depth, int32_t* counts,
                               uint8_t* called, int64_t* n_changed, int64_t* n_other, int32_t* aln) {
    const ovl_ctx* none = nullptr;
    int64_t total = 0;
    const int rc = check_consensus(none, reads, r_off, n_reads, contigs, c_off, n_contigs, place, read_length, match,
                                   min_depth, called, n_changed, n_other, &total);
    if (rc != OVL_OK) return rc;
    zero_aln(aln, n_reads);
    *n_changed = *n_other = 0;
    try {
        std::vector<int32_t> own_counts;
        if (!counts) {
            own_counts.assign((size_t)total * 6, 0);
            counts = own_counts.data();
        } else {
            std::fill(counts, counts + total * 6, 0);
        }
        const int64_t ind = clamp_score(indel);
        std::vector<int8_t> tb, ops;
        std::vector<int64_t> row;
        for (int32_t r = 0; r < n_reads; ++r) {
            const int32_t f = place[r];
            if (f < 0) continue;
            const uint8_t* q = reads + r_off[r];
            const int32_t L = (int32_t)(r_off[r + 1] - r_off[r]);
            const Window w = window_of(L, c_off[f + 1] - c_off[f], read_length);
            if (L == 0 || w.len == 0) continue;
            const Cell a = sw_fill_host<true>(q, L, contigs + c_off[f] + w.lo, w.len, match, mismatch, ind, row, &tb);
            if (a.score <= 0) continue;
            ops.clear();
            const int32_t sj = sw_walk_host(tb, w.len, a.bi, a.bj, [&](int8_t op) { ops.push_back(op); });
            *n_other += pile_ops(ops.data(), (int64_t)ops.size(), q, a.bi, a.bj, (c_off[f] - c_off[0]) + w.lo,
                                 [&](int64_t k) { ++counts[k]; });
            if (aln) {
                aln[3 * (int64_t)r] = (int32_t)a.score;
                aln[3 * (int64_t)r + 1] = w.lo + sj;
                aln[3 * (int64_t)r + 2] = w.lo + a.bj;
            }
        }
        const uint8_t* ref = contigs + (n_contigs > 0 ? c_off[0] : 0);
        for (int64_t b = 0; b < total; ++b) {
            called[b] = call_base(counts + b * 6, ref[b], min_depth);
            *n_changed += called[b] != ref[b];
        }
    } catch (const std::bad_alloc&) {
        return fail(none, OVL_E_OOM, "no memory for the counts or a traceback table");
    }
    return OVL_OK;
}

OVL_API int ovl_consensus(ovl_ctx* ctx, const uint8_t* reads, const int64_t* r_off, int32_t n_reads,
                          const uint8_t* contigs, const int64_t* c_off, int32_t n_contigs, const int32_t* place,
                          int32_t read_length, int32_t match, int32_t mismatch, int64_t indel, int32_t min_depth,
                          int32_t* counts, uint8_t* called, int64_t* n_changed, int64_t* n_other, int32_t* aln) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    StageCall call(ctx);
    Dev* c = call.dev;
    int64_t total = 0;
    const int rc = check_consensus(c, reads, r_off, n_reads, contigs, c_off, n_contigs, place, read_length, match,
                                   min_depth, called, n_changed, n_other, &total);
    if (rc != OVL_OK) return rc;
    zero_aln(aln, n_reads);
    *n_changed = *n_other = 0;
    call.begin();
    c->cs.last = {};
    ConsensusState::Last& last = c->cs.last;
    if (total == 0) return OVL_OK;  // no base to vote on, and every window is empty
    const uint8_t* ref = contigs + c_off[0];
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    // what the copies below read or fill, ahead of the drain
    int64_t host_other = 0;
    std::vector<LocalBatchQuery> batch;
    std::vector<int32_t> single;
    std::vector<OvlLocalBatchRecord> res;
    std::vector<int64_t> hits;
    std::vector<int8_t> ops;
    LocalBatchRun run;  // (local_batch_launch returns with its blob's copy in flight)
    unsigned long long lb_ctr[2] = {0, 0}, ctr[3] = {0, 0, 0};
    StreamDrain drain(s);
    HIPCHK(c, ensure(c->cs.ref, (size_t)total));
    HIPCHK(c, ensure(c->cs.counts, sizeof(int32_t) * 6 * (size_t)total));
    HIPCHK(c, ensure(c->cs.called, (size_t)total));
    HIPCHK(c, ensure(c->cs.ctr, 32));
    HIPCHK(c, hipMemcpyAsync(c->cs.ref.p, ref, (size_t)total, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(c->cs.counts.p, 0, sizeof(int32_t) * 6 * (size_t)total, s));
    HIPCHK(c, hipMemsetAsync(c->cs.ctr.p, 0, 32, s));
    HIPCHK(c, c->cs.timer.arm(ctx->timing));
    unsigned long long* d_ctr = as<unsigned long long>(c->cs.ctr);  // {n_other, n_changed, bad ops}, pileup's counter
    uint32_t* d_take = reinterpret_cast<uint32_t*>(d_ctr + 3);

    for (int32_t r0 = 0; r0 < n_reads;) {
        // a chunk of reads: what the ops budget holds (and no more reads than the test knob allows)
        int32_t r1 = r0;
        int64_t budget = 0;
        batch.clear();
        single.clear();
        hits.clear();
        while (r1 < n_reads) {
            const int32_t f = place[r1];
            const int64_t L = r_off[r1 + 1] - r_off[r1];
            const Window w = f < 0 ? Window{0, 0, 0} : window_of(L, c_off[f + 1] - c_off[f], read_length);
            // an unplaced read, an empty one or an empty window casts no vote; the others always have a traceback
            const LocalRoute route =
                f < 0 ? LocalRoute::Empty : local_route(L, w.len, match, mismatch, indel, true);
            const bool votes = route != LocalRoute::Empty;
            if (votes && r1 > r0 && budget + L + w.len > kOpsBudget) break;
            if (c->k.consensus_chunk > 0 && r1 - r0 >= c->k.consensus_chunk) break;
            if (votes) budget += L + w.len;
            if (route == LocalRoute::Single)
                single.push_back(r1);
            else if (route == LocalRoute::Batch)
                batch.push_back({r1, (int32_t)L, (int32_t)(c_off[f] - c_off[0]) + w.lo, w.len, L * w.len});
            ++r1;
        }
        if (!batch.empty()) {
            HIPCHK(c, c->cs.timer.mark(0, s));
            const int rl = local_batch_launch(ctx, c, reads, r_off, batch, nullptr, (int32_t)total,
                                              as<uint8_t>(c->cs.ref), true, match, mismatch, (int32_t)indel, &run);
            if (rl != OVL_OK) return rl;
            HIPCHK(c, c->cs.timer.mark(1, s));
            HIPCHK(c, hipMemsetAsync(d_take, 0, sizeof(uint32_t), s));
            OvlPileupArgs p{};
            p.items = as<OvlLocalBatchItem>(c->lb.in);
            p.q = as<uint8_t>(c->lb.in) + run.o_q;
            p.out = as<OvlLocalBatchRecord>(c->lb.out);
            p.ops = as<int8_t>(c->lb.ops);
            p.n_items = run.nb;
            p.counter = d_take;
            p.counts = as<int32_t>(c->cs.counts);
            p.ctr = d_ctr;
            const int32_t waves = (int32_t)std::min<int64_t>(run.nb, (int64_t)c->cu_count * 16);
            HIPCHK(c, ovl_launch_consensus_pileup(&p, waves, s));
            HIPCHK(c, c->cs.timer.mark(2, s));
            // the records come back (score and columns for aln, the op counts); the ops stay where they are
            res.resize((size_t)run.nb);
            HIPCHK(c, hipMemcpyAsync(res.data(), c->lb.out.p, res.size() * sizeof(res[0]), hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipMemcpyAsync(lb_ctr, c->lb.ctr.p, sizeof(lb_ctr), hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            if (lb_ctr[1] > (unsigned long long)run.nm_sum)
                return fail(c, OVL_E_INTERNAL, "consensus: %llu ops for a capacity of %lld", lb_ctr[1],
                            (long long)run.nm_sum);
            last.ms[0] += c->cs.timer.ms(0, 1);
            last.ms[1] += c->cs.timer.ms(1, 2);
            for (int32_t b = 0; b < run.nb; ++b) {
                const int32_t r = batch[(size_t)b].k, f = place[r];
                const OvlLocalBatchRecord& o = res[(size_t)b];
                last.ops += o.n_ops;
                if (aln && o.score > 0) {
                    const int32_t lo = batch[(size_t)b].lo - (int32_t)(c_off[f] - c_off[0]);  // in the contig
                    aln[3 * (int64_t)r] = o.score;
                    aln[3 * (int64_t)r + 1] = lo + o.start_j;
                    aln[3 * (int64_t)r + 2] = lo + o.end_j;
                }
            }
            last.batch += run.nb;
            ++last.launches;
        }
        // the reads the batch kernel does not take: one by one, their walks piled up by the host form's routine
        for (int32_t r : single) {
            const int32_t f = place[r], L = (int32_t)(r_off[r + 1] - r_off[r]);
            const Window w = window_of(L, c_off[f + 1] - c_off[f], read_length);
            ops.resize((size_t)L + (size_t)w.len);
            int32_t sc = 0, ei = 0, ej = 0, si = 0, sj = 0;
            int64_t n_ops = 0;
            const int ra = ovl_local_align(ctx, reads + r_off[r], L, contigs + c_off[f] + w.lo, w.len, match, mismatch,
                                           indel, &sc, &ei, &ej, &si, &sj, ops.data(), (int64_t)ops.size(), &n_ops);
            if (ra != OVL_OK) return ra;
            if (sc <= 0) continue;
            host_other += pile_ops(ops.data(), n_ops, reads + r_off[r], ei, ej, (c_off[f] - c_off[0]) + w.lo,
                                   [&](int64_t k) { hits.push_back(k); });
            last.ops += n_ops;
            if (aln) {
                aln[3 * (int64_t)r] = sc;
                aln[3 * (int64_t)r + 1] = w.lo + sj;
                aln[3 * (int64_t)r + 2] = w.lo + ej;
            }
        }
        last.single += (int64_t)single.size();
        if (!hits.empty()) {
            HIPCHK(c, hipSetDevice(c->device));
            HIPCHK(c, ensure(c->cs.hits, sizeof(int64_t) * hits.size()));
            HIPCHK(c, hipMemcpyAsync(c->cs.hits.p, hits.data(), sizeof(int64_t) * hits.size(), hipMemcpyHostToDevice,
                                     s));
            HIPCHK(c, ovl_launch_consensus_add(as<int64_t>(c->cs.hits), (int64_t)hits.size(),
                                               as<int32_t>(c->cs.counts), s));
            HIPCHK(c, hipStreamSynchronize(s));  // `hits` is refilled by the next chunk
        }
        r0 = r1;
    }

    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->cs.timer.mark(0, s));
    HIPCHK(c, ovl_launch_consensus_vote(as<uint8_t>(c->cs.ref), as<int32_t>(c->cs.counts), total, min_depth,
                                        as<uint8_t>(c->cs.called), d_ctr, s));
    HIPCHK(c, c->cs.timer.mark(3, s));
    HIPCHK(c, hipMemcpyAsync(called, c->cs.called.p, (size_t)total, hipMemcpyDeviceToHost, s));
    if (counts)
        HIPCHK(c, hipMemcpyAsync(counts, c->cs.counts.p, sizeof(int32_t) * 6 * (size_t)total, hipMemcpyDeviceToHost,
                                 s));
    HIPCHK(c, hipMemcpyAsync(ctr, c->cs.ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    drain.armed = false;
    last.ms[2] = c->cs.timer.ms(0, 3);
    if (ctr[2])
        return fail(c, OVL_E_INTERNAL, "consensus: %llu ops of the walks fell outside their alignments", ctr[2]);
    *n_other = (int64_t)ctr[0] + host_other;
    *n_changed = (int64_t)ctr[1];
    return call.done(last.ms[0] + last.ms[1] + last.ms[2]);
}

OVL_API int ovl_last_consensus(const ovl_ctx* ctx, int64_t* batch_reads, int64_t* single_reads, int64_t* ops,
                               int32_t* launches) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    const ConsensusState::Last& l = ctx->devs[0]->cs.last;
    if (batch_reads) *batch_reads = l.batch;
    if (single_reads) *single_reads = l.single;
    if (ops) *ops = l.ops;
    if (launches) *launches = l.launches;
    return OVL_OK;
}

OVL_API int ovl_last_consensus_timing(const ovl_ctx* ctx, double* align_ms, double* pileup_ms, double* vote_ms) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    const double* ms = ctx->devs[0]->cs.last.ms;
    if (align_ms) *align_ms = ms[0];
    if (pileup_ms) *pileup_ms = ms[1];
    if (vote_ms) *vote_ms = ms[2];
    return OVL_OK;
}
