// ovl_consensus_api.cpp — consensus polishing: every placed read is aligned to its contig as
// align_read_or_contig_to_reference does it (aligners.py:170-202, the window rule of ovl_local_host.h), the walks are
// piled up into six vote channels per contig base, and every base with enough votes is called by majority.  The host
// form (ovl_consensus_host, over ovl_local_host.h's fill and walk) and the device call (ovl_consensus: the batch
// kernel's walks stay in device memory and ovl_consensus.hip piles them up and votes there).  The pileup routine and
// the vote rule (ovl_consensus_rule.h) are the one statement both forms share.
#include "ovl_consensus_rule.h"
#include "ovl_local_host.h"

namespace {

constexpr int64_t kOpsBudget = int64_t(256) << 20;  // the walks of one chunk of reads (bytes of Dev::lb_ops)

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
    quiet(ctx);
    Dev* c = ctx->devs[0];
    DeviceGuard guard;
    const auto t_call = std::chrono::steady_clock::now();
    int64_t total = 0;
    const int rc = check_consensus(c, reads, r_off, n_reads, contigs, c_off, n_contigs, place, read_length, match,
                                   min_depth, called, n_changed, n_other, &total);
    if (rc != OVL_OK) return rc;
    zero_aln(aln, n_reads);
    *n_changed = *n_other = 0;
    ctx->x_cs_batch = ctx->x_cs_single = ctx->x_cs_ops = 0;
    ctx->x_cs_launches = 0;
    ctx->x_cs_ms[0] = ctx->x_cs_ms[1] = ctx->x_cs_ms[2] = 0.0;
    ctx->t_kernel_ms = ctx->t_call_ms = 0.0;
    if (total == 0) return OVL_OK;  // no base to vote on, and every window is empty
    const uint8_t* ref = contigs + c_off[0];
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIPCHK(c, ensure(c->cs_ref, (size_t)total));
    HIPCHK(c, ensure(c->cs_counts, sizeof(int32_t) * 6 * (size_t)total));
    HIPCHK(c, ensure(c->cs_called, (size_t)total));
    HIPCHK(c, ensure(c->cs_ctr, 32));
    HIPCHK(c, hipMemcpyAsync(c->cs_ref.p, ref, (size_t)total, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(c->cs_counts.p, 0, sizeof(int32_t) * 6 * (size_t)total, s));
    HIPCHK(c, hipMemsetAsync(c->cs_ctr.p, 0, 32, s));
    if (ctx->timing) HIPCHK(c, ensure_events(c->cs_ev));
    unsigned long long* d_ctr = as<unsigned long long>(c->cs_ctr);  // {n_other, n_changed, bad ops}, pileup's counter
    uint32_t* d_take = reinterpret_cast<uint32_t*>(d_ctr + 3);

    int64_t host_other = 0;
    std::vector<LocalBatchQuery> batch;
    std::vector<int32_t> single;
    std::vector<OvlLocalBatchRecord> res;
    std::vector<int64_t> hits;
    std::vector<int8_t> ops;
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
            LocalBatchRun run;
            if (ctx->timing) HIPCHK(c, hipEventRecord(c->cs_ev[0], s));
            const int rl = local_batch_launch(ctx, c, reads, r_off, batch, nullptr, (int32_t)total,
                                              as<uint8_t>(c->cs_ref), true, match, mismatch, (int32_t)indel, &run);
            if (rl != OVL_OK) return rl;
            if (ctx->timing) HIPCHK(c, hipEventRecord(c->cs_ev[1], s));
            HIPCHK(c, hipMemsetAsync(d_take, 0, sizeof(uint32_t), s));
            OvlPileupArgs p{};
            p.items = as<OvlLocalBatchItem>(c->lb_in);
            p.q = as<uint8_t>(c->lb_in) + run.o_q;
            p.out = as<OvlLocalBatchRecord>(c->lb_out);
            p.ops = as<int8_t>(c->lb_ops);
            p.n_items = run.nb;
            p.counter = d_take;
            p.counts = as<int32_t>(c->cs_counts);
            p.ctr = d_ctr;
            const int32_t waves = (int32_t)std::min<int64_t>(run.nb, (int64_t)c->cu_count * 16);
            HIPCHK(c, ovl_launch_consensus_pileup(&p, waves, s));
            if (ctx->timing) HIPCHK(c, hipEventRecord(c->cs_ev[2], s));
            // the records come back (score and columns for aln, the op counts); the ops stay where they are
            res.resize((size_t)run.nb);
            unsigned long long lb_ctr[2] = {0, 0};
            HIPCHK(c, hipMemcpyAsync(res.data(), c->lb_out.p, res.size() * sizeof(res[0]), hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipMemcpyAsync(lb_ctr, c->lb_ctr.p, sizeof(lb_ctr), hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            if (lb_ctr[1] > (unsigned long long)run.nm_sum)
                return fail(c, OVL_E_INTERNAL, "consensus: %llu ops for a capacity of %lld", lb_ctr[1],
                            (long long)run.nm_sum);
            if (ctx->timing) {
                float ms = 0.f;
                HIPCHK(c, hipEventElapsedTime(&ms, c->cs_ev[0], c->cs_ev[1]));
                ctx->x_cs_ms[0] += ms;
                HIPCHK(c, hipEventElapsedTime(&ms, c->cs_ev[1], c->cs_ev[2]));
                ctx->x_cs_ms[1] += ms;
            }
            for (int32_t b = 0; b < run.nb; ++b) {
                const int32_t r = batch[(size_t)b].k, f = place[r];
                const OvlLocalBatchRecord& o = res[(size_t)b];
                ctx->x_cs_ops += o.n_ops;
                if (aln && o.score > 0) {
                    const int32_t lo = batch[(size_t)b].lo - (int32_t)(c_off[f] - c_off[0]);  // in the contig
                    aln[3 * (int64_t)r] = o.score;
                    aln[3 * (int64_t)r + 1] = lo + o.start_j;
                    aln[3 * (int64_t)r + 2] = lo + o.end_j;
                }
            }
            ctx->x_cs_batch += run.nb;
            ++ctx->x_cs_launches;
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
            ctx->x_cs_ops += n_ops;
            if (aln) {
                aln[3 * (int64_t)r] = sc;
                aln[3 * (int64_t)r + 1] = w.lo + sj;
                aln[3 * (int64_t)r + 2] = w.lo + ej;
            }
        }
        ctx->x_cs_single += (int64_t)single.size();
        if (!hits.empty()) {
            HIPCHK(c, hipSetDevice(c->device));
            HIPCHK(c, ensure(c->cs_hits, sizeof(int64_t) * hits.size()));
            HIPCHK(c, hipMemcpyAsync(c->cs_hits.p, hits.data(), sizeof(int64_t) * hits.size(), hipMemcpyHostToDevice,
                                     s));
            HIPCHK(c, ovl_launch_consensus_add(as<int64_t>(c->cs_hits), (int64_t)hits.size(),
                                               as<int32_t>(c->cs_counts), s));
            HIPCHK(c, hipStreamSynchronize(s));  // `hits` is refilled by the next chunk
        }
        r0 = r1;
    }

    HIPCHK(c, hipSetDevice(c->device));
    if (ctx->timing) HIPCHK(c, hipEventRecord(c->cs_ev[0], s));
    HIPCHK(c, ovl_launch_consensus_vote(as<uint8_t>(c->cs_ref), as<int32_t>(c->cs_counts), total, min_depth,
                                        as<uint8_t>(c->cs_called), d_ctr, s));
    if (ctx->timing) HIPCHK(c, hipEventRecord(c->cs_ev[3], s));
    unsigned long long ctr[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(called, c->cs_called.p, (size_t)total, hipMemcpyDeviceToHost, s));
    if (counts)
        HIPCHK(c, hipMemcpyAsync(counts, c->cs_counts.p, sizeof(int32_t) * 6 * (size_t)total, hipMemcpyDeviceToHost,
                                 s));
    HIPCHK(c, hipMemcpyAsync(ctr, c->cs_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (ctx->timing) {
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->cs_ev[0], c->cs_ev[3]));
        ctx->x_cs_ms[2] = ms;
    }
    if (ctr[2])
        return fail(c, OVL_E_INTERNAL, "consensus: %llu ops of the walks fell outside their alignments", ctr[2]);
    *n_other = (int64_t)ctr[0] + host_other;
    *n_changed = (int64_t)ctr[1];
    ctx->t_kernel_ms = ctx->x_cs_ms[0] + ctx->x_cs_ms[1] + ctx->x_cs_ms[2];
    ctx->t_call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    return OVL_OK;
}

OVL_API int ovl_last_consensus(const ovl_ctx* ctx, int64_t* batch_reads, int64_t* single_reads, int64_t* ops,
                               int32_t* launches) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    if (batch_reads) *batch_reads = ctx->x_cs_batch;
    if (single_reads) *single_reads = ctx->x_cs_single;
    if (ops) *ops = ctx->x_cs_ops;
    if (launches) *launches = ctx->x_cs_launches;
    return OVL_OK;
}

OVL_API int ovl_last_consensus_timing(const ovl_ctx* ctx, double* align_ms, double* pileup_ms, double* vote_ms) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    if (align_ms) *align_ms = ctx->x_cs_ms[0];
    if (pileup_ms) *pileup_ms = ctx->x_cs_ms[1];
    if (vote_ms) *vote_ms = ctx->x_cs_ms[2];
    return OVL_OK;
}
