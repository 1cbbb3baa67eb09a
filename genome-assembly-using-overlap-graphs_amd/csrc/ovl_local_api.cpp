// ovl_local_api.cpp — single alignments (ovl_ctx.h): one pair's full DP with its traceback table (ovl_align_one)
// and local alignment of two sequences (ovl_local_align, ovl_local.hip) or of many queries against windows of one
// reference (ovl_local_align_batch, ovl_local_batch.hip), routed by ovl_local_host.h's local_route.
#include "ovl_local_host.h"

OVL_API int ovl_align_one(ovl_ctx* ctx, int32_t a, int32_t b, int32_t match, int32_t mismatch, int64_t indel,
                          int32_t* out_score, int32_t* out_end, int8_t* traceback) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    quiet(ctx);
    Dev* c = ctx->devs[0];
    if (!out_score || !out_end) return fail(c, OVL_E_ARG, "NULL output pointer");
    if (c->n_reads < 0) return fail(c, OVL_E_STATE, "no resident reads: call ovl_set_reads first");
    if (a < 0 || a >= c->n_reads || b < 0 || b >= c->n_reads)
        return fail(c, OVL_E_INDEX, "pair (%d, %d) outside [0, %d)", a, b, c->n_reads);
    if (c->lmax > kDpMaxLen) return fail(c, OVL_E_UNSUPPORTED, "DP supports reads up to %d bases", kDpMaxLen);
    DeviceGuard guard;
    HIPCHK(c, hipSetDevice(c->device));
    // lengths from the host-visible offsets copy
    int64_t offs[2][2];
    HIPCHK(c, hipMemcpy(offs[0], as<int64_t>(c->off) + a, 2 * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(offs[1], as<int64_t>(c->off) + b, 2 * sizeof(int64_t), hipMemcpyDeviceToHost));
    const int64_t n = offs[0][1] - offs[0][0], m = offs[1][1] - offs[1][0];
    const size_t cells = (size_t)(n + 1) * (size_t)(m + 1);
    int32_t idx[2] = {a, b}, res[2];
    StreamDrain drain(c->stream);
    HIPCHK(c, ensure(c->a, sizeof(int32_t) * 2));
    HIPCHK(c, ensure(c->score, sizeof(int32_t) * 2));
    if (traceback) {
        HIPCHK(c, ensure(c->tb, cells));
        HIPCHK(c, hipMemsetAsync(c->tb.p, 0, cells, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(c->a.p, idx, sizeof(idx), hipMemcpyHostToDevice, c->stream));
    const int64_t amax = std::max(iabs64(match), iabs64(mismatch));
    const int64_t M = std::max(amax, iabs64(indel));
    const int64_t L = std::max<int32_t>(c->lmax, 1);
    OvlDpArgs g{};
    g.codes = as<uint8_t>(c->codes);
    g.off = as<int64_t>(c->off);
    g.len = as<int32_t>(c->len);
    g.n_reads = c->n_reads;
    g.a_idx = as<int32_t>(c->a);
    g.b_idx = as<int32_t>(c->a) + 1;
    g.n_pairs = 1;
    g.mcap = (int32_t)std::max<int64_t>(m, 1);
    g.match = match;
    g.mismatch = mismatch;
    g.indel = indel;
    g.out_score = as<int32_t>(c->score);
    g.out_end = as<int32_t>(c->score) + 1;
    g.tb = traceback ? as<int8_t>(c->tb) : nullptr;
    g.err_flag = as<uint32_t>(c->err_flag);
    g.wide = !(indel > INT32_MIN && M < (int64_t(1) << 31) && (2 * L + 1) * M < (int64_t(1) << 31));
    g.band = -1;
    HIPCHK(c, ovl_launch_dp(&g, c->stream));
    HIPCHK(c, hipMemcpyAsync(res, c->score.p, sizeof(res), hipMemcpyDeviceToHost, c->stream));
    if (traceback) HIPCHK(c, hipMemcpyAsync(traceback, c->tb.p, cells, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    drain.armed = false;
    *out_score = res[0];
    *out_end = res[1];
    return OVL_OK;
}

OVL_API int ovl_local_align(ovl_ctx* ctx, const uint8_t* query, int32_t n, const uint8_t* ref, int32_t m,
                            int32_t match, int32_t mismatch, int64_t indel, int32_t* out_score, int32_t* out_end_i,
                            int32_t* out_end_j, int32_t* out_start_i, int32_t* out_start_j, int8_t* ops,
                            int64_t ops_cap, int64_t* out_n_ops) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    quiet(ctx);
    Dev* c = ctx->devs[0];
    DeviceGuard guard;
    if (n < 0 || m < 0) return fail(c, OVL_E_ARG, "negative length");
    if ((n > 0 && !query) || (m > 0 && !ref)) return fail(c, OVL_E_ARG, "NULL sequence");
    if (!out_score || !out_end_i || !out_end_j || !out_start_i || !out_start_j || !out_n_ops)
        return fail(c, OVL_E_ARG, "NULL output pointer");
    if (ops && ops_cap < 0) return fail(c, OVL_E_ARG, "ops_cap < 0");
    if (!local_limits_ok(n, m, match))
        return fail(c, OVL_E_UNSUPPORTED, "local alignment: lengths < 2^20 and match * min(n, m) < 2^24 required");
    *out_score = 0; *out_end_i = 0; *out_end_j = 0; *out_start_i = 0; *out_start_j = 0; *out_n_ops = 0;
    if (n == 0 || m == 0) return OVL_OK;
    const int wide = local_wide(n, m, match, mismatch, indel) ? 1 : 0;
    const int32_t n_strips = (int32_t)local_strips(n);
    const int64_t steps = local_steps(m);  // traceback pitch per strip
    const size_t tb_bytes = local_table_bytes(n, m);
    const size_t row_bytes = (size_t)n_strips * (size_t)(steps + 64) * sizeof(uint64_t);
    if (ops && tb_bytes > (size_t(8) << 30))
        return fail(c, OVL_E_UNSUPPORTED, "local alignment traceback table would exceed 8 GiB");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIPCHK(c, ensure(c->l_q, (size_t)n));
    HIPCHK(c, ensure(c->l_r, (size_t)m));
    if (c->l_row.bytes < row_bytes) {
        // fresh words must not carry a live epoch: zero on (re)allocation, epochs start at 1
        HIPCHK(c, ensure(c->l_row, row_bytes));
        HIPCHK(c, hipMemsetAsync(c->l_row.p, 0, c->l_row.bytes, s));
        c->l_epoch = 0;
    }
    if (++c->l_epoch == 0) {  // 2^32 launches: start over from zeroed words
        HIPCHK(c, hipMemsetAsync(c->l_row.p, 0, c->l_row.bytes, s));
        c->l_epoch = 1;
    }
    HIPCHK(c, ensure(c->l_best, 16));
    if (ops) HIPCHK(c, ensure(c->l_tb, tb_bytes));
    unsigned long long key = 0;
    uint32_t flag = 0;
    StreamDrain drain(s);
    HIPCHK(c, hipMemcpyAsync(c->l_q.p, query, (size_t)n, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->l_r.p, ref, (size_t)m, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(c->l_best.p, 0, 16, s));
    HIPCHK(c, hipMemsetAsync(c->err_flag.p, 0, sizeof(uint32_t), s));
    // strips round-robin over at most 8 one-wavefront blocks per CU: far below residency, so every
    // strip's producer is a resident wavefront (the hand-off polls would otherwise never end)
    const int32_t blocks = std::min<int32_t>(n_strips, c->cu_count * 8);
    HIPCHK(c, ovl_launch_local(as<uint8_t>(c->l_q), n, as<uint8_t>(c->l_r), m, match, mismatch, indel, wide,
                               as<uint64_t>(c->l_row), ops ? as<int8_t>(c->l_tb) : nullptr,
                               as<unsigned long long>(c->l_best), as<uint32_t>(c->err_flag), blocks, c->l_epoch, s));
    HIPCHK(c, hipMemcpyAsync(&key, c->l_best.p, sizeof(key), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&flag, c->err_flag.p, sizeof(flag), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    drain.armed = false;  // (the table's corner below goes into the device's own pinned buffer)
    if (flag) {
        HIPCHK(c, hipMemset(c->err_flag.p, 0, sizeof(uint32_t)));
        return fail(c, OVL_E_HIP, "local alignment: a row hand-off timed out (flag %u)", flag);
    }
    int32_t bi = 0, bj = 0, score = 0;
    if (key) {
        score = (int32_t)(key >> 40);
        bi = (int32_t)(0xFFFFFu - (uint32_t)((key >> 20) & 0xFFFFF));
        bj = (int32_t)(0xFFFFFu - (uint32_t)(key & 0xFFFFF));
    }
    *out_score = score;
    *out_end_i = bi;
    *out_end_j = bj;
    int32_t i = bi, j = bj;
    int64_t k = 0;
    if (ops && bi > 0 && bj > 0) {
        // the walk moves up and left from (bi, bj): it reads strips 0 .. (bi-1)/64 and, in each,
        // steps j + L - 1 <= bj + 62.  Only that corner of the table comes back, as one strided copy
        // into a pinned buffer (the whole table is ~22 MB at contig x PhiX scale).
        const size_t n_st = (size_t)((bi - 1) >> 6) + 1;
        const size_t w = (size_t)(bj + 63) * 64;  // bytes of steps 0 .. bj + 62 in one strip
        const size_t need = n_st * w;
        if (c->l_tb_host_bytes < need) {
            if (c->l_tb_host) (void)hipHostFree(c->l_tb_host);
            c->l_tb_host = nullptr;
            c->l_tb_host_bytes = 0;
            HIPCHK(c, hipHostMalloc((void**)&c->l_tb_host, need, hipHostMallocDefault));
            c->l_tb_host_bytes = need;
        }
        HIPCHK(c, hipMemcpy2DAsync(c->l_tb_host, w, c->l_tb.p, (size_t)steps * 64, w, n_st, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        const int8_t* tb = c->l_tb_host;
        // aligners.py:133-153: walk while i > 0, j > 0 and dp[i][j] > 0
        while (i > 0 && j > 0) {
            const int32_t st = (i - 1) >> 6, L = (i - 1) & 63;
            const int8_t code = tb[(size_t)st * w + (size_t)(j + L - 1) * 64 + (size_t)L];
            if (!(code & 4)) break;
            const int8_t op = code & 3;
            if (op == 1) { --i; --j; }
            else if (op == 2) { --i; }
            else if (op == 3) { --j; }
            else break;
            if (k < ops_cap) ops[k] = op;
            ++k;
        }
    }
    *out_start_i = i;
    *out_start_j = j;
    *out_n_ops = k;
    if (ops && k > ops_cap) return fail(c, OVL_E_RANGE, "ops_cap %lld < walk length %lld", (long long)ops_cap,
                                        (long long)k);
    return OVL_OK;
}

// One launch of the batch kernel, issued and not waited for (ovl_local_host.h): the records and the packed ops stay in
// device memory for the caller -- ovl_local_align_batch copies them back, ovl_consensus piles them up in place.
int local_batch_launch(ovl_ctx* ctx, Dev* c, const uint8_t* queries, const int64_t* q_off,
                       std::vector<LocalBatchQuery>& batch, const uint8_t* reference, int32_t ref_len,
                       const uint8_t* d_reference, bool with_ops, int32_t match, int32_t mismatch, int32_t indel,
                       LocalBatchRun* run) {
    // long queries first: the wavefronts that take the short ones last even the launch's tail out
    std::stable_sort(batch.begin(), batch.end(),
                     [](const LocalBatchQuery& x, const LocalBatchQuery& y) { return x.cost > y.cost; });
    const int32_t nb = (int32_t)batch.size();
    size_t slab_max = 0;
    int64_t row_max = 0, nm_max = 0, nm_sum = 0, q_bytes = 0;
    for (const LocalBatchQuery& x : batch) {
        slab_max = std::max(slab_max, local_table_bytes(x.n, x.m));
        row_max = std::max(row_max, local_steps(x.m));
        nm_max = std::max<int64_t>(nm_max, (int64_t)x.n + x.m);
        nm_sum += (int64_t)x.n + x.m;
        q_bytes += x.n;
    }
    const size_t slab_pitch = (slab_max + 255) & ~size_t(255);
    int64_t waves = std::min<int64_t>(nb, (int64_t)c->cu_count * kBatchWavesPerCu);
    if (with_ops) waves = std::min<int64_t>(waves, std::max<int64_t>(1, (int64_t)(kBatchSlabBudget / slab_pitch)));
    if (c->k.local_batch_waves > 0) waves = std::min<int64_t>(waves, c->k.local_batch_waves);
    const bool row_lds = row_max <= kBatchLdsRow;
    const int64_t wops_pitch = (nm_max + 63) & ~int64_t(63);
    // one upload block: the items, the batched queries' bytes, the reference (unless it is on the device already)
    const size_t o_q = sizeof(OvlLocalBatchItem) * (size_t)nb, o_r = o_q + (size_t)q_bytes;
    std::vector<char>& blob = run->blob;
    blob.assign(o_r + (d_reference ? 0 : (size_t)ref_len), 0);
    OvlLocalBatchItem* items = reinterpret_cast<OvlLocalBatchItem*>(blob.data());
    int64_t qo = 0;
    for (int32_t b = 0; b < nb; ++b) {
        const LocalBatchQuery& x = batch[b];
        items[b] = {qo, x.n, x.lo, x.m, b};
        memcpy(blob.data() + o_q + qo, queries + q_off[x.k], (size_t)x.n);
        qo += x.n;
    }
    if (!d_reference) memcpy(blob.data() + o_r, reference, (size_t)ref_len);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIPCHK(c, ensure(c->lb.in, blob.size()));
    HIPCHK(c, ensure(c->lb.ctr, 16));
    HIPCHK(c, ensure(c->lb.out, sizeof(OvlLocalBatchRecord) * (size_t)nb));
    if (!row_lds) HIPCHK(c, ensure(c->lb.rows, sizeof(int32_t) * (size_t)row_max * (size_t)waves));
    if (with_ops) {
        HIPCHK(c, ensure(c->lb.slabs, slab_pitch * (size_t)waves));
        HIPCHK(c, ensure(c->lb.wops, (size_t)wops_pitch * (size_t)waves));
        HIPCHK(c, ensure(c->lb.ops, (size_t)nm_sum));
    }
    HIPCHK(c, hipMemcpyAsync(c->lb.in.p, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(c->lb.ctr.p, 0, 16, s));
    OvlLocalBatchArgs a{};
    a.items = as<OvlLocalBatchItem>(c->lb.in);
    a.q = as<uint8_t>(c->lb.in) + o_q;
    a.ref = d_reference ? d_reference : as<uint8_t>(c->lb.in) + o_r;
    a.n_items = nb;
    a.match = match;
    a.mismatch = mismatch;
    a.indel = indel;
    a.counter = as<uint32_t>(c->lb.ctr);
    a.ops_total = reinterpret_cast<unsigned long long*>(as<char>(c->lb.ctr) + 8);
    a.rows = row_lds ? nullptr : as<int32_t>(c->lb.rows);
    a.row_pitch = row_lds ? 0 : row_max;
    a.slabs = with_ops ? as<int8_t>(c->lb.slabs) : nullptr;
    a.slab_pitch = (int64_t)slab_pitch;
    a.wave_ops = with_ops ? as<int8_t>(c->lb.wops) : nullptr;
    a.wave_ops_pitch = wops_pitch;
    a.out = as<OvlLocalBatchRecord>(c->lb.out);
    a.ops = with_ops ? as<int8_t>(c->lb.ops) : nullptr;
    HIPCHK(c, c->lb.timer.arm(ctx->timing));
    HIPCHK(c, c->lb.timer.mark(0, s));
    HIPCHK(c, ovl_launch_local_batch(&a, (int32_t)waves, row_lds ? (uint32_t)(row_max * 4) : 0u, s));
    HIPCHK(c, c->lb.timer.mark(1, s));
    run->o_q = o_q;
    run->nb = nb;
    run->waves = (int32_t)waves;
    run->nm_sum = nm_sum;
    return OVL_OK;
}

// Many queries against windows of one reference in one call (ovl_local_batch.hip): every query that fits one
// wavefront goes through one launch of the batch kernel; the rest (long, wide-scoring or with a traceback table
// beyond kBatchSlabMax) go through ovl_local_align afterwards.
OVL_API int ovl_local_align_batch(ovl_ctx* ctx, const uint8_t* queries, const int64_t* q_off, int32_t n_queries,
                                  const uint8_t* reference, int32_t ref_len, const int32_t* win_lo,
                                  const int32_t* win_len, int32_t match, int32_t mismatch, int64_t indel,
                                  int32_t* out_score, int32_t* out_end_i, int32_t* out_end_j, int32_t* out_start_i,
                                  int32_t* out_start_j, int8_t* ops, const int64_t* ops_off, int64_t* out_n_ops) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    StageCall call(ctx);
    Dev* c = call.dev;
    if (n_queries < 0 || ref_len < 0) return fail(c, OVL_E_ARG, "negative count or length");
    if (n_queries > 0 && !q_off) return fail(c, OVL_E_ARG, "q_off is NULL");
    if ((win_lo == nullptr) != (win_len == nullptr))
        return fail(c, OVL_E_ARG, "win_lo and win_len must both be given or both be NULL");
    if (n_queries > 0 && (!out_score || !out_end_i || !out_end_j || !out_start_i || !out_start_j || !out_n_ops))
        return fail(c, OVL_E_ARG, "NULL output pointer");
    if (ops && !ops_off) return fail(c, OVL_E_ARG, "ops without ops_off");
    // every argument check comes before anything is written or run
    for (int32_t k = 0; k < n_queries; ++k) {
        const int64_t n = q_off[k + 1] - q_off[k];
        if (q_off[k] < 0 || n < 0) return fail(c, OVL_E_ARG, "query %d: bad offsets", k);
        const int64_t lo = win_lo ? win_lo[k] : 0, m = win_lo ? win_len[k] : ref_len;
        if (lo < 0 || m < 0 || lo + m > ref_len)
            return fail(c, OVL_E_ARG, "query %d: window [%lld, %lld) outside the reference of %d", k, (long long)lo,
                        (long long)(lo + m), ref_len);
        if ((n > 0 && !queries) || (m > 0 && !reference)) return fail(c, OVL_E_ARG, "NULL sequence");
        if (ops && ops_off[k + 1] - ops_off[k] < n + m)
            return fail(c, OVL_E_ARG, "query %d: ops slot of %lld < n + m = %lld", k,
                        (long long)(ops_off[k + 1] - ops_off[k]), (long long)(n + m));
    }
    for (int32_t k = 0; k < n_queries; ++k) {
        const int64_t n = q_off[k + 1] - q_off[k], m = win_lo ? win_len[k] : ref_len;
        if (!local_limits_ok(n, m, match))
            return fail(c, OVL_E_UNSUPPORTED,
                        "local alignment, query %d: lengths < 2^20 and match * min(n, m) < 2^24 required", k);
    }
    call.begin();
    c->lb.last = {};
    double kernel_ms = 0.0;  // the batch kernel
    // route the queries: the slab limit holds only where a traceback is asked for
    std::vector<LocalBatchQuery> batch;
    std::vector<int32_t> single;
    for (int32_t k = 0; k < n_queries; ++k) {
        out_score[k] = 0; out_end_i[k] = 0; out_end_j[k] = 0; out_start_i[k] = 0; out_start_j[k] = 0;
        out_n_ops[k] = 0;
        const int64_t n = q_off[k + 1] - q_off[k], m = win_lo ? win_len[k] : ref_len;
        const LocalRoute route = local_route(n, m, match, mismatch, indel, ops != nullptr);
        if (route == LocalRoute::Single)
            single.push_back(k);
        else if (route == LocalRoute::Batch)
            batch.push_back({k, (int32_t)n, win_lo ? win_lo[k] : 0, (int32_t)m, n * m});
    }
    if (!batch.empty()) {
        LocalBatchRun run;
        std::vector<OvlLocalBatchRecord> res(batch.size());
        std::vector<int8_t> packed;
        unsigned long long ctr[2] = {0, 0};
        StreamDrain drain(c->stream);  // (local_batch_launch returns with the blob's copy in flight)
        // |indel| < 2^30 here: wider scorings went to `single`
        const int rl = local_batch_launch(ctx, c, queries, q_off, batch, reference, ref_len, nullptr, ops != nullptr,
                                          match, mismatch, (int32_t)indel, &run);
        if (rl != OVL_OK) return rl;
        hipStream_t s = c->stream;
        const int32_t nb = run.nb;
        const int64_t nm_sum = run.nm_sum;
        HIPCHK(c, hipMemcpyAsync(res.data(), c->lb.out.p, res.size() * sizeof(res[0]), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(ctr, c->lb.ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        kernel_ms = c->lb.timer.ms(0, 1);
        const unsigned long long total = ctr[1];
        if (total > (unsigned long long)nm_sum)
            return fail(c, OVL_E_INTERNAL, "batched local alignment: %llu ops for a capacity of %lld", total,
                        (long long)nm_sum);
        packed.resize((size_t)total);
        if (total) {
            HIPCHK(c, hipMemcpyAsync(packed.data(), c->lb.ops.p, (size_t)total, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
        }
        drain.armed = false;
        for (int32_t b = 0; b < nb; ++b) {
            const int32_t k = batch[b].k;
            const OvlLocalBatchRecord& o = res[(size_t)b];
            out_score[k] = o.score; out_end_i[k] = o.end_i; out_end_j[k] = o.end_j;
            out_start_i[k] = ops ? o.start_i : o.end_i;
            out_start_j[k] = ops ? o.start_j : o.end_j;
            if (ops && o.n_ops > 0) {
                const unsigned long long base = o.ops_base();
                if (base + (unsigned long long)o.n_ops > total || o.n_ops > batch[b].n + batch[b].m)
                    return fail(c, OVL_E_INTERNAL, "batched local alignment: query %d's ops lie outside the buffer", k);
                memcpy(ops + ops_off[k], packed.data() + base, (size_t)o.n_ops);
                out_n_ops[k] = o.n_ops;
            }
        }
        c->lb.last.batched = nb;
        c->lb.last.waves = run.waves;
    }
    for (int32_t k : single) {
        const int32_t n = (int32_t)(q_off[k + 1] - q_off[k]);
        const int32_t lo = win_lo ? win_lo[k] : 0, m = win_lo ? win_len[k] : ref_len;
        const int rc = ovl_local_align(ctx, queries + q_off[k], n, reference + lo, m, match, mismatch, indel,
                                       out_score + k, out_end_i + k, out_end_j + k, out_start_i + k, out_start_j + k,
                                       ops ? ops + ops_off[k] : nullptr, ops ? ops_off[k + 1] - ops_off[k] : 0,
                                       out_n_ops + k);
        if (rc != OVL_OK) return rc;
    }
    c->lb.last.single = (int32_t)single.size();
    return call.done(kernel_ms);
}

OVL_API int ovl_last_local_batch(const ovl_ctx* ctx, int32_t* batched, int32_t* single, int32_t* waves) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    const LocalBatchState::Last& l = ctx->devs[0]->lb.last;
    if (batched) *batched = l.batched;
    if (single) *single = l.single;
    if (waves) *waves = l.waves;
    return OVL_OK;
}
