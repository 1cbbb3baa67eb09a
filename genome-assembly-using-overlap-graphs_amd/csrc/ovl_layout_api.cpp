// ovl_layout_api.cpp — best-successor layout: contigs straight from the score columns (the rule: include/ovl.h and
// ovl_layout.hip carry its statement).  The host form (ovl_layout_host: one thread that walks the links) and the
// device calls (ovl_layout over uploaded columns, ovl_layout_candidates over the resident candidate list scored into
// device columns), which share one routine from the link kernel on.  The key of a pair and of a head is
// ovl_layout.h's, the same words on both sides.
#include "ovl_ctx.h"
#include "ovl_layout.h"

// The per-read block of the device forms.  The scan's two arrays share the minimum keys' memory (the doubling is over
// when the scan runs).  (Not in the namespace below: tests/c/stage_block_check.cpp carves it without a device.)
void lay_layout_work(Carve& w, OvlLayoutArgs& g, int32_t n, int32_t levels) {
    const size_t N = (size_t)std::max(n, 1);
    g.best = w.take<unsigned long long>(N);
    g.mk[0] = w.take<unsigned long long>(N);
    g.mk[1] = w.take<unsigned long long>(N);
    g.scan_in = reinterpret_cast<int64_t*>(g.mk[0]);
    g.scan_out = reinterpret_cast<int64_t*>(g.mk[1]);
    g.headkey = w.take<unsigned long long>(N);
    g.c_off = w.take<int64_t>(N + 1);
    g.link = w.take<int32_t>(N);
    g.succ = w.take<int32_t>(N);
    g.tail[0] = w.take<uint32_t>(N);
    g.tail[1] = w.take<uint32_t>(N);
    g.contig = w.take<int32_t>(N);
    g.offset = w.take<int32_t>(N);
    g.jump = w.take<int32_t>(N * ((size_t)levels + 1));
    g.on_path = w.take<uint8_t>(N);
    g.on_cycle = w.take<uint8_t>(N);
    g.ctr = w.take<unsigned long long>(8);
}

namespace {

thread_local LayoutState::Last g_host_stats;  // ovl_last_layout(NULL): this thread's last ovl_layout_host

constexpr int64_t kLayoutMax = int64_t(1) << 31;

// The checks every form shares; `a` .. `end` are host columns or, for the resident list, all NULL with n_pairs its
// length (its indices are the enumeration's own).  *total receives sum len.
template <typename C>
int check_layout(const C* c, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, const int32_t* a,
                 const int32_t* b, const int32_t* score, const int32_t* end, int64_t n_pairs, bool host_pairs,
                 int32_t min_overlap, const uint8_t* bases, const int32_t* n_contigs, int64_t* total) {
    if (!n_contigs) return fail(c, OVL_E_ARG, "layout: n_contigs is NULL");
    if (n_reads < 0 || n_pairs < 0) return fail(c, OVL_E_ARG, "layout: negative count");
    if (n_reads > 0 && !offsets) return fail(c, OVL_E_ARG, "layout: offsets is NULL");
    if (host_pairs && n_pairs > 0 && (!a || !b || !score || !end))
        return fail(c, OVL_E_ARG, "layout: a pair column is NULL");
    if (min_overlap < 1) return fail(c, OVL_E_ARG, "layout: min_overlap %d < 1", min_overlap);
    for (int32_t r = 0; r < n_reads; ++r)
        if (offsets[r + 1] < offsets[r]) return fail(c, OVL_E_ARG, "layout: offsets decrease at read %d", r);
    *total = n_reads > 0 ? offsets[n_reads] - offsets[0] : 0;
    if (bases && *total > 0 && !seqs) return fail(c, OVL_E_ARG, "layout: seqs is NULL");
    if (n_pairs >= kLayoutMax) return fail(c, OVL_E_UNSUPPORTED, "layout: fewer than 2^31 pairs required");
    if (*total >= kLayoutMax) return fail(c, OVL_E_UNSUPPORTED, "layout: the reads together must stay below 2^31 bases");
    if (host_pairs)
        for (int64_t p = 0; p < n_pairs; ++p)
            if (a[p] < 0 || a[p] >= n_reads || b[p] < 0 || b[p] >= n_reads)
                return fail(c, OVL_E_INDEX, "layout: pair %lld (%d, %d) outside [0, %d)", (long long)p, a[p], b[p],
                            n_reads);
    return OVL_OK;
}

// What the device routine works on: the reads and the columns, already in device memory.
struct DeviceColumns {
    int32_t n = 0;
    int64_t n_pairs = 0, total = 0;
    const int32_t* len = nullptr;
    const int64_t* off = nullptr;
    const uint8_t* seqs = nullptr;
    const uint8_t* table = nullptr;
    const int32_t *a = nullptr, *b = nullptr, *score = nullptr, *end = nullptr;
};

// ovl_layout's upload block: lengths, offsets from the first read's, the bytes (when contigs are spelled), the columns
void lay_upload(Carve& b, DeviceColumns& d, size_t N, size_t seq_bytes, size_t E) {
    d.len = b.take<int32_t>(N);
    d.off = b.take<int64_t>(N + 1);
    d.seqs = b.take<uint8_t>(seq_bytes);
    d.a = b.take<int32_t>(E);
    d.b = b.take<int32_t>(E);
    d.score = b.take<int32_t>(E);
    d.end = b.take<int32_t>(E);
}

// ovl_layout_candidates' block: the score and end columns, which the scorer fills, and the code table
void lay_scored(Carve& b, DeviceColumns& d, size_t E) {
    d.score = b.take<int32_t>(E);
    d.end = b.take<int32_t>(E);
    d.table = b.take<uint8_t>(256);
}

struct Outputs {
    int32_t *succ, *link, *contig, *offset;
    uint8_t *on_path, *bases;
    int64_t* c_off;
    int32_t* n_contigs;
};

// The fits check of the two forms: their inputs, the per-read block, the contigs' bytes and the scan's scratch (*temp).
int layout_fits(Dev* c, size_t in_bytes, int32_t n, int64_t total, bool spell, size_t* temp) {
    Carve w;
    OvlLayoutArgs g{};
    lay_layout_work(w, g, n, ovl_layout_levels(n));
    *temp = 0;
    if (n > 0) HIPCHK(c, ovl_layout_scan_bytes(n, temp));
    return check_fits(c, "layout", "columns and tables", in_bytes + w.at + (spell ? (size_t)total : 0) + *temp,
                      {&c->ly.in, &c->ly.work, &c->ly.bases, &c->ly.temp});
}

// From the link kernel to the outputs, on c->stream; the timer's marks are recorded from mark 1 on (the caller armed it
// and recorded 0 and 1).  On success the stream is synchronised and the phases' times are read.
int run_layout(Dev* c, const DeviceColumns& in, int32_t min_score, int32_t min_overlap, size_t temp,
               const Outputs& o) {
    hipStream_t s = c->stream;
    const int32_t n = in.n;
    const int32_t levels = ovl_layout_levels(n);
    c->ly.last.levels = levels;
    OvlLayoutArgs g{};
    Carve size;
    lay_layout_work(size, g, n, levels);
    HIPCHK(c, ensure(c->ly.work, size.at));
    if (temp) HIPCHK(c, ensure(c->ly.temp, temp));
    if (o.bases && in.total > 0) HIPCHK(c, ensure(c->ly.bases, (size_t)in.total));
    Carve w(c->ly.work.p);
    lay_layout_work(w, g, n, levels);
    g.n = n;
    g.levels = levels;
    g.n_pairs = in.n_pairs;
    g.len = in.len;
    g.a = in.a;
    g.b = in.b;
    g.score = in.score;
    g.end = in.end;
    g.min_score = min_score;
    g.min_overlap = min_overlap;
    g.seqs = in.seqs;
    g.off = in.off;
    g.table = in.table;
    g.bases = o.bases && in.total > 0 ? as<uint8_t>(c->ly.bases) : nullptr;
    g.bases_cap = in.total;

    unsigned long long ctr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (n > 0) {
        HIPCHK(c, hipMemsetAsync(g.best, 0, sizeof(unsigned long long) * (size_t)n, s));
        HIPCHK(c, hipMemsetAsync(g.ctr, 0, 64, s));
        HIPCHK(c, ovl_launch_layout_link(&g, c->k.layout_runs, s));
        HIPCHK(c, c->ly.timer.mark(2, s));
        HIPCHK(c, ovl_launch_layout_double(&g, 1, s));
        HIPCHK(c, ovl_launch_layout_cut(&g, s));
        HIPCHK(c, hipMemcpyAsync(ctr, g.ctr, 64, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        if (ctr[3] > 0) {  // a cycle stood: the tables again, over the forest that the cuts left
            if (ctr[0] == 0) return fail(c, OVL_E_INTERNAL, "layout: %llu nodes on cycles and no cut", ctr[3]);
            HIPCHK(c, ovl_launch_layout_double(&g, 0, s));
        }
        HIPCHK(c, ovl_launch_layout_place(&g, c->ly.temp.p, c->ly.temp.bytes, s));
        HIPCHK(c, c->ly.timer.mark(3, s));
        HIPCHK(c, ovl_launch_layout_spell(&g, (int32_t)std::min<int64_t>(n, (int64_t)c->cu_count * 32), s));
        HIPCHK(c, c->ly.timer.mark(4, s));
        HIPCHK(c, hipMemcpyAsync(ctr, g.ctr, 64, hipMemcpyDeviceToHost, s));
        const size_t n4 = sizeof(int32_t) * (size_t)n;
        if (o.succ) HIPCHK(c, hipMemcpyAsync(o.succ, g.succ, n4, hipMemcpyDeviceToHost, s));
        if (o.link) HIPCHK(c, hipMemcpyAsync(o.link, g.link, n4, hipMemcpyDeviceToHost, s));
        if (o.contig) HIPCHK(c, hipMemcpyAsync(o.contig, g.contig, n4, hipMemcpyDeviceToHost, s));
        if (o.offset) HIPCHK(c, hipMemcpyAsync(o.offset, g.offset, n4, hipMemcpyDeviceToHost, s));
        if (o.on_path) HIPCHK(c, hipMemcpyAsync(o.on_path, g.on_path, (size_t)n, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        if ((int64_t)ctr[4] > n || (int64_t)ctr[5] > in.total)
            return fail(c, OVL_E_INTERNAL, "layout: %llu contigs of %llu bases from %d reads of %lld", ctr[4], ctr[5],
                        n, (long long)in.total);
        if (o.c_off)
            HIPCHK(c, hipMemcpyAsync(o.c_off, g.c_off, sizeof(int64_t) * ((size_t)ctr[4] + 1), hipMemcpyDeviceToHost,
                                     s));
        if (g.bases && ctr[5] > 0)
            HIPCHK(c, hipMemcpyAsync(o.bases, g.bases, (size_t)ctr[5], hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    } else if (o.c_off) {
        o.c_off[0] = 0;
    }
    *o.n_contigs = (int32_t)ctr[4];
    c->ly.last.cycles = (int64_t)ctr[0];
    c->ly.last.links = (int64_t)ctr[1];
    c->ly.last.on_path = (int64_t)ctr[2];
    if (n > 0)
        for (int i = 0; i < 4; ++i) c->ly.last.ms[i] = c->ly.timer.ms(i, i + 1);
    return OVL_OK;
}

// A layout call's end, whether run_layout succeeded or not: the phases' sum and the clock
int finish(StageCall& call, int rc) {
    const double* ms = call.dev->ly.last.ms;
    call.done(ms[0] + ms[1] + ms[2] + ms[3]);
    return rc;
}

}  // namespace

OVL_API int ovl_layout_host(const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, const int32_t* a,
                            const int32_t* b, const int32_t* score, const int32_t* end, int64_t n_pairs,
                            int32_t min_score, int32_t min_overlap, int32_t* succ_out, int32_t* link_out,
                            int32_t* contig_out, int32_t* offset_out, uint8_t* on_path_out, uint8_t* bases,
                            int64_t* c_off_out, int32_t* n_contigs) {
    const ovl_ctx* none = nullptr;
    int64_t total = 0;
    const int rc = check_layout(none, seqs, offsets, n_reads, a, b, score, end, n_pairs, true, min_overlap, bases,
                                n_contigs, &total);
    if (rc != OVL_OK) return rc;
    g_host_stats = {};
    const size_t n = (size_t)n_reads;
    try {
        auto len = [&](int32_t r) { return (int32_t)(offsets[r + 1] - offsets[r]); };
        // 1, 2: the greatest key per source
        std::vector<unsigned long long> best(n, 0);
        for (int64_t p = 0; p < n_pairs; ++p) {
            if (a[p] == b[p] || score[p] < min_score || end[p] < min_overlap || end[p] >= len(b[p])) continue;
            const unsigned long long k = ovl_layout_key(score[p], (uint32_t)p);
            if (k > best[(size_t)a[p]]) best[(size_t)a[p]] = k;
        }
        std::vector<int32_t> link(n), succ(n);
        for (size_t r = 0; r < n; ++r) {
            link[r] = best[r] ? ovl_layout_key_pair(best[r]) : -1;
            succ[r] = link[r] >= 0 ? b[link[r]] : -1;
        }
        // 3: every walk stamps its reads; a walk that meets its own stamp has closed a cycle, cut at its least key
        std::vector<int32_t> stamp(n, -1);
        for (int32_t r = 0; r < n_reads; ++r) {
            int32_t x = r;
            while (x >= 0 && stamp[(size_t)x] < 0) {
                stamp[(size_t)x] = r;
                x = succ[(size_t)x];
            }
            if (x < 0 || stamp[(size_t)x] != r) continue;
            unsigned long long least = kLayoutNoKey;
            int32_t at = x, y = x;
            do {
                const unsigned long long k = ovl_layout_key(score[link[(size_t)y]], (uint32_t)link[(size_t)y]);
                if (k < least) {
                    least = k;
                    at = y;
                }
                y = succ[(size_t)y];
            } while (y != x);
            link[(size_t)at] = succ[(size_t)at] = -1;
            ++g_host_stats.cycles;
        }
        // 4: roots and tails, each walk unwound from the first read whose root is known
        std::vector<int32_t> root(n, -1), tail(n, 0), walk;
        for (int32_t r = 0; r < n_reads; ++r) {
            int32_t x = r;
            walk.clear();
            while (root[(size_t)x] < 0 && succ[(size_t)x] >= 0) {
                walk.push_back(x);
                x = succ[(size_t)x];
            }
            if (root[(size_t)x] < 0) root[(size_t)x] = x;
            while (!walk.empty()) {
                const int32_t y = walk.back(), t = succ[(size_t)y];
                walk.pop_back();
                root[(size_t)y] = root[(size_t)t];
                tail[(size_t)y] = tail[(size_t)t] + len(t) - end[link[(size_t)y]];
            }
        }
        // 5: the head per root, the contigs in ascending root index
        std::vector<unsigned long long> headkey(n, 0);
        for (int32_t r = 0; r < n_reads; ++r) {
            const unsigned long long k = ovl_layout_head_key(len(r) + tail[(size_t)r], (uint32_t)r);
            unsigned long long& h = headkey[(size_t)root[(size_t)r]];
            if (k > h) h = k;
            g_host_stats.links += succ[(size_t)r] >= 0;
        }
        std::vector<int32_t> rank(n, -1);
        std::vector<int64_t> c_off(1, 0);
        for (int32_t r = 0; r < n_reads; ++r)
            if (succ[(size_t)r] < 0) {
                rank[(size_t)r] = (int32_t)c_off.size() - 1;
                c_off.push_back(c_off.back() + (int64_t)(headkey[(size_t)r] >> 32));
            }
        const int32_t nc = (int32_t)c_off.size() - 1;
        // 6: the placement, the paths and the spelling
        std::vector<uint8_t> on_path(n, 0);
        for (int32_t r = 0; r < n_reads; ++r) {
            if (succ[(size_t)r] >= 0) continue;
            int32_t x = (int32_t)~(uint32_t)headkey[(size_t)r];
            int64_t at = c_off[(size_t)rank[(size_t)r]];
            if (bases) memcpy(bases + at, seqs + offsets[x], (size_t)len(x));
            at += len(x);
            for (;;) {
                on_path[(size_t)x] = 1;
                ++g_host_stats.on_path;
                const int32_t t = succ[(size_t)x];
                if (t < 0) break;
                const int32_t e = end[link[(size_t)x]];
                if (bases) memcpy(bases + at, seqs + offsets[t] + e, (size_t)(len(t) - e));
                at += len(t) - e;
                x = t;
            }
        }
        for (int32_t r = 0; r < n_reads; ++r) {
            const int32_t rt = root[(size_t)r];
            if (succ_out) succ_out[r] = succ[(size_t)r];
            if (link_out) link_out[r] = link[(size_t)r];
            if (contig_out) contig_out[r] = rank[(size_t)rt];
            if (offset_out) offset_out[r] = (int32_t)(headkey[(size_t)rt] >> 32) - (len(r) + tail[(size_t)r]);
            if (on_path_out) on_path_out[r] = on_path[(size_t)r];
        }
        if (c_off_out) std::copy(c_off.begin(), c_off.end(), c_off_out);
        *n_contigs = nc;
    } catch (const std::bad_alloc&) {
        return fail(none, OVL_E_OOM, "layout: no memory for the per-read tables");
    }
    return OVL_OK;
}

OVL_API int ovl_layout(ovl_ctx* ctx, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, const int32_t* a,
                       const int32_t* b, const int32_t* score, const int32_t* end, int64_t n_pairs, int32_t min_score,
                       int32_t min_overlap, int32_t* succ, int32_t* link, int32_t* contig, int32_t* offset,
                       uint8_t* on_path, uint8_t* bases, int64_t* c_off, int32_t* n_contigs) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    StageCall call(ctx);
    Dev* c = call.dev;
    int64_t total = 0;
    int rc = check_layout(c, seqs, offsets, n_reads, a, b, score, end, n_pairs, true, min_overlap, bases, n_contigs,
                          &total);
    if (rc != OVL_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N = (size_t)std::max(n_reads, 1), E = (size_t)n_pairs;
    const bool spell = bases && total > 0;
    DeviceColumns d;
    d.n = n_reads;
    d.n_pairs = n_pairs;
    d.total = total;
    Carve size;
    lay_upload(size, d, N, spell ? (size_t)total : 0, E);
    size_t temp = 0;
    if ((rc = layout_fits(c, size.at, n_reads, total, spell, &temp)) != OVL_OK) return rc;
    call.begin();
    c->ly.last = {};
    std::vector<int32_t> h_len(N, 0);
    std::vector<int64_t> h_off(N + 1, 0);
    for (int32_t r = 0; r < n_reads; ++r) {
        h_len[(size_t)r] = (int32_t)(offsets[r + 1] - offsets[r]);
        h_off[(size_t)r + 1] = offsets[r + 1] - offsets[0];
    }
    hipStream_t s = c->stream;
    HIPCHK(c, ensure(c->ly.in, size.at));
    HIPCHK(c, c->ly.timer.arm(ctx->timing));
    Carve in(c->ly.in.p);
    lay_upload(in, d, N, spell ? (size_t)total : 0, E);
    StreamDrain drain(s);
    HIPCHK(c, hipMemcpyAsync(writable(d.len), h_len.data(), 4 * N, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(writable(d.off), h_off.data(), 8 * (N + 1), hipMemcpyHostToDevice, s));
    if (spell)
        HIPCHK(c, hipMemcpyAsync(writable(d.seqs), seqs + offsets[0], (size_t)total, hipMemcpyHostToDevice, s));
    if (E > 0) {
        HIPCHK(c, hipMemcpyAsync(writable(d.a), a, 4 * E, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(writable(d.b), b, 4 * E, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(writable(d.score), score, 4 * E, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(writable(d.end), end, 4 * E, hipMemcpyHostToDevice, s));
    }
    HIPCHK(c, c->ly.timer.mark(0, s));  // after the uploads; nothing is scored here
    HIPCHK(c, c->ly.timer.mark(1, s));
    rc = run_layout(c, d, min_score, min_overlap, temp,
                    Outputs{succ, link, contig, offset, on_path, bases, c_off, n_contigs});
    drain.armed = rc != OVL_OK;  // (a successful run_layout ends with the stream synchronised)
    c->ly.last.ms[0] = 0.0;      // (two marks with nothing between them)
    return finish(call, rc);
}

OVL_API int ovl_layout_candidates(ovl_ctx* ctx, int32_t match, int32_t mismatch, int64_t indel, int32_t band,
                                  int32_t min_score, int32_t min_overlap, int32_t* succ, int32_t* link,
                                  int32_t* contig, int32_t* offset, uint8_t* on_path, uint8_t* bases, int64_t* c_off,
                                  int32_t* n_contigs) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    StageCall call(ctx);
    Dev* c = call.dev;
    if (c->n_reads < 0 || !ctx->res_valid) return fail(c, OVL_E_STATE, "no resident reads: call ovl_set_reads first");
    if (c->cand_n < 0) return fail(c, OVL_E_STATE, "no candidate list: call ovl_candidates or ovl_seed_candidates first");
    const int32_t n_reads = c->n_reads;
    const int64_t n_pairs = c->cand_n;
    int64_t total = 0;
    // the resident bytes are on the device: `bases` needs no host bytes, so the check sees it as absent
    int rc = check_layout(c, nullptr, ctx->res_off.data(), n_reads, nullptr, nullptr, nullptr, nullptr, n_pairs, false,
                          min_overlap, nullptr, n_contigs, &total);
    if (rc != OVL_OK) return rc;
    Plan p;
    if ((rc = check_scoring_args(ctx, match, mismatch, indel, band, &p)) != OVL_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t E = (size_t)n_pairs;
    const bool spell = bases && total > 0;
    DeviceColumns d;
    d.n = n_reads;
    d.n_pairs = n_pairs;
    d.total = total;
    d.len = as<int32_t>(c->len);
    d.off = as<int64_t>(c->off);
    d.seqs = as<uint8_t>(c->codes);
    d.a = as<int32_t>(c->cand_a);
    d.b = as<int32_t>(c->cand_b);
    Carve size;
    lay_scored(size, d, E);
    size_t temp = 0;
    if ((rc = layout_fits(c, size.at, n_reads, total, spell, &temp)) != OVL_OK) return rc;
    call.begin();
    c->ly.last = {};
    hipStream_t s = c->stream;
    HIPCHK(c, ensure(c->ly.in, size.at));
    Carve in(c->ly.in.p);
    lay_scored(in, d, E);
    StreamDrain drain(s);
    // the resident reads are symbol codes: code k is the k-th byte value of the read set
    HIPCHK(c, hipMemcpyAsync(writable(d.table), ctx->hreads.inv, 256, hipMemcpyHostToDevice, s));
    HIPCHK(c, c->ly.timer.arm(ctx->timing));
    HIPCHK(c, c->ly.timer.mark(0, s));
    if (n_pairs > 0) {
        LaunchIo io;
        rc = launch_score(c, p, {d.a, d.b, n_pairs}, {match, mismatch, indel}, {writable(d.score), writable(d.end)}, io,
                          s);
        if (rc != OVL_OK) return rc;
    }
    HIPCHK(c, c->ly.timer.mark(1, s));
    rc = run_layout(c, d, min_score, min_overlap, temp,
                    Outputs{succ, link, contig, offset, on_path, bases, c_off, n_contigs});
    drain.armed = rc != OVL_OK;
    return finish(call, rc);
}

OVL_API int ovl_last_layout(const ovl_ctx* ctx, int64_t* links, int64_t* cycles, int32_t* levels,
                            int64_t* on_path_reads) {
    const LayoutState::Last& st = ctx ? ctx->devs[0]->ly.last : g_host_stats;
    if (links) *links = st.links;
    if (cycles) *cycles = st.cycles;
    if (levels) *levels = st.levels;
    if (on_path_reads) *on_path_reads = st.on_path;
    return OVL_OK;
}

OVL_API int ovl_last_layout_timing(const ovl_ctx* ctx, double* score_ms, double* link_ms, double* forest_ms,
                                   double* spell_ms) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    const double* ms = ctx->devs[0]->ly.last.ms;
    if (score_ms) *score_ms = ms[0];
    if (link_ms) *link_ms = ms[1];
    if (forest_ms) *forest_ms = ms[2];
    if (spell_ms) *spell_ms = ms[3];
    return OVL_OK;
}
