// ovl_layout_api.cpp — best-successor layout: contigs straight from the score columns (the rule: include/ovl.h and
// ovl_layout.hip carry its statement).  The host form (ovl_layout_host: one thread that walks the links) and the
// device calls (ovl_layout over uploaded columns, ovl_layout_candidates over the resident candidate list scored into
// device columns), which share one routine from the link kernel on.  The key of a pair and of a head is
// ovl_layout.h's, the same words on both sides.
#include "ovl_ctx.h"
#include "ovl_layout.h"

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

inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

// The per-read block of the device forms: where each table starts, and the block's bytes.  The scan's two arrays
// share the minimum keys' memory (the doubling is over when the scan runs).
struct WorkPlan {
    size_t best, mk0, mk1, headkey, c_off, link, succ, tail0, tail1, contig, offset, jump, on_path, on_cycle, ctr,
        bytes;
    WorkPlan(int32_t n, int32_t levels) {
        const size_t N = (size_t)std::max(n, 1);
        size_t at = 0;
        auto take = [&](size_t b) {
            const size_t o = at;
            at = al256(at + b);
            return o;
        };
        best = take(8 * N);
        mk0 = take(8 * N);
        mk1 = take(8 * N);
        headkey = take(8 * N);
        c_off = take(8 * (N + 1));
        link = take(4 * N);
        succ = take(4 * N);
        tail0 = take(4 * N);
        tail1 = take(4 * N);
        contig = take(4 * N);
        offset = take(4 * N);
        jump = take(4 * N * ((size_t)levels + 1));
        on_path = take(N);
        on_cycle = take(N);
        ctr = take(64);
        bytes = at;
    }
};

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

struct Outputs {
    int32_t *succ, *link, *contig, *offset;
    uint8_t *on_path, *bases;
    int64_t* c_off;
    int32_t* n_contigs;
};

// Device bytes the two forms need beside their inputs: the per-read block, the contigs' bytes and the scan's scratch.
int work_bytes(Dev* c, int32_t n, int64_t total, bool spell, size_t* bytes, size_t* temp) {
    const WorkPlan w(n, ovl_layout_levels(n));
    *temp = 0;
    if (n > 0) HIPCHK(c, ovl_layout_scan_bytes(n, temp));
    *bytes = w.bytes + (spell ? (size_t)total : 0) + *temp;
    return OVL_OK;
}

// OVL_E_UNSUPPORTED when `need` bytes of layout buffers exceed what the device has free plus what those buffers
// already hold
int check_fits(Dev* c, size_t need) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    const size_t held = c->ly.in.bytes + c->ly.work.bytes + c->ly.bases.bytes + c->ly.temp.bytes;
    if (need > free_b + held)
        return fail(c, OVL_E_UNSUPPORTED, "layout: %zu bytes of columns and tables do not fit the device (%zu free)",
                    need, free_b + held);
    return OVL_OK;
}

// From the link kernel to the outputs, on c->stream; the timer's marks are recorded from mark 1 on (the caller armed it
// and recorded 0 and 1).  On success the stream is synchronised and the phases' times are read.
int run_layout(Dev* c, const DeviceColumns& in, int32_t min_score, int32_t min_overlap, size_t temp,
               const Outputs& o) {
    hipStream_t s = c->stream;
    const int32_t n = in.n;
    const int32_t levels = ovl_layout_levels(n);
    c->ly.last.levels = levels;
    const WorkPlan w(n, levels);
    HIPCHK(c, ensure(c->ly.work, w.bytes));
    if (temp) HIPCHK(c, ensure(c->ly.temp, temp));
    if (o.bases && in.total > 0) HIPCHK(c, ensure(c->ly.bases, (size_t)in.total));
    char* base = as<char>(c->ly.work);
    OvlLayoutArgs g{};
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
    g.best = reinterpret_cast<unsigned long long*>(base + w.best);
    g.mk[0] = reinterpret_cast<unsigned long long*>(base + w.mk0);
    g.mk[1] = reinterpret_cast<unsigned long long*>(base + w.mk1);
    g.scan_in = reinterpret_cast<int64_t*>(base + w.mk0);
    g.scan_out = reinterpret_cast<int64_t*>(base + w.mk1);
    g.headkey = reinterpret_cast<unsigned long long*>(base + w.headkey);
    g.c_off = reinterpret_cast<int64_t*>(base + w.c_off);
    g.link = reinterpret_cast<int32_t*>(base + w.link);
    g.succ = reinterpret_cast<int32_t*>(base + w.succ);
    g.tail[0] = reinterpret_cast<uint32_t*>(base + w.tail0);
    g.tail[1] = reinterpret_cast<uint32_t*>(base + w.tail1);
    g.contig = reinterpret_cast<int32_t*>(base + w.contig);
    g.offset = reinterpret_cast<int32_t*>(base + w.offset);
    g.jump = reinterpret_cast<int32_t*>(base + w.jump);
    g.on_path = reinterpret_cast<uint8_t*>(base + w.on_path);
    g.on_cycle = reinterpret_cast<uint8_t*>(base + w.on_cycle);
    g.ctr = reinterpret_cast<unsigned long long*>(base + w.ctr);
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

// From the first copy enqueued to the return: whichever way a device call leaves, the stream is drained before the
// host memory its copies read or write (the call's own vectors, the caller's columns and outputs) can go away.
// Declared after the vectors, so it goes first.
struct StreamDrain {
    hipStream_t s;
    bool armed = true;
    explicit StreamDrain(hipStream_t stream) : s(stream) {}
    ~StreamDrain() {
        if (armed) (void)hipStreamSynchronize(s);
    }
};

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
    // the upload block: lengths, offsets from the first read's, the bytes (when contigs are spelled), the columns
    const size_t N = (size_t)std::max(n_reads, 1), E = (size_t)n_pairs;
    const bool spell = bases && total > 0;
    const size_t o_len = 0, o_off = al256(4 * N), o_seq = al256(o_off + 8 * (N + 1)),
                 o_a = al256(o_seq + (spell ? (size_t)total : 0)), o_b = al256(o_a + 4 * E), o_s = al256(o_b + 4 * E),
                 o_e = al256(o_s + 4 * E), in_bytes = al256(o_e + 4 * E);
    size_t work = 0, temp = 0;
    if ((rc = work_bytes(c, n_reads, total, spell, &work, &temp)) != OVL_OK) return rc;
    if ((rc = check_fits(c, in_bytes + work)) != OVL_OK) return rc;
    call.begin();
    c->ly.last = {};
    std::vector<int32_t> h_len(N, 0);
    std::vector<int64_t> h_off(N + 1, 0);
    for (int32_t r = 0; r < n_reads; ++r) {
        h_len[(size_t)r] = (int32_t)(offsets[r + 1] - offsets[r]);
        h_off[(size_t)r + 1] = offsets[r + 1] - offsets[0];
    }
    hipStream_t s = c->stream;
    HIPCHK(c, ensure(c->ly.in, in_bytes));
    HIPCHK(c, c->ly.timer.arm(ctx->timing));
    char* in = as<char>(c->ly.in);
    StreamDrain drain(s);
    HIPCHK(c, hipMemcpyAsync(in + o_len, h_len.data(), 4 * N, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(in + o_off, h_off.data(), 8 * (N + 1), hipMemcpyHostToDevice, s));
    if (spell) HIPCHK(c, hipMemcpyAsync(in + o_seq, seqs + offsets[0], (size_t)total, hipMemcpyHostToDevice, s));
    if (E > 0) {
        HIPCHK(c, hipMemcpyAsync(in + o_a, a, 4 * E, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(in + o_b, b, 4 * E, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(in + o_s, score, 4 * E, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(in + o_e, end, 4 * E, hipMemcpyHostToDevice, s));
    }
    HIPCHK(c, c->ly.timer.mark(0, s));  // after the uploads; nothing is scored here
    HIPCHK(c, c->ly.timer.mark(1, s));
    DeviceColumns d;
    d.n = n_reads;
    d.n_pairs = n_pairs;
    d.total = total;
    d.len = reinterpret_cast<const int32_t*>(in + o_len);
    d.off = reinterpret_cast<const int64_t*>(in + o_off);
    d.seqs = reinterpret_cast<const uint8_t*>(in + o_seq);
    d.a = reinterpret_cast<const int32_t*>(in + o_a);
    d.b = reinterpret_cast<const int32_t*>(in + o_b);
    d.score = reinterpret_cast<const int32_t*>(in + o_s);
    d.end = reinterpret_cast<const int32_t*>(in + o_e);
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
    const size_t o_s = 0, o_e = al256(4 * E), o_t = al256(o_e + 4 * E), in_bytes = al256(o_t + 256);
    size_t work = 0, temp = 0;
    if ((rc = work_bytes(c, n_reads, total, spell, &work, &temp)) != OVL_OK) return rc;
    if ((rc = check_fits(c, in_bytes + work)) != OVL_OK) return rc;
    call.begin();
    c->ly.last = {};
    hipStream_t s = c->stream;
    HIPCHK(c, ensure(c->ly.in, in_bytes));
    char* in = as<char>(c->ly.in);
    StreamDrain drain(s);
    // the resident reads are symbol codes: code k is the k-th byte value of the read set
    HIPCHK(c, hipMemcpyAsync(in + o_t, ctx->hreads.inv, 256, hipMemcpyHostToDevice, s));
    HIPCHK(c, c->ly.timer.arm(ctx->timing));
    HIPCHK(c, c->ly.timer.mark(0, s));
    if (n_pairs > 0) {
        rc = launch_score(c, p, as<int32_t>(c->cand_a), as<int32_t>(c->cand_b), n_pairs, match, mismatch, indel,
                          reinterpret_cast<int32_t*>(in + o_s), reinterpret_cast<int32_t*>(in + o_e), s);
        if (rc != OVL_OK) return rc;
    }
    HIPCHK(c, c->ly.timer.mark(1, s));
    DeviceColumns d;
    d.n = n_reads;
    d.n_pairs = n_pairs;
    d.total = total;
    d.len = as<int32_t>(c->len);
    d.off = as<int64_t>(c->off);
    d.seqs = as<uint8_t>(c->codes);
    d.table = reinterpret_cast<const uint8_t*>(in + o_t);
    d.a = as<int32_t>(c->cand_a);
    d.b = as<int32_t>(c->cand_b);
    d.score = reinterpret_cast<const int32_t*>(in + o_s);
    d.end = reinterpret_cast<const int32_t*>(in + o_e);
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
