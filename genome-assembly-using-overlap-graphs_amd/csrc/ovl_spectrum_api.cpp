// ovl_spectrum_api.cpp — k-mer spectrum read correction (the rule: include/ovl.h and ovl_spectrum.hip carry its
// statement).  The host forms (ovl_kmer_spectrum_host, ovl_correct_reads_host: one thread, no limits on the reads) and
// the device calls (ovl_kmer_spectrum, ovl_correct_reads), which share one routine up to the spectrum in device
// memory.  The code of a byte and the field a substitution replaces are ovl_spectrum.h's, the same words on both sides.
#include "ovl_ctx.h"
#include "ovl_spectrum.h"

// The call's upload: the reads' offsets from the first read's, their windows' offsets, the bytes.  (This block and the
// next are not in the namespace below: tests/c/stage_block_check.cpp carves them without a device.)
void lay_spectrum_in(Carve& b, OvlSpectrumArgs& g, int32_t n_reads, int64_t total) {
    const size_t N = (size_t)std::max(n_reads, 1);
    g.off = b.take<int64_t>(N + 1);
    g.woff = b.take<int64_t>(N + 1);
    g.seqs = b.take<uint8_t>((size_t)std::max<int64_t>(total, 1));
}

// The tables beside the upload; returns the last, the sort's and the scan's scratch.
void* lay_spectrum_work(Carve& w, OvlSpectrumArgs& g, int32_t n_reads, int64_t n_win, int64_t total, size_t temp_bytes,
                        bool correct) {
    const size_t W = (size_t)std::max<int64_t>(n_win, 1), N = (size_t)std::max(n_reads, 1);
    g.keys = w.take<uint64_t>(W + 1);  // the windows' keys; after the sort, the spectrum's keys
    g.spec_keys = g.keys;              // (the scatter reads `sorted`: the unsorted keys are done with)
    g.sorted = w.take<uint64_t>(W);
    g.flag = w.take<int32_t>(W);
    g.pos = w.take<int32_t>(W);
    g.starts = w.take<int32_t>(W + 2);
    g.spec_counts = w.take<int32_t>(W + 1);
    g.hist = w.take<uint32_t>((size_t)kSpecHistBins);
    g.ctr = w.take<unsigned long long>(8);
    g.out = w.take<uint8_t>(correct ? (size_t)std::max<int64_t>(total, 1) : 1);
    g.changed = w.take<int32_t>(correct ? N : 1);
    return w.take<char>(temp_bytes);
}

namespace {

constexpr int64_t kSpecMax = int64_t(1) << 31;

// The checks every form shares.  *n_win receives the number of windows, *max_win the most of one read, *long_read the
// first read with more than kSpecMaxWindows windows (-1: none).
template <typename C>
int check_reads(const C* c, const char* what, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, int32_t k,
                int64_t* n_win, int32_t* max_win, int32_t* long_read) {
    if (n_reads < 0) return fail(c, OVL_E_ARG, "%s: n_reads %d < 0", what, n_reads);
    if (k < 1 || k > kSpecMaxK) return fail(c, OVL_E_ARG, "%s: k %d outside [1, %d]", what, k, kSpecMaxK);
    if (!offsets) return fail(c, OVL_E_ARG, "%s: offsets is NULL", what);
    for (int32_t r = 0; r < n_reads; ++r)
        if (offsets[r + 1] < offsets[r]) return fail(c, OVL_E_ARG, "%s: offsets decrease at read %d", what, r);
    if (n_reads > 0 && offsets[n_reads] > offsets[0] && !seqs) return fail(c, OVL_E_ARG, "%s: seqs is NULL", what);
    *n_win = 0;
    *max_win = 0;
    *long_read = -1;
    for (int32_t r = 0; r < n_reads; ++r) {
        const int64_t w = std::max<int64_t>(offsets[r + 1] - offsets[r] - k + 1, 0);
        *n_win += w;
        if (w > kSpecMaxWindows && *long_read < 0) *long_read = r;
        *max_win = (int32_t)std::min<int64_t>(std::max<int64_t>(*max_win, w), INT32_MAX);
    }
    return OVL_OK;
}

// every window's key in read order, ~0 for a window without one
void host_keys(const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, int32_t k, std::vector<uint64_t>& keys) {
    const uint64_t mask = (1ull << (2 * k)) - 1ull;
    size_t at = 0;
    for (int32_t r = 0; r < n_reads; ++r) {
        const int64_t len = offsets[r + 1] - offsets[r];
        if (len < k) continue;
        const uint8_t* s = seqs + offsets[r];
        uint64_t key = 0;
        int32_t good = 0;
        for (int64_t q = 0; q < len; ++q) {
            ovl_spec_roll(key, good, s[q], mask);
            if (good > k) good = k;  // (no overflow on long reads)
            if (q >= k - 1) keys[at++] = good >= k ? key : kSpecNoKey;
        }
    }
}

struct Spectrum {
    std::vector<uint64_t> keys;
    std::vector<int32_t> counts;
    int64_t kmers = 0;
    bool solid(uint64_t key, int32_t min_count) const {
        const auto it = std::lower_bound(keys.begin(), keys.end(), key);
        return it != keys.end() && *it == key && counts[(size_t)(it - keys.begin())] >= min_count;
    }
};

// OVL_E_UNSUPPORTED when one key occurs 2^31 times or more (its count is an int32)
int host_spectrum(std::vector<uint64_t> sorted, Spectrum* sp) {
    std::sort(sorted.begin(), sorted.end());
    const size_t n = sorted.size();
    for (size_t i = 0; i < n && sorted[i] != kSpecNoKey;) {
        size_t j = i + 1;
        while (j < n && sorted[j] == sorted[i]) ++j;
        if ((int64_t)(j - i) >= kSpecMax) return OVL_E_UNSUPPORTED;
        sp->keys.push_back(sorted[i]);
        sp->counts.push_back((int32_t)(j - i));
        sp->kmers += (int64_t)(j - i);
        i = j;
    }
    return OVL_OK;
}

// the threshold rule over counts c[0, n)
int32_t threshold_of(const int32_t* c, int64_t n) {
    int32_t most = 0;
    for (int64_t i = 0; i < n; ++i) most = std::max(most, c[i]);
    std::vector<int64_t> h;
    for (int32_t t = 1;; ++t) {
        if (t >= most) return t;
        if (h.empty()) {  // (only when the first candidate is not the answer already)
            h.assign((size_t)most + 2, 0);
            for (int64_t i = 0; i < n; ++i) ++h[(size_t)c[i]];
        }
        if (h[(size_t)t + 1] >= h[(size_t)t]) return t;
    }
}

// the same from the device's histogram (bin b < last: count b; the last bin: every greater count); -1 when the rule
// would read the last bin, where the histogram is not exact
int32_t threshold_of_hist(const uint32_t* h, int32_t bins, int32_t most) {
    for (int32_t t = 1;; ++t) {
        if (t >= most) return t;
        if (t + 1 >= bins - 1) return -1;
        if (h[t + 1] >= h[t]) return t;
    }
}

// Uploads the reads and runs the key, sort and count passes: on return the stream is synchronised, g describes the
// spectrum in device memory (n_distinct, spec_keys, spec_counts, hist) and ctr holds the device's counters.
int device_spectrum(ovl_ctx* ctx, Dev* c, const char* what, const uint8_t* seqs, const int64_t* offsets,
                    int32_t n_reads, int32_t k, int64_t n_win, int32_t max_win, bool correct, OvlSpectrumArgs* g,
                    unsigned long long* ctr) {
    hipStream_t s = c->stream;
    const int64_t total = n_reads > 0 ? offsets[n_reads] - offsets[0] : 0;
    const size_t N = (size_t)std::max(n_reads, 1);
    size_t temp = 0;
    if (n_win > 0) HIPCHK(c, ovl_spectrum_temp_bytes(n_win, k, &temp));
    *g = OvlSpectrumArgs{};
    Carve in_size, work_size;
    lay_spectrum_in(in_size, *g, n_reads, total);
    lay_spectrum_work(work_size, *g, n_reads, n_win, total, temp, correct);
    const int rc = check_fits(c, what, "keys and tables", in_size.at + work_size.at, {&c->sp.in, &c->sp.work});
    if (rc != OVL_OK) return rc;
    std::vector<int64_t> h_off(N + 1, 0), h_woff(N + 1, 0);
    for (int32_t r = 0; r < n_reads; ++r) {
        h_off[(size_t)r + 1] = offsets[r + 1] - offsets[0];
        h_woff[(size_t)r + 1] = h_woff[(size_t)r] + std::max<int64_t>(offsets[r + 1] - offsets[r] - k + 1, 0);
    }
    HIPCHK(c, ensure(c->sp.in, in_size.at));
    HIPCHK(c, ensure(c->sp.work, work_size.at));
    HIPCHK(c, c->sp.timer.arm(ctx->timing));
    Carve in(c->sp.in.p), work(c->sp.work.p);
    lay_spectrum_in(in, *g, n_reads, total);
    void* d_temp = lay_spectrum_work(work, *g, n_reads, n_win, total, temp, correct);
    StreamDrain drain(s);  // the copies read this call's vectors: drained whichever way the routine leaves
    HIPCHK(c, hipMemcpyAsync(writable(g->off), h_off.data(), 8 * (N + 1), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(writable(g->woff), h_woff.data(), 8 * (N + 1), hipMemcpyHostToDevice, s));
    if (total > 0)
        HIPCHK(c, hipMemcpyAsync(writable(g->seqs), seqs + offsets[0], (size_t)total, hipMemcpyHostToDevice, s));
    g->n_reads = n_reads;
    g->k = k;
    g->max_win = std::max(max_win, 1);
    g->ballot = c->k.spec_ballot;
    g->bins = c->k.spec_bins ? c->k.spec_bins : kSpecHistBins;
    g->n_win = n_win;
    HIPCHK(c, hipMemsetAsync(g->ctr, 0, 64, s));
    HIPCHK(c, hipMemsetAsync(g->hist, 0, 4 * (size_t)kSpecHistBins, s));
    HIPCHK(c, c->sp.timer.mark(0, s));
    HIPCHK(c, ovl_launch_spectrum_keys(g, s));
    HIPCHK(c, c->sp.timer.mark(1, s));
    HIPCHK(c, ovl_launch_spectrum_sort(g, d_temp, temp, s));
    HIPCHK(c, c->sp.timer.mark(2, s));
    HIPCHK(c, ovl_launch_spectrum_heads(g, d_temp, temp, s));
    HIPCHK(c, hipMemcpyAsync(ctr, g->ctr, 64, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if ((int64_t)ctr[0] > n_win) return fail(c, OVL_E_INTERNAL, "%s: %llu distinct keys from %lld windows", what, ctr[0], (long long)n_win);
    g->n_distinct = (int32_t)ctr[0];
    HIPCHK(c, ovl_launch_spectrum_counts(g, s));
    HIPCHK(c, c->sp.timer.mark(3, s));
    HIPCHK(c, hipMemcpyAsync(ctr, g->ctr, 64, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    drain.armed = false;
    // the key, sort and count passes' times (the count pass's includes the host's wait for the number of distinct
    // keys); ovl_last_timing has them from here, so that a call refused further on still reports them
    double* ms = c->sp.last.ms;
    for (int i = 0; i < 3; ++i) ms[i] = c->sp.timer.ms(i, i + 1);
    ctx->t_kernel_ms = ms[0] + ms[1] + ms[2];
    return OVL_OK;
}

int device_limits(Dev* c, const char* what, const int64_t* offsets, int32_t k, int64_t n_win, int32_t long_read) {
    if (long_read >= 0)
        return fail(c, OVL_E_UNSUPPORTED, "%s: read %d has %lld bases, more than k + %d", what, long_read,
                    (long long)(offsets[long_read + 1] - offsets[long_read]), kSpecMaxWindows - 1);
    if (n_win >= kSpecMax) return fail(c, OVL_E_UNSUPPORTED, "%s: fewer than 2^31 windows required", what);
    return OVL_OK;
}

}  // namespace

OVL_API int ovl_kmer_spectrum_host(const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, int32_t k,
                                   uint64_t* out_keys, int32_t* out_counts, int64_t capacity, int64_t* out_n_distinct) {
    const ovl_ctx* none = nullptr;
    int64_t n_win = 0;
    int32_t max_win = 0, long_read = -1;
    int rc = check_reads(none, "kmer_spectrum", seqs, offsets, n_reads, k, &n_win, &max_win, &long_read);
    if (rc != OVL_OK) return rc;
    if (!out_n_distinct) return fail(none, OVL_E_ARG, "kmer_spectrum: out_n_distinct is NULL");
    if (capacity < 0 || (capacity > 0 && (!out_keys || !out_counts)))
        return fail(none, OVL_E_ARG, "kmer_spectrum: capacity %lld without output arrays", (long long)capacity);
    try {
        std::vector<uint64_t> keys((size_t)n_win);
        host_keys(seqs, offsets, n_reads, k, keys);
        Spectrum sp;
        if (host_spectrum(std::move(keys), &sp) != OVL_OK)
            return fail(none, OVL_E_UNSUPPORTED, "kmer_spectrum: a key occurs 2^31 times or more");
        *out_n_distinct = (int64_t)sp.keys.size();
        if ((int64_t)sp.keys.size() > capacity)
            return fail(none, OVL_E_RANGE, "kmer_spectrum: %zu distinct keys, capacity %lld", sp.keys.size(),
                        (long long)capacity);
        std::copy(sp.keys.begin(), sp.keys.end(), out_keys);
        std::copy(sp.counts.begin(), sp.counts.end(), out_counts);
    } catch (const std::bad_alloc&) {
        return fail(none, OVL_E_OOM, "kmer_spectrum: no memory for the keys");
    }
    return OVL_OK;
}

OVL_API int ovl_correct_reads_host(const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, int32_t k,
                                   int32_t min_count, uint8_t* out_seqs, int32_t* out_changed, int64_t* out_stats) {
    const ovl_ctx* none = nullptr;
    int64_t n_win = 0;
    int32_t max_win = 0, long_read = -1;
    int rc = check_reads(none, "correct_reads", seqs, offsets, n_reads, k, &n_win, &max_win, &long_read);
    if (rc != OVL_OK) return rc;
    if (min_count < 0) return fail(none, OVL_E_ARG, "correct_reads: min_count %d < 0", min_count);
    if (!out_stats) return fail(none, OVL_E_ARG, "correct_reads: out_stats is NULL");
    if (n_reads > 0 && !out_changed) return fail(none, OVL_E_ARG, "correct_reads: out_changed is NULL");
    const int64_t total = n_reads > 0 ? offsets[n_reads] - offsets[0] : 0;
    if (total > 0 && !out_seqs) return fail(none, OVL_E_ARG, "correct_reads: out_seqs is NULL");
    try {
        std::vector<uint64_t> keys((size_t)n_win);
        host_keys(seqs, offsets, n_reads, k, keys);
        Spectrum sp;
        if (host_spectrum(keys, &sp) != OVL_OK)
            return fail(none, OVL_E_UNSUPPORTED, "correct_reads: a key occurs 2^31 times or more");
        if (min_count == 0) min_count = threshold_of(sp.counts.data(), (int64_t)sp.counts.size());
        int64_t n_solid = 0, n_untrusted = 0, n_changed = 0, n_ties = 0;
        if (total > 0) memmove(out_seqs + offsets[0], seqs + offsets[0], (size_t)total);
        std::vector<int32_t> before;  // before[o]: solid windows among the read's first o
        size_t at = 0;
        for (int32_t r = 0; r < n_reads; ++r) {
            out_changed[r] = 0;
            const int64_t L = offsets[r + 1] - offsets[r];
            if (L < k) continue;
            const int64_t nw = L - k + 1;
            const uint64_t* rk = keys.data() + at;
            at += (size_t)nw;
            const uint8_t* s = seqs + offsets[r];
            before.assign((size_t)nw + 1, 0);
            for (int64_t o = 0; o < nw; ++o)
                before[(size_t)o + 1] = before[(size_t)o] + (rk[o] != kSpecNoKey && sp.solid(rk[o], min_count));
            n_solid += before[(size_t)nw];
            for (int64_t i = 0; i < L; ++i) {
                const int64_t lo = std::max<int64_t>(0, i - k + 1), hi = std::min<int64_t>(i, nw - 1);
                if (before[(size_t)hi + 1] - before[(size_t)lo] > 0) continue;
                ++n_untrusted;
                const int32_t c = ovl_spec_code(s[i]);
                if (c < 0) continue;
                int32_t sx[3] = {0, 0, 0};
                for (int32_t t = 0; t < 3; ++t)
                    for (int64_t o = lo; o <= hi; ++o)
                        if (rk[o] != kSpecNoKey)
                            sx[t] += sp.solid(ovl_spec_replace(rk[o], k, (int32_t)(o - lo), (int32_t)(i - lo),
                                                               (c + 1 + t) & 3),
                                              min_count);
                const int32_t best = std::max(sx[0], std::max(sx[1], sx[2]));
                const int32_t n_best = (sx[0] == best) + (sx[1] == best) + (sx[2] == best);
                if (best >= 1 && n_best == 1) {
                    const int32_t t = sx[0] == best ? 0 : (sx[1] == best ? 1 : 2);
                    out_seqs[offsets[r] + i] = ovl_spec_base((c + 1 + t) & 3);
                    ++out_changed[r];
                    ++n_changed;
                } else if (best >= 1) {
                    ++n_ties;
                }
            }
        }
        const int64_t st[8] = {sp.kmers, (int64_t)sp.keys.size(), n_solid, n_untrusted, n_changed, n_ties, min_count,
                               n_win};
        std::copy(st, st + 8, out_stats);
    } catch (const std::bad_alloc&) {
        return fail(none, OVL_E_OOM, "correct_reads: no memory for the keys");
    }
    return OVL_OK;
}

OVL_API int ovl_kmer_spectrum(ovl_ctx* ctx, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, int32_t k,
                              uint64_t* out_keys, int32_t* out_counts, int64_t capacity, int64_t* out_n_distinct) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    StageCall call(ctx);
    Dev* c = call.dev;
    int64_t n_win = 0;
    int32_t max_win = 0, long_read = -1;
    int rc = check_reads(c, "kmer_spectrum", seqs, offsets, n_reads, k, &n_win, &max_win, &long_read);
    if (rc != OVL_OK) return rc;
    if (!out_n_distinct) return fail(c, OVL_E_ARG, "kmer_spectrum: out_n_distinct is NULL");
    if (capacity < 0 || (capacity > 0 && (!out_keys || !out_counts)))
        return fail(c, OVL_E_ARG, "kmer_spectrum: capacity %lld without output arrays", (long long)capacity);
    if ((rc = device_limits(c, "kmer_spectrum", offsets, k, n_win, long_read)) != OVL_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    call.begin();
    c->sp.last = {};
    OvlSpectrumArgs g;
    unsigned long long ctr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if ((rc = device_spectrum(ctx, c, "kmer_spectrum", seqs, offsets, n_reads, k, n_win, max_win, false, &g, ctr)) !=
        OVL_OK)
        return rc;
    *out_n_distinct = g.n_distinct;
    if (g.n_distinct > capacity)
        return fail(c, OVL_E_RANGE, "kmer_spectrum: %d distinct keys, capacity %lld", g.n_distinct, (long long)capacity);
    if (g.n_distinct > 0) {
        HIPCHK(c, hipMemcpy(out_keys, g.spec_keys, 8 * (size_t)g.n_distinct, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(out_counts, g.spec_counts, 4 * (size_t)g.n_distinct, hipMemcpyDeviceToHost));
    }
    return call.done(ctx->t_kernel_ms);  // (device_spectrum's passes)
}

OVL_API int ovl_correct_reads(ovl_ctx* ctx, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, int32_t k,
                              int32_t min_count, uint8_t* out_seqs, int32_t* out_changed, int64_t* out_stats) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    StageCall call(ctx);
    Dev* c = call.dev;
    int64_t n_win = 0;
    int32_t max_win = 0, long_read = -1;
    int rc = check_reads(c, "correct_reads", seqs, offsets, n_reads, k, &n_win, &max_win, &long_read);
    if (rc != OVL_OK) return rc;
    if (min_count < 0) return fail(c, OVL_E_ARG, "correct_reads: min_count %d < 0", min_count);
    if (!out_stats) return fail(c, OVL_E_ARG, "correct_reads: out_stats is NULL");
    if (n_reads > 0 && !out_changed) return fail(c, OVL_E_ARG, "correct_reads: out_changed is NULL");
    const int64_t total = n_reads > 0 ? offsets[n_reads] - offsets[0] : 0;
    if (total > 0 && !out_seqs) return fail(c, OVL_E_ARG, "correct_reads: out_seqs is NULL");
    if ((rc = device_limits(c, "correct_reads", offsets, k, n_win, long_read)) != OVL_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    call.begin();
    c->sp.last = {};
    OvlSpectrumArgs g;
    unsigned long long ctr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if ((rc = device_spectrum(ctx, c, "correct_reads", seqs, offsets, n_reads, k, n_win, max_win, true, &g, ctr)) !=
        OVL_OK)
        return rc;
    hipStream_t s = c->stream;
    if (min_count == 0) {  // the threshold rule, from the device's histogram where that is exact
        std::vector<uint32_t> hist((size_t)kSpecHistBins, 0);
        if (g.n_distinct > 0) HIPCHK(c, hipMemcpy(hist.data(), g.hist, 4 * hist.size(), hipMemcpyDeviceToHost));
        min_count = threshold_of_hist(hist.data(), g.bins, (int32_t)ctr[6]);
        if (min_count < 0) {
            std::vector<int32_t> counts((size_t)g.n_distinct);
            HIPCHK(c, hipMemcpy(counts.data(), g.spec_counts, 4 * counts.size(), hipMemcpyDeviceToHost));
            min_count = threshold_of(counts.data(), (int64_t)counts.size());
        }
    }
    g.min_count = min_count;
    if (n_win > 0) {
        StreamDrain drain(s);
        HIPCHK(c, hipMemcpyAsync(g.out, g.seqs, (size_t)total, hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemsetAsync(g.changed, 0, 4 * (size_t)n_reads, s));
        HIPCHK(c, c->sp.timer.mark(4, s));
        HIPCHK(c, ovl_launch_spectrum_correct(&g, c->cu_count * 8, s));
        HIPCHK(c, c->sp.timer.mark(5, s));
        HIPCHK(c, hipMemcpyAsync(ctr, g.ctr, 64, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(out_seqs + offsets[0], g.out, (size_t)total, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(out_changed, g.changed, 4 * (size_t)n_reads, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        drain.armed = false;
        c->sp.last.ms[3] = c->sp.timer.ms(4, 5);
    } else {  // no read has a window: nothing to decide
        if (total > 0) memmove(out_seqs + offsets[0], seqs + offsets[0], (size_t)total);
        for (int32_t r = 0; r < n_reads; ++r) out_changed[r] = 0;
    }
    const int64_t st[8] = {(int64_t)ctr[7], g.n_distinct, (int64_t)ctr[2], (int64_t)ctr[3], (int64_t)ctr[4],
                           (int64_t)ctr[5], min_count, n_win};
    std::copy(st, st + 8, out_stats);
    return call.done(ctx->t_kernel_ms + c->sp.last.ms[3]);  // (the spectrum's passes and the correction)
}

OVL_API int ovl_last_correct_timing(const ovl_ctx* ctx, double* keys_ms, double* sort_ms, double* count_ms,
                                    double* correct_ms) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    const double* ms = ctx->devs[0]->sp.last.ms;
    if (keys_ms) *keys_ms = ms[0];
    if (sort_ms) *sort_ms = ms[1];
    if (count_ms) *count_ms = ms[2];
    if (correct_ms) *correct_ms = ms[3];
    return OVL_OK;
}
