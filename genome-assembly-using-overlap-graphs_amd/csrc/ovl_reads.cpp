// ovl_reads.cpp — the resident read set (ovl_ctx.h): host preparation, the pinned upload stage, the upload and
// packing on every device, and the check that spares them when the caller's read set is already resident.
#include "ovl_ctx.h"

namespace {

// Offsets, lengths, the length bitmap and the longest read (split over the host pool for large read sets).
int prep_reads(ovl_ctx* c, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, HostReads& h) {
    const int64_t base = n_reads > 0 ? offsets[0] : 0;
    if (base < 0) return fail(c, OVL_E_ARG, "offsets[0] < 0");
    h.n_reads = n_reads;
    h.off.resize((size_t)n_reads + 1);
    h.len.resize((size_t)std::max(n_reads, 1));
    h.off[0] = 0;
    h.len[0] = 0;
    CopyPool& pool = CopyPool::get();
    // parts of whole 32-read words (the bitmap), each with its longest read and first bad read
    const std::vector<size_t> parts = pool.cut((size_t)n_reads, size_t(1) << 14);
    std::vector<int32_t> pmax(parts.size(), 0), pbad(parts.size(), -1), ptoo(parts.size(), -1);
    pool.parallel_parts(parts, [&](size_t i, size_t lo, size_t hi) {
        int32_t m = 0;
        for (size_t r = lo; r < hi; ++r) {
            const int64_t l = offsets[r + 1] - offsets[r];
            if (l < 0 || l > INT32_MAX / 2) {
                (l < 0 ? pbad[i] : ptoo[i]) = (int32_t)r;
                return;
            }
            h.off[r + 1] = offsets[r + 1] - base;
            h.len[r] = (int32_t)l;
            m = std::max(m, (int32_t)l);
        }
        pmax[i] = m;
    });
    h.lmax = 0;
    for (size_t i = 0; i < parts.size(); ++i) {
        if (pbad[i] >= 0) return fail(c, OVL_E_ARG, "offsets not non-decreasing at read %d", pbad[i]);
        if (ptoo[i] >= 0) return fail(c, OVL_E_UNSUPPORTED, "read %d is too long", ptoo[i]);
        h.lmax = std::max(h.lmax, pmax[i]);
    }
    h.total = n_reads > 0 ? h.off[(size_t)n_reads] : 0;
    h.full.assign(((size_t)std::max(n_reads, 1) + 31) / 32, 0u);
    pool.parallel_parts(parts, [&](size_t, size_t lo, size_t hi) {
        for (size_t r = lo; r < hi; ++r)
            if (h.len[r] == h.lmax) h.full[r >> 5] |= 1u << (r & 31);  // (parts cut at multiples of 64 reads)
    });
    if (h.total > 0 && !seqs) return fail(c, OVL_E_ARG, "seqs is NULL");
    h.src = seqs ? seqs + base : nullptr;
    return OVL_OK;
}

// The pinned upload stage: offsets, lengths, bitmap and code table, and the read bytes -- 2-bit packed by the
// host pool in the same pass that scans them for the alphabet when every byte is A, C, G or T (a quarter of
// the bytes to upload, expanded by unpack2_kernel), else copied as they are.  Sets the code table and the
// bit-plane layout (dense codes in byte order, equality-preserving).
int stage_reads(ovl_ctx* c, ReadStage& st, HostReads& h) {
    auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
    st.o_off = 0;
    st.o_len = al(st.o_off + sizeof(int64_t) * h.off.size());
    st.o_full = al(st.o_len + sizeof(int32_t) * h.len.size());
    st.o_lut = al(st.o_full + sizeof(uint32_t) * h.full.size());
    st.o_pk = al(st.o_lut + 256);
    st.o_raw = al(st.o_pk + (size_t)h.total / 4 + 64);
    const size_t need = al(st.o_raw + (size_t)h.total + 1);
    if (st.bytes < need) {
        if (st.p) (void)hipHostFree(st.p);
        st.p = nullptr;
        st.bytes = 0;
        HIPCHK(c, hipHostMalloc((void**)&st.p, need, hipHostMallocPortable));
        st.bytes = need;
    }
    bool present[256] = {false};
    h.packed2 = false;
    if (h.total > 0) {
        CopyPool& pool = CopyPool::get();
        const std::vector<size_t> parts = pool.cut((size_t)h.total, size_t(1) << 18);  // (multiples of 64)
        std::vector<std::array<uint8_t, 256>> seen(parts.size(), std::array<uint8_t, 256>{});
        std::vector<uint8_t> ok(parts.size() - 1, 0);  // (cut gives parts + 1 bounds)
        const uint8_t* src = h.src;
        uint8_t* pk = reinterpret_cast<uint8_t*>(st.p + st.o_pk);
        pool.parallel_parts(parts, [&](size_t i, size_t lo, size_t hi) {
            ok[i] = ovl_scan::scan_pack(src, lo, hi, seen[i].data(), pk);
        });
        for (const auto& t : seen)
            for (int v = 0; v < 256; ++v) present[v] = present[v] || t[(size_t)v];
        h.packed2 = std::find(ok.begin(), ok.end(), 0) == ok.end();
        if (!h.packed2) host_copy(st.p + st.o_raw, h.src, (size_t)h.total);
    }
    memset(h.lut, 0, sizeof(h.lut));
    memset(h.inv, 0, sizeof(h.inv));
    int k = 0;
    for (int v = 0; v < 256; ++v)
        if (present[v]) {
            h.inv[k] = (uint8_t)v;
            h.lut[v] = (uint8_t)k++;
        }
    h.planes = k <= 4 ? 2 : (k <= 16 ? 4 : 8);
    // bit-plane layouts: W = ceil(lmax/32) words of 32 bases, rows padded to 16 bytes
    h.wmax = 0;
    if (h.lmax <= kFastMaxLen) h.wmax = std::max(1, (h.lmax + 31) / 32);
    h.srow = h.wmax ? ((h.wmax * h.planes + 3) & ~3) : 0;
    h.trow = h.srow;
    memcpy(st.p + st.o_off, h.off.data(), sizeof(int64_t) * h.off.size());
    memcpy(st.p + st.o_len, h.len.data(), sizeof(int32_t) * h.len.size());
    memcpy(st.p + st.o_full, h.full.data(), sizeof(uint32_t) * h.full.size());
    memcpy(st.p + st.o_lut, h.lut, 256);
    h.src = reinterpret_cast<const uint8_t*>(st.p + (h.packed2 ? st.o_pk : st.o_raw));
    return OVL_OK;
}

// Asynchronous upload + pack of one device's copy from the pinned stage; the caller synchronises d->stream.
hipError_t upload_reads(Dev* d, const HostReads& h, const ReadStage& st) {
    hipError_t e = hipSetDevice(d->device);
    if (e != hipSuccess) return e;
    d->n_reads = -1;  // invalid until fully built
    d->cand_n = -1;
    d->heavy_for = -1;
    const int32_t n_reads = h.n_reads;
    // one copy of the stage's block (offsets, lengths, bitmap, code table, then the packed or raw bytes), the
    // arrays used in place as views into it
    const size_t pk_bytes = (((size_t)h.total + 63) / 64) * 16;
    const size_t blk = h.packed2 ? st.o_pk + pk_bytes : st.o_raw + (size_t)h.total;
    for (DevBuf* v : {&d->off, &d->len, &d->full, &d->lut, &d->raw}) release(*v);
    if ((e = ensure(d->rd, blk + 64)) != hipSuccess) return e;
    set_view(d->off, d->rd, st.o_off, sizeof(int64_t) * h.off.size());
    set_view(d->len, d->rd, st.o_len, sizeof(int32_t) * h.len.size());
    set_view(d->full, d->rd, st.o_full, sizeof(uint32_t) * h.full.size());
    set_view(d->lut, d->rd, st.o_lut, 256);
    set_view(d->raw, d->rd, h.packed2 ? st.o_pk : st.o_raw, h.packed2 ? pk_bytes : (size_t)h.total);
    if ((e = ensure(d->codes, (size_t)h.total + 64)) != hipSuccess) return e;  // tail pad: clamped reads
    hipStream_t s = d->stream;
    if ((e = hipMemcpyAsync(d->rd.p, st.p, blk, hipMemcpyHostToDevice, s))) return e;
    if (h.total > 0 && h.packed2) {
        if ((e = ovl_launch_unpack2(as<uint8_t>(d->raw), as<uint8_t>(d->lut), as<uint8_t>(d->codes), h.total, s)))
            return e;
    } else if (h.total > 0) {
        if ((e = ovl_launch_map_codes(as<uint8_t>(d->raw), as<uint8_t>(d->lut), as<uint8_t>(d->codes), h.total, s)))
            return e;
    }
    if (h.wmax > 0) {
        const size_t rows = (size_t)std::max(n_reads, 1);
        if ((e = ensure(d->sfx, rows * h.srow * sizeof(uint32_t)))) return e;
        if ((e = ensure(d->pfx, rows * h.trow * sizeof(uint32_t)))) return e;
        if ((e = ovl_launch_pack(h.planes, as<uint8_t>(d->codes), as<int64_t>(d->off), as<int32_t>(d->len), n_reads,
                                 h.wmax, h.srow, h.trow, as<uint32_t>(d->sfx), as<uint32_t>(d->pfx), s)))
            return e;
    }
    return hipSuccess;
}

// The caller's read set equals the resident one: the same offsets relative to offsets[0] (compared over the host
// pool, a part stops at its first difference) and the same 128-bit digest of the bytes.
bool same_reads(const ovl_ctx* c, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads) {
    if (!c->res_valid || (int64_t)c->res_off.size() != (int64_t)n_reads + 1) return false;
    for (const Dev* d : c->devs)
        if (d->n_reads != n_reads) return false;
    const int64_t base = n_reads > 0 ? offsets[0] : 0;
    if (n_reads > 0 && offsets[n_reads] - base != c->res_total) return false;
    CopyPool& pool = CopyPool::get();
    std::atomic<bool> differ{false};
    pool.parallel((size_t)n_reads + 1, size_t(1) << 14, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi && !differ.load(std::memory_order_relaxed); ++i)
            if (offsets[i] - base != c->res_off[i]) differ.store(true, std::memory_order_relaxed);
    });
    if (differ.load()) return false;
    if (c->res_total == 0) return true;
    if (!seqs) return false;
    uint64_t h[2];
    ovl_digest::reads_hash(seqs + base, c->res_total, h);
    return h[0] == c->res_hash[0] && h[1] == c->res_hash[1];
}

}  // namespace

// ovl_set_reads; sync = false (ovl_score_pairs) leaves the uploads running on each device's kernel stream --
// the scoring launches queue behind them there -- and the caller synchronises those streams before it returns
// (the pinned stage must outlive the copy)
int set_reads(ovl_ctx* c, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, bool sync) {
    if (!c) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    quiet(c);
    if (n_reads < 0) return fail(c, OVL_E_ARG, "n_reads < 0");
    if (n_reads > 0 && !offsets) return fail(c, OVL_E_ARG, "offsets is NULL");
    if (n_reads > 0 && offsets[0] < 0) return fail(c, OVL_E_ARG, "offsets[0] < 0");
    if (n_reads > 0 && offsets[n_reads] > offsets[0] && !seqs) return fail(c, OVL_E_ARG, "seqs is NULL");
    DeviceGuard guard;
    if (same_reads(c, seqs, offsets, n_reads)) {
        // already resident on every device: only the candidate list goes, as after an upload (and the sharer
        // count is refreshed as an upload would, when it is older than its interval)
        CpuShare::get().refresh();
        for (Dev* d : c->devs) {
            d->cand_n = -1;
            d->heavy_for = -1;
        }
        return OVL_OK;
    }
    c->res_valid = false;
    PipeTrace trace;  // OVL_TRACE_PIPE: r recount, p prepared, s staged, u uploads issued, y synchronised
    CpuShare::get().refresh();
    trace.mark('r', 0);
    HostReads& h = c->hreads;
    h.lmax = 0;
    int rc = prep_reads(c, seqs, offsets, n_reads, h);
    if (rc != OVL_OK) return rc;
    trace.mark('p', 0);
    c->h_len.clear();
    hipError_t e = hipSuccess;
    for (Dev* d : c->devs) {
        d->n_reads = -1;
        d->cand_n = -1;
        d->heavy_for = -1;
    }
    // the pinned stage (the previous upload from it is complete: every caller synchronised it), then the
    // upload to every device, then wait for all (the uploads and packs overlap across devices)
    rc = stage_reads(c, c->stage, h);
    if (rc != OVL_OK) return rc;
    trace.mark('s', 0);
    for (Dev* d : c->devs)
        if ((e = upload_reads(d, h, c->stage)) != hipSuccess) break;
    trace.mark('u', 0);
    for (Dev* d : c->devs) {
        if (!sync && e == hipSuccess) break;
        (void)hipSetDevice(d->device);
        hipError_t e2 = hipStreamSynchronize(d->stream);
        if (e == hipSuccess) e = e2;
    }
    trace.mark('y', 0);
    if (e != hipSuccess)
        return fail(c, e == hipErrorOutOfMemory ? OVL_E_OOM : OVL_E_HIP, "ovl_set_reads: %s", hipGetErrorString(e));
    for (Dev* d : c->devs) {
        d->lmax = h.lmax;
        d->codes_bytes = h.total;
        d->planes = h.planes;
        d->wmax = h.wmax;
        d->srow = h.srow;
        d->trow = h.trow;
        d->n_reads = n_reads;
    }
    c->h_len.assign(h.len.begin(), h.len.begin() + n_reads);
    // what is resident now (for same_reads)
    const int64_t base = n_reads > 0 ? offsets[0] : 0;
    c->res_off.resize((size_t)n_reads + 1);
    for (int32_t i = 0; i <= n_reads; ++i) c->res_off[(size_t)i] = n_reads > 0 ? offsets[i] - base : 0;
    // (a digest of the bytes, not a copy: the host memory a resident set costs is its offsets)
    c->res_total = h.total;
    c->res_hash[0] = c->res_hash[1] = 0;
    if (h.total > 0) ovl_digest::reads_hash(seqs + base, h.total, c->res_hash);
    c->res_valid = true;
    return OVL_OK;
}

OVL_API int ovl_set_reads(ovl_ctx* c, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads) {
    return set_reads(c, seqs, offsets, n_reads, true);
}

OVL_API int ovl_reads_info(const ovl_ctx* c, int32_t* n_reads, int32_t* lmax, int32_t* planes, int64_t* device_bytes) {
    if (!c) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    const Dev* d = c->devs[0];
    if (n_reads) *n_reads = d->n_reads;
    if (lmax) *lmax = d->lmax;
    if (planes) *planes = d->planes;
    if (device_bytes)
        *device_bytes = (int64_t)(d->codes.bytes + d->off.bytes + d->len.bytes + d->sfx.bytes + d->pfx.bytes);
    return OVL_OK;
}
