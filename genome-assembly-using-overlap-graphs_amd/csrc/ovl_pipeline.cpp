// ovl_pipeline.cpp — host-array scoring calls (ovl_ctx.h): the pair list sharded over the devices and a chunked
// pipeline per device (run_pipeline), with the compact pair-list encoding and the host expansion of packed results.
#include "ovl_ctx.h"

void host_copy(void* dst, const void* src, size_t bytes) { CopyPool::get().copy(dst, src, bytes); }

namespace {

// Packed results (ovl_sweep.h put_pair, sink 2) into the caller's int32 arrays (ovl_expand.h), split
// over the host pool, at the widest vector width this CPU runs.
void host_expand(int32_t* s, int32_t* e, const uint16_t* pk, const int32_t* esc, int32_t match, int32_t mismatch,
                 bool nt, size_t n, size_t min_part) {
    static const ovl_expand::Fn f = ovl_expand::pick(nullptr);
    CopyPool::get().parallel(n, min_part,
                             [=](size_t lo, size_t hi) { f(s, e, pk, esc, match, mismatch, nt, lo, hi); });
}

// The pipeline's waits for a chunk: polled (a chunk is tens of microseconds away; a blocking wait can
// add its own wake-up latency per chunk, depending on the device's scheduling flags).
hipError_t wait_event(const Dev* d, hipEvent_t ev) {
    (void)d;
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        _mm_pause();
    }
}

// Pairs per pipeline chunk.  Direct kernel stores into pinned arrays need no chunks (a chunk's fixed cost, ~0.1 ms as
// a D2H copy, is more than the kernel time it hides: tools/pipe_ab.py, profiles/r02_pipe_ab_*.json); pageable arrays go
// through the pinned staging slots in chunks of the slot size, 512 K pairs (the host copy of chunk k + 1 overlaps the
// kernel of chunk k).  Packed results (pack_ok) are expanded on the host chunk by chunk while the next chunk is scored,
// 1 M pairs (tools/host_paths_ab.py, target point: 128 K 0.53 ms, 256 K 0.38, 512 K 0.30, 1 M 0.25, one chunk 0.29).
int64_t pick_chunk(const Dev* d, int64_t n, bool staged, bool pack) {
    if (d->k.pipe_chunk > 0) return d->k.pipe_chunk;
    const int64_t cap = int64_t(1) << (pack ? 20 : 19);
    return std::max<int64_t>(1, staged ? std::min(n, cap) : n);
}

// Chunk k's results go through the staging slots (pageable caller arrays, or a packed chunk).
bool chunk_staged(const Call& C, const Job& J, int64_t k) { return !C.out_pinned || (C.pack && k < J.n_packed); }

// The live direct share of the device's packed calls into pinned arrays: one for compact host pair lists
double& pack_share(const Call& C, Dev* d) { return C.compact ? d->pack_pct_h : d->pack_pct; }

// Chunk k of a compact host pair list in the encoding buffer
PairLayout chunk_layout(const Job& J, int64_t k) {
    const int64_t off = J.cb[(size_t)k];
    return PairLayout(off, k, J.cb[(size_t)k + 1] - off, J.d->n_reads <= 65535 ? 2 : 4);
}

int setup_job(const Call& C, Job& J) {
    Dev* d = J.d;
    const int64_t n = J.hi - J.lo;
    J.cb.assign(1, 0);
    J.nchunks = J.n_packed = 0;
    if (n <= 0) return OVL_OK;
    HIPCHK(d, hipSetDevice(d->device));
    const bool need_in = C.h_a && !C.in_pinned && !C.compact, need_out = !C.out_pinned || C.pack;
    J.chunk = pick_chunk(d, n, need_in || need_out, C.pack);
    // packed calls: the packed share in equal chunks of <= J.chunk, then (pinned arrays) the direct share
    int64_t packed = 0;
    if (C.pack) {
        double& share = pack_share(C, d);
        if (share < 0.0) share = C.compact ? 2.0 * d->k.pack_direct_pct : d->k.pack_direct_pct;
        const int64_t pct = d->k.pack_adapt ? (int64_t)(share + 0.5) : d->k.pack_direct_pct;
        packed = C.out_pinned ? (n - n * pct / 100) & ~int64_t(63) : n;
        if (packed >= n - 64) packed = n;
        // (a ramp of growing chunks -- 196 K, x 1.5 each -- to start the host's expansion sooner measured slower:
        // 0.208 against 0.145 ms at the target point, each extra chunk costing an issue and a later direct
        // chunk; profiles/r04_pool_ab_*.json)
        const int64_t pieces = (packed + J.chunk - 1) / J.chunk;
        const int64_t step = pieces ? (((packed + pieces - 1) / pieces + 63) & ~int64_t(63)) : 0;
        for (int64_t o = step; o < packed; o += step) J.cb.push_back(o);
        if (packed > 0) J.cb.push_back(packed);
        J.n_packed = (int64_t)J.cb.size() - 1;
    }
    for (int64_t o = J.cb.back(); o < n;) {  // (the direct chunks)
        o = std::min(n, o + J.chunk);
        J.cb.push_back(o);
    }
    J.nchunks = (int64_t)J.cb.size() - 1;
    J.drained = 0;
    for (int64_t k = 0; k < J.nchunks; ++k) J.chunk = std::max(J.chunk, J.cb[(size_t)k + 1] - J.cb[(size_t)k]);
    const size_t bytes = sizeof(int32_t) * (size_t)n;
    if (C.compact) {
        // decoded pair list in HBM, the pinned encoding buffer (chunk k: chunk_layout) and the chunks' decode events
        HIPCHK(d, ensure(d->a, bytes));
        HIPCHK(d, ensure(d->b, bytes));
        J.ka = as<int32_t>(d->a);
        J.kb = as<int32_t>(d->b);
        const size_t need = PairLayout::job_bytes(n, J.nchunks);
        if (d->cp_bytes < need) {
            if (d->cp_host) (void)hipHostFree(d->cp_host);
            d->cp_host = d->cp_dev = nullptr;
            d->cp_bytes = 0;
            HIPCHK(d, hipHostMalloc((void**)&d->cp_host, need, kHostShared));
            HIPCHK(d, hipHostGetDevicePointer((void**)&d->cp_dev, d->cp_host, 0));
            d->cp_bytes = need;
        }
        if (d->k.pairs_ix) HIPCHK(d, ensure(d->cp_hbm, need));
        while ((int64_t)d->dec_ev.size() < J.nchunks) {
            hipEvent_t ev;
            HIPCHK(d, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            d->dec_ev.push_back(ev);
        }
        d->cp_link = 0;
    }
    if (C.h_a && C.in_pinned && !C.compact) {
        // the kernels read this device's slice of the caller's pinned pair arrays in place
        void* pa = nullptr;
        void* pb = nullptr;
        HIPCHK(d, hipHostGetDevicePointer(&pa, const_cast<int32_t*>(C.h_a + J.lo), 0));
        HIPCHK(d, hipHostGetDevicePointer(&pb, const_cast<int32_t*>(C.h_b + J.lo), 0));
        J.za = reinterpret_cast<const int32_t*>(pa);
        J.zb = reinterpret_cast<const int32_t*>(pb);
    }
    if (C.out_pinned) {
        // the device's address of this slice of the caller's pinned arrays
        void* ps = nullptr;
        void* pe = nullptr;
        HIPCHK(d, hipHostGetDevicePointer(&ps, C.out_s + (J.lo - C.out_base), 0));
        HIPCHK(d, hipHostGetDevicePointer(&pe, C.out_e + (J.lo - C.out_base), 0));
        J.d_score = reinterpret_cast<int32_t*>(ps);
        J.d_end = reinterpret_cast<int32_t*>(pe);
    }
    // pinned staging rings for pageable caller arrays, both allocated with capacity d->st_cap
    if ((need_in || need_out) && J.chunk > d->st_cap) {
        free_staging(d->st_in);
        free_staging(d->st_out);
        d->st_cap = (J.chunk + 63) & ~int64_t(63);  // (a slot's tile records start on 256 bytes)
    }
    if (need_in && !d->st_in) HIPCHK(d, alloc_staging(d->st_in, d->st_in_dev, d->st_cap));
    if (need_out && !d->st_out) {
        HIPCHK(d, alloc_staging(d->st_out, d->st_out_dev, d->st_cap));
    }
    if (C.timing && (int64_t)d->t_ev.size() < 2 * J.nchunks) {
        while ((int64_t)d->t_ev.size() < 2 * J.nchunks) {
            hipEvent_t ev;
            HIPCHK(d, hipEventCreate(&ev));
            d->t_ev.push_back(ev);
            HIPCHK(d, hipEventCreate(&ev));
            d->k_ev.push_back(ev);
        }
    }
    if (C.timing) J.kexact.assign((size_t)J.nchunks, 0);
    return OVL_OK;
}

thread_local PipeTrace* g_trace = nullptr;

// Compact host pair list, chunk k (C.compact): the host pool encodes the caller's int32 pairs into the pinned
// encoding buffer and kernels on the device's second stream decode them into HBM (ovl_pairs.hip), reading the
// encoding through the host mapping; the chunk's scoring launch waits for dec_ev[k].  Encoding of chunk k:
//   b: uint16 when n_reads <= 65,535 (an index outside [0, n_reads) becomes 0xFFFF, decoded to -1, which the
//      scoring kernels report as OVL_E_INDEX like any bad index), else the int32 values;
//   a: runs (value, chunk-relative start; starts[R] = n) when 8 R + 4 < n * width -- the candidate lists of
//      overlapGraphs.py:43-52 are a-major, ~55 pairs per run at the target point --, else like b.
// At the target point 4.3 MB cross the link instead of 16 MB.
int issue_chunk(const Call& C, Job& J, int64_t k);

// `pre` (the previous chunk's issue, when given) runs on the calling thread while the pool encodes
int encode_chunk(const Call& C, Job& J, int64_t k, const std::function<int()>& pre = nullptr) {
    Dev* d = J.d;
    int pre_rc = OVL_OK;
    bool pre_done = !pre;
    const std::function<void()> run_pre = [&] {
        if (!pre_done) {
            pre_done = true;
            pre_rc = pre();
        }
    };
    const int64_t off = J.cb[(size_t)k];
    const int64_t n = J.cb[(size_t)k + 1] - off;
    const int64_t g = J.lo + off;
    const int32_t* A = C.h_a + g;
    const int32_t* B = C.h_b + g;
    const int32_t nr = d->n_reads;
    const PairLayout lay = chunk_layout(J, k);
    const int wd = (int)lay.width;
    char* hb = d->cp_host + lay.base();            // b area
    char* ha = d->cp_host + lay.a();               // a area: tile deltas + bases, runs, or a like b
    CopyPool& pool = CopyPool::get();
    const std::vector<size_t> parts = pool.cut((size_t)n, size_t(1) << 15);
    static const ovl_encode::Fns enc = ovl_encode::pick(nullptr);  // the widest this CPU runs
    J.ixk.resize((size_t)J.nchunks, 0);
    J.ixk[(size_t)k] = 0;
    // In place (uniform_kernel IX): b as uint16 and a as tile deltas (d8[p] = a[p] - a[64t], bases int32),
    // 3 bytes per pair and 4 per tile, copied into HBM by the copy engine on the second stream (large DMA
    // reads; the kernel's own 64-byte reads through the host mapping ran at ~25 GB/s) while the previous
    // chunk scores, and read by the scoring launch as they lie -- no decode launch.  Needs a-major tiles (a
    // within 255 of its tile's first, every a in range; the parts are cut at multiples of 64) and a
    // throughput-mode uniform launch; else the decode below.
    // (OVL_TRACE_PIPE: 'x' marks a chunk that cannot be read in place, with the first failed condition)
    const int ix_why = wd != 2 ? 1 : !d->k.pairs_ix ? 2 : C.plan->kernel != OVL_KERNEL_UNGAPPED ? 3
                       : C.plan->key64 ? 4 : !ix_launch(d, n) ? 5 : 0;
    if (g_trace && ix_why) g_trace->mark('x', ix_why);
    if (ix_why == 0) {
        uint8_t* d8 = reinterpret_cast<uint8_t*>(d->cp_host + lay.d8());
        int32_t* tb = reinterpret_cast<int32_t*>(d->cp_host + lay.tile_bases());
        std::vector<uint8_t> bad(parts.size(), 0);
        pool.parallel_parts(
            parts,
            [&](size_t i, size_t lo, size_t hi) {
                enc.narrow(B, nr, reinterpret_cast<uint16_t*>(hb), lo, hi);
                bad[i] = !enc.d8(A, nr, d8, tb, lo, hi);
            },
            run_pre);
        if (pre_rc != OVL_OK) return pre_rc;
        if (g_trace && std::find(bad.begin(), bad.end(), 1) != bad.end()) g_trace->mark('x', 6);
        if (std::find(bad.begin(), bad.end(), 1) == bad.end()) {
            J.ixk[(size_t)k] = 1;  // (issue_chunk copies the chunk into HBM and launches on it)
            if (g_trace) g_trace->mark('e', k);
            d->cp_link += lay.ix_link();
            return OVL_OK;
        }
    }
    // one pass: b, and the runs of a (a[i] != a[i - 1], and i == 0) into part-local lists, given up (kept
    // short) once a part has more than 1 run per 16 pairs -- then a crosses like b
    std::vector<std::vector<int32_t>> pv(parts.size()), ps(parts.size());
    std::vector<uint8_t> many(parts.size(), 0);
    pool.parallel_parts(parts, [&](size_t i, size_t lo, size_t hi) {
        if (wd == 2) enc.narrow(B, nr, reinterpret_cast<uint16_t*>(hb), lo, hi);
        else memcpy(reinterpret_cast<int32_t*>(hb) + lo, B + lo, sizeof(int32_t) * (hi - lo));
        // (thread-local lists, handed over at the end: the parts' vector objects share cache lines)
        const size_t cap = (hi - lo) / 16 + 1;
        std::vector<int32_t> vv(cap + 1), ss(cap + 1);
        size_t r = enc.runs(A, lo ? A[lo - 1] : (int32_t)~A[0], lo, hi, vv.data(), ss.data(), cap);
        if (r > cap) {
            many[i] = 1;
            r = 0;
        }
        vv.resize(r);
        ss.resize(r);
        pv[i] = std::move(vv);
        ps[i] = std::move(ss);
    }, run_pre);
    if (pre_rc != OVL_OK) return pre_rc;
    int64_t R = 0;
    bool runs = n < (int64_t(1) << 31);
    for (size_t i = 0; i + 1 < parts.size(); ++i) {
        runs = runs && !many[i];
        R += (int64_t)pv[i].size();
    }
    runs = runs && 8 * R + 4 < n * wd;
    int32_t* vals = reinterpret_cast<int32_t*>(d->cp_host + lay.run_values());
    int32_t* starts = reinterpret_cast<int32_t*>(d->cp_host + lay.run_starts(R));
    if (runs) {
        int64_t r = 0;
        for (size_t i = 0; i + 1 < parts.size(); ++i) {
            memcpy(vals + r, pv[i].data(), sizeof(int32_t) * pv[i].size());
            memcpy(starts + r, ps[i].data(), sizeof(int32_t) * ps[i].size());
            r += (int64_t)pv[i].size();
        }
    } else {
        // a like b (a second pass, for lists that are not a-major)
        pool.parallel_parts(parts, [&](size_t, size_t lo, size_t hi) {
            if (wd == 2) {
                enc.narrow(A, nr, reinterpret_cast<uint16_t*>(ha), lo, hi);
            } else {
                memcpy(reinterpret_cast<int32_t*>(ha) + lo, A + lo, sizeof(int32_t) * (hi - lo));
            }
        });
    }
    if (runs) starts[R] = (int32_t)n;
    if (g_trace) g_trace->mark('e', k);
    // decode on the second stream (host-mapped reads) into this chunk's slice of the HBM list
    HIPCHK(d, hipSetDevice(d->device));
    HIPCHK(d, ovl_launch_widen(d->cp_dev + lay.base(), wd, n, J.kb + off, d->s_in));
    if (runs) {
        HIPCHK(d, ovl_launch_runs(reinterpret_cast<int32_t*>(d->cp_dev + lay.run_values()),
                                  reinterpret_cast<int32_t*>(d->cp_dev + lay.run_starts(R)), R, J.ka + off, d->s_in));
    } else {
        HIPCHK(d, ovl_launch_widen(d->cp_dev + lay.a(), wd, n, J.ka + off, d->s_in));
    }
    HIPCHK(d, hipEventRecord(d->dec_ev[(size_t)k], d->s_in));
    d->cp_link += lay.decoded_link(runs, R);
    return OVL_OK;
}

// The kernels read the pair list and store the results through host mappings (no copy-engine transfers);
// pageable arrays are copied into / out of the pinned staging slots on the host.  (Round 1's copy-engine
// form -- H2D, kernel, D2H per chunk -- took 0.395 against 0.186 ms for the target point's step and is gone.)
int issue_chunk(const Call& C, Job& J, int64_t k) {
    Dev* d = J.d;
    HIPCHK(d, hipSetDevice(d->device));
    const int64_t off = J.cb[(size_t)k];
    const int64_t g = J.lo + off;
    const int64_t n = J.cb[(size_t)k + 1] - off;
    const bool staged_out = chunk_staged(C, J, k);
    const size_t nb = sizeof(int32_t) * (size_t)n;
    const int slot = chunk_slot(J, k);
    const size_t so = (size_t)slot * 2 * (size_t)d->st_cap;
    const bool staged_in = C.h_a && !C.in_pinned && !C.compact;
    // the slot's previous user, chunk k - kSlots, must be done (its staged results were drained already)
    if (staged_in && k >= kSlots && !chunk_staged(C, J, k - kSlots)) HIPCHK(d, wait_event(d, d->ev_k[slot]));
    const int32_t* ka;
    const int32_t* kb;
    LaunchIo io;
    io.sink = chunk_sink(J, k);
    io.flag = d->h_flag_dev;
    if (C.compact && J.ixk[(size_t)k]) {
        // read in place by uniform_kernel from its HBM copy (encode_chunk's layout of chunk k), copied by the
        // copy engine on the second stream
        const PairLayout lay = chunk_layout(J, k);
        char* hbm = as<char>(d->cp_hbm);
        HIPCHK(d, hipMemcpyAsync(hbm + lay.base(), d->cp_host + lay.base(), lay.ix_bytes(), hipMemcpyHostToDevice,
                                 d->s_in));
        HIPCHK(d, hipEventRecord(d->dec_ev[(size_t)k], d->s_in));
        HIPCHK(d, hipStreamWaitEvent(d->stream, d->dec_ev[(size_t)k], 0));
        io.ix_b16 = reinterpret_cast<const uint16_t*>(hbm + lay.base());
        io.ix_d8 = reinterpret_cast<const uint8_t*>(hbm + lay.d8());
        io.ix_base = reinterpret_cast<const int32_t*>(hbm + lay.tile_bases());
        ka = kb = nullptr;
    } else if (C.compact) {
        // decoded into HBM by encode_chunk's kernels on the second stream
        HIPCHK(d, hipStreamWaitEvent(d->stream, d->dec_ev[(size_t)k], 0));
        ka = J.ka + off;
        kb = J.kb + off;
    } else if (C.h_a) {
        if (staged_in) {
            host_copy(d->st_in + so, C.h_a + g, nb);
            host_copy(d->st_in + so + d->st_cap, C.h_b + g, nb);
            ka = d->st_in_dev + so;
            kb = d->st_in_dev + so + d->st_cap;
        } else {
            ka = J.za + off;
            kb = J.zb + off;
        }
    } else {
        ka = J.dev_a + g;
        kb = J.dev_b + g;
    }
    int32_t* os = staged_out ? d->st_out_dev + so : J.d_score + off;
    int32_t* oe = staged_out ? d->st_out_dev + so + d->st_cap : J.d_end + off;
    hipStream_t ks = d->stream;
    if (C.timing) {
        HIPCHK(d, hipEventRecord(d->t_ev[2 * k], ks));
        if (C.plan->kernel == OVL_KERNEL_UNGAPPED) {  // (a chunk of one ungapped launch: time the kernel itself)
            io.kev_start = d->k_ev[2 * k];
            io.kev_stop = d->k_ev[2 * k + 1];
        }
    }
    int rc = launch_score(d, *C.plan, {ka, kb, n}, C.sc, {os, oe}, io, ks);
    if (C.timing) J.kexact[(size_t)k] = io.timed;
    if (rc != OVL_OK) return rc;
    if (C.timing) HIPCHK(d, hipEventRecord(d->t_ev[2 * k + 1], ks));
    if (staged_in || staged_out) HIPCHK(d, hipEventRecord(d->ev_k[slot], ks));
    if (C.pack && C.out_pinned && J.n_packed < J.nchunks && k == J.nchunks - 1)
        HIPCHK(d, hipEventRecord(d->ev_last, ks));
    return OVL_OK;
}

// Pageable outputs: copy chunk k out of its staging slot once its results are there (the kernel that stored
// them has finished).
int drain_chunk(const Call& C, Job& J, int64_t k) {
    Dev* d = J.d;
    const int64_t off = J.cb[(size_t)k];
    const int64_t g = J.lo + off;
    const int64_t n = J.cb[(size_t)k + 1] - off;
    const int slot = chunk_slot(J, k);
    HIPCHK(d, wait_event(d, d->ev_k[slot]));
    if (g_trace) g_trace->mark('w', k);
    struct Drained {
        int64_t k;
        ~Drained() {
            if (g_trace) g_trace->mark('d', k);
        }
    } drained{k};
    const int32_t* ss = d->st_out + (size_t)slot * 2 * (size_t)d->st_cap;
    if (C.pack) {
        host_expand(C.out_s + (g - C.out_base), C.out_e + (g - C.out_base), reinterpret_cast<const uint16_t*>(ss),
                    ss + d->st_cap, C.sc.match, C.sc.mismatch, true, (size_t)n, kExpandPart);
        return OVL_OK;
    }
    host_copy(C.out_s + (g - C.out_base), ss, sizeof(int32_t) * (size_t)n);
    host_copy(C.out_e + (g - C.out_base), ss + d->st_cap, sizeof(int32_t) * (size_t)n);
    return OVL_OK;
}

void quiesce(std::vector<Job>& jobs) {
    for (Job& J : jobs) {
        (void)hipSetDevice(J.d->device);
        for (hipStream_t s : {J.d->stream, J.d->s_in}) (void)hipStreamSynchronize(s);
    }
}

// One device's share of a host-array call: its chunks issued and drained in order.  A compact pair list (one device)
// has chunk k issued by this thread while the pool encodes chunk k + 1; staged chunks are drained kSlots - 1
// behind (a streamed record chunk once the chunk after it is queued: its kernel follows on the device while the
// host expands).  With `sync`, the job ends with its streams synchronised (device workers).
int run_job(const Call& C, Job& J, bool sync) {
    int rc = setup_job(C, J);
    if (rc != OVL_OK) return rc;
    if (g_trace) g_trace->mark('s', 0);
    if (C.compact && J.nchunks > 0 && (rc = encode_chunk(C, J, 0)) != OVL_OK) return rc;
    for (int64_t k = 0; k < J.nchunks && rc == OVL_OK; ++k) {
        const auto issue = [&]() -> int {
            const int r = issue_chunk(C, J, k);
            if (g_trace) g_trace->mark('i', k);
            return r;
        };
        if (C.compact && k + 1 < J.nchunks) rc = encode_chunk(C, J, k + 1, issue);
        else rc = issue();
        if (rc != OVL_OK) break;
        while (J.drained <= k) {
            const int64_t j = J.drained;
            if (chunk_staged(C, J, j) && k - j < kSlots - 1) break;
            if (chunk_staged(C, J, j) && (rc = drain_chunk(C, J, j)) != OVL_OK) break;
            ++J.drained;
        }
    }
    for (; rc == OVL_OK && J.drained < J.nchunks; ++J.drained)
        if (chunk_staged(C, J, J.drained)) rc = drain_chunk(C, J, J.drained);
    if (rc == OVL_OK && sync && J.nchunks > 0) {
        HIPCHK(J.d, hipSetDevice(J.d->device));
        HIPCHK(J.d, hipStreamSynchronize(J.d->stream));
    }
    return rc;
}

// Host-side shard bounds of a host pair list over the context's devices (cost len[a]*len[b] + 1,
// the rule of ovl_shard_cut).  Indices are not trusted here: an out-of-range index costs 1.
std::vector<int64_t> host_cuts(const ovl_ctx* c, const int32_t* a, const int32_t* b, int64_t n, int32_t shards) {
    std::vector<int64_t> cuts((size_t)shards + 1, 0);
    cuts[(size_t)shards] = n;
    if (shards == 1 || n == 0) {
        for (int32_t r = 1; r < shards; ++r) cuts[(size_t)r] = 0;
        return cuts;
    }
    const int64_t nr = (int64_t)c->h_len.size();
    auto cost = [&](int64_t p) -> int64_t {
        const int32_t x = a[p], y = b[p];
        if (x < 0 || x >= nr || y < 0 || y >= nr) return 1;
        return (int64_t)c->h_len[(size_t)x] * c->h_len[(size_t)y] + 1;
    };
    int64_t total = 0;
    for (int64_t p = 0; p < n; ++p) total += cost(p);
    int64_t cum = 0, p = 0;
    for (int32_t r = 1; r < shards; ++r) {
        const int64_t want = total * r;
        while (p < n && (cum + cost(p)) * shards < want) cum += cost(p++);
        cuts[(size_t)r] = p;  // first p with cum[p] * shards >= want
    }
    return cuts;
}

}  // namespace

int run_pipeline(ovl_ctx* c, const Call& C, std::vector<Job>& jobs) {
    const auto t0 = std::chrono::steady_clock::now();
    PipeTrace trace;
    g_trace = &trace;
    struct Unset {
        ~Unset() { g_trace = nullptr; }
    } unset;
    int rc = OVL_OK;
    // the kernels flag a bad pair index by storing into the device's pinned host flag (issue_chunk passes it), which
    // the host reads after the call's synchronisation (no flag copy behind the results)
    for (Job& J : jobs) *(volatile uint32_t*)J.d->h_flag = 0;
    if (jobs.size() == 1) {
        rc = run_job(C, jobs[0], false);
    } else {
        // several devices: each device's job on its own host thread (DevWorker, on the GPU's NUMA node), so the
        // devices' launches, polls and synchronisations run side by side; this thread waits for all of them
        std::vector<int> rcs(jobs.size(), OVL_OK);
        std::atomic<int> left{(int)jobs.size()};
        std::mutex mu;
        std::condition_variable cv;
        for (size_t i = 0; i < jobs.size(); ++i) {
            Dev* d = jobs[i].d;
            if (!d->worker) d->worker.reset(new DevWorker(d->device));
            d->worker->post([&, i] {
                rcs[i] = run_job(C, jobs[i], true);
                if (left.fetch_sub(1, std::memory_order_acq_rel) == 1) {
                    std::lock_guard<std::mutex> lk(mu);
                    cv.notify_all();
                }
            });
        }
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return left.load(std::memory_order_acquire) == 0; });
        }
        for (size_t i = 0; i < jobs.size(); ++i)
            if (rcs[i] != OVL_OK) {
                rc = rcs[i];
                break;
            }
    }
    if (rc != OVL_OK) {
        quiesce(jobs);
        return rc;
    }
    // pack_share: the direct share of packed calls into pinned arrays follows which side finished last.  The
    // host pool has expanded every packed chunk now; if the direct chunk is already done, the link idled
    // while the host worked (more direct), if the host still waits for it, the host idles (more packed).
    constexpr double kShareWaitUs = 8.0;  // the host's wait for the direct chunk that counts as idling
    for (Job& J : jobs) {
        Dev* d = J.d;
        if (!C.pack || !C.out_pinned || J.n_packed >= J.nchunks || !d->k.pack_adapt) continue;
        const auto tw = std::chrono::steady_clock::now();
        const hipError_t q = hipEventQuery(d->ev_last);
        double& share = pack_share(C, d);
        if (q == hipSuccess) {
            share = std::min(C.compact ? 80.0 : 50.0, share + 1.0);
        } else if (q == hipErrorNotReady) {
            HIPCHK(c, wait_event(d, d->ev_last));
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tw).count();
            if (us > kShareWaitUs) share = std::max(2.0, share - 1.0);
        }
    }
    for (Job& J : jobs) {
        if (J.nchunks == 0) continue;
        HIPCHK(c, hipSetDevice(J.d->device));
        HIPCHK(c, hipStreamSynchronize(J.d->stream));
    }
    trace.mark('y', 0);
    double kms = 0.0;
    c->t_launches.clear();
    for (Job& J : jobs) {
        Dev* d = J.d;
        if (J.nchunks == 0) continue;
        if (*(volatile uint32_t*)d->h_flag) {
            *d->h_flag = 0;
            rc = fail(c, OVL_E_INDEX, "a pair index is outside [0, %d)", d->n_reads);
        }
        if (C.timing) {
            double s = 0.0;
            for (int64_t k = 0; k < J.nchunks; ++k) {
                float ms = 0.f;
                const bool exact = k < (int64_t)J.kexact.size() && J.kexact[(size_t)k];
                const hipEvent_t* ev = exact ? &d->k_ev[2 * (size_t)k] : &d->t_ev[2 * (size_t)k];
                if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) s += ms;
                // the chunk's result sink (issue_chunk): packed staging, or int32 into host memory
                const int64_t n = J.cb[(size_t)k + 1] - J.cb[(size_t)k];
                c->t_launches.push_back({d->device, chunk_sink(J, k), n, (double)ms});
            }
            kms = std::max(kms, s);
        }
    }
    c->t_kernel_ms = kms;
    c->t_call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    int64_t link = 0, packed = 0, ix = 0, dec = 0, res_all = 0;
    for (const Job& J : jobs) {
        const int64_t n = J.hi - J.lo;
        if (n <= 0) continue;
        const int64_t np = J.n_packed ? J.cb[(size_t)J.n_packed] : 0;
        packed += np;
        const int64_t res = 8 * (n - np) + 2 * np;  // results: int32 pairs, 2 bytes per packed pair
        res_all += res;
        link += (C.compact ? J.d->cp_link : (C.h_a ? 8 * n : 0)) + res;
        if (C.compact)
            for (int64_t k = 0; k < J.nchunks; ++k)
                (J.ixk[(size_t)k] ? ix : dec) += J.cb[(size_t)k + 1] - J.cb[(size_t)k];
    }
    c->x_link_bytes = link;
    c->x_packed_pairs = packed;
    c->x_res_bytes = res_all;
    c->x_rec_pairs = 0;  // (tile records: the resident grid's calls, resident_call)
    c->x_esc = 0;
    c->x_ix_pairs = ix;
    c->x_dec_pairs = dec;
    return rc;
}

// Shard bounds of [lo, hi) of device 0's resident candidate list over `shards` (ovl_shard_cut).
int device_cuts(Dev* d, int64_t lo, int64_t hi, int32_t shards, std::vector<int64_t>& cuts) {
    cuts.assign((size_t)shards + 1, lo);
    cuts[(size_t)shards] = hi;
    if (shards == 1 || hi <= lo) return OVL_OK;
    HIPCHK(d, hipSetDevice(d->device));
    const int64_t n = d->cand_n;
    size_t temp = 0;
    HIPCHK(d, ovl_shard_temp_bytes(n, &temp));
    HIPCHK(d, ensure(d->sh_temp, temp));
    HIPCHK(d, ensure(d->sh_cum, (size_t)n * sizeof(int64_t)));
    HIPCHK(d, ensure(d->sh_cuts, ((size_t)shards + 1) * sizeof(int64_t)));
    HIPCHK(d, ovl_shard_scan(d->sh_temp.p, d->sh_temp.bytes, as<int32_t>(d->cand_a), as<int32_t>(d->cand_b),
                             as<int32_t>(d->len), n, as<int64_t>(d->sh_cum), d->stream));
    HIPCHK(d, ovl_shard_cut(as<int64_t>(d->sh_cum), lo, hi, shards, as<int64_t>(d->sh_cuts), d->stream));
    HIPCHK(d, hipMemcpyAsync(cuts.data(), d->sh_cuts.p, ((size_t)shards + 1) * sizeof(int64_t), hipMemcpyDeviceToHost,
                             d->stream));
    HIPCHK(d, hipStreamSynchronize(d->stream));
    return OVL_OK;
}

// Direct host-array calls move results packed (ovl_sweep.h put_pair, sink 2: end and mismatch count
// in a uint16) when the uniform kernel scores them with int32 keys and reads are at most 254 bases (ends
// and mismatch counts below the 0xFF marker).  One-device contexts only: the calling thread's host pool
// expands every packed chunk, so N devices would funnel N links' results through one pool, where int32
// results take N links in parallel (one process per GPU packs per process).
//   From OVL_PACK_MIN pairs into pinned arrays (256 K: tools/pack_size_ab.py, first n pairs of the target
// list, int32 / packed ms: 131 K 0.040 / 0.041, 262 K 0.065 / 0.057, 524 K 0.099 / 0.082, 1 M 0.182 / 0.100),
// from a quarter of that into pageable arrays, which need a host pass anyway (cfg2, 122 K pairs: 0.052-0.065
// against 0.065-0.079 ms; profiles/r02_pack_ab_cfg2_*.json, profiles/r02_pack_size_*.json).
bool pack_ok(const ovl_ctx* c, const Plan& p, int64_t n_pairs, bool out_pinned, int32_t n_devices) {
    const Dev* d = c->devs[0];
    const int64_t min_pairs = out_pinned ? d->k.pack_min : d->k.pack_min / 4;
    // (the expansion needs the host pool: with fewer than 6 threads -- several processes on one CPU set, e.g.
    // joblib workers or many ranks on one quota (CpuShare) -- the int32 stores over the link are faster)
    return n_devices == 1 && d->k.pack && n_pairs >= min_pairs && CopyPool::threads() >= 6 &&
           p.kernel == OVL_KERNEL_UNGAPPED && !p.key64 &&
           d->planes == 2 &&
           d->wmax > 0 && d->lmax > 0 && d->lmax <= 254;  // (lmax 0: the general kernel scores the list)
}

// Devices (the context's first S) a host-array call over n pairs uses.  Calls over several devices store int32
// results over each device's own link (no packing: one host pool would expand every link's results), ~145 us per
// M pairs per link at 55 GB/s, against ~70 us per M pairs for one device with packed results and its resident grid
// or packed launches: several devices pay only from 3 of them, each with >= kMinPairsPerDevice
// pairs (their fixed per-call cost, ~15 us, against 36 us of link time).  Fewer -> one device, the single-device
// paths.  A context whose slots share a GPU (OVL_SHARE_DEVICES=1, tests) uses every slot.
constexpr int64_t kMinPairsPerDevice = int64_t(1) << 18;
int32_t devices_for(const ovl_ctx* c, int64_t n_pairs) {
    const int32_t k = (int32_t)c->devs.size();
    if (k <= 1) return 1;
    const int32_t s = (int32_t)std::min<int64_t>(k, n_pairs / kMinPairsPerDevice);
    return s >= 3 ? s : 1;
}
int32_t devices_used(const ovl_ctx* c, int64_t n_pairs) {
    return c->shared_slots ? (int32_t)c->devs.size() : devices_for(c, n_pairs);
}

// The Call of a host-array scoring call over n_pairs pairs -- a host pair list (h_a, h_b), or null: the resident list
// from out_base -- and in *n_devices the devices it uses.
Call make_call(ovl_ctx* c, const Plan& p, const Scoring& sc, const int32_t* h_a, const int32_t* h_b, int64_t n_pairs,
               int32_t* out_s, int32_t* out_e, int64_t out_base, int32_t* n_devices) {
    const size_t bytes = sizeof(int32_t) * (size_t)n_pairs;
    const int32_t S = *n_devices = devices_used(c, n_pairs);
    Call C;
    C.plan = &p;
    C.sc = sc;
    C.h_a = h_a;
    C.h_b = h_b;
    C.in_pinned = h_a && host_pinned(h_a, bytes) && host_pinned(h_b, bytes);
    C.out_s = out_s;
    C.out_e = out_e;
    C.out_base = out_base;
    C.out_pinned = host_pinned(out_s, bytes) && host_pinned(out_e, bytes);
    C.timing = c->timing != 0;
    C.pack = pack_ok(c, p, n_pairs, C.out_pinned, S);
    C.compact = h_a && S == 1 && c->devs[0]->k.compact && n_pairs >= kCompactMin;
    return C;
}

// One job per device from the shard bounds; `resident_list`: each over its device's resident candidate list
std::vector<Job> jobs_from_cuts(ovl_ctx* c, const std::vector<int64_t>& cuts, bool resident_list) {
    std::vector<Job> jobs(cuts.size() - 1);
    for (size_t r = 0; r < jobs.size(); ++r) {
        Job& J = jobs[r];
        J.d = c->devs[r];
        J.lo = cuts[r];
        J.hi = cuts[r + 1];
        if (resident_list) {
            J.dev_a = as<int32_t>(J.d->cand_a);
            J.dev_b = as<int32_t>(J.d->cand_b);
        }
    }
    return jobs;
}

OVL_API int ovl_score_host(ovl_ctx* c, const int32_t* a_idx, const int32_t* b_idx, int64_t n_pairs, int32_t match,
                           int32_t mismatch, int64_t indel, int32_t band, int32_t* out_score, int32_t* out_end) {
    if (!c) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    quiet(c);
    if (n_pairs < 0) return fail(c, OVL_E_ARG, "n_pairs < 0");
    if (n_pairs > 0 && (!a_idx || !b_idx || !out_score || !out_end))
        return fail(c, OVL_E_ARG, "NULL host pointer");
    Plan p;
    int rc = check_scoring_args(c, match, mismatch, indel, band, &p);
    if (rc != OVL_OK) return rc;
    if (n_pairs == 0) return OVL_OK;
    if (c->devs[0]->n_reads == 0) return fail(c, OVL_E_INDEX, "pairs given but the read set is empty");
    DeviceGuard guard;
    int32_t S = 1;
    const Call C = make_call(c, p, {match, mismatch, indel}, a_idx, b_idx, n_pairs, out_score, out_end, 0, &S);
    std::vector<Job> jobs = jobs_from_cuts(c, host_cuts(c, a_idx, b_idx, n_pairs, S), false);
    return run_pipeline(c, C, jobs);
}

OVL_API int ovl_score_pairs(ovl_ctx* c, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads,
                            const int32_t* a_idx, const int32_t* b_idx, int64_t n_pairs, int32_t match,
                            int32_t mismatch, int64_t indel, int32_t band, int32_t* out_score, int32_t* out_end) {
    // the read upload runs on the devices while the host encodes the pair list's first chunk; the scoring
    // launches queue behind it on the same streams
    int rc = set_reads(c, seqs, offsets, n_reads, false);
    if (rc != OVL_OK) return rc;
    rc = ovl_score_host(c, a_idx, b_idx, n_pairs, match, mismatch, indel, band, out_score, out_end);
    DeviceGuard guard;
    for (Dev* d : c->devs) {  // (the stage outlives the copy; an upload error surfaces here if nothing else did)
        (void)hipSetDevice(d->device);
        const hipError_t e = hipStreamSynchronize(d->stream);
        if (rc == OVL_OK && e != hipSuccess)
            rc = fail(c, OVL_E_HIP, "ovl_score_pairs: read upload: %s", hipGetErrorString(e));
    }
    return rc;
}
