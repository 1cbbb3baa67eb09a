// ovl_cand.cpp — the device candidate list (ovl_ctx.h): its enumeration on every device, its shard bounds, and
// scoring calls over it, through the resident grid (ovl_resident.h) or the launch pipeline.
#include "ovl_ctx.h"

namespace {

// The resident list's consumers are sized for fewer than 2^31 pairs (device_cuts' cost sums, the tile ids of
// ensure_heavy); a seed list can pass that where the reference's rule would not.
constexpr int64_t kSeedMaxPairs = (int64_t(1) << 31) - 1;

// What ovl_seed_candidates' rule adds to an enumeration (null: ovl_candidates' rule)
struct SeedRule {
    int32_t n_long, max_off;
    bool timing;
};

OvlSeedArgs seed_args(Dev* c, int32_t k, const SeedRule& r) {
    OvlSeedArgs s{};
    s.codes = as<uint8_t>(c->codes);
    s.off = as<int64_t>(c->off);
    s.len = as<int32_t>(c->len);
    s.n_reads = c->n_reads;
    s.k = k;
    s.bits = c->planes;  // symbol codes are dense: < 2^planes
    s.sorted = as<uint64_t>(c->k_sorted);
    s.order = as<int32_t>(c->k_order);
    s.n_long = r.n_long;
    s.pre_key = as<uint64_t>(c->k_pre);
    s.max_off = r.max_off;
    s.grp_lo = as<int32_t>(c->sd.glo);
    s.grp_n = as<int32_t>(c->sd.gn);
    s.cnt = as<int64_t>(c->k_cnt);
    s.offs = as<int64_t>(c->k_offs);
    s.out_a = as<int32_t>(c->cand_a);
    s.out_b = as<int32_t>(c->cand_b);
    s.out_o = as<int32_t>(c->sd.offs);
    return s;
}

// The first half of an enumeration by either rule: keys, sort, per-read counts and their offsets; the list length
// comes back in c->cand_tail.  ovl_candidates' rule (seed null) drops the resident list first and, at k = 0, needs no
// keys; the seed rule works in scratch only (the resident list is untouched) and marks its phases for timing.
int enum_count(Dev* c, int32_t k, const SeedRule* seed) {
    HIPCHK(c, hipSetDevice(c->device));
    if (!seed) {
        c->cand_n = -1;
        c->heavy_for = -1;
    }
    const int32_t n = c->n_reads;
    const size_t nr = (size_t)std::max(n, 1);
    const bool keyed = seed || k != 0;
    hipStream_t s = c->stream;
    for (DevBuf* b : {&c->k_cnt, &c->k_offs}) HIPCHK(c, ensure(*b, nr * sizeof(int64_t)));
    if (!seed)
        for (DevBuf* b : {&c->k_lo, &c->k_hi}) HIPCHK(c, ensure(*b, nr * sizeof(int64_t)));
    if (keyed) {
        for (DevBuf* b : {&c->k_pre, &c->k_sorted}) HIPCHK(c, ensure(*b, nr * sizeof(uint64_t)));
        for (DevBuf* b : {&c->k_iota, &c->k_order}) HIPCHK(c, ensure(*b, nr * sizeof(int32_t)));
        if (!seed) HIPCHK(c, ensure(c->k_suf, nr * sizeof(uint64_t)));
    }
    if (seed && c->k.seed_keep)
        for (DevBuf* b : {&c->sd.glo, &c->sd.gn})
            HIPCHK(c, ensure(*b, (size_t)std::max<int64_t>(c->codes_bytes, 1) * sizeof(int32_t)));
    size_t temp = 0;
    HIPCHK(c, ovl_cand_temp_bytes(n, &temp));
    HIPCHK(c, ensure(c->k_temp, temp));
    StageTimer<6>& t = c->sd.timer;
    HIPCHK(c, t.arm(seed && seed->timing));
    HIPCHK(c, t.mark(0, s));
    if (seed)
        HIPCHK(c, ovl_seed_keys(as<uint8_t>(c->codes), as<int64_t>(c->off), as<int32_t>(c->len), n, k, c->planes,
                                as<uint64_t>(c->k_pre), as<int32_t>(c->k_iota), s));
    else if (keyed)
        HIPCHK(c, ovl_cand_keys(as<uint8_t>(c->codes), as<int64_t>(c->off), as<int32_t>(c->len), n, k, c->planes,
                                as<uint64_t>(c->k_pre), as<uint64_t>(c->k_suf), as<int32_t>(c->k_iota), s));
    HIPCHK(c, t.mark(1, s));
    if (keyed)
        HIPCHK(c, ovl_cand_sort(c->k_temp.p, c->k_temp.bytes, as<uint64_t>(c->k_pre), as<uint64_t>(c->k_sorted),
                                as<int32_t>(c->k_iota), as<int32_t>(c->k_order), n, s));
    HIPCHK(c, t.mark(2, s));
    if (!seed) {
        HIPCHK(c, ovl_cand_count(as<uint64_t>(c->k_sorted), as<uint64_t>(c->k_pre), as<uint64_t>(c->k_suf), n,
                                 keyed ? 0 : 1, as<int64_t>(c->k_lo), as<int64_t>(c->k_hi), as<int64_t>(c->k_cnt), s));
    } else if (seed->max_off > 0) {
        const OvlSeedArgs a = seed_args(c, k, *seed);
        HIPCHK(c, ovl_seed_count(&a, c->k.seed_keep, s));
    } else if (n > 0) {  // no read is longer than k
        HIPCHK(c, hipMemsetAsync(c->k_cnt.p, 0, (size_t)n * sizeof(int64_t), s));
    }
    HIPCHK(c, ovl_cand_scan(c->k_temp.p, c->k_temp.bytes, as<int64_t>(c->k_cnt), as<int64_t>(c->k_offs), n, s));
    HIPCHK(c, t.mark(3, s));
    c->cand_tail[0] = c->cand_tail[1] = 0;
    if (n > 0) {
        HIPCHK(c, hipMemcpyAsync(&c->cand_tail[0], as<int64_t>(c->k_offs) + (n - 1), sizeof(int64_t),
                                 hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&c->cand_tail[1], as<int64_t>(c->k_cnt) + (n - 1), sizeof(int64_t),
                                 hipMemcpyDeviceToHost, s));
    }
    return OVL_OK;
}

int cand_emit(Dev* c, int32_t k) {
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t total = c->cand_tail[0] + c->cand_tail[1];
    HIPCHK(c, ensure(c->cand_a, (size_t)total * sizeof(int32_t)));
    HIPCHK(c, ensure(c->cand_b, (size_t)total * sizeof(int32_t)));
    if (total > 0)
        HIPCHK(c, ovl_cand_emit(as<int32_t>(c->k_order), as<int64_t>(c->k_lo), as<int64_t>(c->k_hi),
                                as<int64_t>(c->k_offs), c->n_reads, k == 0 ? 1 : 0, as<int32_t>(c->cand_a),
                                as<int32_t>(c->cand_b), c->stream));
    return OVL_OK;
}

int seed_emit(Dev* c, int32_t k, const SeedRule& r, int64_t total) {
    HIPCHK(c, hipSetDevice(c->device));
    c->cand_n = -1;  // from here the previous list is gone
    c->heavy_for = -1;
    for (DevBuf* b : {&c->cand_a, &c->cand_b, &c->sd.offs}) HIPCHK(c, ensure(*b, (size_t)total * sizeof(int32_t)));
    const OvlSeedArgs a = seed_args(c, k, r);
    HIPCHK(c, c->sd.timer.mark(4, c->stream));
    if (total > 0) HIPCHK(c, ovl_seed_emit(&a, c->k.seed_keep, c->stream));
    HIPCHK(c, c->sd.timer.mark(5, c->stream));
    return OVL_OK;
}

}  // namespace

OVL_API int ovl_candidates(ovl_ctx* ctx, int32_t k, int64_t* out_n_pairs) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    quiet(ctx);
    if (!out_n_pairs) return fail(ctx, OVL_E_ARG, "out_n_pairs is NULL");
    if (k < 0) return fail(ctx, OVL_E_ARG, "k-mer length must be non-negative (k=%d)", k);
    Dev* d0 = ctx->devs[0];
    if (d0->n_reads < 0) return fail(ctx, OVL_E_STATE, "no resident reads: call ovl_set_reads first");
    const int32_t bits = d0->planes;
    if (k > 0 && (int64_t)k * bits > 58)
        return fail(ctx, OVL_E_UNSUPPORTED, "k=%d with %d-bit symbols does not fit a 64-bit key (k * bits <= 58)", k,
                    bits);
    DeviceGuard guard;
    CpuShare::get().refresh();
    // every device enumerates the same list from its own copy of the reads (no list broadcast); the
    // phases overlap across devices
    int rc = OVL_OK;
    for (Dev* d : ctx->devs)
        if ((rc = enum_count(d, k, nullptr)) != OVL_OK) break;
    if ((rc = sync_devices(ctx, rc, "ovl_candidates")) != OVL_OK) return rc;
    for (Dev* d : ctx->devs)
        if ((rc = cand_emit(d, k)) != OVL_OK) break;
    if ((rc = sync_devices(ctx, rc, "ovl_candidates")) != OVL_OK) return rc;
    const int64_t total = d0->cand_tail[0] + d0->cand_tail[1];
    for (Dev* d : ctx->devs) {
        d->cand_n = total;
        d->cand_seed = false;
        d->heavy_for = -1;  // a new list: heavy tiles rebuilt on its first launch
    }
    *out_n_pairs = total;
    return OVL_OK;
}

OVL_API int ovl_seed_candidates(ovl_ctx* ctx, int32_t k, int64_t* out_n_pairs) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    if (!out_n_pairs) return fail(ctx, OVL_E_ARG, "out_n_pairs is NULL");
    if (k < 1) return fail(ctx, OVL_E_ARG, "seed candidates need a k-mer length of at least 1 (k=%d)", k);
    Dev* d0 = ctx->devs[0];
    if (d0->n_reads < 0) return fail(ctx, OVL_E_STATE, "no resident reads: call ovl_set_reads first");
    const int32_t bits = d0->planes;
    if ((int64_t)k * bits > 58)
        return fail(ctx, OVL_E_UNSUPPORTED, "k=%d with %d-bit symbols does not fit a 64-bit key (k * bits <= 58)", k,
                    bits);
    SeedRule rule{0, std::max(d0->lmax - k, 0), ctx->timing != 0};
    if (rule.max_off > OVL_SEED_MAX_OFFSETS)
        return fail(ctx, OVL_E_UNSUPPORTED, "seed candidates take reads of up to k + %d bases (longest is %d)",
                    OVL_SEED_MAX_OFFSETS, d0->lmax);
    for (int32_t l : ctx->h_len) rule.n_long += l >= k ? 1 : 0;
    quiet(ctx);
    DeviceGuard guard;
    CpuShare::get().refresh();
    // every device enumerates the same list from its own copy of the reads, as in ovl_candidates
    int rc = OVL_OK;
    for (Dev* d : ctx->devs)
        if ((rc = enum_count(d, k, &rule)) != OVL_OK) break;
    if ((rc = sync_devices(ctx, rc, "ovl_seed_candidates")) != OVL_OK) return rc;
    const int64_t total = d0->cand_tail[0] + d0->cand_tail[1];
    if (total > kSeedMaxPairs)
        return fail(ctx, OVL_E_UNSUPPORTED, "seed candidates: %lld pairs, the resident list holds up to %lld",
                    (long long)total, (long long)kSeedMaxPairs);
    for (Dev* d : ctx->devs)
        if ((rc = seed_emit(d, k, rule, total)) != OVL_OK) break;
    if ((rc = sync_devices(ctx, rc, "ovl_seed_candidates")) != OVL_OK) return rc;
    if (rule.timing) (void)hipSetDevice(d0->device);
    for (int i = 0; i < 4; ++i)  // keys, sort, count + scan; the emit has its own start
        d0->sd.last.ms[i] = d0->sd.timer.ms(i < 3 ? i : 4, i < 3 ? i + 1 : 5);
    for (Dev* d : ctx->devs) {
        d->cand_n = total;
        d->cand_seed = true;
        d->heavy_for = -1;
    }
    *out_n_pairs = total;
    return OVL_OK;
}

OVL_API int ovl_seed_offsets_copy(ovl_ctx* ctx, int32_t* out_offset) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    Dev* c = ctx->devs[0];
    if (c->cand_n < 0 || !c->cand_seed)
        return fail(c, OVL_E_STATE, "the resident candidate list did not come from ovl_seed_candidates");
    if (c->cand_n == 0) return OVL_OK;
    if (!out_offset) return fail(c, OVL_E_ARG, "NULL host pointer");
    DeviceGuard guard;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out_offset, c->sd.offs.p, (size_t)c->cand_n * sizeof(int32_t), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OVL_OK;
}

OVL_API int ovl_last_seed_timing(const ovl_ctx* ctx, double* keys_ms, double* sort_ms, double* count_ms,
                                 double* emit_ms) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    const double* ms = ctx->devs[0]->sd.last.ms;
    if (keys_ms) *keys_ms = ms[0];
    if (sort_ms) *sort_ms = ms[1];
    if (count_ms) *count_ms = ms[2];
    if (emit_ms) *emit_ms = ms[3];
    return OVL_OK;
}

OVL_API int ovl_candidates_copy(ovl_ctx* ctx, int32_t* a_idx, int32_t* b_idx) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    Dev* c = ctx->devs[0];
    if (c->cand_n < 0) return fail(c, OVL_E_STATE, "no candidate list: call ovl_candidates first");
    if (c->cand_n == 0) return OVL_OK;
    if (!a_idx || !b_idx) return fail(c, OVL_E_ARG, "NULL host pointer");
    DeviceGuard guard;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)c->cand_n * sizeof(int32_t);
    StreamDrain drain(c->stream);
    HIPCHK(c, hipMemcpyAsync(a_idx, c->cand_a.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(b_idx, c->cand_b.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    drain.armed = false;
    return OVL_OK;
}

OVL_API int ovl_candidates_device(const ovl_ctx* ctx, const int32_t** d_a_idx, const int32_t** d_b_idx,
                                  int64_t* n_pairs) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    const Dev* c = ctx->devs[0];
    if (c->cand_n < 0) return fail(c, OVL_E_STATE, "no candidate list: call ovl_candidates first");
    if (d_a_idx) *d_a_idx = reinterpret_cast<const int32_t*>(c->cand_a.p);
    if (d_b_idx) *d_b_idx = reinterpret_cast<const int32_t*>(c->cand_b.p);
    if (n_pairs) *n_pairs = c->cand_n;
    return OVL_OK;
}

OVL_API int ovl_candidates_shards(ovl_ctx* ctx, int32_t n_shards, int64_t* bounds) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    quiet(ctx);
    if (n_shards <= 0 || !bounds) return fail(ctx, OVL_E_ARG, "n_shards <= 0 or bounds is NULL");
    Dev* d = ctx->devs[0];
    if (d->cand_n < 0) return fail(ctx, OVL_E_STATE, "no candidate list: call ovl_candidates first");
    DeviceGuard guard;
    std::vector<int64_t> cuts;
    int rc = device_cuts(d, 0, d->cand_n, n_shards, cuts);
    if (rc != OVL_OK) return rc;
    std::copy(cuts.begin(), cuts.end(), bounds);
    return OVL_OK;
}

namespace {

constexpr int kResidentFellBack = 1000;  // (resident_call: the call goes through the launch pipeline instead)

// A call over the resident candidate list that the resident grid scores: one device, the uniform kernel's form with
// int32 keys and 2-byte record codes (ends <= 254), timing off (its launch events time the launch pipeline), and a
// host pool of at least 6 threads to expand the records (fewer: several processes share the CPUs, pack_ok)
bool resident_ok(const ovl_ctx* c, const Plan& p, int64_t n) {
    if (devices_used(c, n) != 1 || c->timing || CopyPool::threads() < 6) return false;
    const Dev* d = c->devs[0];
    if (d->k.resident == 0 || d->res.broken) return false;
    if (d->k.resident == 1 && (n < d->k.resident_min || n > d->k.resident_max)) return false;
    return p.kernel == OVL_KERNEL_UNGAPPED && !p.key64 && d->planes == 2 && d->wmax >= 1 && d->wmax <= 8 &&
           d->lmax >= 1 && d->lmax <= 254 && d->cand_n >= 0;
}

int resident_call(ovl_ctx* ctx, int64_t lo, int64_t hi, int32_t match, int32_t mismatch, int32_t* out_s,
                  int32_t* out_e) {
    Dev* d = ctx->devs[0];
    HIPCHK(d, hipSetDevice(d->device));
    // heavy tiles first when the range starts on a list tile (uniform_kernel's order); built once per list, with the
    // grid stopped (ensure_heavy may reallocate)
    ResidentCall rc_;
    if (lo % 64 == 0) {
        if (d->heavy_for != d->cand_n) {
            (void)d->res.stop();
            const int r = ensure_heavy(d);
            if (r != OVL_OK) return r;
        }
        const HeavyWindow w = heavy_window(d, lo, hi - lo);
        rc_.heavy_ids = w.ids;
        rc_.heavy_n = w.count;
        rc_.tile_base = w.tile_base;
    }
    ResidentReads rd;
    rd.sfx = as<uint32_t>(d->sfx);
    rd.pfx = as<uint32_t>(d->pfx);
    rd.len = as<int32_t>(d->len);
    rd.n_reads = d->n_reads;
    rd.lw = d->lmax;
    rd.wmax = d->wmax;
    rd.full = as<uint32_t>(d->full);
    rd.tile_flags = rc_.heavy_n > 0 ? as<uint8_t>(d->tile_flags) : nullptr;
    rc_.d_a = as<int32_t>(d->cand_a) + lo;
    rc_.d_b = as<int32_t>(d->cand_b) + lo;
    rc_.n = hi - lo;
    rc_.match = match;
    rc_.mismatch = mismatch;
    rc_.out_s = out_s;
    rc_.out_e = out_e;
    const auto t0 = std::chrono::steady_clock::now();
    int64_t n_bad = 0;
    hipError_t e = hipSuccess;
    const int r = d->res.score(rd, rc_, &n_bad, &e);
    if (r == ResidentGrid::kFallback) return kResidentFellBack;
    if (r != ResidentGrid::kOk)
        return fail(ctx, OVL_E_HIP, "resident grid: %s", hipGetErrorString(e));
    ctx->t_launches.clear();
    ctx->t_kernel_ms = 0.0;
    ctx->t_call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const int64_t n = hi - lo, nt = (n + 63) / 64;
    ctx->x_res_bytes = 128 * nt + 8 * d->res.last_specials;
    ctx->x_link_bytes = ctx->x_res_bytes;
    ctx->x_packed_pairs = n;
    ctx->x_rec_pairs = n;
    ctx->x_esc = d->res.last_specials;
    ctx->x_ix_pairs = ctx->x_dec_pairs = 0;
    if (n_bad > 0) return fail(ctx, OVL_E_INDEX, "a pair index is outside [0, %d)", d->n_reads);
    return OVL_OK;
}

}  // namespace

OVL_API int ovl_devices_for(const ovl_ctx* ctx, int64_t n_pairs, int32_t* out_devices) {
    if (!ctx || !out_devices) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx or out_devices is NULL");
    if (n_pairs < 0) return fail(ctx, OVL_E_ARG, "n_pairs < 0");
    *out_devices = devices_for(ctx, n_pairs);
    return OVL_OK;
}

OVL_API int ovl_quiesce(ovl_ctx* ctx) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    DeviceGuard guard;
    for (Dev* d : ctx->devs) HIPCHK(ctx, d->res.stop());
    return OVL_OK;
}

OVL_API int ovl_resident_stats(const ovl_ctx* ctx, int32_t* alive, int64_t* launches, int64_t* relaunches,
                               int32_t* broken) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    int32_t al = 0, br = 0;
    int64_t l = 0, rl = 0;
    for (const Dev* d : ctx->devs) {
        al += d->res.alive() ? 1 : 0;
        br += d->res.broken ? 1 : 0;
        l += d->res.n_launches;
        rl += d->res.n_relaunches;
    }
    if (alive) *alive = al;
    if (launches) *launches = l;
    if (relaunches) *relaunches = rl;
    if (broken) *broken = br;
    return OVL_OK;
}

OVL_API int ovl_score_candidates_range(ovl_ctx* ctx, int64_t lo, int64_t hi, int32_t match, int32_t mismatch,
                                       int64_t indel, int32_t band, int32_t* out_score, int32_t* out_end) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    Dev* d0 = ctx->devs[0];
    if (d0->cand_n < 0) return fail(ctx, OVL_E_STATE, "no candidate list: call ovl_candidates first");
    if (lo < 0 || hi < lo || hi > d0->cand_n)
        return fail(ctx, OVL_E_ARG, "range [%lld, %lld) outside the candidate list [0, %lld)", (long long)lo,
                    (long long)hi, (long long)d0->cand_n);
    Plan p;
    int rc = check_scoring_args(ctx, match, mismatch, indel, band, &p);
    if (rc != OVL_OK) return rc;
    if (hi == lo) return OVL_OK;
    if (!out_score || !out_end) return fail(ctx, OVL_E_ARG, "NULL host pointer");
    DeviceGuard guard;
    if (resident_ok(ctx, p, hi - lo)) {
        rc = resident_call(ctx, lo, hi, match, mismatch, out_score, out_end);
        if (rc != kResidentFellBack) return rc;
    }
    quiet(ctx);
    int32_t S = 1;
    const Call C = make_call(ctx, p, {match, mismatch, indel}, nullptr, nullptr, hi - lo, out_score, out_end, lo, &S);
    std::vector<int64_t> cuts;
    rc = device_cuts(d0, lo, hi, S, cuts);
    if (rc != OVL_OK) return rc;
    std::vector<Job> jobs = jobs_from_cuts(ctx, cuts, true);
    return run_pipeline(ctx, C, jobs);
}

OVL_API int ovl_score_candidates(ovl_ctx* ctx, int32_t match, int32_t mismatch, int64_t indel, int32_t band,
                                 int32_t* out_score, int32_t* out_end) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    const int64_t n = ctx->devs[0]->cand_n;
    if (n < 0) return fail(ctx, OVL_E_STATE, "no candidate list: call ovl_candidates first");
    return ovl_score_candidates_range(ctx, 0, n, match, mismatch, indel, band, out_score, out_end);
}
