// ovl_plan.cpp — kernel choice per call (ovl_plan: the ungapped popcount kernel whenever gaps provably cannot win
// and the read store has a bit-plane layout, else a DP kernel) and the scoring launches (ovl_ctx.h).
#include "ovl_ctx.h"

namespace {

// (the range rules -- gaps_cannot_win, the key, cell and hand-off widths -- are ovl_score_range.h's)

int make_plan_full(const Dev* c, int32_t match, int32_t mismatch, int64_t indel, Plan* out);

// band >= 0: the build's seed-and-extend knob (oracle_overlap_banded), exact
// (== the reference) whenever gaps cannot win -- the seed cell (n, j*) is
// always in the band and nothing off the ungapped diagonals can beat it -- and
// whenever the band covers every diagonal (band >= 2 * lmax).
int make_plan(const Dev* c, int32_t match, int32_t mismatch, int64_t indel, int32_t band, Plan* out) {
    if (c->n_reads < 0) return fail(c, OVL_E_STATE, "no resident reads: call ovl_set_reads first");
    const int64_t L = std::max<int32_t>(c->lmax, 1);
    if (band < 0 || band >= 2 * L || gaps_cannot_win(match, mismatch, indel, L))
        return make_plan_full(c, match, mismatch, indel, out);
    // seed: the ungapped closed form (any kernel that evaluates it exactly)
    Plan seed;
    int rc = make_plan_full(c, match, mismatch, INT32_MIN, &seed);
    if (rc != OVL_OK) return rc;
    if (!gaps_cannot_win(match, mismatch, INT32_MIN, L))
        return fail(c, OVL_E_UNSUPPORTED, "banded: the ungapped seed cannot be evaluated exactly at these scores");
    Plan full;
    rc = make_plan_full(c, match, mismatch, indel, &full);
    if (rc != OVL_OK) return rc;
    if (full.kernel != OVL_KERNEL_DP || full.wide)
        return fail(c, OVL_E_UNSUPPORTED, "banded: scores too large for int32 cells (|score| * (2*lmax+1) >= 2^31)");
    Plan p;
    p.kernel = OVL_KERNEL_BANDED;
    p.wide = false;
    p.band = band;
    p.seed_kernel = seed.kernel;
    p.seed_key64 = seed.key64;
    p.seed_wide = seed.wide;
    *out = p;
    return OVL_OK;
}

int make_plan_full(const Dev* c, int32_t match, int32_t mismatch, int64_t indel, Plan* out) {
    const int64_t L = std::max<int32_t>(c->lmax, 1);
    Plan p;
    // ungapped closed form: exact when gaps cannot win and no int32 store can wrap
    if (c->wmax > 0 && gaps_cannot_win(match, mismatch, indel, L) && ungapped_int32_ok(match, mismatch, L)) {
        p.kernel = OVL_KERNEL_UNGAPPED;
        p.key64 = !ungapped_key32_ok(match, mismatch, L);
    } else {
        if (c->lmax > kDpMaxLen)
            return fail(c, OVL_E_UNSUPPORTED, "gapped DP supports reads up to %d bases (longest is %d)", kDpMaxLen,
                        c->lmax);
        p.kernel = OVL_KERNEL_DP;
        p.wide = !dp_int32_ok(match, mismatch, indel, L);
    }
    *out = p;
    return OVL_OK;
}

// Per-device scratch (lane_col, seed_*) is shared by every launch of the device.  A launch on stream s
// first waits for the previous user on another stream; growing a buffer first waits for that user.
struct ScratchNeed {
    DevBuf* buf;
    size_t bytes;
};

hipError_t scratch_acquire(Dev* c, hipStream_t s, std::initializer_list<ScratchNeed> needs) {
    hipError_t e = hipSuccess;
    for (const ScratchNeed& n : needs) {
        if (n.buf->bytes >= n.bytes) continue;
        if (c->scratch_used && (e = hipEventSynchronize(c->scratch_evt)) != hipSuccess) return e;
        if ((e = ensure(*n.buf, n.bytes)) != hipSuccess) return e;
    }
    if (c->scratch_used && c->scratch_stream != s) e = hipStreamWaitEvent(s, c->scratch_evt, 0);
    return e;
}

hipError_t scratch_release(Dev* c, hipStream_t s) {
    hipError_t e = hipEventRecord(c->scratch_evt, s);
    c->scratch_stream = s;
    c->scratch_used = true;
    return e;
}

// Lane-per-pair full DP (ovl_dp_lane.hip): one lane per pair, so it needs many pairs to fill the
// chip (below that the one-wavefront-per-pair dp_fast_kernel is faster), reads short enough for
// the per-wavefront hand-off columns, and G = dp - indel*(i+j) inside int32.
bool use_dp_lane(const Dev* c, int64_t match, int64_t mismatch, int64_t indel, int64_t n_pairs) {
    if (c->k.dp_lane == 0) return false;
    const int64_t L = std::max<int32_t>(c->lmax, 1);
    if (L > kLaneMaxLen || !dp_lane_int32_ok(match, mismatch, indel, L) ||
        c->codes_bytes + 64 >= (int64_t(1) << 32))
        return false;
    return c->k.dp_lane == 1 || n_pairs >= kLaneMinPairs;
}

// rs_log2 of an ungapped launch over n pairs: bit shifts split over 1 << rs_log2 lanes (the general kernel),
// or (uniform kernel, 2 planes) latency mode when rs_log2 > 0: up to kLatTiles tiles per CU for device lists,
// up to kLatTilesIx for a host-encoded list (which only throughput mode reads in place)
int32_t ungapped_rs_log2(const Dev* c, int64_t n_pairs, bool ix = false) {
    int32_t rs_log2 = 0;
    const int64_t want_waves = (int64_t)c->cu_count * 4 * 4;
    while (rs_log2 < 2 && ((n_pairs << rs_log2) + 63) / 64 < want_waves) ++rs_log2;
    if (c->planes == 2)
        rs_log2 = ((n_pairs + 63) / 64 <= (int64_t)c->cu_count * (ix ? kLatTilesIx : kLatTiles)) ? 1 : 0;
    return rs_log2;
}

}  // namespace

// An ungapped launch over n pairs runs uniform_kernel in throughput mode, the one that can read a
// host-encoded pair list in place (uniform_kernel IX)
bool ix_launch(const Dev* c, int64_t n_pairs) {
    return c->planes == 2 && c->lmax > 0 && c->wmax >= 1 && c->wmax <= 8 && ungapped_rs_log2(c, n_pairs, true) == 0;
}

// The candidate list's heavy tiles (flags per list tile on the device, ascending ids on host and device),
// once per list; waits for the list's stream.
int ensure_heavy(Dev* c) {
    if (c->heavy_for == c->cand_n) return OVL_OK;
    const int64_t n_tiles = (c->cand_n + 63) / 64;
    HIPCHK(c, ensure(c->tile_flags, (size_t)std::max<int64_t>(n_tiles, 1)));
    HIPCHK(c, ovl_launch_tile_flags(as<int32_t>(c->cand_a), c->cand_n, as<uint32_t>(c->full), c->n_reads,
                                    as<uint8_t>(c->tile_flags), c->stream));
    std::vector<uint8_t> f((size_t)n_tiles);
    HIPCHK(c, hipMemcpyAsync(f.data(), c->tile_flags.p, (size_t)n_tiles, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->h_heavy.clear();
    for (int64_t t = 0; t < n_tiles; ++t)
        if (f[(size_t)t]) c->h_heavy.push_back((int32_t)t);
    HIPCHK(c, ensure(c->heavy_ids, sizeof(int32_t) * std::max<size_t>(c->h_heavy.size(), 1)));
    if (!c->h_heavy.empty())
        HIPCHK(c, hipMemcpy(c->heavy_ids.p, c->h_heavy.data(), sizeof(int32_t) * c->h_heavy.size(),
                            hipMemcpyHostToDevice));
    c->heavy_for = c->cand_n;
    return OVL_OK;
}

// The heavy tiles among the list tiles of pairs [lo, lo + n_pairs) of the resident list, lo a multiple of 64 (after
// ensure_heavy); tile_base is the range's first list tile.  All zero when the range has none.
HeavyWindow heavy_window(const Dev* c, int64_t lo, int64_t n_pairs) {
    const int64_t t0 = lo / 64, t1 = t0 + (n_pairs + 63) / 64;
    const auto k0 = std::lower_bound(c->h_heavy.begin(), c->h_heavy.end(), t0);
    const auto k1 = std::lower_bound(c->h_heavy.begin(), c->h_heavy.end(), t1);
    HeavyWindow w;
    if (k1 > k0) w = {reinterpret_cast<const int32_t*>(c->heavy_ids.p) + (k0 - c->h_heavy.begin()), k1 - k0, t0};
    return w;
}

namespace {

int launch_score_chunk(Dev* c, const Plan& pl, const PairList& pairs, const Scoring& sc, const ScoreOut& out,
                       LaunchIo& io, hipStream_t s) {
    const int32_t *const d_a = pairs.a, *const d_b = pairs.b;
    const int32_t match = sc.match, mismatch = sc.mismatch;
    const int64_t n_pairs = pairs.n, indel = sc.indel;
    if (n_pairs == 0) return OVL_OK;
    if (io.ix_b16 && (pl.kernel != OVL_KERNEL_UNGAPPED || pl.key64 || !ix_launch(c, n_pairs)))
        return fail(c, OVL_E_UNSUPPORTED, "host-encoded pair list on a launch that cannot read it");
    uint32_t* const flag = io.flag ? io.flag : as<uint32_t>(c->err_flag);
    // ovl_last_score_form: the call's first launch describes itself (a banded launch, not its seed's)
    ScoreForm& f = c->form;
    const bool rec = f.open;
    if (rec) {
        f = ScoreForm{};
        f.kernel = pl.kernel;
        f.key64 = pl.kernel == OVL_KERNEL_BANDED ? pl.seed_key64 : (pl.kernel == OVL_KERNEL_UNGAPPED && pl.key64);
        f.wide = pl.kernel != OVL_KERNEL_UNGAPPED && pl.wide ? 1 : 0;
    }
    const int32_t* seed_end = nullptr;
    if (pl.kernel == OVL_KERNEL_BANDED) {
        // seed j* into device scratch (the outputs may be host memory), then the banded DP reads it
        const size_t sb = sizeof(int32_t) * (size_t)n_pairs;
        HIPCHK(c, scratch_acquire(c, s, {{&c->seed_s, sb}, {&c->seed_e, sb}}));
        const Plan seed{pl.seed_kernel, pl.seed_key64, pl.seed_wide};
        LaunchIo seed_io;  // the seeds stay in HBM, untimed; the call's flag
        seed_io.flag = flag;
        int rc = launch_score_chunk(c, seed, pairs, {match, mismatch, INT32_MIN},
                                    {as<int32_t>(c->seed_s), as<int32_t>(c->seed_e)}, seed_io, s);
        if (rc != OVL_OK) return rc;
        seed_end = as<int32_t>(c->seed_e);
    }
    if (pl.kernel == OVL_KERNEL_UNGAPPED) {
        OvlUngappedArgs g{};
        g.sfx = as<uint32_t>(c->sfx);
        g.pfx = as<uint32_t>(c->pfx);
        g.len = as<int32_t>(c->len);
        g.n_reads = c->n_reads;
        g.a_idx = d_a;
        g.b_idx = d_b;
        g.n_pairs = n_pairs;
        // general kernel: split a pair's bit shifts over 1, 2 or 4 lanes until the grid
        // has enough wavefronts.  Uniform kernel: latency mode (two wavefronts per tile,
        // side pairs beside the sweep) when there is about one tile per wavefront slot.
        g.rs_log2 = ungapped_rs_log2(c, n_pairs, io.ix_b16 != nullptr);
        // uniform-length fast path (2 bit planes): pairs of two reads of length lmax;
        // uniform_kernel scores the other pairs through its LDS side ring
        g.lw = c->planes == 2 ? c->lmax : 0;
        if (rec) f.rs_log2 = g.rs_log2;
        g.full = as<uint32_t>(c->full);
        g.ev_start = io.kev_start;
        g.ev_stop = io.kev_stop;
        g.match = match;
        g.mismatch = mismatch;
        g.out_score = out.score;
        g.out_end = out.end;
        g.err_flag = flag;
        g.planes = c->planes;
        g.wmax = c->wmax;
        g.key64 = pl.key64 ? 1 : 0;
        g.max_blocks = (int64_t)c->cu_count * kBlocksPerCu;
        g.host_out = io.sink;
        g.ix_b16 = io.ix_b16;
        g.ix_d8 = io.ix_d8;
        g.ix_base = io.ix_base;
        // a throughput-mode launch over (a 64-aligned part of) the resident candidate list: heavy tiles first
        const int32_t* ca = as<int32_t>(c->cand_a);
        if (!g.ix_b16 && g.lw > 0 && g.rs_log2 == 0 && c->cand_n > 0 && d_a >= ca &&
            d_a < ca + c->cand_n && d_b == as<int32_t>(c->cand_b) + (d_a - ca) && (d_a - ca) % 64 == 0) {
            int rc = ensure_heavy(c);
            if (rc != OVL_OK) return rc;
            const HeavyWindow w = heavy_window(c, d_a - ca, n_pairs);
            g.heavy_ids = w.ids;
            g.heavy_n = (int32_t)w.count;
            g.tile_flags = w.count ? as<uint8_t>(c->tile_flags) : nullptr;
            g.tile_base = w.tile_base;
        }
        HIPCHK(c, ovl_launch_ungapped(&g, s));
        io.timed = g.ev_start && g.lw > 0;  // (uniform_kernel recorded the events)
    } else {
        OvlDpArgs g{};
        g.codes = as<uint8_t>(c->codes);
        g.off = as<int64_t>(c->off);
        g.len = as<int32_t>(c->len);
        g.n_reads = c->n_reads;
        g.a_idx = d_a;
        g.b_idx = d_b;
        g.n_pairs = n_pairs;
        g.mcap = std::max<int32_t>(c->lmax, 1);
        g.match = match;
        g.mismatch = mismatch;
        g.indel = indel;
        g.out_score = out.score;
        g.out_end = out.end;
        g.tb = nullptr;
        g.err_flag = flag;
        g.wide = pl.wide ? 1 : 0;
        g.band = pl.kernel == OVL_KERNEL_BANDED ? pl.band : -1;
        g.seed = seed_end;
        g.classic = c->k.dp_classic;
        if (g.band < 0 && !g.wide && !g.classic && use_dp_lane(c, match, mismatch, indel, n_pairs)) {
            OvlLaneArgs k{};
            k.cw = 32;
            k.slots = (int64_t)c->cu_count * 4 * ovl_dp_lane_waves_per_simd(k.cw);
            const int64_t L = std::max<int32_t>(c->lmax, 1);
            k.prof = c->k.lane_prof && c->planes == 2 && dp_lane_prof_ok(match, mismatch, indel);
            k.ho = dp_lane_ho1_ok(match, mismatch, indel, L) ? 1 : 0;
            k.sfx = k.prof && c->k.lane_sfx && c->wmax > 0;
            // 4-bit column steps in LDS
            if (k.sfx && dp_lane_ho2_ok(match, mismatch, indel, g.mcap)) k.ho = 2;
            k.h2 = k.ho == 2 && c->k.lane_h2 && ovl_dp_lane_h2_ok(match, mismatch, indel);
            // hand-off columns in HBM: one per resident slot (HO 0 / 1), per tile for the h2 form's HBM variant --
            // which launches at most kH2Slice pairs at a time over one reused column buffer (lcap / 2 bytes per
            // pair: 1 GiB at 256-base reads), and falls back to the int32 form (HO 2: no HBM column) when even that
            // cannot be allocated
            constexpr int64_t kH2Slice = int64_t(1) << 23;
            const int64_t slice = k.h2 ? std::min(n_pairs, kH2Slice) : n_pairs;
            size_t col_bytes =
                k.h2 ? (size_t)ovl_dp_lane_h2_col_bytes(slice, g.mcap)
                     : (k.ho == 2 ? 0 : (size_t)k.slots * ovl_dp_lane_rcap(g.mcap) * 64 * sizeof(uint32_t));
            hipError_t se = scratch_acquire(c, s, {{&c->lane_col, col_bytes}});
            if (se == hipErrorOutOfMemory && k.h2) {
                (void)hipGetLastError();
                k.h2 = 0;
                col_bytes = 0;
                se = scratch_acquire(c, s, {{&c->lane_col, col_bytes}});
            }
            HIPCHK(c, se);
            k.sfx_words = as<uint32_t>(c->sfx);
            k.pfx_words = as<uint32_t>(c->pfx);
            k.srow = c->srow;
            k.wsfx = c->wmax;
            k.colbuf = as<uint32_t>(c->lane_col);
            for (int64_t lo = 0; lo < n_pairs; lo += slice) {
                OvlDpArgs gs = g;
                gs.a_idx = d_a + lo;
                gs.b_idx = d_b + lo;
                gs.out_score = out.score + lo;
                gs.out_end = out.end + lo;
                gs.n_pairs = std::min(slice, n_pairs - lo);
                HIPCHK(c, ovl_launch_dp_lane(&gs, &k, s));
            }
            HIPCHK(c, scratch_release(c, s));
            if (rec) {
                f.lane = 1;
                f.prof = k.prof;
                f.sfx = k.sfx;
                f.ho = k.ho;
                f.h2 = k.h2;
            }
            return OVL_OK;
        }
        if (g.band >= 0) {
            const int64_t L = std::max<int32_t>(c->lmax, 1);
            const bool neg_ok = band_neg_ok(match, mismatch, indel, L);
            const int64_t lanes = 2 * (int64_t)g.band + 1;
            const bool diag_ok = neg_ok && ovl_band_diag_slots(g.band, c->lmax, nullptr) > 0;
            const bool rows_ok = neg_ok && lanes <= 192 && c->lmax <= 1024;
            // lane per pair: <= 4 symbols, byte scores and G in int32 (band_lane_scoring_ok)
            const bool lane_ok = c->planes == 2 && ovl_band_lane_ok(g.band) &&
                                 band_lane_scoring_ok(match, mismatch, indel, L, g.band) &&
                                 c->lmax <= kLaneMaxLen && c->codes_bytes + 64 < (int64_t(1) << 32);
            switch (c->k.band_form) {
                case OVL_BAND_FORM_ROWS: g.band_form = rows_ok ? OVL_BAND_FORM_ROWS : OVL_BAND_FORM_STRIP; break;
                case OVL_BAND_FORM_FAST: g.band_form = OVL_BAND_FORM_FAST; break;
                case OVL_BAND_FORM_STRIP: g.band_form = OVL_BAND_FORM_STRIP; break;
                case OVL_BAND_FORM_DIAG: g.band_form = diag_ok ? OVL_BAND_FORM_DIAG : OVL_BAND_FORM_FAST; break;
                case OVL_BAND_FORM_LANE:
                case OVL_BAND_FORM_LANE1:
                case OVL_BAND_FORM_LANE2:
                    g.band_form = lane_ok ? OVL_BAND_FORM_LANE : (diag_ok ? OVL_BAND_FORM_DIAG : OVL_BAND_FORM_FAST);
                    break;
                default:
                    g.band_form = (lane_ok && n_pairs >= kLaneMinPairs)
                                      ? OVL_BAND_FORM_LANE
                                      : (diag_ok ? OVL_BAND_FORM_DIAG : OVL_BAND_FORM_FAST);
                    break;
            }
            if (rec) f.band_form = g.band_form;
            if (g.band_form == OVL_BAND_FORM_LANE) {
                OvlLaneArgs k{};
                k.sfx = c->k.lane_sfx && c->wmax > 0;
                k.sfx_words = as<uint32_t>(c->sfx);
                k.pfx_words = as<uint32_t>(c->pfx);
                k.srow = c->srow;
                k.wsfx = c->wmax;
                k.split = c->k.band_form == OVL_BAND_FORM_LANE2 ||
                          (c->k.band_form != OVL_BAND_FORM_LANE1 && g.band >= kBandLane2Min);
                if (rec) {
                    f.sfx = k.sfx;
                    f.split = k.split;
                }
                HIPCHK(c, ovl_launch_band_lane(&g, &k, s));
                HIPCHK(c, scratch_release(c, s));
                return OVL_OK;
            }
        }
        HIPCHK(c, ovl_launch_dp(&g, s));
        if (seed_end) HIPCHK(c, scratch_release(c, s));
    }
    return OVL_OK;
}

}  // namespace

// Kernels queue pair indices as int32 (LDS side ring); split huge lists.  An in-place list advances with its piece
// (a piece is whole tiles); the kernel events go to the first piece that records them, as a launch records them once.
int launch_score(Dev* c, const Plan& pl, const PairList& pairs, const Scoring& sc, const ScoreOut& out, LaunchIo& io,
                 hipStream_t s) {
    constexpr int64_t kChunk = int64_t(1) << 30;
    io.timed = false;
    LaunchIo piece = io;
    for (int64_t lo = 0; lo < pairs.n; lo += kChunk) {
        const int64_t n = std::min(kChunk, pairs.n - lo);
        if (io.ix_b16) {
            piece.ix_b16 = io.ix_b16 + lo;
            piece.ix_d8 = io.ix_d8 + lo;
            piece.ix_base = io.ix_base + lo / 64;
        }
        const PairList part{pairs.a + lo, pairs.b + lo, n};
        int rc = launch_score_chunk(c, pl, part, sc, {out.score + lo, out.end + lo}, piece, s);
        if (rc != OVL_OK) return rc;
        if (piece.timed) {
            io.timed = true;
            piece.kev_start = piece.kev_stop = nullptr;
        }
    }
    return OVL_OK;
}

int check_scoring_args(ovl_ctx* c, int32_t match, int32_t mismatch, int64_t indel, int32_t band, Plan* p) {
    // every device holds the same read set, so device 0 plans for all
    c->devs[0]->form = ScoreForm{};
    c->devs[0]->form.open = true;
    return make_plan(c->devs[0], match, mismatch, indel, band, p);
}

OVL_API int ovl_plan(const ovl_ctx* c, int32_t match, int32_t mismatch, int64_t indel, int32_t band,
                     int32_t* out_kernel) {
    if (!c) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    if (!out_kernel) return fail(c, OVL_E_ARG, "out_kernel is NULL");
    Plan p;
    int rc = make_plan(c->devs[0], match, mismatch, indel, band, &p);
    if (rc != OVL_OK) return rc;
    *out_kernel = p.kernel;
    return OVL_OK;
}

OVL_API int ovl_last_score_form(const ovl_ctx* c, int32_t* kernel, int32_t* key64, int32_t* wide, int32_t* lane,
                                int32_t* prof, int32_t* sfx, int32_t* ho, int32_t* h2, int32_t* band_form,
                                int32_t* split, int32_t* rs_log2) {
    if (!c) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    const ScoreForm& f = c->devs[0]->form;
    if (kernel) *kernel = f.kernel;
    if (key64) *key64 = f.key64;
    if (wide) *wide = f.wide;
    if (lane) *lane = f.lane;
    if (prof) *prof = f.prof;
    if (sfx) *sfx = f.sfx;
    if (ho) *ho = f.ho;
    if (h2) *h2 = f.h2;
    if (band_form) *band_form = f.band_form;
    if (split) *split = f.split;
    if (rs_log2) *rs_log2 = f.rs_log2;
    return OVL_OK;
}

// ----------------------------------------------------------------------------- scoring

OVL_API int ovl_score_device(ovl_ctx* c, const int32_t* d_a, const int32_t* d_b, int64_t n_pairs, int32_t match,
                             int32_t mismatch, int64_t indel, int32_t band, int32_t* d_score, int32_t* d_end,
                             void* stream) {
    if (!c) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    quiet(c);
    if (n_pairs < 0) return fail(c, OVL_E_ARG, "n_pairs < 0");
    if (n_pairs > 0 && (!d_a || !d_b || !d_score || !d_end)) return fail(c, OVL_E_ARG, "NULL device pointer");
    Dev* d = c->devs[0];
    Plan p;
    d->form = ScoreForm{};
    d->form.open = true;
    int rc = make_plan(d, match, mismatch, indel, band, &p);
    if (rc != OVL_OK) return rc;
    if (n_pairs > 0 && d->n_reads == 0) return fail(c, OVL_E_INDEX, "pairs given but the read set is empty");
    DeviceGuard guard;
    HIPCHK(c, hipSetDevice(d->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);  // NULL = the default (null) stream
    LaunchIo io;  // (a device call's: HBM results, the device flag)
    return launch_score(d, p, {d_a, d_b, n_pairs}, {match, mismatch, indel}, {d_score, d_end}, io, s);
}

OVL_API int ovl_check_device_errors(ovl_ctx* c) {
    if (!c) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    quiet(c);
    DeviceGuard guard;
    int rc = OVL_OK;
    for (Dev* d : c->devs) {
        HIPCHK(c, hipSetDevice(d->device));
        HIPCHK(c, hipDeviceSynchronize());
        uint32_t flag = 0;
        HIPCHK(c, hipMemcpy(&flag, d->err_flag.p, sizeof(flag), hipMemcpyDeviceToHost));
        if (flag) {
            HIPCHK(c, hipMemset(d->err_flag.p, 0, sizeof(uint32_t)));
            rc = fail(c, OVL_E_INDEX, "a device scoring call saw a pair index outside [0, n_reads)");
        }
    }
    return rc;
}
