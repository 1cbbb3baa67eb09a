// ovl_depth_api.cpp — the selection step of the reference's read-depth coverage (plots.py:115-135): every read
// against every contig through align_read_or_contig_to_reference (aligners.py:170-202), and per read the best
// score, the contigs that attain it and the aligned stretch on the first of them.  The host form
// (ovl_read_best_host) and the device call (ovl_read_best: ovl_local_lane.hip for the scores, the batched
// local-alignment kernel for the start positions and for the reads the lane kernel does not take).
#include "ovl_local_host.h"

namespace {

constexpr size_t kTileBudget = size_t(256) << 20;  // a chunk's {score, cell} tile in HBM
constexpr int64_t kOpsBudget = int64_t(256) << 20;  // the walks of one start-position batch

template <typename C>
int check_read_best(const C* c, const uint8_t* reads, const int64_t* r_off, int32_t n_reads, const uint8_t* contigs,
                    const int64_t* c_off, int32_t n_contigs, int32_t read_length, int32_t match,
                    const int32_t* best_score, const int32_t* first_best, const int32_t* n_best,
                    const int32_t* best_start, const int32_t* best_end, SeqShape* sh) {
    if (int rc = check_seq_counts(c, n_reads, n_contigs, read_length)) return rc;
    if ((n_reads > 0 && !r_off) || (n_contigs > 0 && !c_off)) return fail(c, OVL_E_ARG, "NULL offsets");
    if (n_reads > 0 && (!best_score || !first_best || !n_best || !best_start || !best_end))
        return fail(c, OVL_E_ARG, "NULL output pointer");
    if (int rc = check_seq_sets(c, reads, r_off, n_reads, contigs, c_off, n_contigs, sh)) return rc;
    if (!local_limits_ok(sh->max_n, sh->max_m, match))
        return fail(c, OVL_E_UNSUPPORTED, "read depth: lengths < 2^20 and match * min(n, m) < 2^24 required");
    if (sh->c_total >= (int64_t(1) << 31))
        return fail(c, OVL_E_UNSUPPORTED, "read depth: the contigs together must stay below 2^31 bases");
    return OVL_OK;
}

void zero_outputs(int32_t n_reads, int32_t n_contigs, int32_t* best_score, int32_t* first_best, int32_t* n_best,
                  int32_t* best_start, int32_t* best_end, uint32_t* tie_bits, int32_t* scores) {
    const int64_t words = ((int64_t)n_contigs + 31) / 32;
    for (int32_t r = 0; r < n_reads; ++r) {
        best_score[r] = 0;
        first_best[r] = -1;
        n_best[r] = 0;
        best_start[r] = 0;
        best_end[r] = 0;
    }
    if (tie_bits) std::fill(tie_bits, tie_bits + (int64_t)n_reads * words, 0u);
    if (scores) std::fill(scores, scores + (int64_t)n_reads * n_contigs, 0);
}

// one read's running selection over the contigs in order (plots.py:126-131)
struct Pick {
    int64_t best = 0;
    int32_t first = -1, n = 0, bi = 0, bj = 0;  // (bi, bj): the first best contig's cell, window-relative
    void take(int32_t c, int64_t score, int32_t i, int32_t j, uint32_t* bits) {
        if (first < 0 || score > best) {
            best = score; first = c; n = 1; bi = i; bj = j;
            if (bits) std::fill(bits, bits + (c >> 5) + 1, 0u);
        } else if (score == best) {
            ++n;
        } else {
            return;
        }
        if (bits) bits[c >> 5] |= 1u << (c & 31);
    }
};

}  // namespace

OVL_API int ovl_read_best_host(const uint8_t* reads, const int64_t* r_off, int32_t n_reads, const uint8_t* contigs,
                               const int64_t* c_off, int32_t n_contigs, int32_t read_length, int32_t match,
                               int32_t mismatch, int64_t indel, int32_t* best_score, int32_t* first_best,
                               int32_t* n_best, int32_t* best_start, int32_t* best_end, uint32_t* tie_bits,
                               int32_t* scores) {
    const ovl_ctx* none = nullptr;
    SeqShape sh;
    const int rc = check_read_best(none, reads, r_off, n_reads, contigs, c_off, n_contigs, read_length, match,
                                   best_score, first_best, n_best, best_start, best_end, &sh);
    if (rc != OVL_OK) return rc;
    zero_outputs(n_reads, n_contigs, best_score, first_best, n_best, best_start, best_end, tie_bits, scores);
    const int64_t words = ((int64_t)n_contigs + 31) / 32;
    const int64_t ind = clamp_score(indel);
    std::vector<int64_t> row;
    std::vector<int8_t> tb;
    try {
        for (int32_t r = 0; r < n_reads && n_contigs > 0; ++r) {
            const uint8_t* q = reads + r_off[r];
            const int32_t L = (int32_t)(r_off[r + 1] - r_off[r]);
            Pick p;
            uint32_t* bits = tie_bits ? tie_bits + r * words : nullptr;
            for (int32_t c = 0; c < n_contigs; ++c) {
                const int64_t m = c_off[c + 1] - c_off[c];
                const Window w = window_of(L, m, read_length);
                const Cell cell =
                    sw_fill_host<false>(q, L, contigs + c_off[c] + w.lo, w.len, match, mismatch, ind, row, nullptr);
                if (scores) scores[(int64_t)r * n_contigs + c] = (int32_t)cell.score;
                p.take(c, cell.score, cell.bi, cell.bj, bits);
            }
            const int64_t m = c_off[p.first + 1] - c_off[p.first];
            const Window w = window_of(L, m, read_length);
            int32_t sj = 0;
            if (p.best > 0) {
                // only rows <= bi and columns <= bj matter to the walk: the table of that corner
                sw_fill_host<true>(q, p.bi, contigs + c_off[p.first] + w.lo, p.bj, match, mismatch, ind, row, &tb);
                sj = sw_walk_host(tb, p.bj, p.bi, p.bj, [](int8_t) {});
            }
            best_score[r] = (int32_t)p.best;
            first_best[r] = p.first;
            n_best[r] = p.n;
            best_start[r] = (int32_t)(sj + w.shift);
            best_end[r] = (int32_t)(p.bj + w.shift);
        }
    } catch (const std::bad_alloc&) {
        return fail(none, OVL_E_OOM, "no memory for a traceback table");
    }
    return OVL_OK;
}

OVL_API int ovl_read_best(ovl_ctx* ctx, const uint8_t* reads, const int64_t* r_off, int32_t n_reads,
                          const uint8_t* contigs, const int64_t* c_off, int32_t n_contigs, int32_t read_length,
                          int32_t match, int32_t mismatch, int64_t indel, int32_t* best_score, int32_t* first_best,
                          int32_t* n_best, int32_t* best_start, int32_t* best_end, uint32_t* tie_bits,
                          int32_t* scores) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    StageCall call(ctx);
    Dev* c = call.dev;
    SeqShape sh;
    const int rc = check_read_best(c, reads, r_off, n_reads, contigs, c_off, n_contigs, read_length, match,
                                   best_score, first_best, n_best, best_start, best_end, &sh);
    if (rc != OVL_OK) return rc;
    zero_outputs(n_reads, n_contigs, best_score, first_best, n_best, best_start, best_end, tie_bits, scores);
    call.begin();
    c->rb.last = {};
    if (n_reads == 0 || n_contigs == 0) return OVL_OK;
    const int32_t C = n_contigs;
    const int64_t words = ((int64_t)C + 31) / 32;
    double kernel_ms = 0.0;  // the score pass: the lane kernel's launches and their folds

    // the symbols the lane kernel compares: the bytes in use renumbered from 0, 255 kept for its padding rows
    int32_t code[256];
    std::fill(code, code + 256, -1);
    int32_t n_codes = 0;
    for (const uint8_t* p = reads + r_off[0]; p < reads + r_off[n_reads]; ++p)
        if (code[*p] < 0) code[*p] = n_codes++;
    for (const uint8_t* p = contigs + c_off[0]; p < contigs + c_off[C]; ++p)
        if (code[*p] < 0) code[*p] = n_codes++;
    const bool lane_scoring = read_best_lane_scoring_ok(n_codes, match, mismatch, indel);
    std::vector<int32_t> lane, other;  // the reads by path
    int64_t lane_max = 0;
    for (int32_t r = 0; r < n_reads; ++r) {
        const int64_t L = r_off[r + 1] - r_off[r];
        if (lane_scoring && L <= kLocalLaneMaxRows) {
            lane.push_back(r);
            lane_max = std::max(lane_max, L);
        } else {
            other.push_back(r);
        }
    }
    // per read: the first best contig's cell, window-relative
    std::vector<int32_t> cell_i((size_t)n_reads, 0), cell_j((size_t)n_reads, 0);

    if (!lane.empty()) {
        const int32_t nl = (int32_t)lane.size();
        const int32_t rows = lane_max <= 32 ? 32 : (lane_max <= 64 ? 64 : 128);
        const int64_t pitch = ((int64_t)nl + 63) & ~int64_t(63);
        auto up16 = [](size_t v) { return (v + 15) & ~size_t(15); };
        const size_t o_len = up16((size_t)pitch * rows), o_coff = up16(o_len + sizeof(int32_t) * (size_t)pitch);
        const size_t o_clen = up16(o_coff + sizeof(int64_t) * (size_t)C);
        const size_t o_sym = up16(o_clen + sizeof(int32_t) * (size_t)C);
        std::vector<int64_t> d_off((size_t)C);
        int64_t sym_bytes = 0;
        for (int32_t k = 0; k < C; ++k) {
            d_off[(size_t)k] = sym_bytes;
            sym_bytes += ((c_off[k + 1] - c_off[k]) + 3) & ~int64_t(3);
        }
        std::vector<char> blob(o_sym + (size_t)sym_bytes + 16, 0);
        memset(blob.data(), 0xFF, (size_t)pitch * rows);
        int32_t* h_len = reinterpret_cast<int32_t*>(blob.data() + o_len);
        for (int32_t k = 0; k < nl; ++k) {
            const int32_t r = lane[(size_t)k];
            const int64_t L = r_off[r + 1] - r_off[r];
            h_len[k] = (int32_t)L;
            uint8_t* dst = reinterpret_cast<uint8_t*>(blob.data()) + (size_t)k * rows;
            for (int64_t i = 0; i < L; ++i) dst[i] = (uint8_t)code[reads[r_off[r] + i]];
        }
        memcpy(blob.data() + o_coff, d_off.data(), sizeof(int64_t) * (size_t)C);
        int32_t* h_clen = reinterpret_cast<int32_t*>(blob.data() + o_clen);
        for (int32_t k = 0; k < C; ++k) {
            const int64_t m = c_off[k + 1] - c_off[k];
            h_clen[k] = (int32_t)m;
            uint8_t* dst = reinterpret_cast<uint8_t*>(blob.data()) + o_sym + (size_t)d_off[(size_t)k];
            for (int64_t j = 0; j < m; ++j) dst[j] = (uint8_t)code[contigs[c_off[k] + j]];
        }
        // contigs per launch: what the tile budget holds, in whole words of tie bits
        int64_t chunk = std::max<int64_t>(32, (int64_t)(kTileBudget / ((size_t)pitch * 8)) & ~int64_t(31));
        if (c->k.read_best_chunk > 0) chunk = ((int64_t)c->k.read_best_chunk + 31) & ~int64_t(31);
        chunk = std::min<int64_t>(chunk, (words * 32));
        const size_t tile_half = up16(sizeof(int32_t) * (size_t)pitch * (size_t)chunk);
        const size_t res_bytes = sizeof(int32_t) * (size_t)pitch;
        std::vector<int32_t> h_tile, res(4 * (size_t)pitch);
        std::vector<uint32_t> h_bits(tie_bits ? (size_t)nl * (size_t)words : 0);
        HIPCHK(c, hipSetDevice(c->device));
        hipStream_t s = c->stream;
        StreamDrain drain(s);
        HIPCHK(c, ensure(c->rb.in, blob.size()));
        HIPCHK(c, ensure(c->rb.tile, 2 * tile_half));
        HIPCHK(c, ensure(c->rb.res, 4 * res_bytes));
        if (tie_bits) HIPCHK(c, ensure(c->rb.bits, sizeof(uint32_t) * (size_t)nl * (size_t)words));
        HIPCHK(c, hipMemcpyAsync(c->rb.in.p, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(c->rb.res.p, 0, 4 * res_bytes, s));
        HIPCHK(c, hipMemsetAsync(as<char>(c->rb.res) + res_bytes, 0xFF, res_bytes, s));  // first = -1
        if (tie_bits) HIPCHK(c, hipMemsetAsync(c->rb.bits.p, 0, sizeof(uint32_t) * (size_t)nl * (size_t)words, s));
        OvlLocalLaneArgs a{};
        a.reads = as<uint8_t>(c->rb.in);
        a.r_len = reinterpret_cast<const int32_t*>(as<char>(c->rb.in) + o_len);
        a.c_off = reinterpret_cast<const int64_t*>(as<char>(c->rb.in) + o_coff);
        a.c_len = reinterpret_cast<const int32_t*>(as<char>(c->rb.in) + o_clen);
        a.contigs = as<uint8_t>(c->rb.in) + o_sym;
        a.pitch = pitch;
        a.read_length = read_length;
        a.match = match;
        a.mismatch = mismatch;
        a.indel = (int32_t)std::max<int64_t>(indel, -(int64_t(1) << 30));  // below: never taken either way
        a.tile_score = as<int32_t>(c->rb.tile);
        a.tile_end = reinterpret_cast<uint32_t*>(as<char>(c->rb.tile) + tile_half);
        int32_t* d_best = as<int32_t>(c->rb.res);
        int32_t* d_first = d_best + pitch;
        int32_t* d_nbest = d_first + pitch;
        uint32_t* d_cell = reinterpret_cast<uint32_t*>(d_nbest + pitch);
        const int32_t groups = (int32_t)(pitch / 64);
        HIPCHK(c, c->rb.timer.arm(ctx->timing));
        HIPCHK(c, c->rb.timer.mark(0, s));
        for (int64_t lo = 0; lo < C; lo += chunk) {
            a.c_lo = (int32_t)lo;
            a.c_hi = (int32_t)std::min<int64_t>(C, lo + chunk);
            // enough wavefronts for eight per CU, each sweeping every split-th contig of the chunk
            const int32_t split = (int32_t)std::min<int64_t>(
                a.c_hi - a.c_lo, std::max<int64_t>(1, ((int64_t)c->cu_count * 8 + groups - 1) / groups));
            HIPCHK(c, ovl_launch_local_lane(&a, rows, groups, split, s));
            ++c->rb.last.launches;
            HIPCHK(c, ovl_launch_read_best_fold(&a, nl, (int32_t)words, d_best, d_first, d_nbest, d_cell,
                                                tie_bits ? as<uint32_t>(c->rb.bits) : nullptr, s));
            if (scores) {
                const size_t cnt = (size_t)pitch * (size_t)(a.c_hi - a.c_lo);
                h_tile.resize(cnt);
                HIPCHK(c, hipMemcpyAsync(h_tile.data(), a.tile_score, cnt * sizeof(int32_t), hipMemcpyDeviceToHost,
                                         s));
                HIPCHK(c, hipStreamSynchronize(s));
                for (int32_t k = 0; k < nl; ++k)
                    for (int32_t cc = a.c_lo; cc < a.c_hi; ++cc)
                        scores[(int64_t)lane[(size_t)k] * C + cc] =
                            h_tile[(size_t)(cc - a.c_lo) * (size_t)pitch + (size_t)k];
            }
        }
        HIPCHK(c, c->rb.timer.mark(1, s));
        HIPCHK(c, hipMemcpyAsync(res.data(), c->rb.res.p, 4 * res_bytes, hipMemcpyDeviceToHost, s));
        if (tie_bits)
            HIPCHK(c, hipMemcpyAsync(h_bits.data(), c->rb.bits.p, h_bits.size() * sizeof(uint32_t),
                                     hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        drain.armed = false;
        kernel_ms = c->rb.timer.ms(0, 1);
        for (int32_t k = 0; k < nl; ++k) {
            const int32_t r = lane[(size_t)k];
            const int32_t f = res[(size_t)pitch + (size_t)k];
            if (f < 0 || f >= C) return fail(c, OVL_E_INTERNAL, "read depth: read %d came back without a contig", r);
            best_score[r] = res[(size_t)k];
            first_best[r] = f;
            n_best[r] = res[2 * (size_t)pitch + (size_t)k];
            const uint32_t ce = (uint32_t)res[3 * (size_t)pitch + (size_t)k];
            const Window w = window_of(r_off[r + 1] - r_off[r], c_off[f + 1] - c_off[f], read_length);
            cell_i[(size_t)r] = (int32_t)(ce >> 20);
            cell_j[(size_t)r] = best_score[r] > 0 ? (int32_t)(ce & 0xFFFFF) - w.lo : 0;
            if (tie_bits)
                memcpy(tie_bits + r * words, h_bits.data() + (size_t)k * (size_t)words,
                       sizeof(uint32_t) * (size_t)words);
        }
        c->rb.last.lane = (int64_t)nl * C;
    }

    // the other reads: one batched call per read, its copies against every contig's window, scores only
    if (!other.empty()) {
        std::vector<int32_t> w_lo((size_t)C), w_len((size_t)C), o_s((size_t)C), o_ei((size_t)C), o_ej((size_t)C),
            o_si((size_t)C), o_sj((size_t)C);
        std::vector<int64_t> q_off((size_t)C + 1), o_n((size_t)C);
        std::vector<uint8_t> q;
        for (int32_t r : other) {
            const int64_t L = r_off[r + 1] - r_off[r];
            Pick p;
            uint32_t* bits = tie_bits ? tie_bits + r * words : nullptr;
            if (L > 0) {
                q.resize((size_t)L * (size_t)C);
                for (int32_t k = 0; k < C; ++k) {
                    memcpy(q.data() + (size_t)k * (size_t)L, reads + r_off[r], (size_t)L);
                    q_off[(size_t)k] = (int64_t)k * L;
                    const Window w = window_of(L, c_off[k + 1] - c_off[k], read_length);
                    w_lo[(size_t)k] = (int32_t)(c_off[k] - c_off[0]) + w.lo;
                    w_len[(size_t)k] = w.len;
                }
                q_off[(size_t)C] = (int64_t)C * L;
                const int rb = ovl_local_align_batch(ctx, q.data(), q_off.data(), C, contigs + c_off[0],
                                                     (int32_t)sh.c_total, w_lo.data(), w_len.data(), match, mismatch,
                                                     indel, o_s.data(), o_ei.data(), o_ej.data(), o_si.data(),
                                                     o_sj.data(), nullptr, nullptr, o_n.data());
                if (rb != OVL_OK) return rb;
            } else {
                std::fill(o_s.begin(), o_s.end(), 0);
                std::fill(o_ei.begin(), o_ei.end(), 0);
                std::fill(o_ej.begin(), o_ej.end(), 0);
            }
            for (int32_t k = 0; k < C; ++k) {
                if (scores) scores[(int64_t)r * C + k] = o_s[(size_t)k];
                p.take(k, o_s[(size_t)k], o_ei[(size_t)k], o_ej[(size_t)k], bits);
            }
            best_score[r] = (int32_t)p.best;
            first_best[r] = p.first;
            n_best[r] = p.n;
            cell_i[(size_t)r] = p.bi;
            cell_j[(size_t)r] = p.bj;
        }
        c->rb.last.fallback = (int64_t)other.size() * C;
    }

    // start positions: every read with a positive score against its first best contig, with the traceback.  The
    // window is narrowed to the W columns that end at the best cell (a walk over positive cells has at
    // most floor((match * n - 1) / |indel|) left moves) when match > 0 > indel, else it is the read's whole window.
    const int64_t ind = clamp_score(indel);
    std::vector<int32_t> w_lo, w_len, o_s, o_ei, o_ej, o_si, o_sj;
    std::vector<int64_t> ops_off, o_n;
    std::vector<int8_t> ops;
    for (int32_t r0 = 0; r0 < n_reads;) {
        int32_t r1 = r0;
        int64_t total = 0;
        w_lo.clear();
        w_len.clear();
        ops_off.assign(1, 0);
        while (r1 < n_reads) {
            const int64_t L = r_off[r1 + 1] - r_off[r1];
            const int32_t f = first_best[r1];
            const Window w = window_of(L, c_off[f + 1] - c_off[f], read_length);
            int64_t lo = w.lo, len = 0;
            if (best_score[r1] > 0) {
                const int64_t E = (int64_t)w.lo + cell_j[(size_t)r1];  // the best cell's column in the contig
                if (match > 0 && ind < 0) lo = std::max<int64_t>(lo, E - (L + ((int64_t)match * L - 1) / -ind));
                len = E - lo;
            }
            if (r1 > r0 && total + L + len > kOpsBudget) break;
            w_lo.push_back((int32_t)((c_off[f] - c_off[0]) + lo));
            w_len.push_back((int32_t)len);
            total += L + len;
            ops_off.push_back(total);
            ++r1;
        }
        const int32_t nb = r1 - r0;
        ops.resize((size_t)std::max<int64_t>(total, 1));
        for (auto* v : {&o_s, &o_ei, &o_ej, &o_si, &o_sj}) v->assign((size_t)nb, 0);
        o_n.assign((size_t)nb, 0);
        bool any = false;
        for (int32_t k = 0; k < nb; ++k) any = any || w_len[(size_t)k] > 0;
        if (any) {
            const int rb = ovl_local_align_batch(ctx, reads, r_off + r0, nb, contigs + c_off[0], (int32_t)sh.c_total,
                                                 w_lo.data(), w_len.data(), match, mismatch, indel, o_s.data(),
                                                 o_ei.data(), o_ej.data(), o_si.data(), o_sj.data(), ops.data(),
                                                 ops_off.data(), o_n.data());
            if (rb != OVL_OK) return rb;
        }
        for (int32_t k = 0; k < nb; ++k) {
            const int32_t r = r0 + k;
            const int64_t L = r_off[r + 1] - r_off[r];
            const int32_t f = first_best[r];
            const Window w = window_of(L, c_off[f + 1] - c_off[f], read_length);
            int64_t sj = 0;  // window-relative start column
            if (best_score[r] > 0) {
                const int64_t lo = (int64_t)w_lo[(size_t)k] - (c_off[f] - c_off[0]);  // in the contig
                if (o_s[(size_t)k] != best_score[r] || o_ei[(size_t)k] != cell_i[(size_t)r] ||
                    lo + o_ej[(size_t)k] != (int64_t)w.lo + cell_j[(size_t)r])
                    return fail(c, OVL_E_INTERNAL,
                                "read depth: read %d's second pass found (%d, %d, %d), the score pass (%d, %d, %d)", r,
                                o_s[(size_t)k], o_ei[(size_t)k], (int)(lo + o_ej[(size_t)k]), best_score[r],
                                cell_i[(size_t)r], w.lo + cell_j[(size_t)r]);
                sj = lo + o_sj[(size_t)k] - w.lo;
            }
            best_start[r] = (int32_t)(sj + w.shift);
            best_end[r] = (int32_t)(cell_j[(size_t)r] + w.shift);
        }
        r0 = r1;
    }
    return call.done(kernel_ms);
}

OVL_API int ovl_last_read_best(const ovl_ctx* ctx, int64_t* lane_pairs, int64_t* fallback_pairs, int32_t* launches) {
    if (!ctx) return fail((ovl_ctx*)nullptr, OVL_E_ARG, "ctx is NULL");
    const ReadBestState::Last& r = ctx->devs[0]->rb.last;
    if (lane_pairs) *lane_pairs = r.lane;
    if (fallback_pairs) *fallback_pairs = r.fallback;
    if (launches) *launches = r.launches;
    return OVL_OK;
}
