// consensus_host_check.cpp — the host code of csrc/ovl_consensus_api.cpp (the argument checks and
// ovl_consensus_host) as a stand-alone program, for a sanitizer build on a machine without a GPU:
//
//     make -C genome-assembly-using-overlap-graphs_amd/csrc consensus-host-check
//
// compiles this file and ovl_consensus_api.cpp with -fsanitize=address,undefined (host side) and runs the result.
// It runs hand cases with known answers (the golden file's shapes in miniature), random reads and contigs against
// a plain full-table restatement of aligners.py:85-202 with the pileup and the vote written out again, every
// error case (outputs untouched), and the routing rule of ovl_local_host.h at its boundaries.  The device call is
// linked but never made: its launches and the alignment entry points are stubs here, the context helpers in
// host_check.h.
#include "host_check.h"
#include "ovl_local_host.h"

int local_batch_launch(ovl_ctx*, Dev*, const uint8_t*, const int64_t*, std::vector<LocalBatchQuery>&, const uint8_t*,
                       int32_t, const uint8_t*, bool, int32_t, int32_t, int32_t, LocalBatchRun*) {
    return OVL_E_UNSUPPORTED;
}
extern "C" int ovl_local_align(ovl_ctx*, const uint8_t*, int32_t, const uint8_t*, int32_t, int32_t, int32_t, int64_t,
                               int32_t*, int32_t*, int32_t*, int32_t*, int32_t*, int8_t*, int64_t, int64_t*) {
    return OVL_E_UNSUPPORTED;
}
extern "C" hipError_t ovl_launch_consensus_pileup(const OvlPileupArgs*, int32_t, hipStream_t) {
    return hipErrorNotSupported;
}
extern "C" hipError_t ovl_launch_consensus_add(const int64_t*, int64_t, int32_t*, hipStream_t) {
    return hipErrorNotSupported;
}
extern "C" hipError_t ovl_launch_consensus_vote(const uint8_t*, const int32_t*, int64_t, int32_t, uint8_t*,
                                                unsigned long long*, hipStream_t) {
    return hipErrorNotSupported;
}

struct Out {
    std::vector<int32_t> counts, aln;
    std::vector<uint8_t> called;
    int64_t n_changed = 77, n_other = 77;
    Out(int32_t R, int64_t total)
        : counts((size_t)total * 6 + 1, 77), aln((size_t)R * 3 + 1, 77), called((size_t)total + 1, 77) {}
};

static int run_host(const Seqs& rd, const Seqs& ct, const std::vector<int32_t>& place, int32_t read_length,
                    int32_t match, int32_t mismatch, int64_t indel, int32_t min_depth, Out& o) {
    return ovl_consensus_host(rd.data(), rd.off.data(), rd.n(), ct.data(), ct.off.data(), ct.n(), place.data(),
                              read_length, match, mismatch, indel, min_depth, o.counts.data(), o.called.data(),
                              &o.n_changed, &o.n_other, o.aln.data());
}

static int chan(char b) { return b == 'A' ? 0 : (b == 'C' ? 1 : (b == 'G' ? 2 : (b == 'T' ? 3 : -1))); }

// aligners.py:85-202 on full tables for one read on one contig, its walk piled up into `counts` (the contig's first
// base at counts[6 * base0]); returns {score, first column, one past the last column} in the contig
struct Aln {
    int64_t score, first, last;
};
static Aln pile_plain(const std::string& q, const std::string& contig, int32_t read_length, int64_t match,
                      int64_t mismatch, int64_t indel, int64_t base0, std::vector<int64_t>& counts, int64_t& other) {
    const int64_t L = (int64_t)q.size(), cm = (int64_t)contig.size();
    int64_t lo = 0;
    std::string t = contig;
    if (L < read_length && L > 0 && L < cm) {  // Python's contig[-L:]
        lo = cm - L;
        t = contig.substr((size_t)lo);
    }
    const Triple a = local_plain(q, t, match, mismatch, indel, [&](size_t i, size_t j, int op) {
        const int64_t at = (base0 + lo + (int64_t)j - 1) * 6;
        if (op == 1) {
            if (chan(q[i - 1]) >= 0) ++counts[(size_t)(at + chan(q[i - 1]))];
            else ++other;
        } else {
            ++counts[(size_t)(at + (op == 2 ? 5 : 4))];
        }
    });
    if (a.score == 0) return {0, 0, 0};
    return {a.score, lo + a.start, lo + a.end};
}

static void expect_matches_plain(const Seqs& rd, const Seqs& ct, const std::vector<int32_t>& place,
                                 int32_t read_length, int32_t match, int32_t mismatch, int64_t indel,
                                 int32_t min_depth) {
    const int32_t R = rd.n();
    const int64_t total = ct.total();
    Out o(R, total);
    EXPECT(run_host(rd, ct, place, read_length, match, mismatch, indel, min_depth, o) == OVL_OK);
    std::vector<int64_t> counts((size_t)total * 6, 0);
    int64_t other = 0, changed = 0;
    for (int32_t r = 0; r < R; ++r) {
        Aln a{0, 0, 0};
        if (place[r] >= 0)
            a = pile_plain(rd.at(r), ct.at(place[r]), read_length, match, mismatch, indel, ct.off[place[r]], counts,
                           other);
        EXPECT(o.aln[3 * r] == a.score && o.aln[3 * r + 1] == a.first && o.aln[3 * r + 2] == a.last);
    }
    for (size_t k = 0; k < counts.size(); ++k) EXPECT(o.counts[k] == counts[k]);
    for (int64_t b = 0; b < total; ++b) {
        const int64_t* v = counts.data() + b * 6;
        char call = (char)ct.bytes[(size_t)b];
        if (v[0] + v[1] + v[2] + v[3] >= min_depth) {
            const int64_t top = std::max(std::max(v[0], v[1]), std::max(v[2], v[3]));
            if (!(chan(call) >= 0 && v[chan(call)] == top))
                for (int k = 0; k < 4; ++k)
                    if (v[k] == top) { call = "ACGT"[k]; break; }
        }
        EXPECT(o.called[(size_t)b] == (uint8_t)call);
        changed += call != (char)ct.bytes[(size_t)b];
    }
    EXPECT(o.n_changed == changed && o.n_other == other);
    // the guard elements past the arrays' ends are untouched
    EXPECT(o.counts[(size_t)total * 6] == 77 && o.aln[(size_t)R * 3] == 77 && o.called[(size_t)total] == 77);
}

static std::string rand_seq(uint32_t& state, int n, int alphabet) {
    std::string s;
    for (int i = 0; i < n; ++i) {
        state = state * 1664525u + 1013904223u;
        s.push_back("ACGTN"[(state >> 24) % (uint32_t)alphabet]);
    }
    return s;
}

int main() {
    // hand cases: a gap of three, an insertion of two, a tail window, a short read longer than its contig, an
    // empty read, an empty contig, an unplaced read, a read that scores 0, an N, and the two kinds of tie
    {
        Seqs rd, ct;
        ct.add("TTACGTTTTACGTTT");  // 0
        ct.add("CCCCGGA");          // 1
        ct.add("");                 // 2
        ct.add("ACGTACGT");         // 3
        ct.add("GGA");              // 4
        ct.add("AAAAGAAAA");        // 5: the ties
        rd.add("ACGTACGT");         // gap of three on contig 0: columns 2 .. 13
        rd.add("ACGTCCACGT");       // two inserted bases on contig 3
        rd.add("GGA");              // shorter than read_length: contig 1's last three bases
        rd.add("CGGAT");            // shorter than read_length, longer than contig 4: the whole contig
        rd.add("");
        rd.add("ACGT");             // on the empty contig
        rd.add("ACGTACGT");         // unplaced
        rd.add("TTTTTTTT");         // scores 0 on contig 1
        rd.add("ACNTACGT");         // an N on a diagonal of contig 3
        rd.add("AAAACAAAA");        // contig 5, column 4: C
        rd.add("AAAATAAAA");        //                     T
        std::vector<int32_t> place = {0, 3, 1, 4, 0, 2, -1, 1, 3, 5, 5};
        Out o(rd.n(), ct.total());
        EXPECT(run_host(rd, ct, place, 8, 10, -1, -1, 1, o) == OVL_OK);
        EXPECT(o.aln[0] == 77 && o.aln[1] == 2 && o.aln[2] == 13);
        // the walk ties between diag and left at the T before the second ACGT and takes diag: the gap is columns 5 .. 7
        for (int b = 5; b < 8; ++b) EXPECT(o.counts[(size_t)b * 6 + 4] == 1);
        EXPECT(o.aln[3] == 78 && o.aln[4] == 0 && o.aln[5] == 8);
        const int64_t c3 = ct.off[3];
        EXPECT(o.counts[(size_t)(c3 + 3) * 6 + 5] == 2);  // both inserted bases on the column at their left
        EXPECT(o.aln[6] == 30 && o.aln[7] == 4 && o.aln[8] == 7);
        EXPECT(o.aln[9] == 30 && o.aln[10] == 0 && o.aln[11] == 3);  // real columns, not the shifted -2 .. 1
        for (int r : {4, 5, 6, 7})
            EXPECT(o.aln[3 * r] == 0 && o.aln[3 * r + 1] == 0 && o.aln[3 * r + 2] == 0);
        EXPECT(o.n_other == 1);
        // column 4 of contig 5 (a G): C = T = 1, no G: the first of the tied channels wins
        const int64_t c5 = ct.off[5];
        EXPECT(o.called[(size_t)c5 + 4] == 'C' && o.n_changed == 1);
        // contig 3, column 2 (a G): one G from read 1, none from the read with the N: kept
        EXPECT(o.called[(size_t)c3 + 2] == 'G');
        expect_matches_plain(rd, ct, place, 8, 10, -1, -1, 1);
        expect_matches_plain(rd, ct, place, 8, 10, -1, -1, 2);
        // a tie that holds the contig's own byte: one A against one C on an A
        Seqs r2, c2;
        c2.add("GGGGAGGGG");
        r2.add("GGGGAGGGG");
        r2.add("GGGGCGGGG");
        Out o2(2, c2.total());
        EXPECT(run_host(r2, c2, {0, 0}, 9, 10, -1, -1, 2, o2) == OVL_OK);
        EXPECT(o2.counts[4 * 6] == 1 && o2.counts[4 * 6 + 1] == 1 && o2.called[4] == 'A' && o2.n_changed == 0);
    }
    // random inputs over small alphabets (with N), random placements (-1 included), four scorings
    const int32_t scorings[4][3] = {{10, -1, -1}, {2, -3, -2}, {1, 0, -1}, {5, -4, -100000}};
    uint32_t state = 950;
    for (int round = 0; round < 8; ++round) {
        Seqs rd, ct;
        const int32_t C = 1 + round % 4;
        const int alphabet = 2 + round % 4;
        for (int32_t c = 0; c < C; ++c) {
            state = state * 1664525u + 1013904223u;
            ct.add(rand_seq(state, (int)((state >> 20) % 40), alphabet));
        }
        std::vector<int32_t> place;
        for (int32_t r = 0; r < 24; ++r) {
            state = state * 1664525u + 1013904223u;
            rd.add(rand_seq(state, (int)((state >> 20) % 24), alphabet));
            state = state * 1664525u + 1013904223u;
            place.push_back((int32_t)((state >> 16) % (uint32_t)(C + 1)) - 1);
        }
        const int32_t* s = scorings[round % 4];
        expect_matches_plain(rd, ct, place, 12, s[0], s[1], s[2], 1 + round % 3);
    }
    // no contigs, no reads, no counts, no aln
    {
        Seqs rd, ct;
        rd.add("ACGT");
        int64_t ch = 77, ot = 77;
        const int32_t none[1] = {-1};
        EXPECT(ovl_consensus_host(rd.data(), rd.off.data(), 1, nullptr, nullptr, 0, none, 4, 10, -1, -1, 3, nullptr,
                                  nullptr, &ch, &ot, nullptr) == OVL_OK);
        EXPECT(ch == 0 && ot == 0);
        ct.add("ACGT");
        uint8_t called[5] = {77, 77, 77, 77, 77};
        EXPECT(ovl_consensus_host(nullptr, nullptr, 0, ct.data(), ct.off.data(), 1, nullptr, 4, 10, -1, -1, 3, nullptr,
                                  called, &ch, &ot, nullptr) == OVL_OK);
        EXPECT(memcmp(called, "ACGT", 4) == 0 && called[4] == 77 && ch == 0);
    }
    // argument errors: nothing is written
    {
        Seqs rd, ct;
        rd.add("ACGT");
        ct.add("ACGT");
        Out o(1, 4);
        int32_t place[1] = {0};
        auto untouched = [&] {
            return o.counts[0] == 77 && o.aln[0] == 77 && o.called[0] == 77 && o.n_changed == 77 && o.n_other == 77;
        };
        auto call = [&](const uint8_t* r, const int64_t* ro, int32_t nr, const uint8_t* c, const int64_t* co,
                        int32_t nc, const int32_t* pl, int32_t rl, int32_t match, int32_t min_depth, uint8_t* called,
                        int64_t* changed) {
            return ovl_consensus_host(r, ro, nr, c, co, nc, pl, rl, match, -1, -1, min_depth, o.counts.data(), called,
                                      changed, &o.n_other, o.aln.data());
        };
        const int64_t bad_off[2] = {4, 0};
        uint8_t* cl = o.called.data();
        int64_t* nc = &o.n_changed;
        const int64_t* ro = rd.off.data();
        const int64_t* co = ct.off.data();
        EXPECT(call(rd.data(), ro, -1, ct.data(), co, 1, place, 4, 10, 3, cl, nc) == OVL_E_ARG);
        EXPECT(call(rd.data(), ro, 1, ct.data(), co, -1, place, 4, 10, 3, cl, nc) == OVL_E_ARG);
        EXPECT(call(rd.data(), ro, 1, ct.data(), co, 1, place, -1, 10, 3, cl, nc) == OVL_E_ARG);
        EXPECT(call(rd.data(), ro, 1, ct.data(), co, 1, place, 4, 10, 0, cl, nc) == OVL_E_ARG);
        EXPECT(call(rd.data(), nullptr, 1, ct.data(), co, 1, place, 4, 10, 3, cl, nc) == OVL_E_ARG);
        EXPECT(call(rd.data(), ro, 1, ct.data(), nullptr, 1, place, 4, 10, 3, cl, nc) == OVL_E_ARG);
        EXPECT(call(rd.data(), ro, 1, ct.data(), co, 1, nullptr, 4, 10, 3, cl, nc) == OVL_E_ARG);
        EXPECT(call(nullptr, ro, 1, ct.data(), co, 1, place, 4, 10, 3, cl, nc) == OVL_E_ARG);
        EXPECT(call(rd.data(), ro, 1, nullptr, co, 1, place, 4, 10, 3, cl, nc) == OVL_E_ARG);
        EXPECT(call(rd.data(), bad_off, 1, ct.data(), co, 1, place, 4, 10, 3, cl, nc) == OVL_E_ARG);
        EXPECT(call(rd.data(), ro, 1, ct.data(), bad_off, 1, place, 4, 10, 3, cl, nc) == OVL_E_ARG);
        EXPECT(call(rd.data(), ro, 1, ct.data(), co, 1, place, 4, 10, 3, nullptr, nc) == OVL_E_ARG);
        EXPECT(call(rd.data(), ro, 1, ct.data(), co, 1, place, 4, 10, 3, cl, nullptr) == OVL_E_ARG);
        const int32_t out_of_range[2] = {1, -2};
        EXPECT(call(rd.data(), ro, 1, ct.data(), co, 1, out_of_range, 4, 10, 3, cl, nc) == OVL_E_INDEX);
        EXPECT(call(rd.data(), ro, 1, ct.data(), co, 1, out_of_range + 1, 4, 10, 3, cl, nc) == OVL_E_INDEX);
        EXPECT(call(rd.data(), ro, 1, ct.data(), co, 1, place, 4, 1 << 22, 3, cl, nc) == OVL_E_UNSUPPORTED);
        const int64_t long_off[2] = {0, int64_t(1) << 20};  // (the bytes are never read: the check comes first)
        EXPECT(call(rd.data(), long_off, 1, ct.data(), co, 1, place, 4, 10, 3, cl, nc) == OVL_E_UNSUPPORTED);
        const int64_t huge_off[2] = {0, int64_t(1) << 31};
        EXPECT(call(rd.data(), ro, 1, ct.data(), huge_off, 1, place, 4, 10, 3, cl, nc) == OVL_E_UNSUPPORTED);
        EXPECT(untouched());
        EXPECT(!g_err.empty());
    }
    // the routing rule of ovl_local_align_batch and ovl_consensus (ovl_local_host.h), at each of its boundaries
    {
        using R = LocalRoute;
        // 16 strips of 64 rows stay on the batch kernel, with or without a traceback
        EXPECT(local_route(1024, 1100, 10, -1, -1, true) == R::Batch);
        EXPECT(local_route(1025, 1100, 10, -1, -1, true) == R::Single);
        EXPECT(local_route(1025, 1100, 10, -1, -1, false) == R::Single);
        // 16 strips x 65,536 steps x 64 bytes is kBatchSlabMax exactly: m + 126 reaches 65,600 at m = 65,474
        EXPECT(local_table_bytes(1024, 65473) == kBatchSlabMax);
        EXPECT(local_route(1024, 65473, 10, -1, -1, true) == R::Batch);
        EXPECT(local_route(1024, 65474, 10, -1, -1, true) == R::Single);
        EXPECT(local_route(1024, 65474, 10, -1, -1, false) == R::Batch);  // no table, no slab limit
        // wide scoring: |indel| = 2^30, and top + M = 2^31 (top = 1024 * 1,572,864 = 2^31 - 2^29, M = 2^29)
        EXPECT(local_route(100, 100, 10, -1, -(int64_t(1) << 30), true) == R::Single);
        EXPECT(local_route(100, 100, 10, -1, -(int64_t(1) << 30) + 1, true) == R::Batch);
        EXPECT(local_route(1024, 1024, 1572864, -(1 << 29), -1, false) == R::Single);
        EXPECT(local_route(1024, 1024, 1572864, -(1 << 29) + 1, -1, false) == R::Batch);
        EXPECT(local_route(0, 100, 10, -1, -1, true) == R::Empty);
        EXPECT(local_route(100, 0, 10, -1, -1, false) == R::Empty);
        EXPECT(local_route(0, 0, 1572864, -1, -(int64_t(1) << 30), true) == R::Empty);
    }
    if (g_failed) {
        fprintf(stderr, "consensus_host_check: %d checks failed\n", g_failed);
        return 1;
    }
    printf("consensus_host_check: ok\n");
    return 0;
}
