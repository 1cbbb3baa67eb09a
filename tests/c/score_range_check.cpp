// score_range_check.cpp — the range rules of csrc/ovl_score_range.h at their edges, as a stand-alone host program
// (tests/test_score_range_cpu.py builds and runs it; `make score-range-check` runs it under the sanitizers).
//
// 1. h2_byte_score against the IEEE half encoding worked out here from the integer's bits.
// 2. Every rule on both sides of its edge: the largest accepted and the smallest rejected magnitude found by
//    bisecting the predicate, compared with the closed form, and printed ("edge <rule> <lmax> <in> <out>") for the
//    pytest side to compare with its own; every side clause (signs, byte bounds) at its two neighbouring values.
// A rule whose inequality moves by one fails at least one line here -- except where that changes nothing: the three
// clauses of dp_int32_ok (two implied by the third, whose product never meets its bound) and dp_lane_h2_ok's
// `<= 15` against `< 15` (15 is no byte score); each is noted where it is checked.
#include <cstdint>
#include <cstdio>
#include <functional>

#include "ovl_score_range.h"

static int g_failed = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                       \
        }                                                                     \
    } while (0)

// binary16 of an integer |v| <= 2048 (all exact: 11 significant bits): sign, exponent e + 15 with 2^e the leading
// bit, and the bits below the leading one moved up against the 10-bit fraction
static uint16_t half_bits(int v) {
    if (v == 0) return 0;
    const uint32_t a = (uint32_t)(v < 0 ? -v : v);
    int e = 0;
    while ((a >> (e + 1)) != 0) ++e;
    const uint32_t frac = e <= 10 ? (a << (10 - e)) & 0x3FF : (a >> (e - 10)) & 0x3FF;
    return (uint16_t)((v < 0 ? 0x8000u : 0u) | (uint32_t)(e + 15) << 10 | frac);
}

// the largest M in [0, hi) that ok accepts, for a rule that accepts 0 and is monotone in M
static int64_t edge_of(const std::function<bool(int64_t)>& ok, int64_t hi) {
    int64_t lo = 0;  // accepted
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (ok(mid)) lo = mid; else hi = mid;
    }
    return lo;
}

static void report(const char* rule, int64_t L, int64_t in, int64_t closed) {
    printf("edge %s %lld %lld %lld\n", rule, (long long)L, (long long)in, (long long)(in + 1));
    if (in != closed) {
        fprintf(stderr, "%s at lmax %lld: edge %lld, closed form %lld\n", rule, (long long)L, (long long)in,
                (long long)closed);
        ++g_failed;
    }
}

int main() {
    const int64_t P15 = int64_t(1) << 15, P24 = int64_t(1) << 24, P29 = int64_t(1) << 29, P30 = int64_t(1) << 30,
                  P31 = int64_t(1) << 31;

    // ---- 1. the f16 claim
    int n_byte = 0;
    for (int v = -2048; v <= 2048; ++v) {
        const bool zero_low = (half_bits(v) & 0xFF) == 0;
        if (h2_byte_score(v) != zero_low) {
            fprintf(stderr, "h2_byte_score(%d) = %d, half bits %04x\n", v, (int)h2_byte_score(v), half_bits(v));
            ++g_failed;
        }
        n_byte += zero_low;
    }
    EXPECT(half_bits(1) == 0x3C00 && half_bits(-2) == 0xC000 && half_bits(7) == 0x4700 && half_bits(9) == 0x4880 &&
           half_bits(2048) == 0x6800 && half_bits(-112) == 0xD700 && half_bits(1023) == 0x63FE);
    // beyond the cells' range nothing is accepted, whatever its encoding
    for (int64_t v = 2049; v <= 8192; ++v) EXPECT(!h2_byte_score(v) && !h2_byte_score(-v));
    printf("h2 %d:", n_byte);  // the accepted values, for the pytest side's numpy.float16 witness
    for (int v = -2048; v <= 2048; ++v)
        if (h2_byte_score(v)) printf(" %d", v);
    printf("\n");

    // ---- 2. the magnitude rules, for a few lmax
    for (int64_t L : {1, 100, 256, 257, 1024}) {
        // wide: (2L + 1) M < 2^31, M reached through each score
        const int64_t w = (P31 - 1) / (2 * L + 1);
        report("wide", L, edge_of([&](int64_t M) { return dp_int32_ok(M, 0, 0, L); }, P31), w);
        EXPECT(dp_int32_ok(0, -w, 0, L) && !dp_int32_ok(0, -w - 1, 0, L));
        EXPECT(dp_int32_ok(1, 0, -w, L) && !dp_int32_ok(1, 0, -w - 1, L));
        // lane int32: (4L + 4) M < 2^30
        const int64_t l32 = (P30 - 1) / (4 * L + 4);
        report("lane_int32", L, edge_of([&](int64_t M) { return dp_lane_int32_ok(M, 0, 0, L); }, P31), l32);
        EXPECT(dp_lane_int32_ok(0, -l32, 0, L) && !dp_lane_int32_ok(0, -l32 - 1, 0, L));
        EXPECT(dp_lane_int32_ok(1, 0, -l32, L) && !dp_lane_int32_ok(1, 0, -l32 - 1, L));
        // int16 hand-off column: (4L + 4) M < 2^15
        const int64_t h1 = (P15 - 1) / (4 * L + 4);
        report("ho1", L, edge_of([&](int64_t M) { return dp_lane_ho1_ok(M, 0, 0, L); }, P31), h1);
        EXPECT(dp_lane_ho1_ok(0, -h1, 0, L) && !dp_lane_ho1_ok(0, -h1 - 1, 0, L));
        EXPECT(dp_lane_ho1_ok(1, 0, -h1, L) && !dp_lane_ho1_ok(1, 0, -h1 - 1, L));
        // band "-inf": (4L + 2) M < 2^29
        const int64_t bn = (P29 - 1) / (4 * L + 2);
        report("band_neg", L, edge_of([&](int64_t M) { return band_neg_ok(M, 0, 0, L); }, P31), bn);
        EXPECT(band_neg_ok(0, -bn, 0, L) && !band_neg_ok(0, -bn - 1, 0, L));
        EXPECT(band_neg_ok(1, 0, -bn, L) && !band_neg_ok(1, 0, -bn - 1, L));
        // ungapped int32 stores: amax L < 2^31
        const int64_t u32 = (P31 - 1) / L;
        report("ungapped_int32", L, edge_of([&](int64_t M) { return ungapped_int32_ok(M, 0, L); }, P31 + 1), u32);
        EXPECT(ungapped_int32_ok(0, -u32, L) && !ungapped_int32_ok(0, -u32 - 1, L));
        // 32-bit keys: amax (2L + 32) < 2^15, isolated from the two 128 clauses by mismatch = match - 127 < -127
        const int64_t k32 = (P15 - 1) / (2 * L + 32);
        if (k32 >= 128 && k32 < 254) {
            auto ok = [&](int64_t M) { return M < 128 || ungapped_key32_ok(127 - M, -M, L); };
            report("key32", L, edge_of(ok, P31), k32);
        } else if (k32 < 128) {
            report("key32", L, edge_of([&](int64_t M) { return ungapped_key32_ok(M, 0, L); }, P31), k32);
            EXPECT(ungapped_key32_ok(0, -k32, L) && !ungapped_key32_ok(0, -k32 - 1, L));
        }
        // the band lane kernel's G: (6L + 2 band + 8) M < 2^30.  Its byte scores keep M <= 254, so at the reads the
        // kernel takes (lmax <= 1024) this clause never decides; its edge is pinned below in lmax instead
        for (int64_t band : {8, 64})
            EXPECT(band_lane_scoring_ok(127, -127, 0, L, band) && (6 * L + 2 * band + 8) * 254 < P30);
        // the best-cell key's 24-bit score: match min(n, m) < 2^24
        const int64_t lk = (P24 - 1) / L;
        report("local_key", L, edge_of([&](int64_t M) { return local_limits_ok(L, L + 5, M); }, P31), lk);
        EXPECT(local_limits_ok(L + 5, L, lk) && !local_limits_ok(L + 5, L, lk + 1));
        EXPECT(local_limits_ok(L, L, -P30));  // a negative match never scores
        // local cells in int32: match min(n, m) + M < 2^31, M >= match
        const int64_t lw = (P31 - 1) / (L + 1);
        report("local_int32", L, edge_of([&](int64_t M) { return !local_wide(L, L + 5, M, -1, -1); }, P31),
               lw < P30 ? lw : P30 - 1);
        // gaps cannot win: indel <= min(0, L min) - max(0, L max) exactly
        for (auto s : {std::pair<int64_t, int64_t>{10, -1}, {-1, 10}, {3, 2}, {-2, -3}, {0, 0}, {127, -127}}) {
            const int64_t lo = std::min<int64_t>(0, L * std::min(s.first, s.second));
            const int64_t hi = std::max<int64_t>(0, L * std::max(s.first, s.second));
            EXPECT(gaps_cannot_win(s.first, s.second, lo - hi, L));
            EXPECT(!gaps_cannot_win(s.first, s.second, lo - hi + 1, L));
        }
        EXPECT(gaps_cannot_win(10, -1, -11 * L, L) && !gaps_cannot_win(10, -1, -11 * L + 1, L));
        EXPECT(gaps_cannot_win(3, 2, -3 * L, L) && gaps_cannot_win(-2, -3, -3 * L, L) && gaps_cannot_win(0, 0, 0, L));
    }
    // implied clauses of dp_int32_ok: indel > INT32_MIN and M < 2^31 both follow from 3 M <= (2L + 1) M < 2^31
    EXPECT(!dp_int32_ok(10, -1, INT32_MIN, 1) && !dp_int32_ok(P31, 0, 0, 1) && dp_int32_ok(10, -1, INT32_MIN + 1, 0));

    // bounds that a product can meet exactly (a power of two on the left): the strict side decides
    const int64_t P28 = int64_t(1) << 28;
    EXPECT(ungapped_key32_ok(0, -127, 112) && !ungapped_key32_ok(-1, -128, 112));  // 128 * (2 * 112 + 32) = 2^15
    EXPECT(band_neg_ok(P28 - 1, 0, 0, 0) && !band_neg_ok(P28, 0, 0, 0));            // 2 * 2^28 = 2^29
    EXPECT(band_lane_scoring_ok(63, 0, 0, 2796180, 64) && !band_lane_scoring_ok(64, 0, 0, 2796180, 64));  // 2^24 * 64
    EXPECT(!local_wide(3, 3, P29 - 1, -1, -1) && local_wide(3, 3, P29, -1, -1));    // 3 * 2^29 + 2^29 = 2^31
    // ((2L + 1) M never equals 2^31 for lmax >= 1, so dp_int32_ok's `<` and `<=` agree there)

    // ---- 3. the side clauses, each at its two neighbouring values
    // 32-bit keys: |mismatch - match| and |match| below 128, both signs
    EXPECT(ungapped_key32_ok(100, -27, 1) && !ungapped_key32_ok(100, -28, 1));
    EXPECT(ungapped_key32_ok(-27, 100, 1) && !ungapped_key32_ok(-28, 100, 1));
    EXPECT(ungapped_key32_ok(127, 0, 1) && !ungapped_key32_ok(128, 1, 1));
    EXPECT(ungapped_key32_ok(-127, 0, 1) && !ungapped_key32_ok(-128, -1, 1));
    EXPECT(!ungapped_key32_ok(127, -1, 1));  // |127 - (-1)| = 128: the existing tests' scoring has 64-bit keys
    // the byte profile: indel <= 0, both diagonal scores - 2 indel in int8 (indel -60: match 7 / 8)
    EXPECT(dp_lane_prof_ok(7, -1, -60) && !dp_lane_prof_ok(8, -1, -60));
    EXPECT(dp_lane_prof_ok(-1, 7, -60) && !dp_lane_prof_ok(-1, 8, -60));
    EXPECT(dp_lane_prof_ok(1, -248, -60) && !dp_lane_prof_ok(1, -249, -60));
    EXPECT(dp_lane_prof_ok(-248, 1, -60) && !dp_lane_prof_ok(-249, 1, -60));
    EXPECT(dp_lane_prof_ok(127, -128, 0) && !dp_lane_prof_ok(129, 3, 1) && !dp_lane_prof_ok(3, 2, 1));
    // 4-bit steps: step_max 15 / 16, lcap 256 / 257, indel 0 / 1, max(match, mismatch) against indel
    EXPECT(dp_lane_ho2_ok(13, -1, -1, 256) && !dp_lane_ho2_ok(14, -1, -1, 256));
    EXPECT(dp_lane_ho2_ok(15, -2, 0, 256) && !dp_lane_ho2_ok(16, -2, 0, 256));
    EXPECT(dp_lane_ho2_ok(9, 3, -3, 256) && !dp_lane_ho2_ok(9, 10, -3, 256) && dp_lane_ho2_ok(-20, 9, -3, 256));
    EXPECT(!dp_lane_ho2_ok(13, -1, -1, 257) && dp_lane_ho2_ok(13, -1, -1, 1));
    EXPECT(dp_lane_ho2_ok(2, -1, 0, 256) && !dp_lane_ho2_ok(2, -1, 1, 256));
    EXPECT(dp_lane_ho2_ok(-3, -5, -3, 256) && !dp_lane_ho2_ok(-4, -5, -3, 256) && dp_lane_ho2_ok(-5, -3, -3, 256));
    // packed f16: byte scores on both diagonals, step <= 15 (a step of exactly 15 has no byte score: `< 16` and
    // `<= 15` and `< 15` accept the same scorings next to 14 and reject 16), indel 0 / 1
    EXPECT(dp_lane_h2_ok(14, 0, 0) && !dp_lane_h2_ok(15, 0, 0) && !dp_lane_h2_ok(16, 0, 0) && !dp_lane_h2_ok(0, 16, 0));
    EXPECT(dp_lane_h2_ok(12, -4, -1) && !dp_lane_h2_ok(7, -4, -1) && !dp_lane_h2_ok(12, -11, -1));
    EXPECT(dp_lane_h2_ok(2, 2, 0) && !dp_lane_h2_ok(2, 2, 1));
    EXPECT(dp_lane_h2_ok(1, -128, 0) && dp_lane_h2_ok(1, -112, 0));
    EXPECT(!dp_lane_h2_ok(1, -127, 0) && !dp_lane_h2_ok(1, -129, 0));
    // the band lane kernel's bytes: sma, smm 127 / 128 and -128 / -129, -2 indel at indel -63 / -64, indel 0 / 1
    EXPECT(band_lane_scoring_ok(1, 0, -63, 100, 8) && !band_lane_scoring_ok(2, 0, -63, 100, 8));
    EXPECT(band_lane_scoring_ok(0, 1, -63, 100, 8) && !band_lane_scoring_ok(0, 2, -63, 100, 8));
    EXPECT(band_lane_scoring_ok(1, -128, 0, 100, 8) && !band_lane_scoring_ok(1, -129, 0, 100, 8));
    EXPECT(band_lane_scoring_ok(-128, 1, 0, 100, 8) && !band_lane_scoring_ok(-129, 1, 0, 100, 8));
    EXPECT(band_lane_scoring_ok(-1, -2, -63, 100, 8) && !band_lane_scoring_ok(-1, -2, -64, 100, 8));
    EXPECT(band_lane_scoring_ok(2, 1, 0, 100, 8) && !band_lane_scoring_ok(2, 1, 1, 100, 8));
    for (int64_t band : {8, 64}) {  // (6L + 2 band + 8) * 10 < 2^30 in L, at (10, -1, -2)
        const int64_t l_in = ((P30 - 1) / 10 - 2 * band - 8) / 6;
        report(band == 8 ? "band_lane_lmax8" : "band_lane_lmax64", 0,
               edge_of([&](int64_t L) { return band_lane_scoring_ok(10, -1, -2, L, band); }, P30), l_in);
    }
    // local alignment: 20-bit rows and columns; M < 2^30 on its own (match 0: top is 0); top + M at 64 x 64
    EXPECT(local_limits_ok(0xFFFFF, 0xFFFFF, 16) && !local_limits_ok(0x100000, 5, 1));
    EXPECT(!local_limits_ok(5, 0x100000, 1));
    EXPECT(!local_limits_ok(0xFFFFF, 0xFFFFF, 17));  // 17 * 0xFFFFF >= 2^24 > 16 * 0xFFFFF
    EXPECT(local_limits_ok(64, 0xFFFFF, P24 / 64 - 1) && !local_limits_ok(64, 0xFFFFF, P24 / 64));
    EXPECT(!local_wide(64, 64, 0, -(P30 - 1), -1) && local_wide(64, 64, 0, -P30, -1));
    EXPECT(local_wide(64, 64, 0, -1, -P30));
    EXPECT(!local_wide(64, 64, 33038209, -1, -1) && local_wide(64, 64, 33038210, -1, -1));  // 65 M against 2^31
    EXPECT(int64_t(33038209) * 65 < P31 && int64_t(33038210) * 65 >= P31);
    // read depth, lane scorings: 255 / 256 symbols, mismatch and indel 0 / 1, match 65535 / 65536
    EXPECT(read_best_lane_scoring_ok(255, 65535, 0, 0) && !read_best_lane_scoring_ok(256, 65535, 0, 0));
    EXPECT(!read_best_lane_scoring_ok(255, 65536, 0, 0) && !read_best_lane_scoring_ok(255, 65535, 1, 0) &&
           !read_best_lane_scoring_ok(255, 65535, 0, 1));

    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("ok\n");
    return 0;
}
