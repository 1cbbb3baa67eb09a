// ovl_score_range.h — the integer-range rules of the scoring calls, as pure host functions: each says that a
// narrower representation (32-bit keys, int32 / int16 / 4-bit / f16 cells, a byte profile, a finite "-inf", a packed
// best-cell key) is exact below a bound.  ovl_plan.cpp (make_plan_full, use_dp_lane, launch_score_chunk),
// ovl_dp_lane.hip (ovl_dp_lane_h2_ok), ovl_local_host.h (local_route and the stages' argument checks) and
// ovl_depth_api.cpp (the lane-per-read kernel's scorings) call them; tests/c/score_range_check.cpp pins each edge.
// Standard headers only: a host program includes it without HIP.  DESIGN.md ("Range rules") lists the bounds.
#pragma once

#include <algorithm>
#include <cstdint>

inline int64_t iabs64(int64_t v) { return v < 0 ? -v : v; }

// M of the rules below: the largest magnitude among the three scores
inline int64_t score_mag(int64_t match, int64_t mismatch, int64_t indel) {
    return std::max(std::max(iabs64(match), iabs64(mismatch)), iabs64(indel));
}

// ----------------------------------------------------------------------------- kernel choice (make_plan_full)

// aligners.py:40: diag is taken whenever diag >= up and diag >= left.  Every dp
// value is a sum of <= lmax diagonal terms when that always holds, so it does if
// indel <= min(0, lmax*min(match,mismatch)) - max(0, lmax*max(match,mismatch)).
inline bool gaps_cannot_win(int64_t match, int64_t mismatch, int64_t indel, int64_t lmax) {
    const int64_t lo = std::min<int64_t>(0, lmax * std::min(match, mismatch));
    const int64_t hi = std::max<int64_t>(0, lmax * std::max(match, mismatch));
    return indel <= lo - hi;
}

// ungapped closed form: no int32 store can wrap
inline bool ungapped_int32_ok(int64_t match, int64_t mismatch, int64_t L) {
    const int64_t amax = std::max(iabs64(match), iabs64(mismatch));
    return amax * L < (int64_t(1) << 31);
}

// 32-bit keys (score << 16) - j need |score| < 2^15 on both sides, and the
// folded form X * ((mismatch - match) << 16) + ... a 24-bit multiplier
// (the uniform sweep compares keys without their block constant: |score| + 32*amax
//  must stay below 2^15 as well)
inline bool ungapped_key32_ok(int64_t match, int64_t mismatch, int64_t L) {
    const int64_t amax = std::max(iabs64(match), iabs64(mismatch));
    const int64_t dms = mismatch - match;
    return amax * (2 * L + 32) < (1 << 15) && iabs64(dms) < 128 && iabs64(match) < 128;
}

// full DP: |dp| <= 2*lmax*M; one more term for the candidates: int32 is exact below 2^31
inline bool dp_int32_ok(int64_t match, int64_t mismatch, int64_t indel, int64_t L) {
    const int64_t M = score_mag(match, mismatch, indel);
    return indel > INT32_MIN && M < (int64_t(1) << 31) && (2 * L + 1) * M < (int64_t(1) << 31);
}

// ----------------------------------------------------------------------------- lane-per-pair full DP

// G = dp - indel*(i+j) inside int32
inline bool dp_lane_int32_ok(int64_t match, int64_t mismatch, int64_t indel, int64_t L) {
    return !((4 * L + 4) * score_mag(match, mismatch, indel) >= (int64_t(1) << 30));
}

// the int8 score profile: match/mismatch - 2*indel as bytes, zero-profile virtual rows (indel <= 0)
inline bool dp_lane_prof_ok(int64_t match, int64_t mismatch, int64_t indel) {
    const int64_t sma = match - 2 * indel, smm = mismatch - 2 * indel;
    return indel <= 0 && sma >= -128 && sma <= 127 && smm >= -128 && smm <= 127;
}

// the int16 hand-off column (HO 1)
inline bool dp_lane_ho1_ok(int64_t match, int64_t mismatch, int64_t indel, int64_t L) {
    return (4 * L + 4) * score_mag(match, mismatch, indel) < (int64_t(1) << 15);
}

// column steps G[i][j] - G[i-1][j] lie in [0, max(match, mismatch) - 2*indel]: 4 bits in LDS (HO 2)
inline bool dp_lane_ho2_ok(int64_t match, int64_t mismatch, int64_t indel, int64_t lcap) {
    const int64_t step_max = std::max<int64_t>(match, mismatch) - 2 * indel;
    return indel <= 0 && std::max<int64_t>(match, mismatch) >= indel && step_max <= 15 && lcap <= 256;
}

// dp_lane_h2_kernel: a diagonal score's f16 encoding ends in a zero byte when its odd part is <= 7 (at most three
// significant bits); the relative values stay below 65 * 15 + 128 < 2048 under HO 2's step bound
inline bool h2_byte_score(int64_t v) {
    if (v == 0) return true;
    uint64_t u = (uint64_t)(v < 0 ? -v : v);
    while (!(u & 1)) u >>= 1;
    return u <= 7 && (v < 0 ? -v : v) <= 2048;
}

inline bool dp_lane_h2_ok(int64_t match, int64_t mismatch, int64_t indel) {
    return indel <= 0 && h2_byte_score(match - 2 * indel) && h2_byte_score(mismatch - 2 * indel) &&
           std::max(match, mismatch) - 2 * indel <= 15;
}

// ----------------------------------------------------------------------------- band knob

// "-inf" (kBandNeg) must stay below every value: |values| <= (2*lmax + 1) * M and the row
// form's scan adds up to 2*band*|indel|
inline bool band_neg_ok(int64_t match, int64_t mismatch, int64_t indel, int64_t L) {
    return (4 * L + 2) * score_mag(match, mismatch, indel) < (int64_t(1) << 29);
}

// lane per pair: byte scores (match/mismatch - 2*indel, -2*indel, -indel in int8), indel <= 0,
// G = dp - indel*(i+j) in int32 with j down to -(2*lmax + band)
inline bool band_lane_scoring_ok(int64_t match, int64_t mismatch, int64_t indel, int64_t L, int64_t band) {
    const int64_t sma = match - 2 * indel, smm = mismatch - 2 * indel;
    auto i8 = [](int64_t v) { return v >= -128 && v <= 127; };
    return indel <= 0 && i8(sma) && i8(smm) && i8(-2 * indel) &&
           (6 * L + 2 * band + 8) * score_mag(match, mismatch, indel) < (int64_t(1) << 30);
}

// ----------------------------------------------------------------------------- local alignment

// The best-cell key of the local-alignment kernels: 24-bit score, 20-bit row and column
inline bool local_limits_ok(int64_t n, int64_t m, int64_t match) {
    return n <= 0xFFFFF && m <= 0xFFFFF && std::max<int64_t>(0, match) * std::min(n, m) < (int64_t(1) << 24);
}

// Cells beyond int32: sw_kernel's wide form, and never the batch kernel
inline bool local_wide(int64_t n, int64_t m, int64_t match, int64_t mismatch, int64_t indel) {
    const int64_t M = score_mag(match, mismatch, indel);
    const int64_t top = std::max<int64_t>(0, match) * std::min(n, m);
    return M >= (int64_t(1) << 30) || top + M >= (int64_t(1) << 31);
}

// read depth, the lane-per-read kernel's scorings: the symbols renumbered into bytes with 255 kept for its padding
// rows, no positive mismatch or indel, and the score in a (v << 8) key
inline bool read_best_lane_scoring_ok(int64_t n_codes, int64_t match, int64_t mismatch, int64_t indel) {
    return n_codes <= 255 && mismatch <= 0 && indel <= 0 && match < 65536;
}
