// ovl_ungapped.hip — the gfx950 (CDNA4) scoring kernels of the overlap-scoring engine for gaps that cannot win.
//
// Hot path: aligners.py:27-57, the overlap DP and
// its last-row first-argmax, evaluated for every candidate pair of
// overlapGraphs.py:43-53.
//
// Kernels
//   ungapped      THE hot kernel.  Exact whenever gaps cannot win (the reference's
//                 default indel = -2**31): dp[n][j] is the sum over
//                 the L=min(n,j) diagonal cells ending at (n, j), so
//                   score(j) = match*L + (mismatch-match)*X(j),  X = mismatch count.
//                 Lane-per-pair: a lane holds both reads as bit-planes (P planes, 32
//                 bases per uint32 word) and sweeps every end position j; a mismatch
//                 word is OR_p(S_p ^ T_p) and X accumulates with v_bcnt.  No MFMA:
//                 integer compare/popcount work (BASELINE north_star).
// The rows' layouts are ovl_pack.hip's; the sweep shared with the resident grid is in ovl_sweep.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include <hip/hip_ext.h>

#include "ovl_kernels.h"
#include "ovl_sweep.h"
#include "ovl_wave.h"

namespace ovl {

using ovl_wave::wave_max_i32;

#ifdef OVL_TRACE  // diagnostic build only (make trace): per-wavefront timestamps of the uniform kernel
__device__ unsigned long long ovl_trace_buf[65536 * 8];
#endif

// Bit-shift body shared by both ungapped kernels.
//
// Coordinates: s is right-aligned in W words (s' position 32W - n + i holds
// base i) and t is left-aligned behind W zero words (t'' position 32W + u holds
// base u).  For end position j (aligners.py:54 scans j = 0..m of the last row),
// s' position x meets t'' position x + j.  With j = 32q + r, s' word k meets the
// funnel-shifted t'' word T_r[k + q] = bits [32(k+q) + r, 32(k+q) + r + 32) of t''.
// Words k < W-1-q only meet t padding; T_r[W-1] is partly padding (bits < 32-r).
// X(j) = popcount of OR_p(S_p ^ T_p) over the valid bits, and
//   dp[n][j] = match * L + (mismatch - match) * X,   L = min(n, j)
// whenever gaps cannot win.  T_r is built once per r and
// reused for every q, so the inner loop is xor / bitop3 / popcount with
// compile-time register indices.
//
// UNI (uniform pairs, n = m = lw = lmax): j <= n always, so L = j, the window never
// reaches s padding (no per-lane mask) and the key folds to one mad24.
template <int P, int W, int KM, bool UNI, bool RS1 = false>
__device__ __forceinline__ typename Key<KM>::T sweep_shifts(const uint32_t* Sw, const uint32_t* Tw,
                                                            const uint32_t* SV, int32_t n, int32_t m,
                                                            int32_t jmax, int r0, int rs_log2,
                                                            int32_t match, int32_t dms) {
    using T = typename Key<KM>::T;
    constexpr int TW = W + 1;
    const int RS = RS1 ? 1 : 1 << rs_log2;
    const int32_t d2 = (int32_t)((uint32_t)dms << 16);
    const int32_t m2 = (int32_t)((uint32_t)match << 16) - 1;
    T best = 0;
    for (int it = 0; it < (RS1 ? 32 : (32 >> rs_log2)); ++it) {
        // RS1: one lane per pair, every lane of the wavefront is on the same bit
        // shift, so r and everything derived from it is scalar (SGPR)
        const uint32_t r = RS1 ? (uint32_t)it : (uint32_t)(r0 + it * RS);
        const int rmin = it * RS;                 // smallest / largest r in the wavefront
        const int rmax = rmin + RS - 1;
        if (rmin > jmax) break;                   // j = r > jmax for every lane
        const uint32_t vt = r ? (0xFFFFFFFFu << (32u - r)) : 0u;  // valid bits of T_r[W-1]
        // U[i] = T_r[W - 1 + i], i = 0..W   (T_r[W-1] takes its low word from zero padding)
        uint32_t U[TW][P];
#pragma unroll
        for (int i = 0; i < TW; ++i) {
#pragma unroll
            for (int c = 0; c < P; ++c) {
                const uint32_t hi = i < W ? Tw[i * P + c] : 0u;  // t word W is zero (m <= 32W)
                const uint32_t lo = i ? Tw[(i - 1) * P + c] : 0u;
                U[i][c] = alignbit(hi, lo, r);
            }
        }
        const int32_t kr = (int32_t)r * m2;
#pragma unroll
        for (int q = 0; q <= W; ++q) {
            if (32 * q + rmin > jmax) break;      // wave-uniform
            const int32_t j = 32 * q + (int32_t)r;
            uint32_t X = 0;
#pragma unroll
            for (int k = (W - 1 - q > 0 ? W - 1 - q : 0); k < W; ++k) {
                const int i = k + q - (W - 1);    // U index
                // mismatch word: OR over planes of (S ^ T); v_bitop3 LUT 0xBE = (a ^ b) | c
                uint32_t mm = Sw[k * P] ^ U[i][0];
#pragma unroll
                for (int c = 1; c < P; ++c) mm = __builtin_amdgcn_bitop3_b32(Sw[k * P + c], U[i][c], mm, 0xBE);
                if (i == 0) mm &= vt;
                if constexpr (!UNI) mm &= SV[k];
                X += (uint32_t)__builtin_popcount(mm);
            }
            T key;
            if constexpr (UNI && KM == 0) {
                key = Key<0>::make_folded(X, d2, kr + 32 * q * m2);
            } else if constexpr (KM == 0) {
                // key = L * (match << 16) + X * (dms << 16) - j with two v_mad_i32_i24
                // (v_mul_lo_u32 is quarter rate); host guarantees |match|, |dms| < 128
                const int32_t L = n < j ? n : j;
                const int32_t m16 = (int32_t)((uint32_t)match << 16);
                const int32_t xs = ((int32_t)X << 8) >> 8, ls = (L << 8) >> 8;
                key = ls * ((m16 << 8) >> 8) + (xs * ((d2 << 8) >> 8) - j);
            } else {
                const int32_t L = n < j ? n : j;
                key = Key<KM>::make(match * L + dms * (int32_t)X, j);
            }
            if constexpr (UNI && RS1) {
                if (j <= jmax) best = key > best ? key : best;   // scalar condition
            } else if (UNI && 32 * q + rmax <= jmax) {
                best = key > best ? key : best;   // every lane's j is in range
            } else {
                best = (j <= m && key > best) ? key : best;
            }
        }
    }
    return best;
}

// One general-path unit: up to 64/RS pairs, RS = 2^rs_log2 lanes per pair (lanes
// slot, slot + 64/RS, ...; lane group g sweeps r = g, g + RS, ...), any lengths
// <= 32W, per-lane masks.  Writes (score, end), or (-1, -1) for a bad index.
// score one pair per group of 2^rs_log2 lanes from its rows already in registers
// (n, m = lengths; ok = valid pair); returns the pair's best key on every lane of the group
template <int P, int W, int KM>
__device__ __forceinline__ typename Key<KM>::T general_core(bool ok, int32_t n, int32_t m, const uint32_t* Sw,
                                                            const uint32_t* Tw, int r0, int rs_log2, int32_t jbound,
                                                            int32_t match, int32_t mismatch) {
    if (!ok) { n = 0; m = 0; }
    uint32_t SV[W];  // valid bits of s' word k: positions >= 32W - n
    const int pad = 32 * W - n;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int lo = pad - 32 * k;
        SV[k] = lo <= 0 ? 0xFFFFFFFFu : (lo >= 32 ? 0u : (0xFFFFFFFFu << lo));
    }
    // wave-uniform bound on end positions: the caller's (lmax) or the wave max of m
    const int jmax = jbound > 0 ? jbound : wave_max_i32(m);
    const auto best = sweep_shifts<P, W, KM, false>(Sw, Tw, SV, n, m, jmax, r0, rs_log2, match, mismatch - match);
    return group_max(best, 64 >> rs_log2);
}

template <int P, int W, int KM, int OM = 0>
__device__ __forceinline__ void general_unit(bool mine, int64_t p, int32_t a, int32_t b,
                                             const uint32_t* __restrict__ sfx, const uint32_t* __restrict__ pfx,
                                             const int32_t* __restrict__ len, int32_t n_reads, int r0,
                                             int rs_log2, int32_t jbound, int32_t match, int32_t mismatch,
                                             int32_t* __restrict__ out_score, int32_t* __restrict__ out_end,
                                             uint32_t* __restrict__ err_flag) {
    constexpr int SROW = (W * P + 3) & ~3;
    constexpr int TROW = (W * P + 3) & ~3;
    bool ok = mine && a >= 0 && a < n_reads && b >= 0 && b < n_reads;
    if (!ok) { a = 0; b = 0; }
    int32_t n = len[a], m = len[b];
    ok = ok && n <= 32 * W && m <= 32 * W;
    if (mine && !ok && r0 == 0) ovl_flag_error(err_flag);
    uint32_t Sw[SROW], Tw[TROW];
    load_words<SROW>(sfx + (int64_t)a * SROW, Sw);
    load_words<TROW>(pfx + (int64_t)b * TROW, Tw);
    const auto full = general_core<P, W, KM>(ok, n, m, Sw, Tw, r0, rs_log2, jbound, match, mismatch);
    if (mine && r0 == 0) {
        int32_t sc, en;
        Key<KM>::decode(full, sc, en);
        put_pair<OM>(out_score, out_end, p, ok ? sc : -1, ok ? en : -1, n, match, pack_inv(match, mismatch));
    }
}

// Uniform-pair kernel (P = 2 bit planes, reads of one length lw = lmax, the
// common case of simulated reads).  One lane per pair, so every lane of a
// wavefront sweeps the same bit shift r (scalar).  Pairs that are not (lw, lw)
// -- e.g. reads truncated at the genome end (generateErrorFreeReads.py:45-46) --
// are "side pairs", scored by the general path with 4, 8 or 16 lanes per pair:
//  - throughput mode (LAT = false): one wavefront per tile; side pairs are queued
//    as (p, a, b) in the wavefront's LDS ring and scored whenever 16 are waiting,
//    and once at the end;
//  - latency mode (LAT = true, about one tile per wavefront slot): two wavefronts
//    per tile running concurrently -- role 0 sweeps the uniform pairs, role 1
//    loads lengths and rows in the round trip after the indices, restages its
//    side pairs through LDS into the 4/8/16-lane layout and scores them -- so the
//    side work overlaps the sweep instead of trailing it.
// IX: the pair list is read in its compact encoding (b = ix_b16[p], 0xFFFF a bad index; a = ix_base[tile] +
// ix_d8[p]), which the copy engine moved into HBM beside the previous chunk's launch (3 bytes per pair plus 4 per
// tile over the link; ovl_pipeline.cpp encode_chunk / issue_chunk): no decode launch before it.
template <int W, int KM, bool LAT, int OM, bool IX = false>
__global__ __launch_bounds__(256, UNI_OCC(W, KM)) void uniform_kernel(
    const uint32_t* __restrict__ sfx, const uint32_t* __restrict__ pfx, const int32_t* __restrict__ len,
    int32_t n_reads, const int32_t* __restrict__ a_idx, const int32_t* __restrict__ b_idx, int64_t n_pairs,
    int32_t lw, const uint32_t* __restrict__ full, int32_t match, int32_t mismatch,
    int32_t* __restrict__ out_score, int32_t* __restrict__ out_end, uint32_t* __restrict__ err_flag,
    const int32_t* __restrict__ heavy_ids, const uint8_t* __restrict__ tile_flags, int32_t heavy_n,
    int64_t tile_base, const uint16_t* __restrict__ ix_b16, const uint8_t* __restrict__ ix_d8,
    const int32_t* __restrict__ ix_base) {
    using T = typename Key<KM>::T;
    constexpr int P = 2;
    constexpr int SROW = (W * P + 3) & ~3;
    constexpr int TROW = (W * P + 3) & ~3;
    // t-truncated pairs in the sweep (snapshot): throughput mode with int32 keys.  Not in latency mode,
    // where the side wave scores them concurrently and the sweep is the critical path (A/B, cfg2:
    // 8.2 -> 9.0 us with them in the sweep)
    constexpr bool TT = KM == 0 && !LAT;
    constexpr int RING = 128;                      // >= 15 left over + 64 from one tile
    constexpr int ROWQ = (SROW + TROW) / 4;        // uint4 per staged side pair (latency mode)
    __shared__ int4 ring_all[LAT ? 1 : 4][RING];   // throughput mode: 8 KiB per block
    __shared__ int4 side_ent[LAT ? 2 : 1][64];     // latency mode: (p, -, n, m) per side pair
    __shared__ uint4 side_rows[LAT ? 2 * 64 * ROWQ : 1];
    const int lane = threadIdx.x & 63;
    const int wib = threadIdx.x >> 6;              // wavefront in block
    // latency mode: 0 = sweep, 1 = side pairs; the side wave is the first of each pair in the block
    // (A/B with its drain at priority 1: cfg2 8.40 -> 8.33 us; without the priority 8.85 us)
    const int role = LAT ? ((wib & 1) ^ 1) : 0;
    constexpr int G = LAT ? 2 : 4;                 // tiles per block per iteration
    const int grp = LAT ? (wib >> 1) : wib;
    int4* ring = ring_all[LAT ? 0 : wib];
    const int64_t n_tiles = (n_pairs + 63) >> 6;
    int head = 0, tail = 0;                        // wave-uniform ring cursors
    // score ring[head .. head + count), count <= 16, with 64/count-ish lanes per pair:
    // 4 lanes (16 pairs), 8 lanes (<= 8), 16 lanes (<= 4) or 32 lanes (<= 2): shortest serial r loop
    auto drain = [&](int count) {
        const int rs = count > 8 ? 2 : (count > 4 ? 3 : (count > 2 ? 4 : 5));   // log2(lanes per pair)
        const int ppw = 64 >> rs;
        const int slot = lane & (ppw - 1);
        const bool mine = slot < count;
        int4 e = make_int4(0, 0, 0, 0);
        if (mine) e = ring[(head + slot) & (RING - 1)];
        general_unit<P, W, KM, OM>(mine, e.x, e.y, e.z, sfx, pfx, len, n_reads, lane >> (6 - rs), rs, lw, match,
                                   mismatch, out_score, out_end, err_flag);
        head += count;
    };
#ifdef OVL_TRACE
    const int64_t tr_id = (int64_t)blockIdx.x * 4 + wib;
    {
        uint32_t hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" : "=s"(hw), "=s"(xcc));
        OVL_TR_VAL(5, hw);
        OVL_TR_VAL(6, xcc | (role << 8));
    }
    OVL_TR_CLOCK(0, lane);
#endif
    // Heavy tiles first (throughput mode, a resident candidate list): the tiles holding side pairs cost up to
    // ~2.6x a uniform tile (their ring drains), and one landing in the last round of wavefronts is the
    // launch's tail.  Work item i < heavy_n is heavy tile heavy_ids[i] (ids in list tiles, this launch's
    // tiles start at tile_base); item heavy_n + t is tile t, skipped when it is heavy (done already).
    const bool hf = !LAT && heavy_ids != nullptr;
    const int64_t n_items = hf ? n_tiles + heavy_n : n_tiles;
    for (int64_t base = (int64_t)blockIdx.x * G; base < n_items; base += (int64_t)gridDim.x * G) {
        const int64_t item = base + grp;  // wave-uniform
        int64_t tile = item;
        if (hf) {
            if (item < heavy_n) {
                tile = (int64_t)heavy_ids[item] - tile_base;
            } else {
                tile = item - heavy_n;
                if (tile < n_tiles && tile_flags[tile_base + tile]) continue;  // wave-uniform skip
            }
        }
        const int64_t p = tile * 64 + lane;
        const bool mine = item < n_items && tile < n_tiles && p < n_pairs;
        int32_t a = 0, b = 0;
        if constexpr (IX) {
            if (mine) {
                const uint32_t bv = ix_b16[p];
                b = bv == 0xFFFFu ? -1 : (int32_t)bv;
                a = ix_base[tile] + (int32_t)ix_d8[p];
            }
        } else {
            a = mine ? a_idx[p] : 0;
            b = mine ? b_idx[p] : 0;
        }
        const bool ok = mine && a >= 0 && a < n_reads && b >= 0 && b < n_reads;
        if (!ok) { a = 0; b = 0; }
        if (LAT && role == 1) {
            // lengths and rows in the round trip after the indices; side pairs
            // restaged through LDS and scored 16 at a time
            const int32_t n = len[a], m = len[b];
            uint32_t Sw[SROW], Tw[TROW];
            load_words<SROW>(sfx + (int64_t)a * SROW, Sw);
            load_words<TROW>(pfx + (int64_t)b * TROW, Tw);
            OVL_TR_CLOCK(1, Sw[0] ^ Tw[0]);
            if (mine && !ok) {
                ovl_flag_error(err_flag);
                put_pair<OM>(out_score, out_end, p, -1, -1);
            }
            // (n = lw, m <= lw) pairs are the sweeping wave's: uniform and (TT) t-truncated alike
            const bool push = ok && (TT ? n != lw : !(n == lw && m == lw));
            const uint64_t pm = __ballot(push);
            int4* ent = side_ent[LAT ? grp : 0];
            uint4* rows = side_rows + (LAT ? grp * 64 * ROWQ : 0);
            if (push) {
                const int s = __popcll(pm & ((1ull << lane) - 1ull));
                ent[s] = make_int4((int32_t)p, 0, n, m);
#pragma unroll
                for (int k = 0; k < SROW / 4; ++k)
                    rows[s * ROWQ + k] = make_uint4(Sw[4 * k], Sw[4 * k + 1], Sw[4 * k + 2], Sw[4 * k + 3]);
#pragma unroll
                for (int k = 0; k < TROW / 4; ++k)
                    rows[s * ROWQ + SROW / 4 + k] = make_uint4(Tw[4 * k], Tw[4 * k + 1], Tw[4 * k + 2], Tw[4 * k + 3]);
            }
            const int cnt = __popcll(pm);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            // issue priority over the co-resident sweeps while the side pairs drain: the drain's chain
            // (LDS restaging, a general sweep, the group max) is the launch's tail otherwise (A/B on one
            // box, cfg2: 8.87 -> 8.39 us with levels 1-3 alike; raised from the wave's start: 8.62 us)
            __builtin_amdgcn_s_setprio(1);
            for (int h = 0; h < cnt; h += 16) {
                const int count = cnt - h < 16 ? cnt - h : 16;
                const int rs = count > 8 ? 2 : (count > 4 ? 3 : (count > 2 ? 4 : 5));
                const int slot = lane & ((64 >> rs) - 1);
                const bool own = slot < count;
                const int s = own ? h + slot : 0;
                const int4 en = ent[s];
                uint32_t Sv[SROW], Tv[TROW];
#pragma unroll
                for (int k = 0; k < SROW / 4; ++k) {
                    const uint4 v = rows[s * ROWQ + k];
                    Sv[4 * k] = v.x; Sv[4 * k + 1] = v.y; Sv[4 * k + 2] = v.z; Sv[4 * k + 3] = v.w;
                }
#pragma unroll
                for (int k = 0; k < TROW / 4; ++k) {
                    const uint4 v = rows[s * ROWQ + SROW / 4 + k];
                    Tv[4 * k] = v.x; Tv[4 * k + 1] = v.y; Tv[4 * k + 2] = v.z; Tv[4 * k + 3] = v.w;
                }
                const int r0 = lane >> (6 - rs);
                const auto full = general_core<P, W, KM>(own, en.z, en.w, Sv, Tv, r0, rs, lw, match, mismatch);
                if (own && r0 == 0) {
                    int32_t sc, e2;
                    Key<KM>::decode(full, sc, e2);
                    put_pair<OM>(out_score, out_end, en.x, sc, e2, en.z, match, pack_inv(match, mismatch));
                }
            }
            __builtin_amdgcn_s_setprio(0);
            OVL_TR_CLOCK(2, cnt);
            OVL_TR_VAL(7, cnt);
            continue;
        }
        uint32_t Sw[SROW], Tw[TROW];
        load_words<SROW>(sfx + (int64_t)a * SROW, Sw);
        load_words<TROW>(pfx + (int64_t)b * TROW, Tw);
        // read a of length lw? one bit per read (L1-resident bitmap); b's length decides uniform (m = lw).
        // TT: every other pair is scored by this sweep too -- its keys for j <= min(n, m) are the uniform
        // keys (a snapshot of the block maxima after shift min(n, m) % 32), and a shorter read a (n < m) adds
        // its windows j in (n, m] after the sweep (window_keys); else a shorter read a is a side pair
        const bool fa = ok && ((full[a >> 5] >> (a & 31)) & 1u);
        const int32_t mb = len[b];
        int32_t na = lw;
        if (TT && ok && !fa) na = len[a];
        const bool uni = fa && mb == lw;
        const bool tt = TT && ok && !uni;
        const int32_t tm = tt ? (na < mb ? na : mb) : -1;
        uint32_t tmask = 0;
        for (uint64_t bm = __ballot(tt); bm; bm &= bm - 1)  // scalar loop over the truncated lanes
            tmask |= 1u << (__builtin_amdgcn_readlane(tm, (int)__builtin_ctzll(bm)) & 31);
        OVL_TR_CLOCK(1, Sw[0] ^ Tw[0]);
        if constexpr (!LAT) {
            if (mine && !ok) ovl_flag_error(err_flag);
            const bool push = ok && !uni && !tt;
            const uint64_t pm = __ballot(push);
            if (push)
                ring[(tail + __popcll(pm & ((1ull << lane) - 1ull))) & (RING - 1)] = make_int4((int32_t)p, a, b, 0);
            tail += __popcll(pm);
        }
        T best = sweep_uniform<W, KM>(Sw, Tw, lw, match, mismatch - match, 0u, 32u, tmask, tm);
        if constexpr (TT) {
            const bool win = tt && na < mb;
            uint64_t wm = __ballot(win);
            if (wm) {  // wave-uniform: j from the largest m down to the smallest n + 1 over the window lanes
                int32_t jlo = 1 << 30, jhi = 0;
                for (; wm; wm &= wm - 1) {
                    const int l = (int)__builtin_ctzll(wm);
                    jlo = min(jlo, __builtin_amdgcn_readlane(na, l) + 1);
                    jhi = max(jhi, __builtin_amdgcn_readlane(mb, l));
                }
                const int32_t wk = window_keys<W>(Sw, Tw, na, mb, jlo, jhi, match, mismatch - match);
                if (win && (T)wk > best) best = (T)wk;
            }
        }
        OVL_TR_CLOCK(3, (uint32_t)best);
        if (mine && (uni || tt || (!LAT && !ok))) {
            int32_t sc, en;
            Key<KM>::decode(best, sc, en);
            put_pair<OM>(out_score, out_end, p, ok ? sc : -1, ok ? en : -1, na, match, pack_inv(match, mismatch));
        }
        OVL_TR_CLOCK(4, (uint32_t)best);
        if constexpr (!LAT) {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            while (tail - head >= 16) drain(16);
        }
    }
    if constexpr (!LAT) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (tail > head) drain(tail - head);
    }
}

// General kernel: any lengths <= 32W and P bit planes (used when the read set
// is not 2-plane-encodable or has no single dominant length), RS lanes per pair.
template <int P, int W, int KM>
__global__ __launch_bounds__(256) void general_kernel(
    const uint32_t* __restrict__ sfx, const uint32_t* __restrict__ pfx, const int32_t* __restrict__ len,
    int32_t n_reads, const int32_t* __restrict__ a_idx, const int32_t* __restrict__ b_idx, int64_t n_pairs,
    int32_t rs_log2, int32_t match, int32_t mismatch, int32_t* __restrict__ out_score,
    int32_t* __restrict__ out_end, uint32_t* __restrict__ err_flag) {
    const int lane = threadIdx.x & 63;
    const int ppw = 64 >> rs_log2;
    const int slot = lane & (ppw - 1);
    const int r0 = lane >> (6 - rs_log2);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t n_units = (n_pairs + ppw - 1) / ppw;
    for (int64_t u = wave; u < n_units; u += n_waves) {
        const int64_t p = u * ppw + slot;
        const bool mine = p < n_pairs;
        const int32_t a = mine ? a_idx[p] : 0;
        const int32_t b = mine ? b_idx[p] : 0;
        general_unit<P, W, KM>(mine, p, a, b, sfx, pfx, len, n_reads, r0, rs_log2, 0, match, mismatch, out_score,
                               out_end, err_flag);
    }
}

}  // namespace ovl

// ----------------------------------------------------------------------------- launchers

using namespace ovl;

template <int W, int KM, bool LAT, int OM, bool IX = false>
static void launch_uniform_4(const OvlUngappedArgs& g, unsigned blocks, hipStream_t stream) {
    if (g.ev_start) {
        hipExtLaunchKernelGGL(uniform_kernel<W, KM, LAT, OM, IX>, dim3(blocks), dim3(256), 0, stream, g.ev_start,
                              g.ev_stop, 0, g.sfx, g.pfx, g.len, g.n_reads, g.a_idx, g.b_idx, g.n_pairs, g.lw, g.full,
                              g.match, g.mismatch, g.out_score, g.out_end, g.err_flag, g.heavy_ids, g.tile_flags,
                              g.heavy_n, g.tile_base, g.ix_b16, g.ix_d8, g.ix_base);
        return;
    }
    uniform_kernel<W, KM, LAT, OM, IX><<<blocks, 256, 0, stream>>>(
        g.sfx, g.pfx, g.len, g.n_reads, g.a_idx, g.b_idx, g.n_pairs, g.lw, g.full, g.match, g.mismatch, g.out_score,
        g.out_end, g.err_flag, g.heavy_ids, g.tile_flags, g.heavy_n, g.tile_base, g.ix_b16, g.ix_d8, g.ix_base);
}

template <int W, int KM, bool LAT>
static bool launch_uniform_m(const OvlUngappedArgs& g, unsigned blocks, hipStream_t stream) {
    if (g.ix_b16) {
        // host-encoded pair lists: throughput mode, int32 keys, host-mapped results (the compact one-shot path)
        if constexpr (!LAT && KM == 0) {
            if (g.host_out == 1) {
                launch_uniform_4<W, KM, LAT, 1, true>(g, blocks, stream);
                return true;
            }
            if (g.host_out == 2) {
                launch_uniform_4<W, KM, LAT, 2, true>(g, blocks, stream);
                return true;
            }
        }
        return false;
    }
    switch (g.host_out) {
        case 0: launch_uniform_4<W, KM, LAT, 0>(g, blocks, stream); return true;
        case 1: launch_uniform_4<W, KM, LAT, 1>(g, blocks, stream); return true;
        case 2:
            if constexpr (KM == 0) {  // packed results: int32 keys only (the host asks for them only then)
                launch_uniform_4<W, KM, LAT, 2>(g, blocks, stream);
                return true;
            }
            return false;
    }
    return false;
}

template <int W, int KM>
static bool launch_uniform_t(const OvlUngappedArgs& g, unsigned blocks, hipStream_t stream) {
    // latency mode (two wavefronts per tile) when rs_log2 > 0; host-mapped outputs stream out non-temporally
    return g.rs_log2 > 0 ? launch_uniform_m<W, KM, true>(g, blocks, stream)
                         : launch_uniform_m<W, KM, false>(g, blocks, stream);
}

template <int P, int W, int KM>
static void launch_general_t(const OvlUngappedArgs& g, unsigned blocks, hipStream_t stream) {
    general_kernel<P, W, KM><<<blocks, 256, 0, stream>>>(g.sfx, g.pfx, g.len, g.n_reads, g.a_idx, g.b_idx,
                                                         g.n_pairs, g.rs_log2, g.match, g.mismatch, g.out_score,
                                                         g.out_end, g.err_flag);
}

template <int KM>
static bool dispatch_uniform(const OvlUngappedArgs& g, unsigned blocks, hipStream_t s) {
    switch (g.wmax) {
        case 1: return launch_uniform_t<1, KM>(g, blocks, s);
        case 2: return launch_uniform_t<2, KM>(g, blocks, s);
        case 3: return launch_uniform_t<3, KM>(g, blocks, s);
        case 4: return launch_uniform_t<4, KM>(g, blocks, s);
        case 5: return launch_uniform_t<5, KM>(g, blocks, s);
        case 6: return launch_uniform_t<6, KM>(g, blocks, s);
        case 7: return launch_uniform_t<7, KM>(g, blocks, s);
        case 8: return launch_uniform_t<8, KM>(g, blocks, s);
    }
    return false;
}

template <int P, int KM>
static bool dispatch_general_w(const OvlUngappedArgs& g, unsigned blocks, hipStream_t s) {
    switch (g.wmax) {
        case 1: launch_general_t<P, 1, KM>(g, blocks, s); return true;
        case 2: launch_general_t<P, 2, KM>(g, blocks, s); return true;
        case 3: launch_general_t<P, 3, KM>(g, blocks, s); return true;
        case 4: launch_general_t<P, 4, KM>(g, blocks, s); return true;
        case 5: launch_general_t<P, 5, KM>(g, blocks, s); return true;
        case 6: launch_general_t<P, 6, KM>(g, blocks, s); return true;
        case 7: launch_general_t<P, 7, KM>(g, blocks, s); return true;
        case 8: launch_general_t<P, 8, KM>(g, blocks, s); return true;
    }
    return false;
}

template <int KM>
static bool dispatch_general(const OvlUngappedArgs& g, unsigned blocks, hipStream_t s) {
    switch (g.planes) {
        case 2: return dispatch_general_w<2, KM>(g, blocks, s);
        case 4: return dispatch_general_w<4, KM>(g, blocks, s);
        case 8: return dispatch_general_w<8, KM>(g, blocks, s);
    }
    return false;
}

static unsigned grid_for(int64_t pairs, int rs_log2, int64_t max_blocks) {
    const int64_t ppw = 64 >> rs_log2;
    int64_t blocks = ((pairs + ppw - 1) / ppw + 3) / 4;  // 4 wavefronts per block
    if (blocks > max_blocks) blocks = max_blocks;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

// Uniform path (P = 2 and a dominant read length lw): uniform_kernel, which also
// scores the other pairs through its LDS side ring.  Otherwise general_kernel.
// flags[t] = 1 iff tile t (pairs 64t .. 64t + 63) holds a pair whose read a is not of the dominant length
// (a side pair of uniform_kernel's ring); one wavefront per tile
__global__ __launch_bounds__(256) void tile_flags_kernel(const int32_t* __restrict__ a_idx, int64_t n_pairs,
                                                         const uint32_t* __restrict__ full, int32_t n_reads,
                                                         uint8_t* __restrict__ flags) {
    const int64_t n_tiles = (n_pairs + 63) >> 6;
    const int lane = threadIdx.x & 63;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < n_tiles; t += (int64_t)gridDim.x * 4) {
        const int64_t p = t * 64 + lane;
        bool side = false;
        if (p < n_pairs) {
            const int32_t a = a_idx[p];
            side = a >= 0 && a < n_reads && !((full[a >> 5] >> (a & 31)) & 1u);
        }
        const uint64_t m = __ballot(side);
        if (lane == 0) flags[t] = m ? 1 : 0;
    }
}

extern "C" hipError_t ovl_launch_tile_flags(const int32_t* a_idx, int64_t n_pairs, const uint32_t* full,
                                            int32_t n_reads, uint8_t* flags, hipStream_t stream) {
    const int64_t n_tiles = (n_pairs + 63) >> 6;
    if (n_tiles <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((n_tiles + 3) / 4, 8192);
    tile_flags_kernel<<<(unsigned)blocks, 256, 0, stream>>>(a_idx, n_pairs, full, n_reads, flags);
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_ungapped(const OvlUngappedArgs* g, hipStream_t stream) {
    if (g->n_pairs <= 0) return hipSuccess;
    bool ok;
    if (g->host_out >= 2 && (g->lw <= 0 || g->key64)) return hipErrorInvalidValue;  // packed: uniform, int32 keys
    if (g->host_out < 0 || g->host_out > 2) return hipErrorInvalidValue;
    if (g->ix_b16 && (g->lw <= 0 || g->key64 || g->rs_log2 > 0 || g->heavy_ids || !g->ix_d8 || !g->ix_base))
        return hipErrorInvalidValue;  // host-encoded lists: uniform throughput mode only
    if (g->lw > 0) {
        // rs_log2 > 0 here selects the latency mode
        const unsigned nb = grid_for((g->n_pairs << (g->rs_log2 > 0 ? 1 : 0)) +
                                         (g->heavy_ids && g->rs_log2 == 0 ? 64 * (int64_t)g->heavy_n : 0),
                                     0, g->max_blocks);
        ok = g->key64 ? dispatch_uniform<1>(*g, nb, stream) : dispatch_uniform<0>(*g, nb, stream);
    } else {
        const unsigned nb = grid_for(g->n_pairs, g->rs_log2, g->max_blocks);
        ok = g->key64 ? dispatch_general<1>(*g, nb, stream) : dispatch_general<0>(*g, nb, stream);
    }
    if (!ok) return hipErrorInvalidValue;
    return hipGetLastError();
}

#ifdef OVL_TRACE
extern "C" __attribute__((visibility("default"))) int ovl_debug_trace_read(void* host, size_t bytes) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(ovl::ovl_trace_buf), bytes, 0, hipMemcpyDeviceToHost);
}
#endif
