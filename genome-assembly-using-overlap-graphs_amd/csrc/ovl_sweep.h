// ovl_sweep.h — the ungapped closed-form sweep over a pair's bit-plane rows (layouts: ovl_pack.hip), shared by
// the scoring kernels of ovl_ungapped.hip and the resident grid of ovl_resident.hip.  Device-only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace ovl {

// (the trace buffer ovl_trace_buf lives in ovl_ungapped.hip, the only file built with OVL_TRACE)
#ifdef OVL_TRACE  // diagnostic build only (make trace): per-wavefront timestamps of the uniform kernel
#define OVL_TR_CLOCK(k, dep)                                                                           \
    do {                                                                                               \
        unsigned long long t_;                                                                         \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)"            \
                     : "=s"(t_) : "v"(dep) : "memory");                                                \
        if (lane == 0 && tr_id < 65536) ovl_trace_buf[tr_id * 8 + (k)] = t_;                            \
    } while (0)
#define OVL_TR_VAL(k, v) \
    do { if (lane == 0 && tr_id < 65536) ovl_trace_buf[tr_id * 8 + (k)] = (unsigned long long)(v); } while (0)
#else
#define OVL_TR_CLOCK(k, dep) do {} while (0)
#define OVL_TR_VAL(k, v) do {} while (0)
#endif

__device__ __forceinline__ uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t r) {
    return __builtin_amdgcn_alignbit(hi, lo, r);
}

// A result store: results that leave the GPU (host-mapped output arrays) go out as non-temporal stores, so
// they stream to the link without allocating in L2; device outputs are plain stores.
template <bool HOUT>
__device__ __forceinline__ void put_result(int32_t* p, int32_t v) {
    if constexpr (HOUT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// The (score, end) of pair p into the call's result sink (OvlUngappedArgs::host_out):
//   OM 0: the int32 arrays in HBM;  OM 1: the int32 arrays, host-mapped (non-temporal stores);
//   OM 2: packed, host-mapped into a pinned staging slot that the host expands into the int32 arrays
//         (2 instead of 8 link bytes per pair).  An end j <= n (the read a's length) has L = j compared
//         bases (aligners.py:27-48 with gaps that cannot win), so score = match*(j - X) + mismatch*X and the
//         pair is (j, X): one uint16 j << 8 | X.  X = 0xFF marks the rest: j << 8 | 0xFF with the score in
//         out_end[p] (j > n: a shorter read a inside b's window), or 0xFFFF for a bad pair.  The host asks
//         for it when lmax <= 254 (so j, X <= 254) and the keys are int32; inv = 1 / (match - mismatch),
//         or 0 when they are equal (X is then immaterial and 0).
template <int OM>
__device__ __forceinline__ void put_pair(int32_t* out_score, int32_t* out_end, int64_t p, int32_t sc, int32_t en,
                                         int32_t n = 0, int32_t match = 0, float inv = 0.f) {
    if constexpr (OM == 2) {
        uint32_t v;
        if (en < 0) {
            v = 0xFFFFu;
        } else if (en > n) {
            v = ((uint32_t)en << 8) | 0xFFu;
            __builtin_nontemporal_store(sc, out_end + p);
        } else {
            // X = (match*j - score) / (match - mismatch), an exact quotient below 2^8: float is exact
            const uint32_t x = (uint32_t)__builtin_rintf((float)(match * en - sc) * inv);
            v = ((uint32_t)en << 8) | x;
        }
        __builtin_nontemporal_store((uint16_t)v, reinterpret_cast<uint16_t*>(out_score) + p);
    } else {
        put_result<OM == 1>(out_score + p, sc);
        put_result<OM == 1>(out_end + p, en);
    }
}

__device__ __forceinline__ float pack_inv(int32_t match, int32_t mismatch) {
    return match != mismatch ? 1.0f / (float)(match - mismatch) : 0.f;
}

// popcount(v) + acc as one v_bcnt_u32_b32 with its accumulator operand; kept as a chain (the compiler
// would otherwise sum a block's word counts with an extra v_add3)
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t v, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(v), "v"(acc));
    return r;
}

// (score, end) keys: key = score * 2^B - j, positive iff score > 0; the larger
// score wins, then the smaller j -- exactly the strict '>' first-argmax scan of
// aligners.py:54-57, which starts from dp[n][0] = 0 (so key <= 0 means (0, 0)).
template <int KM>
struct Key;

template <>
struct Key<0> {  // int32 keys, B = 16: needs |score| < 2^15 and j < 2^16
    using T = int32_t;
    __device__ static T make(int32_t score, int32_t j) { return (int32_t)((uint32_t)score << 16) - j; }
    // uniform pairs: key = X * (dms << 16) + j * ((match << 16) - 1), one v_mad_i32_i24
    __device__ static T make_folded(uint32_t X, int32_t d2, int32_t kj) {
        const int32_t xs = ((int32_t)X << 8) >> 8;   // both factors provably 24-bit:
        const int32_t ds = (d2 << 8) >> 8;           // one v_mad_i32_i24
        return xs * ds + kj;
    }
    __device__ static void decode(T key, int32_t& score, int32_t& end) {
        score = key > 0 ? (key + 0xFFFF) >> 16 : 0;
        end = key > 0 ? (int32_t)((uint32_t)score << 16) - key : 0;
    }
};

template <>
struct Key<1> {  // int64 keys, B = 32: any int32 score
    using T = int64_t;
    __device__ static T make(int32_t score, int32_t j) { return (int64_t)score * 4294967296ll - j; }
    __device__ static void decode(T key, int32_t& score, int32_t& end) {
        score = key > 0 ? (int32_t)((key + 0xFFFFFFFFll) >> 32) : 0;
        end = key > 0 ? (int32_t)((int64_t)score * 4294967296ll - key) : 0;
    }
};

template <int N>
__device__ __forceinline__ void load_words(const uint32_t* __restrict__ src, uint32_t (&dst)[N]) {
    static_assert(N % 4 == 0, "rows are padded to 16 bytes");
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
        const uint4 v = *reinterpret_cast<const uint4*>(src + 4 * q);
        dst[4 * q + 0] = v.x; dst[4 * q + 1] = v.y; dst[4 * q + 2] = v.z; dst[4 * q + 3] = v.w;
    }
}

template <typename T>
__device__ __forceinline__ T group_max(T best, int ppw) {
    // combine the RS lanes of a pair (lanes slot, slot + ppw, ...): across rows (offsets 32, 16) with
    // ds_bpermute, inside a 16-lane row with DPP row rotations (offsets 8, 4, 2, 1 reach the same lanes
    // as xor for a max, as one VALU op each instead of an LDS round trip)
    auto xchg = [&](T v, auto off_tag) -> T {
        constexpr int OFF = decltype(off_tag)::value;
        auto one = [&](int x) -> int {
            if constexpr (OFF >= 16) return __shfl_xor(x, OFF, 64);
            else return __builtin_amdgcn_update_dpp(x, x, 0x120 + OFF, 0xF, 0xF, false);  // row_ror:OFF
        };
        if constexpr (sizeof(T) == 4) {
            return (T)one((int)v);
        } else {
            const uint32_t lo = (uint32_t)one((int)(uint32_t)v);
            const uint32_t hi = (uint32_t)one((int)(uint32_t)((uint64_t)v >> 32));
            return (T)(((uint64_t)hi << 32) | lo);
        }
    };
    auto step = [&](auto off_tag) {
        if (ppw <= decltype(off_tag)::value) {
            const T o = xchg(best, off_tag);
            best = o > best ? o : best;
        }
    };
    step(std::integral_constant<int, 32>{});
    step(std::integral_constant<int, 16>{});
    step(std::integral_constant<int, 8>{});
    step(std::integral_constant<int, 4>{});
    step(std::integral_constant<int, 2>{});
    step(std::integral_constant<int, 1>{});
    return best;
}

// Sweep for uniform pairs (n = m = lw, P = 2, one lane per pair): every lane of
// the wavefront is on the same bit shift r, so r-derived values are scalar and
// no per-lane masking is needed (j <= lw = n means L = j and the window never
// reaches s padding).  Blocks q <= W-2 are always in range; block W-1 holds
// j = 32(W-1) + r <= lw iff r <= rcut = lw - 32(W-1); block W only j = 32W
// (r = 0, lw = 32W).  The r loop is split on rcut, so no end position needs a
// branch.  Per block q the running max is kept without its q-constant
// (key = keyq + 32q*M', M' = (match << 16) - 1), so an end position costs one
// v_mad_i32_i24 and one v_max.
//
// t-truncated pairs (n = lw, m < lw: read b cut at the genome end, generateErrorFreeReads.py:45-46) ride
// the same sweep: their end positions j <= m compare only real t bases, so their keys are the uniform
// keys, and only j > m must be dropped.  Blocks q < m/32 are always valid, blocks above m/32 never;
// block qm = m/32 is valid for r <= m % 32, so the lane snapshots best[qm] right after shift r = m % 32.
// tmask (scalar) has bit r set iff some lane of the wavefront snapshots at shift r, so a step takes the
// snapshot branch only on those shifts; tm = m for a t-truncated lane, -1 otherwise.
// Rows of at most kShiftSMaxW words shift s (W above: t; every W <= 8 the layouts have).
constexpr int kShiftSMaxW = 8;
template <int W, int KM>
__device__ __forceinline__ typename Key<KM>::T sweep_uniform(const uint32_t* Sw, const uint32_t* Tw, int32_t lw,
                                                             int32_t match, int32_t dms, uint32_t r_lo,
                                                             uint32_t r_hi, uint32_t tmask = 0u,
                                                             int32_t tm = -1) {
    using T = typename Key<KM>::T;
    constexpr int P = 2;
    constexpr int TW = W + 1;
    const int32_t rcut = lw - 32 * (W - 1);  // 1..32
    T best[W + 1];
    T qoff[W + 1];
    T mq;  // M' as T
    if constexpr (KM == 0) {
        mq = (int32_t)((uint32_t)match << 16) - 1;
    } else {
        mq = (int64_t)match * 4294967296ll - 1;
    }
#pragma unroll
    for (int q = 0; q <= W; ++q) {
        qoff[q] = (T)(32 * q) * mq;
        best[q] = -qoff[q];  // "key <= 0" for block q
    }
    const int32_t d16 = (int32_t)((uint32_t)dms << 16);
    // the mismatch factor in a VGPR: v_mad_i32_i24 then reads only one SGPR (the scalar row offset
    // rm), within gfx9's one-scalar operand limit, and needs no per-shift v_mov of rm
    int32_t dv;
    {
        const int32_t ds = (__builtin_amdgcn_readfirstlane(d16) << 8) >> 8;
        asm volatile("v_mov_b32 %0, %1" : "=v"(dv) : "s"(ds));
    }
    // keys of one r over blocks [0, NQ) (NQ compile-time), r scalar
    auto keys = [&](uint32_t r, uint32_t vt, T rm, auto nq_tag, T (&kq)[W + 1]) {
        constexpr int NQ = decltype(nq_tag)::value;
        uint32_t U[TW][P];
#pragma unroll
        for (int i = 0; i < TW; ++i) {
            if (i < NQ || (NQ > W && i <= W)) {
#pragma unroll
                for (int c = 0; c < P; ++c) {
                    const uint32_t hi = i < W ? Tw[i * P + c] : 0u;  // t word W is zero (m <= 32W)
                    const uint32_t lo = i ? Tw[(i - 1) * P + c] : 0u;
                    U[i][c] = alignbit(hi, lo, r);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            uint32_t X = 0;
#pragma unroll
            for (int k = (W - 1 - q > 0 ? W - 1 - q : 0); k < W; ++k) {
                const int i = k + q - (W - 1);
                uint32_t mm = __builtin_amdgcn_bitop3_b32(Sw[k * P + 1], U[i][1], Sw[k * P] ^ U[i][0], 0xBE);
                if (i == 0) mm &= vt;
                X = k == (W - 1 - q > 0 ? W - 1 - q : 0) ? (uint32_t)__builtin_popcount(mm) : bcnt_acc(mm, X);
            }
            if constexpr (KM == 0) {
                kq[q] = ((((int32_t)X << 8) >> 8) * ((dv << 8) >> 8)) + rm;    // v_mad_i32_i24 (dv: 24-bit)
            } else {
                kq[q] = (int64_t)dms * 4294967296ll * (int64_t)X + rm;
            }
        }
    };
    // the same keys for r >= 1 with s shifted down by 32 - r instead of t up by it (the same base pairs
    // meet): the word shifted in from above is zero, so the top word of s is one v_lshrrev (fast class)
    // where t's bottom word needed a v_alignbit with zero (slow class).  Compared positions end inside
    // s word W-1 (its low r bits, mask vt = ~0 >> (32 - r)); block q pairs shifted s word k with t word
    // k - (W-1-q).  NQ <= W (block W only at r = 0).
    auto keys_s = [&](uint32_t r, uint32_t vt, T rm, auto nq_tag, T (&kq)[W + 1]) {
        constexpr int NQ = decltype(nq_tag)::value;
        static_assert(NQ <= W, "keys_s: r >= 1 has at most W blocks");
        const uint32_t sg = 32u - r;  // 1..31
        uint32_t V[W][P];
#pragma unroll
        for (int k = W - NQ; k < W; ++k) {
#pragma unroll
            for (int c = 0; c < P; ++c)
                V[k][c] = k < W - 1 ? alignbit(Sw[(k + 1) * P + c], Sw[k * P + c], sg) : Sw[k * P + c] >> sg;
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            uint32_t X = 0;
#pragma unroll
            for (int k = W - 1 - q; k < W; ++k) {
                const int i = k - (W - 1 - q);
                uint32_t mm = __builtin_amdgcn_bitop3_b32(V[k][1], Tw[i * P + 1], V[k][0] ^ Tw[i * P], 0xBE);
                if (k == W - 1) mm &= vt;
                X = k == W - 1 - q ? (uint32_t)__builtin_popcount(mm) : bcnt_acc(mm, X);
            }
            if constexpr (KM == 0) {
                kq[q] = ((((int32_t)X << 8) >> 8) * ((dv << 8) >> 8)) + rm;    // v_mad_i32_i24 (dv: 24-bit)
            } else {
                kq[q] = (int64_t)dms * 4294967296ll * (int64_t)X + rm;
            }
        }
    };
    // r = 0 (t unshifted, block W when lw = 32W) through keys; r >= 1 through keys_s for W <= 4 (A/B on
    // one box: cfg2 -0.7 %, target -0.4 %; at W = 5, cfg3, +1.3 %, so W >= 5 kept the t shift) -- and with
    // two shifts per shifted row for every W (cfg3, W = 5: 191 against 194-197 us with the t shift; cfg5's
    // default scoring, W = 8: 445-449 against 448-452 us, and W = 6 no longer spills; three interleaved passes
    // each, profiles/r03_shift_s_w5_ab.json, r03_shift_s_w8_ab.json)
    constexpr bool SHIFT_S = W <= kShiftSMaxW;
    // Two shifts from one shifted s (keys_s2): s shifted down by 31 - r serves shift r + 1 against t as it
    // is and shift r against t moved up one bit (Tup, built once per pair), so a step of two shifts shifts
    // s once.  In Tup, bit 0 of word 0 is t position -1 (no base): that bit of a block's bottom word is
    // masked out (one v_and for blocks q >= 1; folded into the top-word mask for q = 0).
    constexpr bool PAIR = SHIFT_S && KM == 0;
    uint32_t Tup[PAIR ? W : 1][P];
    if constexpr (PAIR) {
#pragma unroll
        for (int i = 0; i < W; ++i) {
#pragma unroll
            for (int c = 0; c < P; ++c) Tup[i][c] = alignbit(Tw[i * P + c], i ? Tw[(i - 1) * P + c] : 0u, 31u);
        }
    }
    // The same for the t shift (W > kShiftSMaxW, keys_t2): t shifted up by r + 1 serves shift r + 1
    // against s as it is and shift r against s moved down one bit (Sdn); bit 31 of Sdn's word W-1 is position
    // 32W (no base): that bit of a block's top word is masked out.
    constexpr bool PAIR_T = !SHIFT_S && KM == 0;
    uint32_t Sdn[PAIR_T ? W : 1][P];
    if constexpr (PAIR_T) {
#pragma unroll
        for (int k = 0; k < W; ++k) {
#pragma unroll
            for (int c = 0; c < P; ++c)
                Sdn[k][c] = k < W - 1 ? alignbit(Sw[(k + 1) * P + c], Sw[k * P + c], 1u) : Sw[k * P + c] >> 1;
        }
    }
    auto keys_t2 = [&](uint32_t r, T rm, auto nq_tag, T (&k0)[W + 1], T (&k1)[W + 1]) {
        constexpr int NQ = decltype(nq_tag)::value;
        static_assert(NQ <= W, "keys_t2: r >= 1 has at most W blocks");
        const uint32_t r1 = r + 1;                                // 2..31
        const uint32_t vt = (uint32_t)((int32_t)0x80000000 >> r);  // U[0]: its top r + 1 bits hold bases
        uint32_t U[W][P];
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
#pragma unroll
            for (int c = 0; c < P; ++c) U[i][c] = alignbit(Tw[i * P + c], i ? Tw[(i - 1) * P + c] : 0u, r1);
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            uint32_t X0 = 0, X1 = 0;
#pragma unroll
            for (int k = W - 1 - q; k < W; ++k) {
                const int i = k + q - (W - 1);
                uint32_t m1 = __builtin_amdgcn_bitop3_b32(Sw[k * P + 1], U[i][1], Sw[k * P] ^ U[i][0], 0xBE);
                uint32_t m0 = __builtin_amdgcn_bitop3_b32(Sdn[k][1], U[i][1], Sdn[k][0] ^ U[i][0], 0xBE);
                if (i == 0) {
                    m1 &= vt;
                    m0 &= k == W - 1 ? (vt & 0x7FFFFFFFu) : vt;
                } else if (k == W - 1) {
                    m0 &= 0x7FFFFFFFu;
                }
                const bool first = k == W - 1 - q;
                X1 = first ? (uint32_t)__builtin_popcount(m1) : bcnt_acc(m1, X1);
                X0 = first ? (uint32_t)__builtin_popcount(m0) : bcnt_acc(m0, X0);
            }
            k0[q] = ((((int32_t)X0 << 8) >> 8) * ((dv << 8) >> 8)) + rm;
            k1[q] = ((((int32_t)X1 << 8) >> 8) * ((dv << 8) >> 8)) + (rm + mq);
        }
    };
    auto keys_s2 = [&](uint32_t r, T rm, auto nq_tag, T (&k0)[W + 1], T (&k1)[W + 1]) {
        constexpr int NQ = decltype(nq_tag)::value;
        static_assert(NQ <= W, "keys_s2: r >= 1 has at most W blocks");
        const uint32_t sg = 31u - r;                  // 1..30 (r + 1 <= 31)
        const uint32_t vt = 0xFFFFFFFFu >> sg;        // s word W-1: its low r + 1 bits hold bases
        uint32_t V[W][P];
#pragma unroll
        for (int k = W - NQ; k < W; ++k) {
#pragma unroll
            for (int c = 0; c < P; ++c)
                V[k][c] = k < W - 1 ? alignbit(Sw[(k + 1) * P + c], Sw[k * P + c], sg) : Sw[k * P + c] >> sg;
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            uint32_t X0 = 0, X1 = 0;
#pragma unroll
            for (int k = W - 1 - q; k < W; ++k) {
                const int i = k - (W - 1 - q);
                uint32_t m1 = __builtin_amdgcn_bitop3_b32(V[k][1], Tw[i * P + 1], V[k][0] ^ Tw[i * P], 0xBE);
                uint32_t m0 = __builtin_amdgcn_bitop3_b32(V[k][1], Tup[i][1], V[k][0] ^ Tup[i][0], 0xBE);
                if (k == W - 1) {
                    m1 &= vt;
                    m0 &= i == 0 ? (vt & ~1u) : vt;
                } else if (i == 0) {
                    m0 &= ~1u;
                }
                const bool first = k == W - 1 - q;
                X1 = first ? (uint32_t)__builtin_popcount(m1) : bcnt_acc(m1, X1);
                X0 = first ? (uint32_t)__builtin_popcount(m0) : bcnt_acc(m0, X0);
            }
            k0[q] = ((((int32_t)X0 << 8) >> 8) * ((dv << 8) >> 8)) + rm;
            k1[q] = ((((int32_t)X1 << 8) >> 8) * ((dv << 8) >> 8)) + (rm + mq);
        }
    };
    // t-truncated lanes: the best key of blocks 0..qm as they stand after shift m % 32 (block qm's last
    // valid end position).  A max under "q <= qm" masks, not a select on "q == qm": the compiler turns
    // an equality select chain into an indexed table, and the block maxima into an LDS array.
    T snap = 0;
    auto snapshot = [&](uint32_t r) {
        if (tm >= 0 && (uint32_t)(tm & 31) == r) {
            const int32_t qm = tm >> 5;
            T v = best[0] + qoff[0];
#pragma unroll
            for (int q = 1; q < W; ++q) {
                const T k = best[q] + qoff[q];
                v = q <= qm && k > v ? k : v;
            }
            snap = v;
        }
    };
    auto body = [&](uint32_t r, uint32_t vt, T rm, auto nq_tag) {
        constexpr int NQ = decltype(nq_tag)::value;
        T kq[W + 1];
        if constexpr (NQ > W || !SHIFT_S) {
            keys(r, vt, rm, nq_tag, kq);
        } else {
            if (r == 0) keys(r, vt, rm, nq_tag, kq);
            else keys_s(r, 0xFFFFFFFFu >> (32u - r), rm, nq_tag, kq);
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) best[q] = kq[q] > best[q] ? kq[q] : best[q];
        if ((tmask >> r) & 1u) snapshot(r);  // scalar branch
    };
    // two consecutive r per step: per block one 3-way max (v_max3_i32) for both keys
    auto body2 = [&](uint32_t r, T rm, auto nq_tag) {
        constexpr int NQ = decltype(nq_tag)::value;
        T k0[W + 1], k1[W + 1];
        if constexpr (PAIR) {
            keys_s2(r, rm, nq_tag, k0, k1);
        } else if constexpr (PAIR_T) {
            keys_t2(r, rm, nq_tag, k0, k1);
        } else if constexpr (SHIFT_S) {
            keys_s(r, 0xFFFFFFFFu >> (32u - r), rm, nq_tag, k0);
            keys_s(r + 1, 0xFFFFFFFFu >> (31u - r), rm + mq, nq_tag, k1);
        } else {
            keys(r, (uint32_t)((int32_t)0x80000000 >> (r - 1)), rm, nq_tag, k0);
            keys(r + 1, (uint32_t)((int32_t)0x80000000 >> r), rm + mq, nq_tag, k1);
        }
        // scalar branch: a lane snapshots after r or r + 1, from the block maxima before this step's
        // update (kept apart from it, so the update stays one v_max3_i32 per block)
        if ((tmask >> r) & 3u) {
            const uint32_t d = (uint32_t)(tm & 31) - r;
            if (tm >= 0 && d <= 1u) {
                const int32_t qm = tm >> 5;
                T v = 0;
#pragma unroll
                for (int q = 0; q < W; ++q) {
                    T k = best[q];
                    if (q < NQ) {
                        const T kk = d ? (k0[q] > k1[q] ? k0[q] : k1[q]) : k0[q];
                        k = kk > k ? kk : k;
                    }
                    k += qoff[q];
                    v = q <= qm && k > v ? k : v;
                }
                snap = v;
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const T m01 = k0[q] > k1[q] ? k0[q] : k1[q];
            best[q] = m01 > best[q] ? m01 : best[q];
        }
    };
    // r = 0: j = 32q (q >= 1); block W only when lw == 32W
    if (r_lo == 0) {
        T rm0 = 0;
        if (rcut == 32) {
            body(0u, 0u, rm0, std::integral_constant<int, W + 1>{});
        } else {
            body(0u, 0u, rm0, std::integral_constant<int, W>{});
        }
    }
    uint32_t r = r_lo > 1 ? r_lo : 1;
    T rm = (T)r * mq;
    const uint32_t rc = (uint32_t)(rcut < 31 ? rcut : 31);
    const uint32_t ra = rc < r_hi - 1 ? rc : r_hi - 1;
    // (int64 keys have no 3-way max and no registers to spare: one r per step)
    for (; KM == 0 && r + 1 <= ra; r += 2) {  // blocks 0..W-1, two r per step
        body2(r, rm, std::integral_constant<int, W>{});
        rm += 2 * mq;
    }
    for (; KM != 0 && r < ra; ++r) {
        body(r, (uint32_t)((int32_t)0x80000000 >> (r - 1)), rm, std::integral_constant<int, W>{});
        rm += mq;
    }
    if (r <= ra) {
        body(r, (uint32_t)((int32_t)0x80000000 >> (r - 1)), rm, std::integral_constant<int, W>{});
        ++r;
        rm += mq;
    }
    for (; KM == 0 && r + 1 < r_hi; r += 2) {  // blocks 0..W-2, two r per step
        body2(r, rm, std::integral_constant<int, W - 1>{});
        rm += 2 * mq;
    }
    for (; KM != 0 && r + 1 < r_hi; ++r) {
        body(r, (uint32_t)((int32_t)0x80000000 >> (r - 1)), rm, std::integral_constant<int, W - 1>{});
        rm += mq;
    }
    if (r < r_hi) {
        body(r, (uint32_t)((int32_t)0x80000000 >> (r - 1)), rm, std::integral_constant<int, W - 1>{});
        ++r;
        rm += mq;
    }
    T out = 0;
#pragma unroll
    for (int q = 0; q <= W; ++q) {
        const T k = best[q] + qoff[q];
        out = k > out ? k : out;
    }
    if (tm >= 0) {  // t-truncated: blocks below qm whole, block qm up to its snapshot
        const int32_t qm = tm >> 5;
        T t = snap > 0 ? snap : 0;
#pragma unroll
        for (int q = 0; q < W - 1; ++q) {
            const T k = best[q] + qoff[q];
            t = q < qm && k > t ? k : t;
        }
        out = t;
    }
    return out;
}

// Read a inside b's window (a lane of uniform_kernel's sweep whose read a is shorter than b, n < m): the end
// positions j in (n, m] compare all n bases of a with t[j - n, j) (L = n), which the sweep's shifts do not
// see.  j is wave-uniform -- the loop runs it from jhi down to jlo, the bounds over the wave's such lanes --
// and each lane keeps the keys of its own range.  In the rows, s base i sits at position 32W - n + i (suffix
// layout) and t base i at position i (prefix layout), so t shifted up by 32W - j puts t[j - n + i] on s base
// i; the shifted t moves up one bit per step (one v_alignbit per word and plane), and the s-padding
// positions below 32W - n are masked out.  Returns the best key of the lane's range (INT32_MIN if empty).
template <int W>
__device__ __forceinline__ int32_t window_keys(const uint32_t* Sw, const uint32_t* Tw, int32_t n, int32_t m,
                                            int32_t jlo, int32_t jhi, int32_t match, int32_t dms) {
    constexpr int P = 2;
    uint32_t SV[W];  // valid s bits: positions >= 32W - n
    const int32_t s0 = 32 * W - n;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int32_t lo = 32 * k;
        SV[k] = s0 <= lo ? ~0u : (s0 >= lo + 32 ? 0u : (~0u << (uint32_t)(s0 - lo)));
    }
    // t shifted up by sh0 = 32W - jhi (wave-uniform: word shift ws, bit shift bs)
    const int32_t sh0 = 32 * W - jhi;
    const int ws = sh0 >> 5, bs = sh0 & 31;
    uint32_t U[W][P];
#pragma unroll
    for (int k = 0; k < W; ++k) {
#pragma unroll
        for (int c = 0; c < P; ++c) {
            uint32_t hi = 0u, lo = 0u;
#pragma unroll
            for (int q = 0; q < W; ++q) {  // (scalar select on ws: no dynamic register indexing)
                if (q == ws) {
                    hi = k - q >= 0 ? Tw[(k - q) * P + c] : 0u;
                    lo = k - q - 1 >= 0 ? Tw[(k - q - 1) * P + c] : 0u;
                }
            }
            U[k][c] = bs ? alignbit(hi, lo, 32u - (uint32_t)bs) : hi;
        }
    }
    const int32_t d16 = (int32_t)((uint32_t)dms << 16);
    const int32_t kn = (int32_t)((uint32_t)(match * n) << 16);
    int32_t best = INT32_MIN;
    for (int32_t j = jhi; j >= jlo; --j) {
        uint32_t X = 0;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const uint32_t mm = __builtin_amdgcn_bitop3_b32(Sw[k * P + 1], U[k][1], Sw[k * P] ^ U[k][0], 0xBE) & SV[k];
            X = bcnt_acc(mm, X);
        }
        const int32_t key = (int32_t)X * d16 + (kn - j);
        if (j > n && j <= m && key > best) best = key;
        // j - 1: t one bit further up
#pragma unroll
        for (int k = W - 1; k >= 0; --k) {
#pragma unroll
            for (int c = 0; c < P; ++c) U[k][c] = alignbit(U[k][c], k ? U[k - 1][c] : 0u, 31u);
        }
    }
    return best;
}

// waves per SIMD uniform_kernel is compiled for (VGPR budget 512 / occupancy): the
// most that fits without spilling
#define UNI_OCC(W, KM) ((KM) == 0 ? ((W) <= 4 ? 8 : ((W) <= 5 ? 7 : ((W) <= 6 ? 6 : 4))) \
                                  : ((W) <= 4 ? 7 : ((W) <= 5 ? 6 : ((W) <= 6 ? 5 : 4))))

}  // namespace ovl
