// ovl_band.hip — the band knob's row and anti-diagonal kernels (gfx950), reached from ovl_launch_dp (ovl_dp.hip)
// through launch_band_rows and launch_band_diag.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "ovl_kernels.h"

namespace ovl {

// Banded knob, row form (used when 2*band+1 <= 192, lmax <= 1024 and magnitudes are small):
// lanes own band diagonals t = j - (i - d* - band) in [0, 2*band] and the sweep walks rows.
// diag = same lane of the previous row, up = lane t+1 of the previous row (wave_shl:1; out of the
// band at t = 2*band), and the row's left dependency H[t] = max(C[t], H[t-1] + indel) becomes an
// inclusive prefix maximum of C[t] - t*indel (DPP row_shr 1/2/4/8, row_bcast 15/31), segmented per
// pair: SEG = 16, 32 or 64 lanes (4, 2 or 1 pairs per wavefront), or NC = 2/3 chunks of 64 lanes
// carried left to right.  Same values as dp_kernel<int32_t, true> (only values matter: no traceback
// in band mode).  Column 0 is the boundary (value 0) inside the band; j < 0 and j > m are not cells.
constexpr int32_t kBandNeg = -(1 << 30);  // "-inf": host keeps (4*lmax + 2) * |score| < 2^29

template <int SEG>
__device__ __forceinline__ int32_t seg_scan_max(int32_t v) {
    // inclusive prefix max inside aligned SEG-lane segments (identity kBandNeg)
    v = max(v, __builtin_amdgcn_update_dpp(kBandNeg, v, 0x111, 0xF, 0xF, false));  // row_shr:1
    v = max(v, __builtin_amdgcn_update_dpp(kBandNeg, v, 0x112, 0xF, 0xF, false));  // row_shr:2
    v = max(v, __builtin_amdgcn_update_dpp(kBandNeg, v, 0x114, 0xF, 0xF, false));  // row_shr:4
    v = max(v, __builtin_amdgcn_update_dpp(kBandNeg, v, 0x118, 0xF, 0xF, false));  // row_shr:8
    if constexpr (SEG >= 32) v = max(v, __builtin_amdgcn_update_dpp(kBandNeg, v, 0x142, 0xA, 0xF, false));  // row_bcast:15
    if constexpr (SEG >= 64) v = max(v, __builtin_amdgcn_update_dpp(kBandNeg, v, 0x143, 0xC, 0xF, false));  // row_bcast:31
    return v;
}

template <int SEG, int NC>
__global__ __launch_bounds__(256) void band_row_kernel(
    const uint8_t* __restrict__ codes, const int64_t* __restrict__ off, const int32_t* __restrict__ len,
    int32_t n_reads, const int32_t* __restrict__ a_idx, const int32_t* __restrict__ b_idx, int64_t n_pairs,
    int32_t lcap, int32_t match, int32_t mismatch, int32_t indel, int32_t band, int32_t* __restrict__ out_score,
    int32_t* __restrict__ out_end, const int32_t* __restrict__ seed, uint32_t* __restrict__ err_flag) {
    constexpr int PPW = 64 / SEG;  // pairs per wavefront
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wib = threadIdx.x >> 6;
    const int seg = lane / SEG;      // pair slot in the wavefront
    const int t0 = lane % SEG;       // band lane inside the segment (chunk 0)
    uint8_t* sq = smem + (size_t)(wib * PPW + seg) * 2 * lcap;  // this pair's s, then t
    uint8_t* st = sq + lcap;
    const int64_t n_slots = (n_pairs + PPW - 1) / PPW;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + wib;
    for (int64_t slot = wave0; slot < n_slots; slot += (int64_t)gridDim.x * 4) {
        const int64_t p = slot * PPW + seg;
        const bool mine = p < n_pairs;
        int32_t a = mine ? a_idx[p] : 0, b = mine ? b_idx[p] : 0;
        bool ok = mine && a >= 0 && a < n_reads && b >= 0 && b < n_reads;
        if (!ok) { a = 0; b = 0; }
        const int32_t n = ok ? len[a] : 0, m = ok ? len[b] : 0;
        ok = ok && n <= lcap && m <= lcap;
        if (mine && !ok && t0 == 0) {
            ovl_flag_error(err_flag);
            out_score[p] = -1;
            out_end[p] = -1;
        }
        const int32_t jstar = ok ? seed[p] : 0;  // seed from the ungapped launch
        const int32_t dstar = n - jstar;
        // stage s and t of this pair in LDS (the segment's lanes copy them)
        if (ok) {
            const uint8_t* gs = codes + off[a];
            const uint8_t* gt = codes + off[b];
            for (int q = t0; q < n; q += SEG) sq[q] = gs[q];
            for (int q = t0; q < m; q += SEG) st[q] = gt[q];
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        // rows: from r0 (first row with a cell of column >= 1 in the band) to n
        const int32_t r0 = dstar - band + 1 > 1 ? dstar - band + 1 : 1;
        int32_t rows = ok && n > 0 && m > 0 ? n - r0 + 1 : 0;
        // previous row (r0 - 1) in band lanes: row 0 is all zero, otherwise only column 0 is a value
        int32_t hp[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int32_t t = t0 + 64 * c;
            const int32_t j = (r0 - 1) - dstar - band + t;
            hp[c] = (t <= 2 * band && (j == 0 || (r0 == 1 && j >= 0 && j <= m))) ? 0 : kBandNeg;
        }
        // segments of a wavefront run different pairs: iterate to the longest
        int32_t rows_max = rows;
#pragma unroll
        for (int o = SEG; o < 64; o <<= 1) rows_max = max(rows_max, __shfl_xor(rows_max, o, 64));
        int64_t bestkey = INT64_MIN;
        for (int32_t k = 0; k < rows_max; ++k) {
            const int32_t i = r0 + k;
            const bool live = k < rows;
            const int32_t jlo = i - dstar - band;
            const uint32_t sc = live ? (uint32_t)sq[i - 1] : 0xFFFFu;
            int32_t h[NC];
            int32_t carry = kBandNeg;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int32_t t = t0 + 64 * c;
                const int32_t j = jlo + t;
                const bool cell = live && t <= 2 * band && j >= 1 && j <= m;
                const uint32_t tc = cell ? (uint32_t)st[j - 1] : 0xFFFFFu;
                // up: lane t+1 of the previous row (wave_shl:1; chunk c+1's lane 0 for lane 63)
                int32_t upv = __builtin_amdgcn_update_dpp(kBandNeg, hp[c], 0x130, 0xF, 0xF, false);
                if constexpr (NC > 1) {
                    if (c + 1 < NC) {
                        const int32_t nxt = __builtin_amdgcn_readlane(hp[c + 1 < NC ? c + 1 : c], 0);
                        if (lane == 63) upv = nxt;
                    }
                }
                const bool up_ok = t < 2 * band;
                const int32_t dv = hp[c] + (sc == tc ? match : mismatch);
                int32_t cv = up_ok ? max(dv, upv + indel) : dv;
                cv = cell ? cv : ((live && j == 0 && t <= 2 * band) ? 0 : kBandNeg);
                const int32_t tind = t * indel;
                int32_t g = seg_scan_max<SEG>(cv - tind);
                if constexpr (NC > 1) {
                    g = max(g, carry);
                    carry = __builtin_amdgcn_readlane(g, 63);
                }
                int32_t hv = g + tind;
                hv = (cell || (live && j == 0 && t <= 2 * band)) ? hv : kBandNeg;
                h[c] = hv;
                if (live && i == n && t <= 2 * band && j >= 0 && j <= m) {
                    // last row: strict '>' first argmax = max value, then smallest j
                    const int64_t key = (int64_t)hv * 2048 + (2047 - j);
                    bestkey = key > bestkey ? key : bestkey;
                }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) hp[c] = h[c];
        }
        // reduce the segment's keys
#pragma unroll
        for (int o = 1; o < SEG; o <<= 1) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)bestkey, o, 64);
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)bestkey >> 32), o, 64);
            const int64_t ok2 = (int64_t)(((uint64_t)hi << 32) | lo);
            bestkey = ok2 > bestkey ? ok2 : bestkey;
        }
        if (mine && ok && t0 == 0) {
            int32_t sc_out = 0, en_out = 0;
            if (n > 0 && m > 0 && bestkey != INT64_MIN) {
                // floor division of the packed key (value may be negative)
                const int64_t v = bestkey >= 0 ? bestkey / 2048 : -((-bestkey + 2047) / 2048);
                sc_out = (int32_t)v;
                en_out = 2047 - (int32_t)(bestkey - v * 2048);
            }
            out_score[p] = sc_out;
            out_end[p] = en_out;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // LDS reuse by the next slot
    }
}

}  // namespace ovl

using namespace ovl;  // (band_diag_kernel and the launchers are in the global namespace)

// Banded knob, anti-diagonal form (default for bands up to 255 when values fit int32).
//
// Lanes sit on band diagonals and a step is one anti-diagonal a = i + j: every cell of the band
// depends only on anti-diagonals a-1 (up: diagonal d-1, left: diagonal d+1) and a-2 (diag: own
// diagonal), so no in-step scan is needed.  A cell of diagonal d exists on every second
// anti-diagonal; each lane therefore holds D consecutive diagonals (slots k = 0..D-1, relative
// band index r = D*lane + k) and updates the even slots on even steps and the odd slots on odd
// ones, which keeps every lane busy on every step.  A segment of P = ceil((2W+1)/D) lanes holds
// one pair; 64/P segments share a wavefront.  The slot holding r = 2W is KW = 2W - D(P-1) of the
// segment's last lane; the slots above it are padding.  Band-edge predecessors ("up" of r = 0,
// "left" of r = 2W) are -inf (kBandNeg), as in oracle_overlap_banded; cells left of column 1 or
// above row 1 are the table's zero boundary.
//
// Values are kept as w = dp + indel, so both gap moves are read as stored and a cell is
// w' = max3(w_diag + (score - indel), w_up, w_left) + indel (5 VALU per cell with the compare).
// The s and t codes of each segment's pair are staged in LDS; slot k of lane l at iteration kap
// (steps 2kap, 2kap+1) reads s[I0 + kap + ceil(k/2) - 1] and t[J0 + kap - floor(k/2) - 1].
template <int D, int KW>
__global__ __launch_bounds__(64, (D <= 4 ? 8 : 6)) void band_diag_kernel(
    const uint8_t* __restrict__ codes, const int64_t* __restrict__ off, const int32_t* __restrict__ len,
    int32_t n_reads, const int32_t* __restrict__ a_idx, const int32_t* __restrict__ b_idx, int64_t n_pairs,
    int32_t lcap, int32_t match, int32_t mismatch, int32_t indel, int32_t W, int32_t nseg,
    int32_t* __restrict__ out_score, int32_t* __restrict__ out_end, const int32_t* __restrict__ seed,
    uint32_t* __restrict__ err_flag) {
    constexpr int U = 8;       // iterations (2 anti-diagonal steps each) per unrolled block
    constexpr int H = D / 2;   // slots of one parity
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int64_t* keys = reinterpret_cast<int64_t*>(smem);  // per-lane row-n keys for the segment max
    const int front = W + D + 16;
    unsigned char* chars = smem + 512 + front;
    const int lane = threadIdx.x;
    const int P = (2 * W + D) / D;
    const int seg_raw = lane / P;
    const bool real = seg_raw < nseg;
    const int seg = real ? seg_raw : nseg - 1;
    const int sl = real ? lane - seg * P : 0;
    const bool first = sl == 0;
    const bool last = real && sl == P - 1;
    unsigned char* ss = chars + (size_t)seg * 2 * lcap;
    unsigned char* ts = ss + lcap;
    const int32_t wneg = kBandNeg;
    const int32_t sc_ma = match - indel, sc_mm = mismatch - indel;
    const int64_t n_tasks = (n_pairs + nseg - 1) / nseg;
    for (int64_t task = blockIdx.x; task < n_tasks; task += gridDim.x) {
        const int64_t pair = task * nseg + seg;
        const bool live = real && pair < n_pairs;
        int32_t n = 0, m = 0, jstar = 0;
        const uint8_t* sg = codes;
        const uint8_t* tg = codes;
        bool bad = false;
        if (live) {
            const int32_t a = a_idx[pair], b = b_idx[pair];
            bad = a < 0 || a >= n_reads || b < 0 || b >= n_reads;
            if (!bad) {
                n = len[a];
                m = len[b];
                jstar = seed[pair];
                bad = n > lcap || m > lcap || jstar < 0 || jstar > m;
                sg = codes + off[a];
                tg = codes + off[b];
            }
            if (bad) n = m = jstar = 0;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // previous task's LDS readers are done
        if (live) {
#pragma unroll 4
            for (int x = sl; x < n; x += P) ss[x] = sg[x];
#pragma unroll 4
            for (int x = sl; x < m; x += P) ts[x] = tg[x];
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        // geometry: band diagonals d = dlo + r, first anti-diagonal amin (parity of dlo)
        const int32_t dstar = n - jstar, dlo = dstar - W, dhi = dstar + W;
        int32_t amin = (dlo <= 0 && dhi >= 0) ? 2 : (dlo > 0 ? dlo + 2 : 2 - dhi);
        amin -= (amin - dlo) & 1;
        const int32_t d0 = dlo + D * sl;
        const int32_t I0 = (amin + d0) >> 1, J0 = (amin - d0) >> 1;
        const int32_t KN = (2 * n - d0 - amin) >> 1;  // slot k meets row n at iteration KN - ceil(k/2)
        int32_t kend = 0, kpro = 0, ktlo = INT32_MAX, kthi = -1;
        if (live && !bad) {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const int32_t r = D * sl + k, d = d0 + k;
                if (r > 2 * W) continue;
                const int32_t par = k & 1;
                const int32_t ast = (d < 0 ? -d : d) + 2;
                const int32_t aend = min(2 * n - d, 2 * m + d);
                kpro = max(kpro, (ast - amin - par) >> 1);
                if (ast > aend) continue;
                kend = max(kend, ((aend - amin - par) >> 1) + 1);
                const int32_t jn = n - d;
                if (jn >= 1 && jn <= m) {
                    const int32_t kn = KN - ((k + 1) >> 1);
                    ktlo = min(ktlo, kn);
                    kthi = max(kthi, kn);
                }
            }
        }
        for (int o = 32; o; o >>= 1) {
            kend = max(kend, __shfl_xor(kend, o, 64));
            kpro = max(kpro, __shfl_xor(kpro, o, 64));
            ktlo = min(ktlo, __shfl_xor(ktlo, o, 64));
            kthi = max(kthi, __shfl_xor(kthi, o, 64));
        }
        // wave-uniform block bounds (multiples of U): masks before KP, row-n capture in [TL, TH)
        kend = __builtin_amdgcn_readfirstlane(kend);
        kpro = __builtin_amdgcn_readfirstlane(kpro);
        ktlo = __builtin_amdgcn_readfirstlane(ktlo);
        kthi = __builtin_amdgcn_readfirstlane(kthi);
        const int32_t KE = (kend + U - 1) / U * U;
        const int32_t KP = min(KE, (kpro + U - 1) / U * U);
        const int32_t TL = kthi < 0 ? KE : ktlo / U * U;
        const int32_t TH = kthi < 0 ? KE : min(KE, (kthi + U) / U * U);

        int32_t w[D], cap[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            w[k] = indel;  // zero boundary (w = dp + indel)
            cap[k] = wneg;
        }
        const int32_t Ai = 1 - I0, Bj = 1 - J0;  // slot k valid once kap + ceil(k/2) >= Ai, kap - floor(k/2) >= Bj
        const unsigned char* sp = ss + I0 - 1;
        const unsigned char* tp = ts + J0 - H;
        auto block = [&](int32_t kb, auto pro_t, auto trk_t) {
            constexpr bool PRO = decltype(pro_t)::value;
            constexpr bool TRK = decltype(trk_t)::value;
            int32_t S[U + H], T[U + H];
            const unsigned char* spb = sp + kb;
            const unsigned char* tpb = tp + kb;
#pragma unroll
            for (int x = 0; x < U + H; ++x) {
                S[x] = spb[x];
                T[x] = tpb[x];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int32_t kap = kb + u;
                // even step: even slots read the odd slots of the previous step
                // wave_shr:1 (lane 0 is a segment's first lane: the mask covers it)
                int32_t upsh = __builtin_amdgcn_mov_dpp(w[D - 1], 0x138, 0xF, 0xF, true);
                upsh = first ? wneg : upsh;
#pragma unroll
                for (int k = 0; k < D; k += 2) {
                    const int32_t up = k == 0 ? upsh : w[k - 1];
                    const int32_t left = (k == KW) ? (last ? wneg : w[k + 1]) : w[k + 1];
                    const int32_t sc = S[u + k / 2] == T[u + H - 1 - k / 2] ? sc_ma : sc_mm;
                    int32_t nv = max(max(w[k] + sc, up), left) + indel;
                    if constexpr (PRO) nv = ((kap + k / 2 >= Ai) & (kap - k / 2 >= Bj)) ? nv : indel;
                    w[k] = nv;
                    if constexpr (TRK) cap[k] = kap + k / 2 == KN ? nv : cap[k];
                }
                // odd step: odd slots read the even slots just written
                // wave_shl:1 (lane 63 holds padding or an unused lane: its input is never read)
                const int32_t lsh = __builtin_amdgcn_mov_dpp(w[0], 0x130, 0xF, 0xF, true);
#pragma unroll
                for (int k = 1; k < D; k += 2) {
                    const int32_t up = w[k - 1];
                    const int32_t left = k == D - 1 ? lsh : w[k + 1];
                    const int32_t sc = S[u + (k + 1) / 2] == T[u + H - 1 - (k - 1) / 2] ? sc_ma : sc_mm;
                    int32_t nv = max(max(w[k] + sc, up), left) + indel;
                    if constexpr (PRO) nv = ((kap + (k + 1) / 2 >= Ai) & (kap - (k - 1) / 2 >= Bj)) ? nv : indel;
                    w[k] = nv;
                    if constexpr (TRK) cap[k] = kap + (k + 1) / 2 == KN ? nv : cap[k];
                }
            }
        };
        using T_ = std::true_type;
        using F_ = std::false_type;
        for (int32_t kb = 0; kb < KE;) {
            const bool pro = kb < KP, trk = kb >= TL && kb < TH;
            int32_t nx = KE;
            if (KP > kb) nx = min(nx, KP);
            if (TL > kb) nx = min(nx, TL);
            if (TH > kb) nx = min(nx, TH);
            if (pro && trk) for (; kb < nx; kb += U) block(kb, T_{}, T_{});
            else if (pro) for (; kb < nx; kb += U) block(kb, T_{}, F_{});
            else if (trk) for (; kb < nx; kb += U) block(kb, F_{}, T_{});
            else for (; kb < nx; kb += U) block(kb, F_{}, F_{});
        }
        // row-n keys: max value, ties to the smallest column (the reference's first strict '>')
        int64_t key = INT64_MIN;
        if (live && !bad) {
            if (first && jstar <= W) key = (int64_t)0xFFFFFFFFll;  // j = 0 inside the band: value 0
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const int32_t r = D * sl + k, d = d0 + k, jn = n - d;
                if (r <= 2 * W && jn >= 1 && jn <= m) {
                    const int64_t kk = ((int64_t)(cap[k] - indel) << 32) | (uint32_t)~jn;
                    key = kk > key ? kk : key;
                }
            }
        }
        keys[lane] = key;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (live && first) {
            for (int x = 1; x < P; ++x) {
                const int64_t kx = keys[lane + x];
                key = kx > key ? kx : key;
            }
            if (bad) {
                ovl_flag_error(err_flag);
                out_score[pair] = -1;
                out_end[pair] = -1;
            } else {
                out_score[pair] = (int32_t)(key >> 32);
                out_end[pair] = (int32_t)~(uint32_t)key;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
}

template <int SEG, int NC>
static void launch_band_row_t(const OvlDpArgs* g, hipStream_t stream) {
    constexpr int PPW = 64 / SEG;
    const int64_t slots = (g->n_pairs + PPW - 1) / PPW;
    int64_t blocks = (slots + 3) / 4;
    if (blocks > 16384) blocks = 16384;
    const size_t lds = (size_t)4 * PPW * 2 * g->mcap;
    band_row_kernel<SEG, NC><<<(unsigned)blocks, 256, lds, stream>>>(
        g->codes, g->off, g->len, g->n_reads, g->a_idx, g->b_idx, g->n_pairs, g->mcap, (int32_t)g->match,
        (int32_t)g->mismatch, (int32_t)g->indel, g->band, g->out_score, g->out_end, g->seed, g->err_flag);
}

template <int D, int KW>
static void launch_band_diag_t(const OvlDpArgs* g, int nseg, hipStream_t stream) {
    const int W = g->band;
    const int64_t lcap = g->mcap > 0 ? g->mcap : 1;
    // keys + front pad + one 2*lcap stride per segment (s then t) + the over-read tail
    const size_t lds = 512 + (size_t)(W + D + 16) + (size_t)(nseg + 1) * 2 * lcap + W + 64;
    int64_t blocks = (g->n_pairs + nseg - 1) / nseg;
    if (blocks > 32768) blocks = 32768;
    band_diag_kernel<D, KW><<<(unsigned)blocks, 64, lds, stream>>>(
        g->codes, g->off, g->len, g->n_reads, g->a_idx, g->b_idx, g->n_pairs, (int32_t)lcap, (int32_t)g->match,
        (int32_t)g->mismatch, (int32_t)g->indel, W, nseg, g->out_score, g->out_end, g->seed, g->err_flag);
}

// Slots per lane for the anti-diagonal form: the VALU cost per pair-iteration is about
// (5 D + 8) / segments-per-wave; the smallest wins.  Returns D (0: band too wide).
extern "C" int ovl_band_diag_slots(int32_t band, int32_t lcap, int32_t* nseg_out) {
    int bestD = 0, bestseg = 0;
    double bestc = 1e30;
    for (int D = 2; D <= 8; D *= 2) {
        const int P = (2 * band + D) / D;
        if (P > 64) continue;
        int nseg = 64 / P;
        // keep the per-wave LDS near 24 KiB (at least one segment)
        const int64_t per = 2 * (int64_t)(lcap > 0 ? lcap : 1);
        const int64_t fit = (24576 - 1024 - 2 * (int64_t)band) / per - 1;
        if (nseg > fit) nseg = fit > 1 ? (int)fit : 1;
        const double c = (5.0 * D + 8.0) / nseg;
        if (c < bestc - 1e-9) {
            bestc = c;
            bestD = D;
            bestseg = nseg;
        }
    }
    if (nseg_out) *nseg_out = bestseg;
    return bestD;
}

hipError_t ovl::launch_band_diag(const OvlDpArgs* g, hipStream_t stream) {
    int nseg = 0;
    const int D = ovl_band_diag_slots(g->band, g->mcap, &nseg);
    if (D == 0) return hipErrorInvalidValue;
    const int P = (2 * g->band + D) / D;
    const int KW = 2 * g->band - D * (P - 1);
    switch (D * 16 + KW) {
        case 2 * 16 + 0: launch_band_diag_t<2, 0>(g, nseg, stream); break;
        case 4 * 16 + 0: launch_band_diag_t<4, 0>(g, nseg, stream); break;
        case 4 * 16 + 2: launch_band_diag_t<4, 2>(g, nseg, stream); break;
        case 8 * 16 + 0: launch_band_diag_t<8, 0>(g, nseg, stream); break;
        case 8 * 16 + 2: launch_band_diag_t<8, 2>(g, nseg, stream); break;
        case 8 * 16 + 4: launch_band_diag_t<8, 4>(g, nseg, stream); break;
        case 8 * 16 + 6: launch_band_diag_t<8, 6>(g, nseg, stream); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t ovl::launch_band_rows(const OvlDpArgs* g, hipStream_t stream) {
    const int lanes = 2 * g->band + 1;
    if (lanes <= 16) launch_band_row_t<16, 1>(g, stream);
    else if (lanes <= 32) launch_band_row_t<32, 1>(g, stream);
    else if (lanes <= 64) launch_band_row_t<64, 1>(g, stream);
    else if (lanes <= 128) launch_band_row_t<64, 2>(g, stream);
    else if (lanes <= 192) launch_band_row_t<64, 3>(g, stream);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
