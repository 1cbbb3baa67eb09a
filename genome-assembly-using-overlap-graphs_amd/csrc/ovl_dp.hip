// ovl_dp.hip — the generic DP kernels of the overlap-scoring engine (gfx950) and ovl_launch_dp.
//
// Kernels
//   dp            anti-diagonal wavefront DP for any scoring (finite indel), int64
//                 arithmetic with int32 stores like Numba; lanes own rows, the row
//                 carried between 64-row strips and the t symbols are staged in LDS.
//   dp_fast       the same strips and anti-diagonals, scores only, in unrolled 64-step chunks.
// The band knob's row and anti-diagonal forms are in ovl_band.hip; ovl_launch_dp switches between the forms.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "ovl_kernels.h"
#include "ovl_wave.h"

namespace ovl {

using namespace ovl_wave;

// One wavefront (block of 64) per pair, grid-stride over pairs.  Strip of 64
// rows i = 64*st + 1 + lane; anti-diagonal step tau has lane l on column
// j = tau - l + 1.  up / t-symbol arrive from lane l-1 by DPP; lane 0 reads
// them from the staged LDS row (the previous strip's last row) and t codes.
// Cell rule of aligners.py:35-48 with Acc-width arithmetic; the stored value
// is narrowed to int32 as the reference's int32 table does.
// BANDED (the build's band knob, oracle_overlap_banded; not a reference mode):
// seed[pair] holds the seed end j* (the ungapped closed form's first argmax,
// written by the launch before into a separate buffer, so out_* may be host memory); only cells with
// |(i - j) - d*| <= band, d* = n - j*, are filled, out-of-band predecessors
// count as -inf, and only strips and anti-diagonal steps that meet the band are
// swept.  A cell's diagonal predecessor is always in the band; "up" leaves it
// only at the row's last band cell and "left" only at its first.
template <typename Acc, bool BANDED>
__global__ __launch_bounds__(64) void dp_kernel(
    const uint8_t* __restrict__ codes, const int64_t* __restrict__ off, const int32_t* __restrict__ len,
    int32_t n_reads, const int32_t* __restrict__ a_idx, const int32_t* __restrict__ b_idx,
    int64_t n_pairs, int32_t mcap, int64_t match, int64_t mismatch, int64_t indel, int32_t band,
    int32_t* __restrict__ out_score, int32_t* __restrict__ out_end, const int32_t* __restrict__ seed,
    int8_t* __restrict__ tb, uint32_t* __restrict__ err_flag) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int32_t* row0 = reinterpret_cast<int32_t*>(smem);
    int32_t* row1 = row0 + (mcap + 1);
    uint8_t* tcodes = reinterpret_cast<uint8_t*>(row1 + (mcap + 1));
    const int lane = threadIdx.x;
    for (int64_t pair = blockIdx.x; pair < n_pairs; pair += gridDim.x) {
        const int32_t a = a_idx[pair];
        const int32_t b = b_idx[pair];
        if (a < 0 || a >= n_reads || b < 0 || b >= n_reads || len[b] > mcap) {
            if (lane == 0) {
                ovl_flag_error(err_flag);
                out_score[pair] = -1;
                out_end[pair] = -1;
            }
            continue;
        }
        const int32_t n = len[a];
        const int32_t m = len[b];
        const uint8_t* s = codes + off[a];
        const uint8_t* t = codes + off[b];
        // band: seed diagonal d* and the rows [rlo, rhi] that hold band cells
        const int32_t dstar = BANDED ? n - seed[pair] : 0;
        const int32_t W = BANDED ? band : 0;
        const int32_t rlo = BANDED ? (dstar - W + 1 > 1 ? dstar - W + 1 : 1) : 1;
        __syncthreads();  // previous pair's LDS readers are done
        for (int j = lane; j <= m; j += 64) row0[j] = 0;
        for (int j = lane; j < m; j += 64) tcodes[j] = t[j];
        __syncthreads();
        int32_t* rin = row0;
        int32_t* rout = row1;
        // tracked by the lane that owns row n; dp[n][0] = 0 is the j = 0 candidate
        // (in banded mode only when (n, 0) is in the band)
        int32_t best = (!BANDED || n - dstar - W <= 0) ? 0 : INT32_MIN, bend = 0;
        const int nstrips = (n + 63) >> 6;
        const int st0 = BANDED ? (rlo - 1) >> 6 : 0;
        for (int st = st0; st < nstrips; ++st) {
            const int32_t i = 64 * st + 1 + lane;
            const bool row_ok = i <= n;
            const uint32_t sc = row_ok ? (uint32_t)s[i - 1] : 0xFFFFFFFFu;
            // anti-diagonal steps: lane L is on column j = tau - L + 1
            int tau_lo = 0, tau_hi = m + 62;
            if (BANDED) {
                const int lmax = (n - 64 * st - 1) < 63 ? (n - 64 * st - 1) : 63;
                const int lo = 64 * st - dstar - W;
                const int hi = 64 * st + 2 * lmax - dstar + W;
                tau_lo = lo > 0 ? lo : 0;
                tau_hi = hi < tau_hi ? hi : tau_hi;
            }
            const int32_t jlo = i - dstar - W, jhi = i - dstar + W;  // unclamped band edges of row i
            int32_t cur = 0;      // dp[i][j-1] (starts as dp[i][0] = 0)
            // dp[i-1][j-1]; lane 0 starts mid-row in banded mode
            int32_t uprev = (BANDED && lane == 0) ? rin[tau_lo] : 0;
            uint32_t tch = 0;
            const bool last_strip_row = (lane == 63) && (st + 1 < nstrips);
            for (int tau = tau_lo; tau <= tau_hi; ++tau) {
                const int32_t j = tau - lane + 1;
                // lane 0's inputs come from LDS (uniform address: broadcast)
                const int32_t jj = tau + 1 <= m ? tau + 1 : m;
                const int32_t lds_up = rin[jj];
                const uint32_t lds_t = tau < m ? (uint32_t)tcodes[tau] : 0u;
                int32_t upin = shr1<int32_t>(cur);
                uint32_t tin = (uint32_t)shr1<int32_t>((int32_t)tch);
                if (lane == 0) { upin = lds_up; tin = lds_t; }
                const bool in_band = !BANDED || (j >= jlo && j <= jhi);
                if (row_ok && j >= 1 && j <= m && in_band) {
                    const Acc diag = (Acc)uprev + (sc == tin ? (Acc)match : (Acc)mismatch);
                    const Acc up = (Acc)upin + (Acc)indel;
                    const Acc left = (Acc)cur + (Acc)indel;
                    const bool up_ok = !BANDED || j != jhi;
                    const bool left_ok = !BANDED || j != jlo;
                    int8_t dir;
                    Acc v;
                    if ((!up_ok || diag >= up) && (!left_ok || diag >= left)) { v = diag; dir = 0; }
                    else if (up_ok && (!left_ok || up >= left))               { v = up;   dir = 1; }
                    else                                                      { v = left; dir = 2; }
                    cur = (int32_t)v;
                    if (!BANDED && tb) tb[(int64_t)i * (m + 1) + j] = dir;
                    if (i == n && cur > best) { best = cur; bend = j; }
                    if (last_strip_row) rout[j] = cur;
                }
                uprev = upin;
                tch = tin;
            }
            __syncthreads();
            if (lane == 0 && st + 1 < nstrips) rout[0] = 0;
            __syncthreads();
            int32_t* tmp = rin; rin = rout; rout = tmp;
        }
        // row n lives in lane (n-1) % 64 of the last strip
        const int owner = (n - 1) & 63;
        const int32_t bs = __shfl(best, owner, 64);
        const int32_t be = __shfl(bend, owner, 64);
        __syncthreads();  // every lane is done with this pair's LDS rows
        if (lane == 0) {
            out_score[pair] = n > 0 && m > 0 ? bs : 0;
            out_end[pair] = n > 0 && m > 0 ? be : 0;
        }
    }
}

// Full DP, scores only (no traceback, no band): the scoring path for gapped parameters.
// Same strips and anti-diagonals as dp_kernel, restructured for issue: 64-step chunks with the step
// loop unrolled at compile time and branch-free; lane 0's inputs (the previous strip's last row and
// t) come from one LDS read per chunk and readlane per step; lane 63's values for the next strip are
// staged with v_writelane (inline-constant lane) and written once per chunk.  A cell's value is
// max(diag, up, left) whatever the tie order (aligners.py:40-48 keeps the maximum), and the int32
// store wraps like the reference's table.
template <typename Acc, bool BANDED>
__global__ __launch_bounds__(64) void dp_fast_kernel(
    const uint8_t* __restrict__ codes, const int64_t* __restrict__ off, const int32_t* __restrict__ len,
    int32_t n_reads, const int32_t* __restrict__ a_idx, const int32_t* __restrict__ b_idx,
    int64_t n_pairs, int32_t mcap, int64_t match, int64_t mismatch, int64_t indel, int32_t band,
    int32_t* __restrict__ out_score, int32_t* __restrict__ out_end, const int32_t* __restrict__ seed,
    uint32_t* __restrict__ err_flag) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // rows hold columns 0 .. 64*nch + 64 (hand-off chunks of 64 columns); t codes padded likewise
    const int32_t pitch = ((mcap + 126) / 64) * 64 + 64;
    int32_t* row0 = reinterpret_cast<int32_t*>(smem);
    int32_t* row1 = row0 + pitch;
    uint8_t* tcodes = reinterpret_cast<uint8_t*>(row1 + pitch);
    const int lane = threadIdx.x;
    for (int64_t pair = blockIdx.x; pair < n_pairs; pair += gridDim.x) {
        const int32_t a = a_idx[pair];
        const int32_t b = b_idx[pair];
        if (a < 0 || a >= n_reads || b < 0 || b >= n_reads || len[b] > mcap) {
            if (lane == 0) {
                ovl_flag_error(err_flag);
                out_score[pair] = -1;
                out_end[pair] = -1;
            }
            continue;
        }
        const int32_t n = len[a];
        const int32_t m = len[b];
        const uint8_t* s = codes + off[a];
        const uint8_t* t = codes + off[b];
        const int32_t nch = (m + 126) / 64;  // chunks covering tau = 0 .. m + 62
        // band: seed diagonal d* (seed holds the ungapped seed end j*) and the first row with
        // a band cell of column >= 1; the band of row i is columns [i - d* - W, i - d* + W]
        const int32_t W = BANDED ? band : 0;
        const int32_t dstar = BANDED ? n - seed[pair] : 0;
        const int32_t rlo = BANDED ? (dstar - W + 1 > 1 ? dstar - W + 1 : 1) : 1;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // previous pair's LDS readers are done
        for (int j = lane; j < pitch; j += 64) row0[j] = 0;
        for (int j = lane; j < 64 * nch; j += 64) tcodes[j] = j < m ? t[j] : 0;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        int32_t* rin = row0;
        int32_t* rout = row1;
        // tracked by the lane that owns row n; dp[n][0] = 0 is the j = 0 candidate when in the band
        int32_t best = (!BANDED || n - dstar - W <= 0) ? 0 : INT32_MIN, bend = 0;
        const int nstrips = (n + 63) >> 6;
        const int st0 = BANDED ? (rlo - 1) >> 6 : 0;
        for (int st = st0; st < nstrips; ++st) {
            const int32_t i = 64 * st + 1 + lane;
            const bool last_row = i == n;
            // rows past n (last strip only) compute unread values: no row mask is needed
            const uint32_t sc = i <= n ? (uint32_t)s[i - 1] : 0xFFFFFFFFu;
            const bool last = st + 1 == nstrips;  // last strip: track row n; else carry the last row
            const int32_t jlo = i - dstar - W, jhi = i - dstar + W;  // this lane's band (BANDED)
            // chunks whose steps meet the band (all chunks when not banded)
            int32_t c_lo = 0, c_hi = nch - 1;
            if constexpr (BANDED) {
                const int lmax = (n - 64 * st - 1) < 63 ? (n - 64 * st - 1) : 63;
                const int32_t tlo = 64 * st - dstar - W;                 // lane 0's first band step
                const int32_t thi = 64 * st + 2 * lmax - dstar + W;      // last lane's last band step
                c_lo = tlo > 0 ? tlo / 64 : 0;
                c_hi = thi / 64 < nch - 1 ? thi / 64 : nch - 1;
                if (c_hi < c_lo) c_hi = c_lo;
            }
            // state entering chunk c_lo: lane L used t[64 c_lo - 1 - L] at the step before, lane 0's
            // diagonal is dp[64 st][64 c_lo]; other lanes' carried values only meet masked cells
            int32_t cur = 0, uprev = 0, tch = 0;
            if (BANDED && c_lo > 0) {
                const int32_t tp = 64 * c_lo - 1 - lane;
                tch = tp >= 0 && tp < m ? (int32_t)tcodes[tp] : 0;
                uprev = lane == 0 ? rin[64 * c_lo] : 0;
            }
            int32_t out_a = 0, out_b = 0;
            // one chunk of 64 steps; EDGE: chunk 0 (lanes still left of column 1 keep dp[i][0] = 0);
            // LAST: best tracking of row n instead of the carry staging.
            auto chunk = [&](int32_t c, auto edge_tag, auto last_tag) {
                constexpr bool EDGE = decltype(edge_tag)::value;
                constexpr bool LAST = decltype(last_tag)::value;
                int32_t v_rin = rin[64 * c + 1 + lane];        // lane u: dp[64 st][64c+1+u]
                int32_t v_t = (int32_t)tcodes[64 * c + lane];  // lane u: t[64c+u]
                // the column as a running register: per-step lane masks built from constants would be
                // hoisted as 64 loop invariants (SGPR pairs spilled to VGPR lanes)
                int32_t jv = 64 * c - lane + 1;
                unroll<0, 64>([&](auto uc) {
                    constexpr int u = decltype(uc)::value;
                    const int32_t j = jv;
                    // lane 0 takes its inputs from the chunk registers' lane 0, then they rotate down
                    const int32_t upin = __builtin_amdgcn_update_dpp(v_rin, cur, 0x138, 0xF, 0xF, false);
                    const int32_t tin = __builtin_amdgcn_update_dpp(v_t, tch, 0x138, 0xF, 0xF, false);
                    v_rin = __builtin_amdgcn_mov_dpp(v_rin, 0x130, 0xF, 0xF, true);  // wave_shl:1, lane 63 <- 0
                    v_t = __builtin_amdgcn_mov_dpp(v_t, 0x130, 0xF, 0xF, true);
                    const Acc diag = (Acc)uprev + ((uint32_t)tin == sc ? (Acc)match : (Acc)mismatch);
                    Acc up = (Acc)upin + (Acc)indel;
                    Acc left = (Acc)cur + (Acc)indel;
                    if constexpr (BANDED) {
                        // out-of-band predecessors: "up" leaves the band only at the row's last band
                        // cell, "left" only at its first; diag is always in the band, so substituting
                        // it leaves the maximum exact
                        up = j != jhi ? up : diag;
                        left = j != jlo ? left : diag;
                    }
                    const Acc mx = diag > up ? diag : up;
                    const int32_t nv = (int32_t)(mx > left ? mx : left);
                    if constexpr (EDGE) cur = j >= 1 ? nv : cur;
                    else cur = nv;
                    if constexpr (LAST) {
                        bool better = last_row && j >= 1 && j <= m && nv > best;
                        if constexpr (BANDED) better = better && j >= jlo && j <= jhi;
                        best = better ? nv : best;
                        bend = better ? j : bend;
                    } else {
                        const int32_t v63 = __builtin_amdgcn_readlane(cur, 63);
                        if constexpr (u <= 62) out_a = writelane<u + 1>(out_a, v63);
                        else out_b = writelane<0>(out_b, v63);
                    }
                    uprev = upin;
                    tch = tin;
                    jv += 1;
                    asm volatile("" : "+v"(jv), "+v"(v_rin), "+v"(v_t));
                });
                if constexpr (!LAST) {
                    if (c >= 1) rout[64 * (c - 1) + 1 + lane] = out_a;  // columns 64(c-1)+1 .. 64c
                    out_a = out_b;
                }
            };
            using T_ = std::true_type;
            using F_ = std::false_type;
            if (last) {
                if (c_lo == 0) chunk(0, T_{}, T_{});
                for (int32_t c = c_lo > 1 ? c_lo : 1; c <= c_hi; ++c) chunk(c, F_{}, T_{});
            } else {
                if (c_lo == 0) chunk(0, T_{}, F_{});
                for (int32_t c = c_lo > 1 ? c_lo : 1; c <= c_hi; ++c) chunk(c, F_{}, F_{});
                rout[64 * c_hi + 1 + lane] = out_a;  // the last processed hand-off chunk's first column
                if (lane == 0) rout[0] = 0;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            int32_t* tmp = rin; rin = rout; rout = tmp;
        }
        // row n lives in lane (n-1) % 64 of the last strip
        const int owner = (n - 1) & 63;
        const int32_t bs = __shfl(best, owner, 64);
        const int32_t be = __shfl(bend, owner, 64);
        if (lane == 0) {
            out_score[pair] = n > 0 && m > 0 ? bs : 0;
            out_end[pair] = n > 0 && m > 0 ? be : 0;
        }
    }
}

}  // namespace ovl

// ----------------------------------------------------------------------------- launchers

using namespace ovl;

template <typename Acc, bool BANDED>
static void launch_dp_t(const OvlDpArgs* g, unsigned blocks, size_t lds, hipStream_t stream) {
    dp_kernel<Acc, BANDED><<<blocks, 64, lds, stream>>>(g->codes, g->off, g->len, g->n_reads, g->a_idx, g->b_idx,
                                                         g->n_pairs, g->mcap, g->match, g->mismatch, g->indel,
                                                         g->band, g->out_score, g->out_end, g->seed, g->tb, g->err_flag);
}

extern "C" hipError_t ovl_launch_dp(const OvlDpArgs* g, hipStream_t stream) {
    if (g->n_pairs <= 0) return hipSuccess;
    int64_t blocks = g->n_pairs;
    if (blocks > 16384) blocks = 16384;
    const size_t lds = (size_t)2 * (g->mcap + 1) * sizeof(int32_t) + (size_t)g->mcap + 16;
    const unsigned nb = (unsigned)blocks;
    if (g->band >= 0) {
        // banded mode runs only where values fit int32 (the host checks) and never writes tb
        if (g->wide || g->tb) return hipErrorInvalidValue;
        switch (g->band_form) {
            case OVL_BAND_FORM_DIAG:
                return launch_band_diag(g, stream);
            case OVL_BAND_FORM_ROWS:
                return launch_band_rows(g, stream);
            case OVL_BAND_FORM_FAST: {
                const int32_t pitch = ((g->mcap + 126) / 64) * 64 + 64;
                const size_t lds2 = (size_t)2 * pitch * sizeof(int32_t) + (size_t)pitch;
                dp_fast_kernel<int32_t, true><<<nb, 64, lds2, stream>>>(
                    g->codes, g->off, g->len, g->n_reads, g->a_idx, g->b_idx, g->n_pairs, g->mcap, g->match,
                    g->mismatch, g->indel, g->band, g->out_score, g->out_end, g->seed, g->err_flag);
                return hipGetLastError();
            }
            default:
                break;
        }
        launch_dp_t<int32_t, true>(g, nb, lds, stream);
    } else if (!g->tb && !g->classic) {
        // scores only: the chunked kernel (LDS: two padded rows + padded t)
        const int32_t pitch = ((g->mcap + 126) / 64) * 64 + 64;
        const size_t lds2 = (size_t)2 * pitch * sizeof(int32_t) + (size_t)pitch;
        if (g->wide)
            dp_fast_kernel<int64_t, false><<<nb, 64, lds2, stream>>>(
                g->codes, g->off, g->len, g->n_reads, g->a_idx, g->b_idx, g->n_pairs, g->mcap, g->match,
                g->mismatch, g->indel, -1, g->out_score, g->out_end, g->seed, g->err_flag);
        else
            dp_fast_kernel<int32_t, false><<<nb, 64, lds2, stream>>>(
                g->codes, g->off, g->len, g->n_reads, g->a_idx, g->b_idx, g->n_pairs, g->mcap, g->match,
                g->mismatch, g->indel, -1, g->out_score, g->out_end, g->seed, g->err_flag);
    } else if (g->wide) {
        launch_dp_t<int64_t, false>(g, nb, lds, stream);
    } else {
        launch_dp_t<int32_t, false>(g, nb, lds, stream);
    }
    return hipGetLastError();
}
