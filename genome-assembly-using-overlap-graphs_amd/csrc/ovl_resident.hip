// ovl_resident.hip — the resident scoring grid (gfx950): uniform_kernel's throughput-mode sweep (ovl_sweep.h) as a
// kernel that stays on the GPU and serves requests from a host mailbox, its results going out as ring records.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ovl_kernels.h"
#include "ovl_grid.h"
#include "ovl_sweep.h"
#include "ovl_wave.h"

namespace ovl {

using ovl_wave::vm_drain;

// One tile's results as a ring record (ovl_grid.h OvlResidentBody), which host threads read while the grid runs
// (ovl_expand.h rec_tile_ready_scalar / rec_tile_scalar_t / rec_tile_avx512_t):
//   dword w (w < 32) = phase << 31 | c[w + 32] << 15 | c[w]   (c[l]: lane l's 15-bit code)
// The phase bit (the ring lap's) tells the host which dwords this request has written: every dword is one aligned
// 32-bit store, so a dword whose phase bit is the lap's holds this request's payload, and a record is complete
// when all 32 are.  Code c of a pair with end j <= n (read a's length; L = j compared bases, aligners.py:27-48
// with gaps that cannot win, so score = match*j + (mismatch - match)*X) is j(j + 1)/2 + X, X <= j <= 254
// (< 0x7FFF).  Every other pair has c = 0x7FFF and a special word, stored as one 8-byte {payload, seq}:
//   1 << 31 | j << 16 | X << 8 | n   a shorter read a inside b's window (j > n: L = n, score = match*n +
//                                    (mismatch - match)*X);
//   0xFFFFFFFF                       a bad pair (-1, -1).
// 2 link bytes per pair (+ 8 per special).  Every lane of the wavefront calls it (the cross-half exchange); lanes
// with !mine code 0, which the host never reads.  The
// stores are non-temporal 128-byte lines into fine-grained host memory, which the XCD's L2 keeps (write-back) until
// the wavefront's release fence after its last tile of the request (resident_kernel): a resident grid never reaches
// the end-of-kernel write-back.  (Measured against the alternatives, target point, N = 8 / N = 1 shards: write-through
// 16-byte sc1 stores 0.056 / 0.326 ms, 8-byte system-scope stores 0.071 / 0.344, non-temporal stores into uncached
// (MTYPE_UC) memory 0.062 / 0.340, this form 0.049 / 0.223; profiles/r06_resident_store_ab.json.)
__device__ __forceinline__ void put_ring_rec(uint32_t* rec, uint64_t* sp, int64_t ri, uint32_t phase, uint32_t seq,
                                             bool mine, int32_t sc, int32_t en, int32_t n, int32_t match, float inv,
                                             int lane) {
    uint32_t c = 0;
    if (mine) {
        uint32_t special = 0;
        if (en < 0) {
            special = 0xFFFFFFFFu;
        } else if (en > n) {
            const uint32_t x = (uint32_t)__builtin_rintf((float)(match * n - sc) * inv);
            special = 0x80000000u | (uint32_t)en << 16 | x << 8 | (uint32_t)n;
        } else {
            const uint32_t x = (uint32_t)__builtin_rintf((float)(match * en - sc) * inv);
            c = ((uint32_t)en * (uint32_t)(en + 1) >> 1) + x;
        }
        if (special) {
            c = 0x7FFFu;
            __builtin_nontemporal_store((uint64_t)seq << 32 | special, sp + 64 * ri + lane);
        }
    }
    const uint32_t hi = (uint32_t)__shfl_xor((int)c, 32, 64);
    if (lane < 32) __builtin_nontemporal_store(phase << 31 | hi << 15 | c, rec + 32 * ri + lane);
}

// One 64-pair tile of a resident request: uniform_kernel's throughput-mode sweep with every pair in it (TT: reads
// b cut at the genome end snapshot their block maxima, shorter reads a add their window keys), into the ring.
// Split in stages so a wavefront can have the next tiles' loads in flight during a sweep (resident_kernel):
// the indices (ResIdx), then the rows and lengths they select (ResRows), then the sweep (resident_sweep).
struct ResIdx {
    int32_t a, b;
    bool mine, ok;
};
template <int W>
struct ResRows {
    uint32_t Sw[(W * 2 + 3) & ~3], Tw[(W * 2 + 3) & ~3];
    uint32_t fw;  // read a's word of the length bitmap
    int32_t la, lb;
};

__device__ __forceinline__ ResIdx resident_idx(int64_t tile, const OvlResidentBody& q, int32_t n_reads, int lane) {
    ResIdx x;
    const int64_t p = tile * 64 + lane;
    x.mine = tile >= 0 && p < q.n_pairs;
    x.a = x.mine ? q.a_idx[p] : 0;
    x.b = x.mine ? q.b_idx[p] : 0;
    x.ok = x.mine && x.a >= 0 && x.a < n_reads && x.b >= 0 && x.b < n_reads;
    if (!x.ok) {
        x.a = 0;
        x.b = 0;
    }
    return x;
}

template <int W>
__device__ __forceinline__ void resident_rows(const ResIdx& x, ResRows<W>& r, const uint32_t* __restrict__ sfx,
                                              const uint32_t* __restrict__ pfx, const int32_t* __restrict__ len,
                                              const uint32_t* __restrict__ full) {
    constexpr int SROW = (W * 2 + 3) & ~3;
    load_words<SROW>(sfx + (int64_t)x.a * SROW, r.Sw);
    load_words<SROW>(pfx + (int64_t)x.b * SROW, r.Tw);
    r.fw = full[x.a >> 5];
    r.la = len[x.a];
    r.lb = len[x.b];
}

template <int W>
__device__ __forceinline__ void resident_sweep(int64_t tile, const ResIdx& x, const ResRows<W>& r,
                                               const OvlResidentBody& q, int32_t lw, int32_t match, int32_t mismatch,
                                               int lane) {
    const bool ok = x.ok;
    const bool fa = ok && ((r.fw >> (x.a & 31)) & 1u);
    const int32_t mb = r.lb;
    int32_t na = lw;
    if (ok && !fa) na = r.la;
    const bool uni = fa && mb == lw;
    const bool tt = ok && !uni;
    const int32_t tm = tt ? (na < mb ? na : mb) : -1;
    uint32_t tmask = 0;
    for (uint64_t bm = __ballot(tt); bm; bm &= bm - 1)
        tmask |= 1u << (__builtin_amdgcn_readlane(tm, (int)__builtin_ctzll(bm)) & 31);
    int32_t best = sweep_uniform<W, 0>(r.Sw, r.Tw, lw, match, mismatch - match, 0u, 32u, tmask, tm);
    const bool win = tt && na < mb;
    uint64_t wm = __ballot(win);
    if (wm) {
        int32_t jlo = 1 << 30, jhi = 0;
        for (; wm; wm &= wm - 1) {
            const int l = (int)__builtin_ctzll(wm);
            jlo = min(jlo, __builtin_amdgcn_readlane(na, l) + 1);
            jhi = max(jhi, __builtin_amdgcn_readlane(mb, l));
        }
        const int32_t wk = window_keys<W>(r.Sw, r.Tw, na, mb, jlo, jhi, match, mismatch - match);
        if (win && wk > best) best = wk;
    }
    int32_t sc, en;
    Key<0>::decode(best, sc, en);
    const int64_t g = q.pos + tile;
    const int64_t ri = g & ((int64_t(1) << q.ring_log2) - 1);
    const uint32_t phase = (uint32_t)((g >> q.ring_log2) + 1) & 1u;
    put_ring_rec(q.rec, q.sp, ri, phase, (uint32_t)q.seq, x.mine, ok ? sc : -1, ok ? en : -1, na, match,
                 pack_inv(match, mismatch), lane);
}

// The resident scoring grid: launched once, it serves requests posted by the host in pinned memory until the host
// asks it to leave or none comes for idle_ticks (the host relaunches it on its next request), so a call pays
// neither a launch nor a completion signal -- the results' ring records tell the host when it is done.
//   Block 0's thread 0 polls the host mailbox (a relaxed system-scope load per poll, s_sleep between), reads the
// request body, writes a device copy of it under a seqlock (8-byte agent-scope atomics, each group drained) and
// forwards the sequence number through one device word; the other blocks' thread 0 polls that word and reads the
// copy (the hand-off of MI355X_MICROARCH.md's first valid row: sc1 stores drained, one flag, sc1 loads).  Each
// block then scores tiles: wavefront w of the grid takes items w, w + waves, ... (heavy tiles first, as
// uniform_kernel orders them).  No fan-in across blocks: nothing is waited for on the device.  The records are
// non-temporal stores into fine-grained host memory, which stay in the XCD's L2 until written back: a release
// fence after a block's last tile (body.fence 2: the block's last wavefront, counted in LDS after each wavefront's
// stores drained; 1: every wavefront) -- each fence writes back the whole L2, and 2,048 of them per request queue
// behind each other (MI355X_MICROARCH.md: the write-back costs a few microseconds).
//   Every wait is bounded: block 0 leaves (and tells the others) after idle_ticks without a request; the other
// blocks leave after twice that without a new forward, so a grid whose block 0 never ran still ends.
// PF: tiles software-pipelined (fewer, fatter wavefronts: 2-4 per SIMD) or one tile at a time (UNI_OCC(W, 0)
// wavefronts per SIMD, uniform_kernel's register budget)
#define RES_OCC(W, PF) ((PF) ? ((W) >= 3 ? 2 : 4) : UNI_OCC(W, 0))
template <int W, bool PF>
__global__ __launch_bounds__(256, RES_OCC(W, PF)) void resident_kernel(
    const uint32_t* __restrict__ sfx, const uint32_t* __restrict__ pfx, const int32_t* __restrict__ len,
    int32_t n_reads, int32_t lw, const uint32_t* __restrict__ full, const uint8_t* __restrict__ tile_flags,
    const OvlResidentCtl* mailbox, uint32_t* fwd, OvlResidentBody* dslot, uint32_t seq_base, uint64_t idle_ticks,
    uint64_t* status, uint32_t poll_sleep, uint64_t* tbuf) {
    __shared__ uint64_t s_body[kResidentBodyWords];
    __shared__ int s_go;
    __shared__ int s_done;  // (fence 2: wavefronts of this block done with the request)
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    uint32_t last = seq_base;  // (thread 0)
    for (;;) {
        if (threadIdx.x == 0) {
            int go = 0;
            uint64_t v[kResidentBodyWords];
            if (blockIdx.x == 0) {
                const uint64_t t_end = wall_clock64() + idle_ticks;
                uint32_t seq = 0;
                for (;;) {
                    const uint64_t c = __hip_atomic_load(&mailbox->ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    if (c >> 32) break;  // asked to leave
                    if ((uint32_t)c != last) {
                        seq = (uint32_t)c;
                        go = 1;
                        break;
                    }
                    if (wall_clock64() > t_end) break;
                    __builtin_amdgcn_s_sleep(2);
                }
                int why = go ? 0 : 2;  // (status: 1 asked to leave, 2 idle, 3 a body that is not the request's)
                if (!go && wall_clock64() <= t_end) why = 1;
                if (go) {
                    vm_drain();
                    const uint64_t* src = reinterpret_cast<const uint64_t*>(&mailbox->body[seq & 1]);
#pragma unroll
                    for (int k = 0; k < kResidentBodyWords; ++k)
                        v[k] = __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    go = (uint32_t)v[0] == seq;  // (the host writes the body before ctl: always)
                    if (!go) why = 3;
                }
                if (!go && status) {  // why block 0 left, for the host's trace (pinned, written only here)
                    __hip_atomic_store(status + 1, (uint64_t)last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(status + 2, (uint64_t)seq | (v[0] << 32), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(status + 3, idle_ticks, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    vm_drain();
                    __hip_atomic_store(status, (uint64_t)why, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
                if (go) {
                    uint64_t* ds = reinterpret_cast<uint64_t*>(&dslot[seq & 3]);
                    __hip_atomic_store(ds, (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    vm_drain();
#pragma unroll
                    for (int k = 1; k < kResidentBodyWords; ++k)
                        __hip_atomic_store(ds + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    vm_drain();
                    __hip_atomic_store(ds, (uint64_t)seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    vm_drain();
                    __hip_atomic_store(fwd, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    last = seq;
                    if (tbuf) __builtin_nontemporal_store(wall_clock64(), tbuf + 4 * (int64_t)gridDim.x * 4);
                } else {
                    __hip_atomic_store(fwd, kResidentLeave, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            } else {
                const uint64_t t_end = wall_clock64() + 2 * idle_ticks;
                for (;;) {
                    const uint32_t f = __hip_atomic_load(fwd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (f == kResidentLeave) break;
                    if (f != 0u && f != last) {
                        vm_drain();
                        const uint64_t* ds = reinterpret_cast<const uint64_t*>(&dslot[f & 3]);
                        const uint64_t s1 = __hip_atomic_load(ds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        vm_drain();
#pragma unroll
                        for (int k = 1; k < kResidentBodyWords; ++k)
                            v[k] = __hip_atomic_load(ds + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        vm_drain();
                        const uint64_t s2 = __hip_atomic_load(ds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (s1 == (uint64_t)f && s2 == (uint64_t)f) {  // (else rewritten meanwhile: poll again)
                            v[0] = s1;
                            last = f;
                            go = 1;
                            break;
                        }
                    }
                    if (wall_clock64() > t_end) break;
                    for (uint32_t z = 0; z < poll_sleep; ++z) __builtin_amdgcn_s_sleep(4);  // (~0.1 us each)
                }
                if (!go && status)  // (a block that left on its own deadline, not told to)
                    if (__hip_atomic_load(fwd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kResidentLeave)
                        __hip_atomic_store(status + 4, (uint64_t)blockIdx.x + 1, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_SYSTEM);
            }
            if (go) {
#pragma unroll
                for (int k = 0; k < kResidentBodyWords; ++k) s_body[k] = v[k];
            }
            s_go = go;
            s_done = 0;
        }
        __syncthreads();
        if (!s_go) return;
        // (trace, OVL_TRACE_PIPE: per wavefront the wall clock when it knew the request, finished its last tile
        // and had its records written back; block 0 stored when it saw the request)
        if (tbuf && lane == 0) __builtin_nontemporal_store(wall_clock64(), tbuf + 4 * wave);
        OvlResidentBody q;  // (wave-uniform: scalar registers, as kernel arguments would be)
        {
            uint64_t* d = reinterpret_cast<uint64_t*>(&q);
#pragma unroll
            for (int k = 0; k < kResidentBodyWords; ++k) {
                const uint64_t x = s_body[k];
                const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x);
                const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
                d[k] = (uint64_t)hi << 32 | lo;
            }
        }
        const int32_t match = (int32_t)(uint32_t)q.scoring, mismatch = (int32_t)(uint32_t)(q.scoring >> 32);
        const int64_t n_tiles = (q.n_pairs + 63) >> 6;
        const bool hf = q.heavy_ids != nullptr && q.heavy_n > 0;
        const int64_t n_items = hf ? n_tiles + q.heavy_n : n_tiles;
        // The wave's items w, w + waves, ... (heavy tiles first, as uniform_kernel orders them; an item whose tile
        // was done among the heavy ones is skipped): item -> tile, or -1 past the last.  Software-pipelined: while
        // tile i sweeps, the rows of tile i + 1 and the indices of tile i + 2 are in flight (a resident grid runs
        // a few wavefronts per SIMD, too few to hide a tile's two dependent loads by switching waves).
        if constexpr (!PF) {
            for (int64_t item = wave; item < n_items; item += n_waves) {  // (wave-uniform)
                int64_t tile = item;
                if (hf) {
                    if (item < q.heavy_n) {
                        tile = (int64_t)q.heavy_ids[item] - q.tile_base;
                    } else {
                        tile = item - q.heavy_n;
                        if (tile_flags[q.tile_base + tile]) continue;  // done among the heavy ones
                    }
                }
                const ResIdx x = resident_idx(tile, q, n_reads, lane);
                ResRows<W> r;
                resident_rows<W>(x, r, sfx, pfx, len, full);
                resident_sweep<W>(tile, x, r, q, lw, match, mismatch, lane);
            }
        }
        int64_t item = PF ? wave : n_items;
        const auto next_tile = [&]() -> int64_t {  // (wave-uniform; leaves `item` on the tile's item)
            for (; item < n_items; item += n_waves) {
                if (!hf) return item;
                if (item < q.heavy_n) return (int64_t)q.heavy_ids[item] - q.tile_base;
                const int64_t t = item - q.heavy_n;
                if (!tile_flags[q.tile_base + t]) return t;
            }
            return -1;
        };
        int64_t t0 = next_tile();
        ResIdx x0 = resident_idx(t0, q, n_reads, lane);
        ResRows<W> r0;
        if (t0 >= 0) resident_rows<W>(x0, r0, sfx, pfx, len, full);
        item += n_waves;
        int64_t t1 = t0 >= 0 ? next_tile() : -1;
        ResIdx x1 = resident_idx(t1, q, n_reads, lane);
        while (t0 >= 0) {
            ResRows<W> r1;
            if (t1 >= 0) resident_rows<W>(x1, r1, sfx, pfx, len, full);
            item += n_waves;
            const int64_t t2 = t1 >= 0 ? next_tile() : -1;
            const ResIdx x2 = resident_idx(t2, q, n_reads, lane);
            resident_sweep<W>(t0, x0, r0, q, lw, match, mismatch, lane);
            t0 = t1;
            x0 = x1;
            r0 = r1;
            t1 = t2;
            x1 = x2;
        }
        // this wavefront's records out of the XCD's L2 (system-scope release: an L2 write-back)
        if (tbuf && lane == 0) __builtin_nontemporal_store(wall_clock64(), tbuf + 4 * wave + 1);
        if (q.fence == 1) {
            if (wave < n_items) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        } else if (q.fence == 2 && (int64_t)blockIdx.x * 4 < n_items) {
            vm_drain();  // (this wavefront's records are in the L2: the fence of the block's last one covers them)
            int k = 0;
            if (lane == 0) k = atomicAdd(&s_done, 1);
            k = __builtin_amdgcn_readfirstlane(k);
            if (k == 3) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        }
        if (tbuf && lane == 0) {
            __hip_atomic_store(tbuf + 4 * wave + 2, (uint64_t)wall_clock64(), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(tbuf + 4 * wave + 3, q.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __syncthreads();  // (thread 0 rewrites s_body for the next request)
    }
}

extern "C" hipError_t ovl_launch_resident(const OvlResidentArgs* g, hipStream_t stream) {
    if (g->lw <= 0 || g->lw > 254 || g->blocks <= 0 || !g->mailbox || !g->fwd || !g->dslot) return hipErrorInvalidValue;
    const dim3 grid((unsigned)g->blocks), block(256);
#define OVL_RESIDENT_CASE(Wc)                                                                                       \
    case Wc:                                                                                                        \
        if (g->pipelined)                                                                                           \
            resident_kernel<Wc, true><<<grid, block, 0, stream>>>(g->sfx, g->pfx, g->len, g->n_reads, g->lw,        \
                                                                  g->full, g->tile_flags, g->mailbox, g->fwd,       \
                                                                  g->dslot, g->seq_base, g->idle_ticks, g->status,  \
                                                                  g->poll_sleep, g->tbuf);                          \
        else                                                                                                        \
            resident_kernel<Wc, false><<<grid, block, 0, stream>>>(g->sfx, g->pfx, g->len, g->n_reads, g->lw,       \
                                                                   g->full, g->tile_flags, g->mailbox, g->fwd,      \
                                                                   g->dslot, g->seq_base, g->idle_ticks, g->status, \
                                                                   g->poll_sleep, g->tbuf);                         \
        break;
    switch (g->wmax) {
        OVL_RESIDENT_CASE(1)
        OVL_RESIDENT_CASE(2)
        OVL_RESIDENT_CASE(3)
        OVL_RESIDENT_CASE(4)
        OVL_RESIDENT_CASE(5)
        OVL_RESIDENT_CASE(6)
        OVL_RESIDENT_CASE(7)
        OVL_RESIDENT_CASE(8)
        default: return hipErrorInvalidValue;
    }
#undef OVL_RESIDENT_CASE
    return hipGetLastError();
}

}  // namespace ovl
