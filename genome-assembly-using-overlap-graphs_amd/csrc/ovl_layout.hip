// Best-successor layout (ovl_layout, ovl_layout_candidates; ovl_layout_api.cpp): contigs straight from the score
// columns, without a graph object.
//
//   Inputs: n reads with lengths len[r]; E pairs (a[p], b[p], score[p], end[p]) in list order; min_score and
//   min_overlap.
//   1. Eligible.  Pair p is eligible iff a[p] != b[p], score[p] >= min_score and min_overlap <= end[p] < len[b[p]].
//      A link that adds no base is no link.
//   2. Link.  link[a] is the eligible pair of a with the greatest score; ties go to the smallest p.
//      succ[a] = b[link[a]].  A read without an eligible pair has link = succ = -1.
//   3. Cycles.  succ is a functional graph.  Every cycle is cut at its pair with the least score; ties go to the
//      greatest p.  The source of that pair gets link = succ = -1.  What remains is a forest of in-trees, each with
//      one root (succ = -1).
//   4. Span.  tail[root] = 0; otherwise tail[a] = tail[succ[a]] + len[succ[a]] - end[link[a]].
//      span[a] = len[a] + tail[a] is the length of the contig spelled from a.
//   5. Contigs.  One contig per root, in ascending root index.  Its head is the read of the tree with the greatest
//      span; ties go to the smallest read index.  The contig is the head followed, along succ, by
//      read[succ][end[link]:] (the reference's own concatenation, create_contig).  Its length is span[head].
//   6. Placement.  Every read r gets contig[r], its tree's contig; offset[r] = span[head] - span[r], which for a read
//      on the head's path is where its first base lies; and on_path[r].
//   Everything is integer and independent of pair order, except the tie rules, which name p.
//
// layout_link_kernel, the sweep over the pairs: one lane per pair builds the key of ovl_layout.h (0 for a pair that
// is not eligible) and the wavefront reduces runs of equal a by a segmented maximum over shuffles -- lane L takes
// lane L - d's key while that lane holds the same a -- so that the last lane of a run issues the run's one 64-bit
// atomicMax into best[a].  Both candidate rules emit a read's pairs one after the other, so a wavefront over such a
// list issues one or two atomics where the plain form issues up to 64 on one address; a list in any other order
// only issues more of them (lanes that hold the same a apart from each other may also merge: a maximum does not
// mind).  The plain form (runs = 0) is kept for the measurement.
//
// The forest kernels are one thread per read.  Table k of `jump` holds the read 2^k links on, a root standing for
// itself, so that roots are fixed points and every table is total; mk and tail carry the minimum key and the sum of
// the links' new bases over the same 2^k links (a root adds the identity).  After `levels` doublings, 2^levels >= n:
// jump[levels][r] is r's root or, when it still has a successor, a node on a cycle; every node of a cycle is such a
// node for the read 2^levels links behind it on the same cycle, and mk[levels] of a cycle node is the minimum around
// its whole cycle.  Keys are unique per pair, so exactly one node per cycle finds its own key there and is cut.
// The head per root is a 64-bit atomicMax of span << 32 | ~r, reduced per root inside the wavefront first (the
// reads of one tree are not neighbours, so the wavefront takes its distinct roots one by one).  The path of every
// head is marked from the highest level down: a marked read marks the read 2^k links on, for k = levels - 1 .. 0,
// which reaches every distance below 2^levels; marks written during a level may or may not be seen by it, and both
// are right, since a marked read's jump is on the path too.
//
// layout_spell_kernel: a wavefront per on-path read copies the bases its successor adds, read[succ][end[link]:], to
// c_off[contig] + offset[succ] + end[link]; the head's wavefront copies the head itself first.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>

#include "ovl_layout.h"

namespace ovl_layout {

typedef unsigned long long u64;

constexpr int kThreads = 256;

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const u64 o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

template <bool RUNS>
__global__ __launch_bounds__(kThreads) void layout_link_kernel(OvlLayoutArgs g) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    // p0 is the same for the 64 lanes of a wavefront, so they take every trip (and every shuffle) together
    for (int64_t p0 = (int64_t)blockIdx.x * kThreads + (threadIdx.x & ~63); p0 < g.n_pairs; p0 += stride) {
        const int64_t p = p0 + lane;
        int32_t a = -1;
        u64 key = 0;
        if (p < g.n_pairs) {
            const int32_t pa = g.a[p], pb = g.b[p], sc = g.score[p], en = g.end[p];
            if ((uint32_t)pa < (uint32_t)g.n && (uint32_t)pb < (uint32_t)g.n) {
                a = pa;
                if (pa != pb && sc >= g.min_score && en >= g.min_overlap && en < g.len[pb])
                    key = ovl_layout_key(sc, (uint32_t)p);
            }
        }
        if (RUNS) {
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int32_t oa = __shfl_up(a, d, 64);
                const u64 ok = __shfl_up(key, d, 64);
                if (lane >= d && oa == a && ok > key) key = ok;
            }
            const int32_t next = __shfl_down(a, 1, 64);
            if ((lane == 63 || next != a) && key != 0) atomicMax(g.best + a, key);
        } else if (key != 0) {
            atomicMax(g.best + a, key);
        }
    }
}

__global__ __launch_bounds__(kThreads) void layout_init_kernel(OvlLayoutArgs g, int32_t resolve) {
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < g.n; r += (int64_t)gridDim.x * kThreads) {
        int32_t link, succ;
        if (resolve) {
            const u64 k = g.best[r];
            link = k != 0 ? ovl_layout_key_pair(k) : -1;
            succ = link >= 0 ? g.b[link] : -1;
            g.link[r] = link;
            g.succ[r] = succ;
        } else {
            link = g.link[r];
            succ = g.succ[r];
        }
        g.jump[r] = succ >= 0 ? succ : (int32_t)r;
        g.mk[0][r] = link >= 0 ? ovl_layout_key(g.score[link], (uint32_t)link) : kLayoutNoKey;
        g.tail[0][r] = succ >= 0 ? (uint32_t)(g.len[succ] - g.end[link]) : 0u;
        g.on_cycle[r] = 0;
    }
}

// table k -> table k + 1 (the sums wrap while a cycle stands; they are read only from a forest)
__global__ __launch_bounds__(kThreads) void layout_level_kernel(OvlLayoutArgs g, int32_t k) {
    const int32_t* from = g.jump + (int64_t)k * g.n;
    int32_t* to = g.jump + (int64_t)(k + 1) * g.n;
    const u64* mk = g.mk[k & 1];
    const uint32_t* tl = g.tail[k & 1];
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < g.n; r += (int64_t)gridDim.x * kThreads) {
        const int32_t j = from[r];
        to[r] = from[j];
        const u64 m0 = mk[r], m1 = mk[j];
        g.mk[(k + 1) & 1][r] = m1 < m0 ? m1 : m0;
        g.tail[(k + 1) & 1][r] = tl[r] + tl[j];
    }
}

__global__ __launch_bounds__(kThreads) void layout_cycle_mark_kernel(OvlLayoutArgs g) {
    const int32_t* top = g.jump + (int64_t)g.levels * g.n;
    for (int64_t r0 = (int64_t)blockIdx.x * kThreads; r0 < g.n; r0 += (int64_t)gridDim.x * kThreads) {
        const int64_t r = r0 + threadIdx.x;
        bool hit = false;
        if (r < g.n) {
            const int32_t x = top[r];
            hit = g.succ[x] >= 0;  // 2^levels >= n links on and still not at a root: x is on a cycle
            if (hit) g.on_cycle[x] = 1;
        }
        const u64 m = __ballot(hit);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(g.ctr + 3, (u64)__popcll(m));
    }
}

__global__ __launch_bounds__(kThreads) void layout_cycle_cut_kernel(OvlLayoutArgs g) {
    const u64* mk = g.mk[g.levels & 1];
    for (int64_t r0 = (int64_t)blockIdx.x * kThreads; r0 < g.n; r0 += (int64_t)gridDim.x * kThreads) {
        const int64_t r = r0 + threadIdx.x;
        bool cut = false;
        if (r < g.n && g.on_cycle[r]) {
            const int32_t link = g.link[r];
            cut = link >= 0 && mk[r] == ovl_layout_key(g.score[link], (uint32_t)link);
            if (cut) {
                g.link[r] = -1;
                g.succ[r] = -1;
            }
        }
        const u64 m = __ballot(cut);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(g.ctr + 0, (u64)__popcll(m));
    }
}

__global__ __launch_bounds__(kThreads) void layout_head_kernel(OvlLayoutArgs g) {
    const int lane = threadIdx.x & 63;
    const int32_t* top = g.jump + (int64_t)g.levels * g.n;
    const uint32_t* tl = g.tail[g.levels & 1];
    for (int64_t r0 = (int64_t)blockIdx.x * kThreads + (threadIdx.x & ~63); r0 < g.n;
         r0 += (int64_t)gridDim.x * kThreads) {
        const int64_t r = r0 + lane;
        const bool valid = r < g.n;
        const int32_t root = valid ? top[r] : -1;
        const u64 key = valid ? ovl_layout_head_key((int32_t)((uint32_t)g.len[r] + tl[r]), (uint32_t)r) : 0;
        // the wavefront's distinct roots one by one: the maximum over the lanes of that root, one atomic
        u64 todo = __ballot(valid);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            const int32_t lr = __shfl(root, src, 64);
            const bool mine = valid && root == lr;
            const u64 v = wave_max_u64(mine ? key : 0);
            if (lane == src) atomicMax(g.headkey + lr, v);
            todo &= ~__ballot(mine);
        }
    }
}

// every root: its head goes on the path, and its contig's rank and length go into the scan
__global__ __launch_bounds__(kThreads) void layout_root_kernel(OvlLayoutArgs g) {
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < g.n; r += (int64_t)gridDim.x * kThreads) {
        int64_t v = 0;
        if (g.succ[r] < 0) {
            const u64 hk = g.headkey[r];
            g.on_path[(uint32_t)~(uint32_t)hk] = 1;
            v = (int64_t(1) << 32) + (int64_t)(hk >> 32);
        }
        g.scan_in[r] = v;
    }
}

__global__ __launch_bounds__(kThreads) void layout_place_kernel(OvlLayoutArgs g) {
    const int32_t* top = g.jump + (int64_t)g.levels * g.n;
    const uint32_t* tl = g.tail[g.levels & 1];
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < g.n; r += (int64_t)gridDim.x * kThreads) {
        const int32_t root = top[r];
        const int64_t x = g.scan_out[root];
        const int32_t span = (int32_t)((uint32_t)g.len[r] + tl[r]);
        g.contig[r] = (int32_t)(x >> 32);
        g.offset[r] = (int32_t)(g.headkey[root] >> 32) - span;
        if (g.succ[r] < 0) g.c_off[x >> 32] = x & 0xFFFFFFFFll;
        if (r == g.n - 1) {
            const int64_t tot = g.scan_out[r] + g.scan_in[r];
            g.c_off[tot >> 32] = tot & 0xFFFFFFFFll;
            g.ctr[4] = (u64)(tot >> 32);
            g.ctr[5] = (u64)(tot & 0xFFFFFFFFll);
        }
    }
}

__global__ __launch_bounds__(kThreads) void layout_path_kernel(OvlLayoutArgs g, int32_t k) {
    const int32_t* jump = g.jump + (int64_t)k * g.n;
    for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < g.n; r += (int64_t)gridDim.x * kThreads)
        if (g.on_path[r]) g.on_path[jump[r]] = 1;
}

__global__ __launch_bounds__(kThreads) void layout_count_kernel(OvlLayoutArgs g) {
    for (int64_t r0 = (int64_t)blockIdx.x * kThreads; r0 < g.n; r0 += (int64_t)gridDim.x * kThreads) {
        const int64_t r = r0 + threadIdx.x;
        const u64 ml = __ballot(r < g.n && g.succ[r] >= 0), mp = __ballot(r < g.n && g.on_path[r] != 0);
        if ((threadIdx.x & 63) == 0) {
            if (ml) atomicAdd(g.ctr + 1, (u64)__popcll(ml));
            if (mp) atomicAdd(g.ctr + 2, (u64)__popcll(mp));
        }
    }
}

// bytes [from, len) of read s to bases[dst ..): the 64 lanes stride over them; nothing is stored at or past `cap`
__device__ __forceinline__ void copy_read(const OvlLayoutArgs& g, int32_t s, int32_t from, int64_t dst, int64_t cap,
                                          int lane) {
    const uint8_t* src = g.seqs + g.off[s];
    const int32_t len = g.len[s];
    for (int32_t i = from + lane; i < len; i += 64) {
        const int64_t at = dst + (i - from);
        if (at < 0 || at >= cap) continue;
        const uint8_t byte = src[i];
        g.bases[at] = g.table ? g.table[byte] : byte;
    }
}

__global__ __launch_bounds__(kThreads) void layout_spell_kernel(OvlLayoutArgs g, int64_t cap) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
    const int64_t waves = ((int64_t)gridDim.x * kThreads) >> 6;
    const int32_t* top = g.jump + (int64_t)g.levels * g.n;
    for (int64_t r = wave; r < g.n; r += waves) {
        if (!g.on_path[r]) continue;
        const int64_t base = g.c_off[g.contig[r]];
        const u64 hk = g.headkey[top[r]];
        if ((uint32_t)r == (uint32_t)~(uint32_t)hk) copy_read(g, (int32_t)r, 0, base, cap, lane);
        const int32_t s = g.succ[r];
        if (s >= 0) {
            const int32_t e = g.end[g.link[r]];
            copy_read(g, s, e, base + g.offset[s] + e, cap, lane);
        }
    }
}

inline unsigned blocks_for(int64_t items) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + kThreads - 1) / kThreads, 8192));
}

}  // namespace ovl_layout

extern "C" hipError_t ovl_launch_layout_link(const OvlLayoutArgs* g, int32_t runs, hipStream_t stream) {
    if (g->n_pairs <= 0 || g->n <= 0) return hipSuccess;
    const unsigned blocks = ovl_layout::blocks_for(g->n_pairs);
    if (runs) ovl_layout::layout_link_kernel<true><<<blocks, ovl_layout::kThreads, 0, stream>>>(*g);
    else ovl_layout::layout_link_kernel<false><<<blocks, ovl_layout::kThreads, 0, stream>>>(*g);
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_layout_double(const OvlLayoutArgs* g, int32_t resolve, hipStream_t stream) {
    if (g->n <= 0) return hipSuccess;
    const unsigned blocks = ovl_layout::blocks_for(g->n);
    ovl_layout::layout_init_kernel<<<blocks, ovl_layout::kThreads, 0, stream>>>(*g, resolve);
    for (int32_t k = 0; k < g->levels; ++k)
        ovl_layout::layout_level_kernel<<<blocks, ovl_layout::kThreads, 0, stream>>>(*g, k);
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_layout_cut(const OvlLayoutArgs* g, hipStream_t stream) {
    if (g->n <= 0) return hipSuccess;
    const unsigned blocks = ovl_layout::blocks_for(g->n);
    ovl_layout::layout_cycle_mark_kernel<<<blocks, ovl_layout::kThreads, 0, stream>>>(*g);
    ovl_layout::layout_cycle_cut_kernel<<<blocks, ovl_layout::kThreads, 0, stream>>>(*g);
    return hipGetLastError();
}

extern "C" hipError_t ovl_layout_scan_bytes(int32_t n, size_t* bytes) {
    *bytes = 0;
    return hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (const int64_t*)nullptr, (int64_t*)nullptr, n);
}

extern "C" hipError_t ovl_launch_layout_place(const OvlLayoutArgs* g, void* temp, size_t temp_bytes,
                                              hipStream_t stream) {
    if (g->n <= 0) return hipSuccess;
    const unsigned blocks = ovl_layout::blocks_for(g->n);
    hipError_t e = hipMemsetAsync(g->headkey, 0, sizeof(unsigned long long) * (size_t)g->n, stream);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(g->on_path, 0, (size_t)g->n, stream)) != hipSuccess) return e;
    ovl_layout::layout_head_kernel<<<blocks, ovl_layout::kThreads, 0, stream>>>(*g);
    ovl_layout::layout_root_kernel<<<blocks, ovl_layout::kThreads, 0, stream>>>(*g);
    if ((e = hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, (const int64_t*)g->scan_in, g->scan_out, g->n,
                                              stream)) != hipSuccess)
        return e;
    ovl_layout::layout_place_kernel<<<blocks, ovl_layout::kThreads, 0, stream>>>(*g);
    for (int32_t k = g->levels - 1; k >= 0; --k)
        ovl_layout::layout_path_kernel<<<blocks, ovl_layout::kThreads, 0, stream>>>(*g, k);
    ovl_layout::layout_count_kernel<<<blocks, ovl_layout::kThreads, 0, stream>>>(*g);
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_layout_spell(const OvlLayoutArgs* g, int32_t waves, hipStream_t stream) {
    if (g->n <= 0 || !g->bases || waves <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((waves + 3) / 4);
    ovl_layout::layout_spell_kernel<<<blocks, ovl_layout::kThreads, 0, stream>>>(*g, g->bases_cap);
    return hipGetLastError();
}
