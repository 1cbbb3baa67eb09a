// k-mer candidate-pair enumeration on the device, with the
// reference's exact output order (overlapGraphs.py:30-52):
//
//   prefix key of read i = read[:k] (the whole read when shorter, :34-37)
//   suffix key of read a = read[-k:] (the whole read when shorter, :44-47)
//   for a in read order (read_copies order, :43):
//     for b in prefix_index[suffix key of a], in read order (:38-40, :49-50):
//       if b != a (distinct reads, so index inequality is string inequality, :52): emit (a, b)
//   k == 0: every b != a in read order (:49).
//
// Device plan (all integer/byte work, HBM-light):
//   1. keys:   one thread per read packs its prefix / suffix symbol codes into a
//              64-bit key, (length << 58) | codes (2, 4 or 8 bits per symbol), so
//              equal keys <=> equal strings (lengths < k stay distinct);
//   2. sort:   stable LSD radix sort of (prefix key, read index) -> reads grouped
//              by prefix, index order kept inside a group (= prefix_index lists);
//   3. count:  per read a, binary search of its suffix key in the sorted keys ->
//              group [lo, hi); count = group size minus a itself if a is in it
//              (prefix key of a == suffix key of a);
//   4. scan:   exclusive prefix sum of the counts (int64) -> output offsets;
//   5. emit:   one wavefront per read walks its group 64 members at a time,
//              drops b == a with a ballot, writes (a, b) coalesced.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "ovl_kernels.h"

namespace ovl_cand {

__global__ __launch_bounds__(256) void key_kernel(const uint8_t* __restrict__ codes, const int64_t* __restrict__ off,
                                                  const int32_t* __restrict__ len, int32_t n_reads, int32_t k,
                                                  int32_t bits, uint64_t* __restrict__ pre_key,
                                                  uint64_t* __restrict__ suf_key, int32_t* __restrict__ iota) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_reads;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t n = len[i];
        const int32_t l = n < k ? n : k;
        const uint8_t* r = codes + off[i];
        uint64_t p = 0, s = 0;
        for (int q = 0; q < l; ++q) {
            p = (p << bits) | r[q];
            s = (s << bits) | r[n - l + q];
        }
        pre_key[i] = ((uint64_t)l << 58) | p;
        suf_key[i] = ((uint64_t)l << 58) | s;
        iota[i] = (int32_t)i;
    }
}

// first index in sorted[0, n) with sorted[idx] >= key (lower) or > key (upper)
__device__ __forceinline__ int64_t bound(const uint64_t* __restrict__ sorted, int64_t n, uint64_t key, bool upper) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const uint64_t v = sorted[mid];
        if (upper ? (v <= key) : (v < key)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void count_kernel(const uint64_t* __restrict__ sorted, const uint64_t* __restrict__ pre_key,
                                                    const uint64_t* __restrict__ suf_key, int32_t n_reads, int32_t all_pairs,
                                                    int64_t* __restrict__ lo_out, int64_t* __restrict__ hi_out,
                                                    int64_t* __restrict__ cnt) {
    for (int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < n_reads;
         a += (int64_t)gridDim.x * blockDim.x) {
        if (all_pairs) {  // k == 0: every other read
            lo_out[a] = 0;
            hi_out[a] = n_reads;
            cnt[a] = n_reads - 1;
            continue;
        }
        const uint64_t key = suf_key[a];
        const int64_t lo = bound(sorted, n_reads, key, false);
        const int64_t hi = bound(sorted, n_reads, key, true);
        lo_out[a] = lo;
        hi_out[a] = hi;
        // a is in its own group iff its prefix key equals its suffix key
        cnt[a] = (hi - lo) - (hi > lo && pre_key[a] == key ? 1 : 0);
    }
}

// one wavefront per read a: its group is order[lo, hi) (positions 0 .. n_reads-1
// themselves when all_pairs), members in index order; b == a is dropped
__global__ __launch_bounds__(256) void emit_kernel(const int32_t* __restrict__ order, const int64_t* __restrict__ lo_in,
                                                   const int64_t* __restrict__ hi_in, const int64_t* __restrict__ offs,
                                                   int32_t n_reads, int32_t all_pairs, int32_t* __restrict__ out_a,
                                                   int32_t* __restrict__ out_b) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t a = wave; a < n_reads; a += n_waves) {
        const int64_t lo = lo_in[a];
        const int64_t g = hi_in[a] - lo;
        const int64_t base = offs[a];
        int64_t written = 0;
        for (int64_t q0 = 0; q0 < g; q0 += 64) {
            const int64_t q = q0 + lane;
            const bool valid = q < g;
            const int32_t b = valid ? (all_pairs ? (int32_t)q : order[lo + q]) : -1;
            const bool keep = valid && b != (int32_t)a;
            const uint64_t m = __ballot(keep);
            if (keep) {
                const int64_t slot = base + written + __popcll(m & ((1ull << lane) - 1ull));
                out_a[slot] = (int32_t)a;
                out_b[slot] = b;
            }
            written += __popcll(m);
        }
    }
}

}  // namespace ovl_cand

using namespace ovl_cand;

static unsigned grid_for_threads(int64_t threads, int64_t cap) {
    int64_t b = (threads + 255) / 256;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}

extern "C" hipError_t ovl_cand_keys(const uint8_t* codes, const int64_t* off, const int32_t* len, int32_t n_reads,
                                    int32_t k, int32_t bits, uint64_t* pre_key, uint64_t* suf_key, int32_t* iota,
                                    hipStream_t stream) {
    if (n_reads <= 0) return hipSuccess;
    key_kernel<<<grid_for_threads(n_reads, 8192), 256, 0, stream>>>(codes, off, len, n_reads, k, bits, pre_key,
                                                                    suf_key, iota);
    return hipGetLastError();
}

extern "C" hipError_t ovl_cand_temp_bytes(int32_t n_reads, size_t* bytes) {
    size_t s1 = 0, s2 = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, s1, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                      (const int32_t*)nullptr, (int32_t*)nullptr, n_reads, 0, 64);
    if (e != hipSuccess) return e;
    e = hipcub::DeviceScan::ExclusiveSum(nullptr, s2, (const int64_t*)nullptr, (int64_t*)nullptr, n_reads);
    if (e != hipSuccess) return e;
    *bytes = s1 > s2 ? s1 : s2;
    return hipSuccess;
}

extern "C" hipError_t ovl_cand_sort(void* temp, size_t temp_bytes, const uint64_t* keys_in, uint64_t* keys_out,
                                    const int32_t* vals_in, int32_t* vals_out, int32_t n_reads, hipStream_t stream) {
    if (n_reads <= 0) return hipSuccess;
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n_reads, 0, 64,
                                              stream);
}

extern "C" hipError_t ovl_cand_count(const uint64_t* sorted, const uint64_t* pre_key, const uint64_t* suf_key,
                                     int32_t n_reads, int32_t all_pairs, int64_t* lo, int64_t* hi, int64_t* cnt,
                                     hipStream_t stream) {
    if (n_reads <= 0) return hipSuccess;
    count_kernel<<<grid_for_threads(n_reads, 8192), 256, 0, stream>>>(sorted, pre_key, suf_key, n_reads, all_pairs,
                                                                      lo, hi, cnt);
    return hipGetLastError();
}

extern "C" hipError_t ovl_cand_scan(void* temp, size_t temp_bytes, const int64_t* cnt, int64_t* offs, int32_t n_reads,
                                    hipStream_t stream) {
    if (n_reads <= 0) return hipSuccess;
    return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, cnt, offs, n_reads, stream);
}

extern "C" hipError_t ovl_cand_emit(const int32_t* order, const int64_t* lo, const int64_t* hi, const int64_t* offs,
                                    int32_t n_reads, int32_t all_pairs, int32_t* out_a, int32_t* out_b,
                                    hipStream_t stream) {
    if (n_reads <= 0) return hipSuccess;
    emit_kernel<<<grid_for_threads((int64_t)n_reads * 64, 16384), 256, 0, stream>>>(order, lo, hi, offs, n_reads,
                                                                                    all_pairs, out_a, out_b);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------- shard bounds
// Contiguous shards of a pair list balanced by cost(p) = len[a]*len[b] + 1 (the
// DP work of a pair is n*m cells), the cut rule of ovlgraph/sharded.py:shard_bounds: inside
// [lo, hi), cut_r = the first p with (cum[p] - base) * S >= total * r, where cum is the inclusive
// prefix sum of the costs, base = cum[lo - 1] and total = cum[hi - 1] - base; cuts are made
// non-decreasing, cut_0 = lo and cut_S = hi.  cum fits int64 (<= 2^31 pairs x 2^30 + 1).
namespace ovl_cand {

struct PairCost {
    const int32_t* a;
    const int32_t* b;
    const int32_t* len;
    __host__ __device__ int64_t operator()(const int64_t& p) const {
        return (int64_t)len[a[p]] * (int64_t)len[b[p]] + 1;
    }
};

__global__ void cut_kernel(const int64_t* __restrict__ cum, int64_t lo, int64_t hi, int32_t shards,
                           int64_t* __restrict__ cuts) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t base = lo > 0 ? cum[lo - 1] : 0;
    const int64_t total = hi > lo ? cum[hi - 1] - base : 0;
    int64_t prev = lo;
    cuts[0] = lo;
    for (int32_t r = 1; r < shards; ++r) {
        int64_t a = lo, b = hi;
        const int64_t want = total * r;
        while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if ((cum[mid] - base) * shards >= want) b = mid;
            else a = mid + 1;
        }
        prev = a > prev ? a : prev;
        cuts[r] = prev;
    }
    cuts[shards] = hi;
}

}  // namespace ovl_cand

using ovl_cand::PairCost;
typedef hipcub::TransformInputIterator<int64_t, PairCost, hipcub::CountingInputIterator<int64_t>> CostIter;

extern "C" hipError_t ovl_shard_temp_bytes(int64_t n_pairs, size_t* bytes) {
    PairCost f{nullptr, nullptr, nullptr};
    CostIter it(hipcub::CountingInputIterator<int64_t>(0), f);
    return hipcub::DeviceScan::InclusiveSum(nullptr, *bytes, it, (int64_t*)nullptr, n_pairs);
}

extern "C" hipError_t ovl_shard_scan(void* temp, size_t temp_bytes, const int32_t* a, const int32_t* b,
                                     const int32_t* len, int64_t n_pairs, int64_t* cum, hipStream_t stream) {
    if (n_pairs <= 0) return hipSuccess;
    PairCost f{a, b, len};
    CostIter it(hipcub::CountingInputIterator<int64_t>(0), f);
    return hipcub::DeviceScan::InclusiveSum(temp, temp_bytes, it, cum, n_pairs, stream);
}

extern "C" hipError_t ovl_shard_cut(const int64_t* cum, int64_t lo, int64_t hi, int32_t shards, int64_t* cuts,
                                    hipStream_t stream) {
    ovl_cand::cut_kernel<<<1, 64, 0, stream>>>(cum, lo, hi, shards, cuts);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------- seed candidates
// The second candidate rule (include/ovl.h, ovl_seed_candidates):
//
//   Reads are the distinct reads in read_copies order, and k >= 1.  The prefix key of read b is b[:k]; a read
//   shorter than k has no key and takes no part.  For each read a in order, for each offset o = 1, 2, ...,
//   len(a) - k ascending, for each read b != a in read order whose prefix key equals a[o:o+k]: emit (a, b, o),
//   unless (a, b) was already emitted at a smaller offset.
//
// Each b has exactly one prefix key, so two offsets of a with different k-mers have disjoint groups and two with
// equal k-mers the same group: "already emitted" is "a's k-mer at o also occurs at an offset o' with 1 <= o' < o",
// and such an offset emits nothing.  No sort of the output is needed.
//
// Device plan, the keys packed as key_kernel packs them, (k << 58) | codes:
//   1. keys:   seed_key_kernel, one thread per read: its prefix key, or ~0 for a read shorter than k -- no k-mer
//              key equals it (its length field is 63 > 29 >= k), and it sorts behind every group, so the sort's
//              first n_long entries are exactly the reads with len >= k and only those are searched;
//   2. sort:   the stable radix sort of (prefix key, read) of rule 1 (ovl_cand_sort);
//   3. count:  seed_count_kernel, one wavefront per read a.  It forms the len(a) - k keys of a's offsets into LDS:
//              lane j owns a run of ceil((len(a) - k) / 64) consecutive offsets, packs the first key and rolls the
//              others ((key << bits | next symbol) & mask).  Then, 64 offsets at a time, a lane binary-searches its
//              key's group [lo, hi) in the sorted keys, and the lanes that found one compare their key with the keys
//              of all earlier offsets (one LDS broadcast read per earlier offset) and drop theirs if it occurred.
//              The keys stay in LDS, not registers: an offset is compared with every earlier one of the read, not only
//              with its own 64.  That comparison is (len - k)^2 / 64 LDS reads per read, below the len^2 cells that
//              scoring one pair of such reads costs.  Count = group sizes, minus one where a is in the group (its
//              own prefix key equals the k-mer);
//   4. scan:   exclusive int64 prefix sum of the counts (ovl_cand_scan) -> output offsets;
//   5. emit:   seed_emit_kernel, one wavefront per read, 64 offsets at a time: an inclusive scan of the 64 group
//              sizes lays the groups' members end to end in the rule's order (offset ascending, then read order),
//              and the wavefront walks them 64 members at a time -- a lane finds its member's offset by a six-step
//              search of the scan -- drops b == a by ballot as emit_kernel does and writes a, b and o coalesced.
//              A group's (lo, size) per offset comes from HBM, where the count pass left it (KEEP, the default), or
//              is searched again (the keys formed again into LDS; OVL_SEED_GROUPS=search).  Measured, DESIGN.md §4.6a:
//              PhiX N = 50,000, k = 12, 15.6 M pairs, the emit kernel takes 69 us from HBM against 294 us.
namespace ovl_cand {

__global__ __launch_bounds__(256) void seed_key_kernel(const uint8_t* __restrict__ codes, const int64_t* __restrict__ off,
                                                       const int32_t* __restrict__ len, int32_t n_reads, int32_t k,
                                                       int32_t bits, uint64_t* __restrict__ pre_key,
                                                       int32_t* __restrict__ iota) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_reads;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t key = ~0ull;
        if (len[i] >= k) {
            const uint8_t* r = codes + off[i];
            uint64_t p = 0;
            for (int q = 0; q < k; ++q) p = (p << bits) | r[q];
            key = ((uint64_t)k << 58) | p;
        }
        pre_key[i] = key;
        iota[i] = (int32_t)i;
    }
}

// The keys of read r's offsets 1 .. n_off into this wavefront's LDS (keys[i] is offset i + 1's): lane j packs the
// first key of its run and rolls the others.
__device__ __forceinline__ void seed_wave_keys(const uint8_t* __restrict__ r, int32_t n_off, int32_t k, int32_t bits,
                                               int lane, uint64_t* keys) {
    const int32_t run = (n_off + 63) >> 6;
    const int32_t i0 = lane * run;
    const int32_t i1 = min(i0 + run, n_off);
    if (i0 < i1) {
        const uint64_t mask = (1ull << (k * bits)) - 1ull;  // k * bits <= 58
        const uint64_t tag = (uint64_t)k << 58;
        uint64_t p = 0;
        for (int q = 0; q < k; ++q) p = (p << bits) | r[i0 + 1 + q];
        keys[i0] = tag | p;
        for (int32_t i = i0 + 1; i < i1; ++i) {
            p = ((p << bits) | r[i + k]) & mask;  // offset i + 1's last symbol
            keys[i] = tag | p;
        }
    }
    // the other lanes' keys are read next: LDS writes of this wavefront retired, and no reordering across
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Offsets c0 + 1 .. c0 + 64 of a read, lane = offset - 1 - c0: the lane's key, and its group sorted[lo, lo + g) --
// g = 0 past the read's offsets, without a group, and where the key occurred at an earlier offset of the read.
__device__ __forceinline__ void seed_chunk_group(const uint64_t* __restrict__ sorted, int32_t n_long,
                                                 const uint64_t* keys, int32_t n_off, int32_t c0, int lane,
                                                 uint64_t& key, int32_t& lo, int32_t& g) {
    const int32_t i = c0 + lane;
    const bool valid = i < n_off;
    key = valid ? keys[i] : 0ull;
    lo = 0;
    g = 0;
    if (valid) {
        lo = (int32_t)bound(sorted, n_long, key, false);
        if (lo < n_long && sorted[lo] == key) {
            int64_t a = lo + 1, b = n_long;  // upper bound within (lo, n_long)
            while (a < b) {
                const int64_t mid = (a + b) >> 1;
                if (sorted[mid] <= key) a = mid + 1;
                else b = mid;
            }
            g = (int32_t)a - lo;
        }
    }
    if (__ballot(g > 0) != 0ull) {
        const int32_t jend = min(c0 + 63, n_off - 1);  // the largest offset index of the chunk: j < i <= jend
        bool dup = false;
        for (int32_t j = 0; j < jend; ++j) dup |= (keys[j] == key) & (j < i);
        if (dup) g = 0;
    }
}

template <bool KEEP>
__global__ __launch_bounds__(256) void seed_count_kernel(const uint8_t* __restrict__ codes, const int64_t* __restrict__ off,
                                                         const int32_t* __restrict__ len, int32_t n_reads, int32_t k,
                                                         int32_t bits, const uint64_t* __restrict__ sorted,
                                                         int32_t n_long, const uint64_t* __restrict__ pre_key,
                                                         int32_t max_off, int32_t* __restrict__ grp_lo,
                                                         int32_t* __restrict__ grp_n, int64_t* __restrict__ cnt) {
    extern __shared__ uint64_t seed_lds[];
    const int lane = threadIdx.x & 63;
    uint64_t* keys = seed_lds + (size_t)(threadIdx.x >> 6) * max_off;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t a = wave; a < n_reads; a += n_waves) {
        const int32_t n_off = min(len[a] - k, max_off);  // (max_off = lmax - k: never the smaller one)
        int64_t total = 0;
        if (n_off > 0) {
            const int64_t base = off[a];
            seed_wave_keys(codes + base, n_off, k, bits, lane, keys);
            const uint64_t own = pre_key[a];
            for (int32_t c0 = 0; c0 < n_off; c0 += 64) {
                uint64_t key;
                int32_t lo, g;
                seed_chunk_group(sorted, n_long, keys, n_off, c0, lane, key, lo, g);
                if (KEEP && c0 + lane < n_off) {
                    grp_lo[base + c0 + lane] = lo;
                    grp_n[base + c0 + lane] = g;
                }
                total += g - (g > 0 && key == own ? 1 : 0);
            }
            // the next read's keys overwrite these: this read's LDS reads are done first
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) total += __shfl_xor(total, s, 64);
        if (lane == 0) cnt[a] = total;
    }
}

template <bool KEEP>
__global__ __launch_bounds__(256) void seed_emit_kernel(const uint8_t* __restrict__ codes, const int64_t* __restrict__ off,
                                                        const int32_t* __restrict__ len, int32_t n_reads, int32_t k,
                                                        int32_t bits, const uint64_t* __restrict__ sorted,
                                                        int32_t n_long, const int32_t* __restrict__ order,
                                                        int32_t max_off, const int32_t* __restrict__ grp_lo,
                                                        const int32_t* __restrict__ grp_n,
                                                        const int64_t* __restrict__ cnt, const int64_t* __restrict__ offs,
                                                        int32_t* __restrict__ out_a, int32_t* __restrict__ out_b,
                                                        int32_t* __restrict__ out_o) {
    extern __shared__ uint64_t seed_lds[];
    const int lane = threadIdx.x & 63;
    uint64_t* keys = seed_lds + (size_t)(threadIdx.x >> 6) * max_off;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t a = wave; a < n_reads; a += n_waves) {
        const int64_t mine = cnt[a];
        if (mine == 0) continue;
        const int32_t n_off = min(len[a] - k, max_off);
        const int64_t base = off[a];
        const int64_t out0 = offs[a], out1 = out0 + mine;  // this read's slots: nothing is written outside them
        if (!KEEP) seed_wave_keys(codes + base, n_off, k, bits, lane, keys);
        int64_t written = 0;
        for (int32_t c0 = 0; c0 < n_off; c0 += 64) {
            int32_t lo = 0, g = 0;
            if (KEEP) {
                if (c0 + lane < n_off) {
                    lo = grp_lo[base + c0 + lane];
                    g = grp_n[base + c0 + lane];
                }
            } else {
                uint64_t key;
                seed_chunk_group(sorted, n_long, keys, n_off, c0, lane, key, lo, g);
            }
            // the 64 groups' members end to end: lane l's are positions [P[l] - g[l], P[l])
            int64_t P = g;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const int64_t up = __shfl_up(P, s, 64);
                if (lane >= s) P += up;
            }
            const int64_t T = __shfl(P, 63, 64);
            for (int64_t t0 = 0; t0 < T; t0 += 64) {
                const int64_t t = t0 + lane;
                const bool valid = t < T;
                int l = 0;  // the lanes whose P <= t: the first lane with P > t owns member t
#pragma unroll
                for (int s = 32; s >= 1; s >>= 1) {
                    const int64_t pv = __shfl(P, l + s - 1, 64);
                    if (pv <= t) l += s;
                }
                l = min(l, 63);
                const int64_t pl = __shfl(P, l, 64);
                const int32_t gl = __shfl(g, l, 64);
                const int32_t ll = __shfl(lo, l, 64);
                const int64_t pos = (int64_t)ll + (t - (pl - gl));
                const bool in = valid && pos >= 0 && pos < n_long;
                const int32_t b = in ? order[pos] : -1;
                const bool keep = in && b != (int32_t)a;
                const uint64_t m = __ballot(keep);
                const int64_t slot = out0 + written + __popcll(m & ((1ull << lane) - 1ull));
                if (keep && slot < out1) {
                    out_a[slot] = (int32_t)a;
                    out_b[slot] = b;
                    out_o[slot] = c0 + l + 1;
                }
                written += __popcll(m);
            }
        }
        if (!KEEP) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
}

}  // namespace ovl_cand

extern "C" hipError_t ovl_seed_keys(const uint8_t* codes, const int64_t* off, const int32_t* len, int32_t n_reads,
                                    int32_t k, int32_t bits, uint64_t* pre_key, int32_t* iota, hipStream_t stream) {
    if (n_reads <= 0) return hipSuccess;
    ovl_cand::seed_key_kernel<<<grid_for_threads(n_reads, 8192), 256, 0, stream>>>(codes, off, len, n_reads, k, bits,
                                                                                   pre_key, iota);
    return hipGetLastError();
}

// One wavefront per read; a block is 4 wavefronts while their keys (max_off each) fit 64 KiB of LDS, else one.
static void seed_shape(int32_t n_reads, int32_t max_off, unsigned* grid, unsigned* block, size_t* lds) {
    const int waves = max_off <= OVL_SEED_MAX_OFFSETS / 4 ? 4 : 1;
    *block = 64u * waves;
    *lds = (size_t)waves * (size_t)max_off * sizeof(uint64_t);
    int64_t b = ((int64_t)n_reads + waves - 1) / waves;
    if (b > 16384) b = 16384;
    *grid = (unsigned)(b < 1 ? 1 : b);
}

extern "C" hipError_t ovl_seed_count(const OvlSeedArgs* s, int32_t keep, hipStream_t stream) {
    if (s->n_reads <= 0 || s->max_off <= 0) return hipSuccess;
    if (s->max_off > OVL_SEED_MAX_OFFSETS) return hipErrorInvalidValue;
    unsigned grid, block;
    size_t lds;
    seed_shape(s->n_reads, s->max_off, &grid, &block, &lds);
    if (keep)
        ovl_cand::seed_count_kernel<true><<<grid, block, lds, stream>>>(s->codes, s->off, s->len, s->n_reads, s->k,
                                                                        s->bits, s->sorted, s->n_long, s->pre_key,
                                                                        s->max_off, s->grp_lo, s->grp_n, s->cnt);
    else
        ovl_cand::seed_count_kernel<false><<<grid, block, lds, stream>>>(s->codes, s->off, s->len, s->n_reads, s->k,
                                                                         s->bits, s->sorted, s->n_long, s->pre_key,
                                                                         s->max_off, s->grp_lo, s->grp_n, s->cnt);
    return hipGetLastError();
}

extern "C" hipError_t ovl_seed_emit(const OvlSeedArgs* s, int32_t keep, hipStream_t stream) {
    if (s->n_reads <= 0 || s->max_off <= 0) return hipSuccess;
    if (s->max_off > OVL_SEED_MAX_OFFSETS) return hipErrorInvalidValue;
    unsigned grid, block;
    size_t lds;
    seed_shape(s->n_reads, s->max_off, &grid, &block, &lds);
    if (keep)
        ovl_cand::seed_emit_kernel<true><<<grid, block, 0, stream>>>(
            s->codes, s->off, s->len, s->n_reads, s->k, s->bits, s->sorted, s->n_long, s->order, s->max_off, s->grp_lo,
            s->grp_n, s->cnt, s->offs, s->out_a, s->out_b, s->out_o);
    else
        ovl_cand::seed_emit_kernel<false><<<grid, block, lds, stream>>>(
            s->codes, s->off, s->len, s->n_reads, s->k, s->bits, s->sorted, s->n_long, s->order, s->max_off, s->grp_lo,
            s->grp_n, s->cnt, s->offs, s->out_a, s->out_b, s->out_o);
    return hipGetLastError();
}
