// k-mer spectrum read correction on the device (include/ovl.h, ovl_kmer_spectrum / ovl_correct_reads; DESIGN.md
// §4.16).  The rule:
//
//   Codes, keys and windows.  Codes are A = 0, C = 1, G = 2, T = 3, taken from the bytes ACGT; any other byte has no
//   code.  k is in [1, 31].  The key of a window r[o:o+k] whose bytes all have codes is
//   sum_j code(r[o+j]) << 2(k-1-j), a uint64 below 2^62, so key order is the k-mers' order as byte strings.  A window
//   that holds a byte without a code has no key, and so has every window of a read shorter than k.
//   Spectrum.  The distinct keys over all windows of all reads (reads counted as given, duplicates included) in
//   ascending order, each with its number of occurrences as an int32.
//   Threshold.  h[c] = the number of distinct keys with count c.  solid_threshold is the smallest c >= 1 with
//   c >= max count or h[c+1] >= h[c] (the first valley of the histogram).  A key is solid when its count is >=
//   min_count; a window without a key is never solid.
//   Correction, one round.  Every decision reads the original reads only.  For a read r of length L >= k and a
//   position i the covering windows are the offsets o in [max(0, i-k+1), min(i, L-k)].  Position i is trusted when at
//   least one covering window is solid, and stays.  An untrusted position whose byte has no code stays.  Otherwise,
//   for each of the three other bases x, s(x) is the number of covering windows that are solid after r[i] alone is
//   replaced by x; if the largest s(x) is >= 1 and strictly greater than the other two, r[i] becomes that x; on a
//   tie, or when all are 0, r[i] stays.  Reads shorter than k are returned as they are.  Lengths never change.
//
// Device plan:
//   1. keys:    key_kernel, one wavefront per read.  Lane j owns a run of ceil(windows / 64) consecutive windows, packs
//               the first key and rolls the others, as seed_count_kernel does; a window without a key stores ~0.  The
//               keys of read r go to keys[woff[r] ..), woff the scan of max(len - k + 1, 0) (made on the host beside
//               the argument checks, which walk the offsets anyway).
//   2. sort:    hipcub::DeviceRadixSort::SortKeys over bits [0, 2k + 1): bit 2k is 0 in every key and 1 in ~0, so ~0
//               sorts behind every key.  (Over 2k bits alone ~0 would tie with the key of k T's.)
//   3. count:   head_kernel flags the first entry of every run of equal values, hipcub's exclusive scan numbers the
//               runs, scatter_kernel stores each run's key and start, and counts_kernel turns the starts into run
//               lengths and a histogram of them (per block in LDS, then one atomic per non-empty bin).  The run of ~0,
//               when there is one, is the last and is cut off by the count of distinct keys.
//   4. correct: correct_kernel, one wavefront per read, four per block while their LDS fits 64 KiB.  The read's keys
//               are rolled into LDS.  64 windows at a time each lane binary-searches its key in the spectrum and the
//               ballot of the solid bits goes into a per-read mask in LDS.  64 positions at a time a lane derives its
//               position's trusted bit from the mask (the covering windows are at most 31 consecutive bits: two
//               words) and the untrusted positions are compacted by ballot.  Their work items (untrusted position,
//               x, covering offset) are flattened as position * 3k + x * k + offset and taken 64 at a time: a lane
//               forms its substituted key from the LDS key by replacing one 2-bit field, searches it and adds into
//               the position's three counters: with an LDS atomic, or (OVL_SPECTRUM_VOTE=ballot) the first
//               lane of a (position, x) segment counts the step's ballot over its k lanes and adds once.  Measured,
//               PhiX N = 50,000, k = 12, the pass takes 0.617 ms against 0.613 ms, inside the spreads;
//               the atomics stay the default.  One lane per untrusted position decides and stores the byte into the
//               output, which starts as a copy of the input.  All stores are ordinary vector stores.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "ovl_spectrum.h"

namespace ovl_spec {

// The keys of read r's n_win windows into dst (LDS or HBM): lane j packs the first key of its run and rolls the others.
__device__ __forceinline__ void wave_keys(const uint8_t* __restrict__ r, int32_t n_win, int32_t k, int lane,
                                          uint64_t* dst) {
    const int32_t run = (n_win + 63) >> 6;
    const int32_t i0 = lane * run;
    const int32_t i1 = min(i0 + run, n_win);
    if (i0 < i1) {
        const uint64_t mask = (1ull << (2 * k)) - 1ull;  // 2k <= 62
        uint64_t key = 0;
        int32_t good = 0;
        for (int q = 0; q < k; ++q) ovl_spec_roll(key, good, r[i0 + q], mask);
        dst[i0] = good >= k ? key : kSpecNoKey;
        for (int32_t i = i0 + 1; i < i1; ++i) {
            ovl_spec_roll(key, good, r[i + k - 1], mask);  // window i's last byte; i + k - 1 <= len - 1
            dst[i] = good >= k ? key : kSpecNoKey;
        }
    }
}

// what one lane wrote to LDS is read by the others next (and the reverse before it is overwritten)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void key_kernel(OvlSpectrumArgs g) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < g.n_reads; r += n_waves) {
        const int64_t w0 = g.woff[r];
        const int64_t nw = g.woff[r + 1] - w0;
        if (nw <= 0 || w0 < 0 || w0 + nw > g.n_win) continue;
        wave_keys(g.seqs + g.off[r], (int32_t)nw, g.k, lane, g.keys + w0);
    }
}

__global__ __launch_bounds__(256) void head_kernel(OvlSpectrumArgs g) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.n_win;
         i += (int64_t)gridDim.x * blockDim.x)
        g.flag[i] = (i == 0 || g.sorted[i] != g.sorted[i - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(256) void scatter_kernel(OvlSpectrumArgs g) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.n_win;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t f = g.flag[i], p = g.pos[i];
        const uint64_t v = g.sorted[i];
        if (f) {  // p < n_win: there are at most n_win runs
            g.starts[p] = (int32_t)i;
            g.spec_keys[p] = v;
        }
        if (i == g.n_win - 1) {
            const int32_t runs = p + f;  // <= n_win
            g.starts[runs] = (int32_t)g.n_win;
            g.ctr[0] = (unsigned long long)(runs - (v == kSpecNoKey ? 1 : 0));
        }
    }
}

__global__ __launch_bounds__(256) void counts_kernel(OvlSpectrumArgs g) {
    __shared__ uint32_t h[kSpecHistBins];
    for (int q = threadIdx.x; q < kSpecHistBins; q += blockDim.x) h[q] = 0;
    __syncthreads();
    int32_t most = 0;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < g.n_distinct;
         j += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = g.starts[j + 1] - g.starts[j];
        g.spec_counts[j] = c;
        atomicAdd(&h[min(c, g.bins - 1)], 1u);
        most = max(most, c);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) most = max(most, __shfl_xor(most, s, 64));
    if ((threadIdx.x & 63) == 0 && most > 0) atomicMax(&g.ctr[6], (unsigned long long)most);
    if (blockIdx.x == 0 && threadIdx.x == 0) g.ctr[7] = (unsigned long long)g.starts[g.n_distinct];
    __syncthreads();
    for (int q = threadIdx.x; q < kSpecHistBins; q += blockDim.x)
        if (h[q]) atomicAdd(&g.hist[q], h[q]);
}

// key is in the spectrum with a count >= min_count
__device__ __forceinline__ bool solid(const OvlSpectrumArgs& g, uint64_t key) {
    int32_t lo = 0, hi = g.n_distinct;
    while (lo < hi) {
        const int32_t mid = (int32_t)(((uint32_t)lo + (uint32_t)hi) >> 1);
        if (g.spec_keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < g.n_distinct && g.spec_keys[lo] == key && g.spec_counts[lo] >= g.min_count;
}

// any bit of mask in [lo, hi], 0 <= lo <= hi, hi - lo < 64
__device__ __forceinline__ bool any_bit(const uint64_t* mask, int32_t lo, int32_t hi) {
    const int32_t w0 = lo >> 6, w1 = hi >> 6;
    uint64_t m = mask[w0] & (~0ull << (lo & 63));
    const uint64_t upto = ~0ull >> (63 - (hi & 63));
    if (w0 == w1) return (m & upto) != 0ull;
    return m != 0ull || (mask[w1] & upto) != 0ull;
}

// LDS of one wavefront, in uint64 words: max_win keys, ceil(max_win / 64) mask words, 64 untrusted positions and their
// 3 * 64 counters (int32: 128 words)
__host__ __device__ inline size_t wave_words(int32_t max_win) {
    return (size_t)max_win + (size_t)((max_win + 63) >> 6) + 128;
}

// BALLOT: how a work item's solid bit reaches its position's counter.  false: one LDS atomic per solid item.  true: the
// items of one (position, x) are k consecutive lanes, so the first of them inside the step counts the step's ballot
// over its segment and adds once, without an atomic (a segment cut by a step is added to in two steps, one after the
// other).
template <bool BALLOT>
__global__ __launch_bounds__(256) void correct_kernel(OvlSpectrumArgs g) {
    extern __shared__ uint64_t spec_lds[];
    const int lane = threadIdx.x & 63;
    const uint64_t below = (1ull << lane) - 1ull;
    uint64_t* keys = spec_lds + (size_t)(threadIdx.x >> 6) * wave_words(g.max_win);
    uint64_t* mask = keys + g.max_win;
    int32_t* ulist = reinterpret_cast<int32_t*>(mask + ((g.max_win + 63) >> 6));
    int32_t* cnt = ulist + 64;
    const int32_t k = g.k, k3 = 3 * g.k;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    unsigned long long t_solid = 0, t_untrusted = 0, t_changed = 0, t_ties = 0;  // the same in every lane
    for (int64_t r = wave; r < g.n_reads; r += n_waves) {
        const int32_t n_win = (int32_t)min(g.woff[r + 1] - g.woff[r], (int64_t)g.max_win);
        if (n_win <= 0) {
            if (lane == 0) g.changed[r] = 0;
            continue;
        }
        const int64_t base = g.off[r];
        const int32_t L = n_win + k - 1;
        const uint8_t* s = g.seqs + base;
        wave_keys(s, n_win, k, lane, keys);
        wave_sync();
        for (int32_t c0 = 0; c0 < n_win; c0 += 64) {
            const int32_t i = c0 + lane;
            bool sol = false;
            if (i < n_win) {
                const uint64_t key = keys[i];
                sol = key != kSpecNoKey && solid(g, key);
            }
            const uint64_t m = __ballot(sol);
            if (lane == 0) mask[c0 >> 6] = m;
            t_solid += __popcll(m);
        }
        wave_sync();
        int32_t read_changed = 0;
        for (int32_t p0 = 0; p0 < L; p0 += 64) {
            const int32_t i = p0 + lane;
            const bool un = i < L && !any_bit(mask, max(0, i - k + 1), min(i, n_win - 1));
            const uint64_t um = __ballot(un);
            const int32_t n_u = __popcll(um);
            if (n_u == 0) continue;
            t_untrusted += n_u;
            if (un) ulist[__popcll(um & below)] = i;
            for (int q = lane; q < 192; q += 64) cnt[q] = 0;
            wave_sync();
            const int32_t items = n_u * k3;  // <= 64 * 93
            for (int32_t e0 = 0; e0 < items; e0 += 64) {
                const int32_t e = e0 + lane;
                const bool item = e < items;
                const int32_t u = item ? e / k3 : 0, rem = e - u * k3, t = item ? rem / k : 0, j = rem - t * k;
                bool sol = false;
                if (item) {
                    const int32_t pi = ulist[u];
                    const int32_t c = ovl_spec_code(s[pi]);
                    const int32_t o = max(0, pi - k + 1) + j;
                    if (c >= 0 && o <= min(pi, n_win - 1)) {
                        const uint64_t key = keys[o];
                        sol = key != kSpecNoKey && solid(g, ovl_spec_replace(key, k, o, pi, (c + 1 + t) & 3));
                    }
                }
                if (BALLOT) {
                    const uint64_t m = __ballot(sol);
                    if (item && (j == 0 || lane == 0)) {  // the segment's lanes of this step: [lane, lane + k - j)
                        const int32_t n = min(k - j, 64 - lane);  // 1 .. 31
                        const int32_t add = __popcll(m & (((1ull << n) - 1ull) << lane));
                        if (add) cnt[u * 3 + t] += add;
                    }
                    wave_sync();  // the next step's head may add to the same counter from another lane
                } else if (sol) {
                    atomicAdd(&cnt[u * 3 + t], 1);
                }
            }
            wave_sync();
            bool ch = false, tie = false;
            if (lane < n_u) {
                const int32_t pi = ulist[lane];
                const int32_t c = ovl_spec_code(s[pi]);
                if (c >= 0) {
                    const int32_t s0 = cnt[lane * 3], s1 = cnt[lane * 3 + 1], s2 = cnt[lane * 3 + 2];
                    const int32_t best = max(s0, max(s1, s2));
                    const int32_t n_best = (s0 == best) + (s1 == best) + (s2 == best);
                    if (best >= 1 && n_best == 1) {
                        const int32_t t = s0 == best ? 0 : (s1 == best ? 1 : 2);
                        g.out[base + pi] = ovl_spec_base((c + 1 + t) & 3);  // pi < L: inside read r
                        ch = true;
                    } else if (best >= 1) {
                        tie = true;
                    }
                }
            }
            read_changed += __popcll(__ballot(ch));
            t_ties += __popcll(__ballot(tie));
            wave_sync();  // the next 64 positions overwrite ulist and cnt
        }
        if (lane == 0) g.changed[r] = read_changed;
        t_changed += read_changed;
        wave_sync();  // the next read's keys overwrite these
    }
    if (lane == 0) {
        if (t_solid) atomicAdd(&g.ctr[2], t_solid);
        if (t_untrusted) atomicAdd(&g.ctr[3], t_untrusted);
        if (t_changed) atomicAdd(&g.ctr[4], t_changed);
        if (t_ties) atomicAdd(&g.ctr[5], t_ties);
    }
}

static unsigned grid_for(int64_t threads, int64_t cap) {
    int64_t b = (threads + 255) / 256;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}

}  // namespace ovl_spec

using namespace ovl_spec;

extern "C" hipError_t ovl_spectrum_temp_bytes(int64_t n_win, int32_t k, size_t* bytes) {
    size_t s1 = 0, s2 = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortKeys(nullptr, s1, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                     (int)n_win, 0, 2 * k + 1);
    if (e != hipSuccess) return e;
    e = hipcub::DeviceScan::ExclusiveSum(nullptr, s2, (const int32_t*)nullptr, (int32_t*)nullptr, (int)n_win);
    if (e != hipSuccess) return e;
    *bytes = s1 > s2 ? s1 : s2;
    return hipSuccess;
}

extern "C" hipError_t ovl_launch_spectrum_keys(const OvlSpectrumArgs* g, hipStream_t stream) {
    if (g->n_reads <= 0 || g->n_win <= 0) return hipSuccess;
    key_kernel<<<grid_for((int64_t)g->n_reads * 64, 16384), 256, 0, stream>>>(*g);
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_spectrum_sort(const OvlSpectrumArgs* g, void* temp, size_t temp_bytes,
                                               hipStream_t stream) {
    if (g->n_win <= 0) return hipSuccess;
    return hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, (const uint64_t*)g->keys, g->sorted, (int)g->n_win, 0,
                                             2 * g->k + 1, stream);
}

extern "C" hipError_t ovl_launch_spectrum_heads(const OvlSpectrumArgs* g, void* temp, size_t temp_bytes,
                                                hipStream_t stream) {
    if (g->n_win <= 0) return hipSuccess;
    const unsigned grid = grid_for(g->n_win, 8192);
    head_kernel<<<grid, 256, 0, stream>>>(*g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, (const int32_t*)g->flag, g->pos, (int)g->n_win, stream);
    if (e != hipSuccess) return e;
    scatter_kernel<<<grid, 256, 0, stream>>>(*g);
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_spectrum_counts(const OvlSpectrumArgs* g, hipStream_t stream) {
    if (g->n_distinct <= 0) return hipSuccess;
    if (g->bins < 4 || g->bins > kSpecHistBins) return hipErrorInvalidValue;
    counts_kernel<<<grid_for(g->n_distinct, 1024), 256, 0, stream>>>(*g);
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_spectrum_correct(const OvlSpectrumArgs* g, int32_t max_blocks, hipStream_t stream) {
    if (g->n_reads <= 0 || g->n_win <= 0) return hipSuccess;
    if (g->max_win < 1 || g->max_win > kSpecMaxWindows) return hipErrorInvalidValue;
    const size_t per_wave = wave_words(g->max_win) * sizeof(uint64_t);
    const int waves = 4 * per_wave <= 65536 ? 4 : 1;
    const size_t lds = per_wave * waves;
    if (lds > 65536) {  // one wavefront of the longest reads: 64 KiB of keys and 2 KiB beside them
        const hipError_t e = hipFuncSetAttribute(
            g->ballot ? reinterpret_cast<const void*>(&correct_kernel<true>)
                      : reinterpret_cast<const void*>(&correct_kernel<false>),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    int64_t blocks = ((int64_t)g->n_reads + waves - 1) / waves;
    if (blocks > max_blocks) blocks = max_blocks;
    if (blocks < 1) blocks = 1;
    if (g->ballot) correct_kernel<true><<<(unsigned)blocks, 64u * waves, lds, stream>>>(*g);
    else correct_kernel<false><<<(unsigned)blocks, 64u * waves, lds, stream>>>(*g);
    return hipGetLastError();
}
