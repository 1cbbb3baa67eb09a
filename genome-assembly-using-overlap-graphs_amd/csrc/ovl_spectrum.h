// ovl_spectrum.h — what ovl_spectrum.hip and ovl_spectrum_api.cpp share: the code of a byte, the field of a key that a
// substitution replaces (one statement for the kernels and the host form), the device limits and the launches.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int32_t kSpecMaxK = 31;
constexpr int32_t kSpecMaxWindows = 8192;  // windows of one read on the device: 64 KiB of keys in LDS
constexpr int32_t kSpecHistBins = 1024;    // most bins of the device histogram of the counts (OvlSpectrumArgs::bins)
constexpr uint64_t kSpecNoKey = ~0ull;     // a window without a key; above every key (keys are < 2^62)

// A = 0, C = 1, G = 2, T = 3; any other byte has no code (-1)
__host__ __device__ inline int32_t ovl_spec_code(uint8_t c) {
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
}
__host__ __device__ inline uint8_t ovl_spec_base(int32_t code) { return (uint8_t)(0x54474341u >> (8 * code)); }
// the key of a window at offset o with the base at position i (o <= i < o + k) replaced by code x
__host__ __device__ inline uint64_t ovl_spec_replace(uint64_t key, int32_t k, int32_t o, int32_t i, int32_t x) {
    const int32_t sh = 2 * (k - 1 - (i - o));
    return (key & ~(3ull << sh)) | ((uint64_t)x << sh);
}
// one more base rolled into a window's key; `good` counts the coded bytes since the last byte without a code, so
// the window ending at this byte has a key iff good >= k
__host__ __device__ inline void ovl_spec_roll(uint64_t& key, int32_t& good, uint8_t byte, uint64_t mask) {
    const int32_t c = ovl_spec_code(byte);
    good = c < 0 ? 0 : good + 1;
    key = ((key << 2) | (uint64_t)(c & 3)) & mask;
}

// Everything in device memory.  Read r is seqs[off[r] .. off[r+1]); its windows' keys are keys[woff[r] .. woff[r+1]),
// woff the scan of max(len - k + 1, 0); n_win = woff[n_reads] < 2^31.  sorted: the keys sorted; flag / pos: the head
// flags of the runs and their exclusive scan; starts[j]: where run j begins (n_win + 2 entries); spec_keys /
// spec_counts: the spectrum (n_distinct entries once the count pass has run).  hist: kSpecHistBins entries.
// ctr: {0 distinct, 1 unused, 2 solid windows, 3 untrusted positions, 4 changed, 5 ties, 6 greatest count, 7 k-mers}.
struct OvlSpectrumArgs {
    int32_t n_reads, k, max_win, n_distinct, min_count;
    int32_t bins;  // of hist, 4 .. kSpecHistBins: bin c holds count c for c < bins - 1, the last bin every greater count
    int32_t ballot;  // the correction pass counts solid work items by ballot (else one LDS atomic each)
    int64_t n_win;
    const uint8_t* seqs;
    const int64_t* off;
    const int64_t* woff;
    uint64_t* keys;
    uint64_t* sorted;
    int32_t* flag;
    int32_t* pos;
    int32_t* starts;
    uint64_t* spec_keys;
    int32_t* spec_counts;
    uint32_t* hist;
    unsigned long long* ctr;
    uint8_t* out;      // the corrected bytes, a copy of seqs when the correction pass starts
    int32_t* changed;  // per read
};

extern "C" hipError_t ovl_spectrum_temp_bytes(int64_t n_win, int32_t k, size_t* bytes);
extern "C" hipError_t ovl_launch_spectrum_keys(const OvlSpectrumArgs* g, hipStream_t stream);
extern "C" hipError_t ovl_launch_spectrum_sort(const OvlSpectrumArgs* g, void* temp, size_t temp_bytes,
                                               hipStream_t stream);
// head flags, their scan and the scatter of (key, run start); ctr[0] = distinct keys
extern "C" hipError_t ovl_launch_spectrum_heads(const OvlSpectrumArgs* g, void* temp, size_t temp_bytes,
                                                hipStream_t stream);
// run lengths from the starts (g->n_distinct known), the histogram of the counts, ctr[6] and ctr[7]
extern "C" hipError_t ovl_launch_spectrum_counts(const OvlSpectrumArgs* g, hipStream_t stream);
extern "C" hipError_t ovl_launch_spectrum_correct(const OvlSpectrumArgs* g, int32_t max_blocks, hipStream_t stream);
