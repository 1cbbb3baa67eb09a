// ovl_layout.h — the launches of ovl_layout.hip as ovl_layout_api.cpp drives them, and the key both sides (and the
// host form) build: one statement of how a pair and a read become a 64-bit word that an integer maximum orders.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// The key of pair p with `score`: greater score first, then smaller p.  Never 0 (p < 2^31), so 0 means "no pair";
// around a cycle the least key is the least score and, among those, the greatest p.
__host__ __device__ inline unsigned long long ovl_layout_key(int32_t score, uint32_t p) {
    return ((unsigned long long)((uint32_t)score ^ 0x80000000u) << 32) | (uint32_t)~p;
}
__host__ __device__ inline int32_t ovl_layout_key_pair(unsigned long long key) { return (int32_t)~(uint32_t)key; }
// The head key of read r with `span` (0 <= span < 2^31): greater span first, then smaller r.  Never 0.
__host__ __device__ inline unsigned long long ovl_layout_head_key(int32_t span, uint32_t r) {
    return ((unsigned long long)(uint32_t)span << 32) | (uint32_t)~r;
}
constexpr unsigned long long kLayoutNoKey = ~0ull;  // the identity of the minimum around a cycle

// Doubling levels for n reads: the least L with 2^L >= n (0 for n <= 1).
inline int32_t ovl_layout_levels(int32_t n) {
    int32_t L = 0;
    while (L < 31 && (int64_t(1) << L) < n) ++L;
    return L;
}

// Everything lives in device memory.  Per pair: a, b, score, end.  Per read: len; best (zeroed by the caller before
// the link kernel); link, succ; jump, levels + 1 tables of n (table k: the read 2^k links on, a root standing for
// itself); mk and tail, two tables each that the levels write in turn (the minimum key and the sum of
// len[succ] - end over those links); headkey (zeroed before the head kernel); scan_in / scan_out (the rank and the
// start of every root's contig, packed as rank << 32 | start; they may share mk's memory: the doubling is over
// when they are written); contig, offset, on_path, on_cycle; c_off (n + 1).  ctr: {cycles cut, links, on-path reads,
// nodes seen on a cycle, n_contigs, contig bytes}.
struct OvlLayoutArgs {
    int32_t n;
    int32_t levels;
    int64_t n_pairs;
    const int32_t* len;
    const int32_t* a;
    const int32_t* b;
    const int32_t* score;
    const int32_t* end;
    int32_t min_score, min_overlap;
    unsigned long long* best;
    int32_t* link;
    int32_t* succ;
    int32_t* jump;
    unsigned long long* mk[2];
    uint32_t* tail[2];
    unsigned long long* headkey;
    int64_t* scan_in;
    int64_t* scan_out;
    int32_t* contig;
    int32_t* offset;
    uint8_t* on_path;
    uint8_t* on_cycle;
    int64_t* c_off;
    unsigned long long* ctr;
    // the reads' bytes for the spelling: read r is seqs[off[r] .. off[r] + len[r]), each byte through `table` when
    // that is not NULL (the resident reads are held as symbol codes)
    const uint8_t* seqs;
    const int64_t* off;
    const uint8_t* table;
    uint8_t* bases;     // NULL: nothing is spelled
    int64_t bases_cap;  // bytes of `bases` (sum len): the spelling stores nothing at or past it
};

// best[a] = max key over a's eligible pairs.  runs != 0: runs of equal a inside a wavefront are reduced first and
// issue one atomic each; 0: one atomic per eligible pair.
extern "C" hipError_t ovl_launch_layout_link(const OvlLayoutArgs* g, int32_t runs, hipStream_t stream);
// link, succ from best (resolve != 0; else they are taken as they stand, after a cut), then level 0 of the tables
// and the levels' doubling; the final tables are jump[levels], mk[levels & 1], tail[levels & 1]
extern "C" hipError_t ovl_launch_layout_double(const OvlLayoutArgs* g, int32_t resolve, hipStream_t stream);
// marks the nodes on cycles (ctr[3] counts them) and cuts every cycle at its least key (ctr[0] counts the cuts)
extern "C" hipError_t ovl_launch_layout_cut(const OvlLayoutArgs* g, hipStream_t stream);
// heads, contig ranks and starts (through `temp`, ovl_layout_scan_bytes of it), placement, the path marks from the
// highest level down and the counts; then the spelling
extern "C" hipError_t ovl_layout_scan_bytes(int32_t n, size_t* bytes);
extern "C" hipError_t ovl_launch_layout_place(const OvlLayoutArgs* g, void* temp, size_t temp_bytes,
                                              hipStream_t stream);
extern "C" hipError_t ovl_launch_layout_spell(const OvlLayoutArgs* g, int32_t waves, hipStream_t stream);
