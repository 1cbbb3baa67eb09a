// ovl_kernels.h — launch interface between the C ABI's host files (ovl_ctx.h) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Scoring kernels flag a pair index outside [0, n_reads): a relaxed system-scope store of 1 (idempotent,
// so no read-modify-write), because for host-array calls the flag is pinned host memory that the host
// reads after the call's synchronisation.
__device__ __forceinline__ void ovl_flag_error(uint32_t* flag) {
    __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct OvlUngappedArgs {
    const uint32_t* sfx;
    const uint32_t* pfx;
    const int32_t* len;
    int32_t n_reads;
    const int32_t* a_idx;
    const int32_t* b_idx;
    int64_t n_pairs;
    int32_t rs_log2;     // lanes per pair = 1 << rs_log2 (splits the bit shifts r)
    int32_t match;
    int32_t mismatch;
    int32_t* out_score;
    int32_t* out_end;
    uint32_t* err_flag;
    int32_t planes;      // 2, 4 or 8 bit planes per base
    int32_t wmax;        // W = 1..8 words of 32 bases (read length <= 32*W)
    int32_t key64;       // 64-bit (score, end) keys (else 32-bit folded keys)
    int32_t lw;          // dominant read length for uniform_kernel (0: general kernel only)
    const uint32_t* full; // bit r set iff len[r] == lw
    int64_t max_blocks;  // grid cap (grid-stride beyond it)
    const int32_t* heavy_ids;   // throughput mode over a resident candidate list: heavy tiles first (list tile
    const uint8_t* tile_flags;  // ids, ascending; per-list-tile flags); null: natural order
    int32_t heavy_n;            // heavy tiles of this launch: heavy_ids[0 .. heavy_n)
    int64_t tile_base;          // the launch's first pair / 64 within the list
    const uint16_t* ix_b16;  // non-null: uniform_kernel (throughput mode, int32 keys) reads a compact pair list
    const uint8_t* ix_d8;    // instead of a_idx / b_idx: b = ix_b16[p] (0xFFFF: a bad index), a = ix_base[p / 64]
    const int32_t* ix_base;  // + ix_d8[p]; the host pool encodes each chunk (ovl_pipeline.cpp encode_chunk) and the
                             // copy engine moves it into HBM on the second stream, where the kernel reads it
    int32_t host_out;    // result sink of uniform_kernel (put_pair): 0 int32 arrays in HBM, 1 host-mapped int32
                         // arrays (non-temporal stores), 2 host-mapped packed (end, mismatches) per pair in
                         // out_score as uint16, the score of the few pairs that need it in out_end
    hipEvent_t ev_start; // non-null (timing): uniform_kernel's launch records these at the kernel's own start and
    hipEvent_t ev_stop;  // end (hipExtLaunchKernelGGL), without the dispatch wait that stream events include
};

// kernels of the band knob (ovl_launch_dp); OVL_BAND_FORM env picks one for tests
enum {
    OVL_BAND_FORM_STRIP = 0,  // dp_kernel<int32_t, true>: any length, one row per lane, masks per cell
    OVL_BAND_FORM_ROWS = 1,   // band_row_kernel: lanes on band diagonals, a row per step (<= 192 lanes)
    OVL_BAND_FORM_FAST = 2,   // dp_fast_kernel<int32_t, true>: chunked strips with band masks
    OVL_BAND_FORM_DIAG = 3,   // band_diag_kernel: lanes on band diagonals, an anti-diagonal per step
    OVL_BAND_FORM_LANE = 4,   // band_lane_kernel (a lane per pair, band diagonals in registers) or, from
                              // kBandLane2Min, band_lane2_kernel (two lanes per pair, one row apart)
    OVL_BAND_FORM_LANE1 = 5,  // band_lane_kernel at every width it has (tests, A/B)
    OVL_BAND_FORM_LANE2 = 6,  // band_lane2_kernel at every width it has (tests, A/B)
};

struct OvlDpArgs {
    const uint8_t* codes;
    const int64_t* off;
    const int32_t* len;
    int32_t n_reads;
    const int32_t* a_idx;
    const int32_t* b_idx;
    int64_t n_pairs;
    int32_t mcap;        // longest t read (LDS row capacity)
    int64_t match;
    int64_t mismatch;
    int64_t indel;
    int32_t* out_score;
    int32_t* out_end;
    int8_t* tb;          // optional traceback (single pair)
    uint32_t* err_flag;
    int32_t wide;        // int64 arithmetic (else int32, when magnitudes allow)
    int32_t band;        // < 0: full DP; >= 0: banded around the seed diagonal n - seed[pair]
    const int32_t* seed; // banded: the seed ends j* (device memory, never aliases out_*)
    int32_t band_form;   // banded: OVL_BAND_FORM_* -- the host checks each form's limits
    int32_t classic;     // full DP without traceback: use dp_kernel instead of dp_fast_kernel (tests)
};

// 2-bit packed ACGT bytes (base i at bits 2(i % 4) of byte i / 4; pk 16-byte aligned, readable up to the next
// 16-byte boundary) -> codes[i] = lut["ACGT"[code]]
extern "C" hipError_t ovl_launch_unpack2(const uint8_t* pk, const uint8_t* lut, uint8_t* codes, int64_t n,
                                         hipStream_t stream);
extern "C" hipError_t ovl_launch_map_codes(const uint8_t* raw, const uint8_t* lut, uint8_t* codes, int64_t n,
                                           hipStream_t stream);
extern "C" hipError_t ovl_launch_pack(int planes, const uint8_t* codes, const int64_t* off, const int32_t* len,
                                      int32_t n_reads, int32_t w, int32_t srow, int32_t trow, uint32_t* sfx,
                                      uint32_t* pfx, hipStream_t stream);
extern "C" hipError_t ovl_launch_ungapped(const OvlUngappedArgs* args, hipStream_t stream);
// flags[t] = 1 iff tile t of the pair list holds a pair whose read a is shorter than the dominant length
extern "C" hipError_t ovl_launch_tile_flags(const int32_t* a_idx, int64_t n_pairs, const uint32_t* full,
                                            int32_t n_reads, uint8_t* flags, hipStream_t stream);

extern "C" hipError_t ovl_launch_dp(const OvlDpArgs* args, hipStream_t stream);
// the band knob's row and anti-diagonal forms (ovl_band.hip): internal, reached only through ovl_launch_dp's
// form switch (ovl_dp.hip)
namespace ovl {
hipError_t launch_band_rows(const OvlDpArgs* args, hipStream_t stream);
hipError_t launch_band_diag(const OvlDpArgs* args, hipStream_t stream);
}  // namespace ovl
// compact host pair lists (ovl_pairs.hip): dst[i] = src[i] from 2- or 4-byte elements (uint16 0xFFFF -> -1; src and
// dst 16-byte aligned), and runs: dst[starts[r] .. starts[r + 1]) = vals[r]
extern "C" hipError_t ovl_launch_widen(const void* src, int32_t width, int64_t n, int32_t* dst, hipStream_t stream);
extern "C" hipError_t ovl_launch_runs(const int32_t* vals, const int32_t* starts, int64_t n_runs, int32_t* dst,
                                      hipStream_t stream);
extern "C" int ovl_band_diag_slots(int32_t band, int32_t lcap, int32_t* nseg_out);
// lane-per-pair full DP (ovl_dp_lane.hip): colbuf holds slots x ovl_dp_lane_rcap(mcap) x 64 dwords
struct OvlLaneArgs {
    int32_t cw;                 // strip width: 16 or 32 columns
    int32_t prof;               // byte score profile (<= 4 symbols, diagonal scores in int8, indel <= 0)
    int32_t ho;                 // hand-off column: 0 int32 in HBM, 1 int16 in HBM (|G| < 2^15), 2 4-bit steps
                                // in LDS (sfx, cw 32, max(match, mismatch) - 2*indel <= 15, lmax <= 256)
    int32_t sfx;                // (prof) row symbols from the resident suffix bit planes
    const uint32_t* sfx_words;  // sfx / pfx layouts of ovl_set_reads (2 planes), srow words per read, wsfx words
    const uint32_t* pfx_words;
    int32_t srow;
    int32_t wsfx;
    uint32_t* colbuf;
    int64_t slots;              // resident wavefront slots (one hand-off column each)
    int32_t split;              // band knob: two lanes per pair (band_lane2_kernel) instead of one
    int32_t h2;                 // full DP (prof, sfx, ho 2): two pairs per lane as packed f16 cells
                                // (dp_lane_h2_kernel; the diagonal scores' f16 encodings end in a zero byte)
};
extern "C" int32_t ovl_dp_lane_rcap(int32_t lcap);
extern "C" int32_t ovl_dp_lane_waves_per_simd(int32_t cw);
extern "C" int32_t ovl_dp_lane_lds_bytes(int32_t lcap);
extern "C" int32_t ovl_dp_lane_h2_ok(int64_t match, int64_t mismatch, int64_t indel);
extern "C" int64_t ovl_dp_lane_h2_col_bytes(int64_t n_pairs, int32_t lcap);
extern "C" hipError_t ovl_launch_dp_lane(const OvlDpArgs* args, const OvlLaneArgs* lane, hipStream_t stream);
// band knob, a lane per pair (ovl_dp_lane.hip): ovl_band_lane_ok(band), <= 4 symbols, scores in int8;
// uses lane->split, and lane->sfx (row symbols and t codes from the bit planes) with sfx/pfx_words
extern "C" int32_t ovl_band_lane_ok(int32_t band);
extern "C" hipError_t ovl_launch_band_lane(const OvlDpArgs* args, const OvlLaneArgs* lane, hipStream_t stream);

// candidate enumeration (ovl_candidates.hip)
extern "C" hipError_t ovl_cand_keys(const uint8_t* codes, const int64_t* off, const int32_t* len, int32_t n_reads,
                                    int32_t k, int32_t bits, uint64_t* pre_key, uint64_t* suf_key, int32_t* iota,
                                    hipStream_t stream);
extern "C" hipError_t ovl_cand_temp_bytes(int32_t n_reads, size_t* bytes);
extern "C" hipError_t ovl_cand_sort(void* temp, size_t temp_bytes, const uint64_t* keys_in, uint64_t* keys_out,
                                    const int32_t* vals_in, int32_t* vals_out, int32_t n_reads, hipStream_t stream);
extern "C" hipError_t ovl_cand_count(const uint64_t* sorted, const uint64_t* pre_key, const uint64_t* suf_key,
                                     int32_t n_reads, int32_t all_pairs, int64_t* lo, int64_t* hi, int64_t* cnt,
                                     hipStream_t stream);
extern "C" hipError_t ovl_cand_scan(void* temp, size_t temp_bytes, const int64_t* cnt, int64_t* offs, int32_t n_reads,
                                    hipStream_t stream);
extern "C" hipError_t ovl_cand_emit(const int32_t* order, const int64_t* lo, const int64_t* hi, const int64_t* offs,
                                    int32_t n_reads, int32_t all_pairs, int32_t* out_a, int32_t* out_b,
                                    hipStream_t stream);

// seed candidates (ovl_candidates.hip, ovl_seed_candidates): every k-mer of a read at offsets >= 1 looked up among
// the prefix keys.  ovl_seed_keys writes the prefix keys (~0 for a read shorter than k) and the identity for
// ovl_cand_sort; ovl_seed_count the per-read pair counts (and, keep != 0, every offset's group into grp_lo / grp_n,
// indexed off[a] + offset - 1); ovl_seed_emit the list at offs (ovl_cand_scan of the counts), its groups taken from
// grp_lo / grp_n (keep != 0) or searched again.  max_off = lmax - k, the most offsets a read has: a wavefront holds
// that many keys in LDS, at most OVL_SEED_MAX_OFFSETS (64 KiB).
#define OVL_SEED_MAX_OFFSETS 8192
struct OvlSeedArgs {
    const uint8_t* codes;
    const int64_t* off;
    const int32_t* len;
    int32_t n_reads, k, bits;
    const uint64_t* sorted;   // the sorted prefix keys, of which the first n_long are reads with len >= k
    const int32_t* order;     // their reads
    int32_t n_long;
    const uint64_t* pre_key;  // per read
    int32_t max_off;
    int32_t* grp_lo;          // per base: the group of the offset's key (keep)
    int32_t* grp_n;
    int64_t* cnt;             // per read: its pairs
    const int64_t* offs;      // per read: its first output slot
    int32_t* out_a;
    int32_t* out_b;
    int32_t* out_o;
};
extern "C" hipError_t ovl_seed_keys(const uint8_t* codes, const int64_t* off, const int32_t* len, int32_t n_reads,
                                    int32_t k, int32_t bits, uint64_t* pre_key, int32_t* iota, hipStream_t stream);
extern "C" hipError_t ovl_seed_count(const OvlSeedArgs* s, int32_t keep, hipStream_t stream);
extern "C" hipError_t ovl_seed_emit(const OvlSeedArgs* s, int32_t keep, hipStream_t stream);

// local alignment (ovl_local.hip)
// rowbuf: n_strips x (64 * n_chunks + 64) words {value, epoch}, n_chunks = (m + 126) / 64; tb (nullable):
// n_strips x 64 * n_chunks x 64 bytes, [strip][tau][lane]
extern "C" hipError_t ovl_launch_local(const uint8_t* q, int32_t n, const uint8_t* r, int32_t m, int64_t match,
                                       int64_t mismatch, int64_t indel, int32_t wide, uint64_t* rowbuf, int8_t* tb,
                                       unsigned long long* best, uint32_t* err_flag, int32_t blocks, uint32_t epoch,
                                       hipStream_t stream);

// batched local alignment (ovl_local_batch.hip): `waves` one-wavefront blocks take items[0 .. n_items) from
// *counter (zeroed by the caller).  Item k aligns q[q_off .. q_off + n) to ref[win_lo .. win_lo + m), n, m >= 1,
// in int32 cells.  Per wavefront w: rows + w * row_pitch (int32; row_pitch 0: the row lives in the launch's
// lds_row_bytes of dynamic LDS), and with a traceback slabs + w * slab_pitch (bytes, >= the largest item's
// n_strips x 64 * n_chunks x 64) and wave_ops + w * wave_ops_pitch (>= the largest n + m).  out: one record per
// item at out[item.out], its ops at ops_base() of `ops` (reserved from *ops_total, zeroed by the caller).
// slabs == NULL: score only (starts = ends, no ops).
struct OvlLocalBatchItem {
    int64_t q_off;
    int32_t n, win_lo, m, out;
};
struct OvlLocalBatchRecord {
    int32_t score, end_i, end_j, start_i, start_j, n_ops;
    uint32_t ops_lo, ops_hi;  // the 64-bit position of the item's ops
    __host__ __device__ unsigned long long ops_base() const {
        return (unsigned long long)ops_lo | ((unsigned long long)ops_hi << 32);
    }
};
static_assert(sizeof(OvlLocalBatchRecord) == 32, "the batch record is eight 32-bit words");
struct OvlLocalBatchArgs {
    const uint8_t* q;
    const uint8_t* ref;
    const OvlLocalBatchItem* items;
    int32_t n_items;
    int32_t match, mismatch, indel;
    uint32_t* counter;
    unsigned long long* ops_total;
    int32_t* rows;
    int64_t row_pitch;
    int8_t* slabs;
    int64_t slab_pitch;
    int8_t* wave_ops;
    int64_t wave_ops_pitch;
    OvlLocalBatchRecord* out;
    int8_t* ops;
};
extern "C" hipError_t ovl_launch_local_batch(const OvlLocalBatchArgs* a, int32_t waves, uint32_t lds_row_bytes,
                                             hipStream_t stream);

// lane-per-read local alignment scores (ovl_local_lane.hip): reads is pitch rows of `rows` symbols (0 .. 254, 255
// beyond the read's r_len; pitch a multiple of 64, 16-byte aligned), contigs the renumbered contig symbols with every
// c_off a multiple of four and readable up to the next multiple of four past its end.  A launch of `groups` =
// pitch / 64 by `split` one-wavefront blocks scores contigs [c_lo, c_hi) and stores tile_score / tile_end
// [(c - c_lo) * pitch + read]: the score and, when it is positive, end_i << 20 | end_j (end_j counted from the
// contig's first column).  Needs mismatch <= 0, indel <= 0, match * rows < 2^23, contigs shorter than 2^20.
// ovl_launch_read_best_fold then folds that tile into the per-read results (first < 0: no contig seen yet) and,
// when tie_bits is not NULL, the rows of `words` = ceil(n_contigs / 32) bit words; c_lo must be a multiple of 32.
struct OvlLocalLaneArgs {
    const uint8_t* reads;
    const int32_t* r_len;
    const uint8_t* contigs;
    const int64_t* c_off;
    const int32_t* c_len;
    int64_t pitch;
    int32_t c_lo, c_hi;
    int32_t read_length;
    int32_t match, mismatch, indel;
    int32_t* tile_score;
    uint32_t* tile_end;
};
constexpr int32_t kLocalLaneMaxRows = 128;
extern "C" hipError_t ovl_launch_local_lane(const OvlLocalLaneArgs* a, int32_t rows, int32_t groups, int32_t split,
                                            hipStream_t stream);
extern "C" hipError_t ovl_launch_read_best_fold(const OvlLocalLaneArgs* a, int32_t n_reads, int32_t words,
                                                int32_t* best, int32_t* first, int32_t* n_best, uint32_t* cell,
                                                uint32_t* tie_bits, hipStream_t stream);

// consensus (ovl_consensus.hip).  pileup: one-wavefront blocks take items[0 .. n_items) of a finished batch launch
// from *counter (zeroed by the caller), read each item's record out[item.out] (end_i, end_j = bi, bj; n_ops = cnt;
// ops_base() = base) and its walk ops[base .. base + cnt) (1 diag, 2 up, 3 left from cell (bi, bj)), and add one
// vote per op to counts[(item.win_lo + column) * 6 + channel]: A, C, G, T by the query byte of a diag, 4 for a left,
// 5 for an up.
// ctr[0] counts the diag ops whose byte is none of ACGT, ctr[2] the ops that fell outside their item (none, unless
// the walk is broken; they cast no vote).  add: counts[hits[i]] += 1.  vote: called[b] for b < n_bases from
// counts[6 * b ..] and ref[b] (the largest of the four base channels once they hold min_depth votes; ties to the
// contig's own byte, else the first of A, C, G, T), ctr[1] += the bases that changed.
struct OvlPileupArgs {
    const OvlLocalBatchItem* items;
    const uint8_t* q;
    const OvlLocalBatchRecord* out;
    const int8_t* ops;
    int32_t n_items;
    uint32_t* counter;
    int32_t* counts;
    unsigned long long* ctr;
};
extern "C" hipError_t ovl_launch_consensus_pileup(const OvlPileupArgs* a, int32_t waves, hipStream_t stream);
extern "C" hipError_t ovl_launch_consensus_add(const int64_t* hits, int64_t n_hits, int32_t* counts,
                                               hipStream_t stream);
extern "C" hipError_t ovl_launch_consensus_vote(const uint8_t* ref, const int32_t* counts, int64_t n_bases,
                                                int32_t min_depth, uint8_t* called, unsigned long long* ctr,
                                                hipStream_t stream);

// placed consensus (ovl_consensus_placed.hip): one lane per item, an item being a read that has a window on its
// contig (include/ovl.h, ovl_consensus_placed: the rule).  Lane g of the launch takes items[g]: its bytes are
// q[q_off .. q_off + L), its window is ref[col0 .. col0 + w), whose first base is column lo of its contig, and d is
// its placement's diagonal (offset - lo).  The lane fills the 2 * slack + 1 diagonals of the band row by row in
// registers, writes each row's codes (2 bits per diagonal) as one 64-bit word to slab[(row - 1) * pitch + g]
// (pitch >= n_items, rows up to the longest item of the launch), and, when its best score reaches min_vote_score,
// walks its own words back and adds `weight` per op to counts[(col0 + column) * 6 + channel] and writes
// aln[3 * read ..] = (score, lo + stop column, lo + best column).  ctr[0] += weight per diag op whose byte is none of
// ACGT, ctr[3] += the items that voted, ctr[4] += their ops.  The scores are int32: the caller clamps negative ones
// at -2^30 and keeps max(0, scores) * (L + w) below 2^30.
struct OvlPlacedItem {
    int64_t q_off;
    int32_t L, w, d, col0, lo, weight, read, pad;
};
struct OvlPlacedArgs {
    const OvlPlacedItem* items;
    const uint8_t* q;
    const uint8_t* ref;
    unsigned long long* slab;
    int32_t n_items, pitch;
    int32_t slack, match, mismatch, indel, min_vote_score;
    int32_t* counts;
    int32_t* aln;
    unsigned long long* ctr;
};
constexpr int32_t kPlacedMaxSlack = 15;  // 31 diagonals: 62 bits of codes per row
extern "C" hipError_t ovl_launch_consensus_placed(const OvlPlacedArgs* a, hipStream_t stream);

// transitive reduction of an overlap graph (ovl_reduce.hip): `blocks` persistent workgroups of kReduceThreads take
// order[0 .. n_order) -- the nodes with out-edges, heaviest first by two-hop work -- from *counter (zeroed by the
// caller).  edge[e] = {head, weight} of CSR edge e (heads validated in [0, n_nodes), |weight| < 2^30); a window of
// `window` entries of the current node's out-row lives in the launch's 4 * window bytes of dynamic LDS; `group`
// (a power of two, 8 .. 64) lanes share one successor's list, kReduceLoads entries per lane and trip.
// reduced[e] is written for every edge.
constexpr int kReduceThreads = 512;
constexpr int kReduceLoads = 4;  // entries of a successor list a lane loads per trip, all in flight before the first is used
struct OvlReduceArgs {
    const int64_t* off;
    const int2* edge;
    const int32_t* order;
    int32_t n_nodes, n_order;
    int32_t window, group;
    uint32_t* counter;
    uint8_t* reduced;
};
extern "C" hipError_t ovl_launch_reduce(const OvlReduceArgs* a, int32_t blocks, hipStream_t stream);

// reachability reduction of a string graph (ovl_reach.hip): matrix is n_nodes rows of `words` = ceil(n_nodes / 64)
// uint64 (bit x of row u: a path of at least one edge from u to x), pivot 64 rows of the same width.  In stream
// order: fill (the rows from the CSR; heads validated in [0, n_nodes)), then for K = 0 .. words - 1 pivot and
// update (`group` lanes per row: a power of two, 1 .. 64), then mark over order[0 .. n_order) -- the nodes with at
// least two out-edges, heaviest first -- with `group` lanes per node holding kReachAccWords words each of a column
// window of window_words <= min(words, group * kReachAccWords) words (window_words <= group: one word per lane and
// kReachAhead * kReachAccWords rows in flight).  mark stores reduced[e] for every edge of those nodes.
constexpr int kReachLoads = 16;    // pivot rows a lane of update loads per trip over a dense pivot word, all in
                                   // flight before the first OR (four per trip over a sparse one)
constexpr int kReachAhead = 4;     // successors whose rows a lane of mark loads before the first is used
                                   // (kReachAhead * kReachAccWords where a lane holds one word of acc)
constexpr int kReachAccWords = 4;  // words of acc per lane of mark
struct OvlReachArgs {
    const int64_t* off;
    const int32_t* head;
    const int32_t* order;
    int32_t n_nodes, n_order;
    int32_t words;
    uint64_t* matrix;
    uint64_t* pivot;
    uint8_t* reduced;
};
extern "C" hipError_t ovl_launch_reach_fill(const OvlReachArgs* a, hipStream_t stream);
extern "C" hipError_t ovl_launch_reach_pivot(const OvlReachArgs* a, int32_t K, hipStream_t stream);
extern "C" hipError_t ovl_launch_reach_update(const OvlReachArgs* a, int32_t K, int32_t group, hipStream_t stream);
extern "C" hipError_t ovl_launch_reach_mark(const OvlReachArgs* a, int32_t group, int32_t window_words,
                                            hipStream_t stream);

// shard bounds of a pair list balanced by len[a]*len[b] + 1 (ovl_candidates.hip): ovl_shard_scan writes
// the inclusive prefix sum of the costs (n_pairs int64), ovl_shard_cut the shards + 1 cuts of [lo, hi)
extern "C" hipError_t ovl_shard_temp_bytes(int64_t n_pairs, size_t* bytes);
extern "C" hipError_t ovl_shard_scan(void* temp, size_t temp_bytes, const int32_t* a, const int32_t* b,
                                     const int32_t* len, int64_t n_pairs, int64_t* cum, hipStream_t stream);
extern "C" hipError_t ovl_shard_cut(const int64_t* cum, int64_t lo, int64_t hi, int32_t shards, int64_t* cuts,
                                    hipStream_t stream);
