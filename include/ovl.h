/*
 * ovl.h — C ABI of the MI355X-native overlap-scoring engine (libovl.so).
 *
 * Replaces the per-pair Python->Numba boundary of the reference:
 *   overlapGraphs.py:53   overlap_alignment(read_a, read_b) once per candidate pair
 *   aligners.py:6-82      @njit overlap_alignment(s, t, match_score=10, mismatch=-1, indel=-2**31)
 * with one batched call per candidate list.  Only (score, end) reach the
 * graph (overlapGraphs.py:53-60), so that is what the batch entry points return.
 *
 * Conventions
 *  - Plain C types only; the caller owns every pointer it passes in.
 *  - Return value 0 (OVL_OK) on success, a negative OVL_E_* code on failure;
 *    ovl_last_error() then describes it.  Nothing throws or aborts across the ABI.
 *  - One call at a time per ovl_ctx.  Contexts are independent.  A context
 *    drives one or more GPUs from the calling thread: host-array
 *    scoring calls shard the pair list over its devices (contiguous ranges
 *    balanced by sum len(a)*len(b)) and every device writes its range of the
 *    results straight into the caller's arrays.  joblib-style multi-process
 *    callers create one single-device context per process.
 *  - Host arrays may be pageable or pinned (ovl_host_alloc / ovl_host_register /
 *    hipHostMalloc).  Pinned arrays are read and written by DMA in place;
 *    pageable ones go through pinned staging.  Either way copies, kernels and
 *    result copies of consecutive chunks overlap.
 *  - Read i is the byte string seqs[offsets[i] .. offsets[i+1]).  Bytes are
 *    symbols compared for equality only (any alphabet of <= 256 symbols).
 *  - Semantics are the reference's: DP fill of aligners.py:27-48 with int64
 *    arithmetic and int32 stores, last-row strict-'>' first argmax of
 *    aligners.py:50-57.  score >= 0 and 0 <= end <= len(t) always.
 *  - Graph stages on a CSR of the DiGraph: cycle removal (ovl_remove_cycles, host) and the string pipeline's
 *    transitive reduction (ovl_transitive_reduce, device; overlapGraphs.py:235-303), and the unitig pipeline's
 *    reachability reduction (ovl_reach_reduce, device; overlapGraphs.py:354-367).
 */
#ifndef OVL_H
#define OVL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OVL_ABI_VERSION 4

enum {
    OVL_OK = 0,
    OVL_E_ARG = -1,          /* bad argument (null pointer, negative size, bad offsets) */
    OVL_E_HIP = -2,          /* HIP runtime error */
    OVL_E_OOM = -3,          /* device allocation failed */
    OVL_E_UNSUPPORTED = -4,  /* read too long, >256 symbols, band at scores too large for int32 cells */
    OVL_E_RANGE = -5,        /* scoring magnitudes would overflow the int32 DP table */
    OVL_E_STATE = -6,        /* no resident reads (ovl_set_reads not called) */
    OVL_E_INDEX = -7,        /* a pair index is outside [0, n_reads) */
    OVL_E_INTERNAL = -8      /* a streamed result record never completed although its kernel had finished */
};

enum {
    OVL_KERNEL_NONE = 0,
    OVL_KERNEL_UNGAPPED = 1, /* 2-bit (or 4/8-bit) bit-plane popcount kernel; exact when gaps cannot win */
    OVL_KERNEL_DP = 2,       /* anti-diagonal wavefront DP, int64-exact, any scoring */
    OVL_KERNEL_BANDED = 3    /* ungapped seed + banded DP around its diagonal (band >= 0, gaps can win) */
};

typedef struct ovl_ctx ovl_ctx;

/* ABI version (OVL_ABI_VERSION). */
int ovl_version(void);

/* Number of visible HIP devices. */
int ovl_device_count(int32_t* out_count);

/*
 * Create a context on n_devices GPUs: 0 = every visible device;
 * otherwise the n_devices consecutive devices starting at the calling thread's
 * current device (so 1 = the current device).  The caller's current device is
 * never changed by any entry point.
 */
int ovl_create(int32_t n_devices, ovl_ctx** out_ctx);
/* Create a context on an explicit list of distinct device ordinals (device 0 of the context = devices[0]). */
int ovl_create_on_devices(const int32_t* devices, int32_t n_devices, ovl_ctx** out_ctx);
/* The context's device ordinals: *out_n = count, ids[0 .. min(cap, count)) = ordinals. */
int ovl_ctx_devices(const ovl_ctx* ctx, int32_t* ids, int32_t cap, int32_t* out_n);
int ovl_destroy(ovl_ctx* ctx);

/* Pinned host memory for result / pair arrays (DMA in place, visible to every device). */
int ovl_host_alloc(int64_t bytes, void** out_ptr);
int ovl_host_free(void* ptr);
/* Pin (register) / unpin an existing host range, e.g. a shared-memory result buffer. */
int ovl_host_register(void* ptr, int64_t bytes);
int ovl_host_unregister(void* ptr);

/* Host thread pool of the result transport (expansion of packed results, copies of pageable arrays), recounted
 * now: *cpus = this process's CPUs (affinity set, capped by the cgroup quota), *sharers = processes driving
 * libovl on the same CPU set (other libovl processes of this user with the same affinity, e.g. joblib workers,
 * or LOCAL_WORLD_SIZE when larger), *threads = threads a call uses (ovl_host_pool_rule), *packed = 1 when the
 * packed transport may be used (>= 6 threads; otherwise results cross as int32 and the pool does not poll).
 * Any output pointer may be NULL. */
int ovl_host_pool(int32_t* threads, int32_t* sharers, int32_t* cpus, int32_t* packed);
/* The sizing rule: env_threads > 0 (OVL_POOL_THREADS) wins, else min(12, cpus / sharers - 1), at least 1. */
int32_t ovl_host_pool_rule(int32_t cpus, int32_t sharers, int32_t env_threads);

/* Per-call timing of host-array scoring calls (off by default; on adds HIP timing events):
 * kernel_ms = summed kernel time of the busiest device, call_ms = wall time of the call. */
int ovl_set_timing(ovl_ctx* ctx, int32_t on);
int ovl_last_timing(const ovl_ctx* ctx, double* kernel_ms, double* call_ms);
/* The scoring launches of the last host-array call made with timing on, in issue order: *out_n = count;
 * entry i < cap gives the device ordinal, the result sink (1 int32 stored into host memory; 2 packed 2 B/pair
 * into host staging, expanded by host threads after the launch; 0, HBM, only in ovl_score_device), the pairs and
 * the launch's
 * duration in ms (HIP events recorded by the kernel's own launch for ungapped chunks, else on its stream).
 * Any output pointer may be NULL. */
int ovl_last_launches(const ovl_ctx* ctx, int32_t cap, int32_t* device, int32_t* sink, int64_t* pairs, double* ms,
                      int32_t* out_n);
/* Link traffic of the last host-array scoring call (always recorded): link_bytes = pair-list bytes the
 * devices read from host memory + result bytes they stored there (ovl_last_results: 2 per pair in packed
 * chunks, 8 per pair otherwise; the resident grid's calls 128 per 64-pair tile record plus 8 per special pair; the
 * few pairs of a 2 B/pair chunk whose score travels separately add 4 each and are not counted); packed_pairs =
 * pairs whose results crossed packed and were expanded on the host. */
int ovl_last_transfer(const ovl_ctx* ctx, int64_t* link_bytes, int64_t* packed_pairs);
/* The results' part of the last host-array call's link bytes (always recorded): result_bytes = what the kernels
 * stored into host memory for the results (8 per int32 pair, 2 per packed pair; a resident-grid call 128 per
 * tile record of 64 pairs plus 8 per special pair); record_pairs = pairs that crossed as the resident grid's tile
 * records; escapes = the special pairs among them (a shorter read a inside b's window, or a bad pair), whose word
 * travels apart. */
int ovl_last_results(const ovl_ctx* ctx, int64_t* result_bytes, int64_t* record_pairs, int64_t* escapes);
/* How the last host-array call's pair list reached the kernels (always recorded): in_place_pairs = pairs of
 * chunks the scoring kernel read in their compact encoding (b as uint16, a as tile deltas); decoded_pairs =
 * pairs of compact chunks decoded into HBM first (runs / widen kernels).  Both 0 for a call whose list crossed
 * as the caller's int32 arrays, or that had no host list. */
int ovl_last_pair_list(const ovl_ctx* ctx, int64_t* in_place_pairs, int64_t* decoded_pairs);

/* Last error message of `ctx`, or of the calling thread when ctx is NULL. */
const char* ovl_last_error(const ovl_ctx* ctx);

/*
 * One-shot batch scoring: uploads and packs the reads, scores
 * n_pairs candidates (a_idx[p], b_idx[p]) and writes out_score[p], out_end[p].
 * Replaces the loop body of overlapGraphs.py:50-53 for a whole candidate list.
 *
 * band < 0: the full DP of aligners.py:27-57 (reference semantics, bit-exact).
 * band >= 0: the build's seed-and-extend knob (not a reference mode): seed
 *   j* = the ungapped first argmax, diagonal d* = n - j*; the aligners.py:33-48
 *   recurrence on cells with |(i - j) - d*| <= band only, out-of-band
 *   predecessors = -inf; last-row strict '>' first argmax over in-band cells.
 *   Identical to band < 0 whenever gaps cannot win (e.g. the default
 *   indel = -2^31) and when band >= 2 * (longest read).
 */
int ovl_score_pairs(ovl_ctx* ctx, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads,
                    const int32_t* a_idx, const int32_t* b_idx, int64_t n_pairs,
                    int32_t match, int32_t mismatch, int64_t indel, int32_t band,
                    int32_t* out_score, int32_t* out_end);

/* Upload + pack a read set and keep it resident in HBM (replaces any previous set). */
int ovl_set_reads(ovl_ctx* ctx, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads);

/* Resident read-set facts: count, longest read, bit planes per base, device bytes held. */
int ovl_reads_info(const ovl_ctx* ctx, int32_t* n_reads, int32_t* lmax, int32_t* planes,
                   int64_t* device_bytes);

/* Which kernel a score call with these parameters would use on the resident reads. */
int ovl_plan(const ovl_ctx* ctx, int32_t match, int32_t mismatch, int64_t indel, int32_t band,
             int32_t* out_kernel);

/* The form the first scoring launch of the last scoring call took on the context's first device (host-array
 * calls, ovl_score_candidates*, ovl_score_device): kernel (OVL_KERNEL_*; OVL_KERNEL_NONE when nothing was
 * launched), key64 (the ungapped kernel's 64-bit keys; for a banded call, its seed's), wide (cells beyond int32),
 * lane (the lane-per-pair full DP ran) with its arguments prof (byte score profile), sfx (row symbols from the bit
 * planes), ho (hand-off column: 0 int32, 1 int16, 2 four-bit steps in LDS) and h2 (two pairs per lane as packed f16
 * cells), band_form (the band knob's form as launched: 0 strip, 1 rows, 2 fast, 3 diag, 4 lane;
 * -1 without a band), split (its lane kernel's two lanes per pair) and rs_log2 (an ungapped launch: 0 in throughput
 * mode; above 0 the uniform kernel's latency mode or the general kernel's lanes per pair).  Any pointer may be
 * NULL.  Additions like this one leave OVL_ABI_VERSION as it is: the version changes when an existing signature
 * does. */
int ovl_last_score_form(const ovl_ctx* ctx, int32_t* kernel, int32_t* key64, int32_t* wide, int32_t* lane,
                        int32_t* prof, int32_t* sfx, int32_t* ho, int32_t* h2, int32_t* band_form, int32_t* split,
                        int32_t* rs_log2);

/* Score against the resident reads; host pair/result arrays; synchronous.  Sharded over the
 * context's devices; chunked H2D / kernel / D2H pipeline per device.  A pair index outside
 * [0, n_reads) makes the call return OVL_E_INDEX (checked on the device, its results are -1). */
int ovl_score_host(ovl_ctx* ctx, const int32_t* a_idx, const int32_t* b_idx, int64_t n_pairs,
                   int32_t match, int32_t mismatch, int64_t indel, int32_t band,
                   int32_t* out_score, int32_t* out_end);

/*
 * Score against the resident reads with DEVICE pointers (on the context's first device),
 * asynchronously on `stream` (a hipStream_t; NULL = the default stream, as in the HIP API).  Pairs with an index
 * outside [0, n_reads) get score = end = -1 and set a device error flag that
 * ovl_check_device_errors() reports.
 */
int ovl_score_device(ovl_ctx* ctx, const int32_t* d_a_idx, const int32_t* d_b_idx, int64_t n_pairs,
                     int32_t match, int32_t mismatch, int64_t indel, int32_t band,
                     int32_t* d_score, int32_t* d_end, void* stream);

/* Synchronise the device; OVL_E_INDEX if a previous ovl_score_device saw a bad index (flag is cleared). */
int ovl_check_device_errors(ovl_ctx* ctx);

/*
 * One resident pair (a, b) through the DP kernel, optionally returning the
 * (len(a)+1) x (len(b)+1) int8 traceback table of aligners.py:30,42-48
 * (0 = diagonal, 1 = up, 2 = left) for the backtrack of aligners.py:59-78.
 */
int ovl_align_one(ovl_ctx* ctx, int32_t a, int32_t b, int32_t match, int32_t mismatch, int64_t indel,
                  int32_t* out_score, int32_t* out_end, int8_t* traceback);

/*
 * k-mer candidate enumeration on the device over the resident reads, which must
 * be the distinct reads in read_copies order (overlapGraphs.py:18-20).  Produces
 * exactly the pair list the reference scores, in its order (overlapGraphs.py:30-52):
 * for each read a in order, every read b != a whose prefix read[:k] equals a's
 * suffix read[-k:] (whole reads when shorter than k), b in read order; k == 0:
 * every b != a.  The list stays in the context (until the next ovl_candidates or
 * ovl_set_reads); *out_n_pairs receives its length.  OVL_E_UNSUPPORTED when
 * k * (bits per symbol: 2, 4 or 8) > 58.  Replaces the Python loops of
 * overlapGraphs.py:30-52 (which the host path, ovlgraph/candidates.py, restates).
 */
int ovl_candidates(ovl_ctx* ctx, int32_t k, int64_t* out_n_pairs);

/*
 * Seed candidates: the second candidate rule, every k-mer of a read looked up among the reads' prefixes.
 *
 *   Reads are the distinct reads in read_copies order, and k >= 1.  The prefix key of read b is b[:k]; a read
 *   shorter than k has no key and takes no part.  For each read a in order, for each offset o = 1, 2, ...,
 *   len(a) - k ascending, for each read b != a in read order whose prefix key equals a[o:o+k]: emit (a, b, o),
 *   unless (a, b) was already emitted at a smaller offset.
 *
 * Each b has one prefix key, so offsets of a with different k-mers have disjoint groups and offsets with equal
 * k-mers the same group: an offset whose k-mer occurs at an earlier offset >= 1 of a emits nothing.  Offset 0 is
 * left out: reads sharing their first k bases start at the same place.  For reads longer than k the list of
 * ovl_candidates at the same k is a subset of this one up to order (its hit is o = len(a) - k).
 *
 * The list becomes the context's candidate list exactly as after ovl_candidates -- enumerated on every device,
 * replaced by the next ovl_candidates, ovl_seed_candidates or ovl_set_reads -- so ovl_candidates_copy,
 * ovl_candidates_device, ovl_score_candidates(_range) and ovl_candidates_shards work on it unchanged;
 * *out_n_pairs receives its length.  Every argument is checked before anything runs, and a failed check leaves the
 * previous list as it was: OVL_E_ARG for k < 1 or a null pointer, OVL_E_STATE without resident reads,
 * OVL_E_UNSUPPORTED when k * (bits per symbol: 2, 4 or 8) > 58, when a read is longer than k + 8192, or (after the
 * count pass, the previous list still intact) when the list would hold 2^31 pairs or more.
 */
int ovl_seed_candidates(ovl_ctx* ctx, int32_t k, int64_t* out_n_pairs);

/* The offset o of each pair of the list of ovl_seed_candidates (as many entries as the list has pairs);
 * OVL_E_STATE when the context's candidate list did not come from ovl_seed_candidates. */
int ovl_seed_offsets_copy(ovl_ctx* ctx, int32_t* out_offset);

/* With ovl_set_timing on, the device time (ms, HIP events on the context's first device) of the last
 * ovl_seed_candidates: the key kernel, the sort, the count kernel with the scan, the emit kernel.  Each may be
 * NULL; zeros when timing was off. */
int ovl_last_seed_timing(const ovl_ctx* ctx, double* keys_ms, double* sort_ms, double* count_ms, double* emit_ms);

/* Copy the context's candidate list to host arrays of *out_n_pairs entries each. */
int ovl_candidates_copy(ovl_ctx* ctx, int32_t* a_idx, int32_t* b_idx);

/* Device pointers (and length) of the context's candidate list, for ovl_score_device. */
int ovl_candidates_device(const ovl_ctx* ctx, const int32_t** d_a_idx, const int32_t** d_b_idx, int64_t* n_pairs);

/* Score the context's candidate list (no pair upload); host outputs; synchronous.  Every device
 * of the context enumerated the same list, each scores its shard and copies its results into its
 * slice of out_score / out_end (the "gather" of SURVEY.md §8e is these per-device D2H copies). */
int ovl_score_candidates(ovl_ctx* ctx, int32_t match, int32_t mismatch, int64_t indel, int32_t band,
                         int32_t* out_score, int32_t* out_end);

/* The same for pairs [lo, hi) of the candidate list: out_score[p - lo], out_end[p - lo].  A
 * process of a multi-process job scores its shard this way (bounds from ovl_candidates_shards). */
int ovl_score_candidates_range(ovl_ctx* ctx, int64_t lo, int64_t hi, int32_t match, int32_t mismatch,
                               int64_t indel, int32_t band, int32_t* out_score, int32_t* out_end);

/* The resident grid (one per device of a single-device context): ovl_score_candidates(_range) calls of the
 * uniform kernel's form (ungapped plan, int32 keys, <= 4 symbols, reads <= 254 bases) are served by a kernel that
 * stays on the device between calls, fed requests through pinned memory -- a call pays no launch and no completion
 * signal.  It leaves by itself after ~20 ms without a request, when another entry point of the context needs the
 * device, and at ovl_destroy.  Opt-in: OVL_RESIDENT=1 at context creation (the default, 0, routes every call
 * through the launch pipeline, which the grid did not beat on the boxes measured).  ovl_quiesce makes the
 * context's grids leave now (before a whole-device synchronisation such as torch.cuda.synchronize(), which would
 * otherwise wait for the idle deadline); the next call relaunches them.  ovl_resident_stats reports how many grids
 * are resident, their launches (relaunches: calls that found their grid gone) and whether a failed call disabled
 * the path (its calls then go through the launch pipeline). */
int ovl_quiesce(ovl_ctx* ctx);
/* How many of the context's devices (its first ones) a host-array scoring call over n_pairs uses: several only from
 * 3 devices with >= 262,144 pairs each (multi-device calls store int32 results over every device's link; below
 * that one device with packed results is faster), else 1 -- so a context over every GPU is never slower than one
 * GPU.  (A context whose slots share a GPU, OVL_SHARE_DEVICES=1, uses every slot whatever this reports.) */
int ovl_devices_for(const ovl_ctx* ctx, int64_t n_pairs, int32_t* out_devices);
int ovl_resident_stats(const ovl_ctx* ctx, int32_t* alive, int64_t* launches, int64_t* relaunches, int32_t* broken);

/* Contiguous shard bounds of the candidate list, balanced by sum len(a)*len(b) + 1:
 * bounds[0] = 0 <= bounds[1] <= ... <= bounds[n_shards] = n_pairs (the rule of
 * ovlgraph/sharded.py:shard_bounds, computed on the device). */
int ovl_candidates_shards(ovl_ctx* ctx, int32_t n_shards, int64_t* bounds);

/*
 * local_alignment (aligners.py:85-167) of query[0..n) against reference[0..m) on the whole GPU:
 * Smith-Waterman with the reference's tie order and int64-exact arithmetic; bytes are compared
 * for equality only.  Outputs: the best score and its cell (end_i, end_j) -- the first strict
 * maximum in fill order; with ops != NULL also the traceback walk of aligners.py:133-153 from
 * that cell: ops[k] in walk order (1 diag, 2 up, 3 left), *n_ops its length (OVL_E_RANGE when
 * > ops_cap; n + m always suffices) and the cell where it stopped (start_i, start_j; start_j is
 * the reference's start position, aligners.py:156).  Needs n, m < 2^20 and match*min(n,m) < 2^24.
 */
int ovl_local_align(ovl_ctx* ctx, const uint8_t* query, int32_t n, const uint8_t* reference, int32_t m,
                    int32_t match, int32_t mismatch, int64_t indel, int32_t* out_score, int32_t* out_end_i,
                    int32_t* out_end_j, int32_t* out_start_i, int32_t* out_start_j, int8_t* ops,
                    int64_t ops_cap, int64_t* out_n_ops);
/*
 * ovl_local_align for many queries against one reference in one call (the evaluation stage's shape:
 * every contig of an assembly against the genome).  Query k is queries[q_off[k] .. q_off[k+1]) and is
 * aligned to reference[win_lo[k] .. win_lo[k] + win_len[k]) (win_lo and win_len both NULL: the whole
 * reference for every query); its results, at index k of the output arrays, are what ovl_local_align
 * returns for that query and that slice, positions relative to the window.  ops == NULL: scores only
 * (starts equal ends, out_n_ops[k] = 0); otherwise query k's walk goes to ops[ops_off[k] ..), and
 * ops_off[k+1] - ops_off[k] must be at least n_k + m_k (OVL_E_ARG otherwise).  Every argument is checked
 * before anything runs or is written: OVL_E_ARG for null or negative arguments and windows outside the
 * reference, OVL_E_UNSUPPORTED (naming the query) for ovl_local_align's per-query limits.  Empty queries
 * and empty windows give zeros.  Queries that fit one wavefront (up to 16 strips of 64 rows, int32 cells,
 * a traceback table up to 64 MiB) run in one launch of a kernel that gives each query to one wavefront;
 * the others run one by one as ovl_local_align does.  Runs on the context's first device.
 * ovl_last_local_batch: how many of the last call's queries took the batch kernel, how many the
 * single-pair path, and the wavefronts the batch kernel was launched with (at most
 * OVL_LOCAL_BATCH_WAVES when that is set at context creation).
 */
int ovl_local_align_batch(ovl_ctx* ctx, const uint8_t* queries, const int64_t* q_off, int32_t n_queries,
                          const uint8_t* reference, int32_t ref_len, const int32_t* win_lo,
                          const int32_t* win_len, int32_t match, int32_t mismatch, int64_t indel,
                          int32_t* out_score, int32_t* out_end_i, int32_t* out_end_j, int32_t* out_start_i,
                          int32_t* out_start_j, int8_t* ops, const int64_t* ops_off, int64_t* out_n_ops);
int ovl_last_local_batch(const ovl_ctx* ctx, int32_t* batched, int32_t* single, int32_t* waves);

/* Cycle removal of overlapGraphs.py:106-130 (remove_cycles_from_graph), host-side, no context.
 * Replaces:  while True: cycle = nx.find_cycle(G, orientation='original') ... G.remove_edge(u, v)
 * The graph is CSR: n_nodes nodes in the DiGraph's node order; node v's out-edges are
 * head[off[v] .. off[v+1]) in its adjacency (insertion) order with integer weight[] ("weight").
 * Writes to removed[] (capacity off[n_nodes]) the CSR indices of the edges the reference loop
 * removes, in its removal order, and their count to *n_removed: networkx 3.x find_cycle's
 * cycle (edge DFS from the first unexplored node in node order), its first minimum-weight edge. */
int ovl_remove_cycles(const int64_t* off, const int32_t* head, const int64_t* weight, int32_t n_nodes,
                      int64_t* removed, int64_t* n_removed);
/* ovl_remove_cycles publishing its progress to a consumer on another thread (the C builder of the surviving
 * edges' dicts, ovlgraph/_digraph build_overlap_stream, builds each node's successors as soon as they are
 * final): alive[e] (off[n_nodes] entries) is set to 1, then 0 when edge e is removed; final_nodes[0 .. *n_final)
 * lists each node once, when its out-edges are final (it can reach no cycle: settled, or explored by a start
 * whose walk found none); *n_final is stored with release order (read it with an acquire load) and reaches
 * n_nodes before a successful call returns. */
int ovl_remove_cycles_stream(const int64_t* off, const int32_t* head, const int64_t* weight, int32_t n_nodes,
                             int64_t* removed, int64_t* n_removed, uint8_t* alive, int32_t* final_nodes,
                             int64_t* n_final);

/*
 * Transitive reduction of overlapGraphs.py:235-303 (transitive_reduction) on the context's first device.
 * Replaces the marking loops over every two-hop path v -> w -> x (networkx dict lookups and a print per step).
 * The graph is the CSR of ovl_remove_cycles: node order, adjacency order, int64 weights.  Heads within one node's
 * list must be distinct (it is a DiGraph); self-loops are allowed.  reduced[e] (capacity off[n_nodes]) = 1 iff
 * the reference removes CSR edge e, else 0, and *n_reduced their count.  What the reference's loops compute:
 *   edge (v, x) is removed iff some w in succ(v) -- v and x themselves included when they are successors of v
 *   -- has an edge (w, x) with weight(v, w) + weight(w, x) >= weight(v, x).
 * Its fuzz argument is never read, eliminated successors are still expanded, so the result does not depend on the
 * visiting order.  Every argument is checked on the host before anything is launched or written: OVL_E_ARG for
 * null pointers, a negative n_nodes, off[0] != 0 or an off that decreases; OVL_E_INDEX for a head outside
 * [0, n_nodes); OVL_E_RANGE for |weight| >= 2^30 (the device holds int32 weights and forms sums of two).
 * A window of a node's out-row lives in LDS; a graph with more nodes than the window takes several passes per
 * node (OVL_TR_WINDOW at context creation lowers the window's entries, for tests).  No device memory grows
 * faster than the edge count.  With ovl_set_timing on, ovl_last_timing reports the kernel and the call.
 * ovl_transitive_reduce_host: the same checks and result from a plain host loop (a mark array per source node),
 * with no context and no GPU -- the small-graph path and the baseline the device call is measured against.
 * ovl_last_transitive: the window's entries, the passes per node and the two-hop steps
 * (sum over v, over w in succ(v), of deg(w)) of the last ovl_transitive_reduce.
 */
int ovl_transitive_reduce(ovl_ctx* ctx, const int64_t* off, const int32_t* head, const int64_t* weight,
                          int32_t n_nodes, uint8_t* reduced, int64_t* n_reduced);
int ovl_transitive_reduce_host(const int64_t* off, const int32_t* head, const int64_t* weight, int32_t n_nodes,
                               uint8_t* reduced, int64_t* n_reduced);
int ovl_last_transitive(const ovl_ctx* ctx, int32_t* window_nodes, int32_t* passes, int64_t* two_hop_steps);

/*
 * Reachability reduction of overlapGraphs.py:354-367 (transitive_reduction2) on the context's first device.
 * Replaces one nx.has_path search per ordered pair of successors of every node.  The graph is a CSR without
 * weights: node order, adjacency order; self-loops and cycles are allowed.  With R[u][x] true iff the graph has a
 * path of at least one edge from u to x, reduced[e] (capacity off[n_nodes]) = 1 iff the reference removes edge
 * e = (v, w):
 *   some u that stands before w in v's successor order has R[u][w].
 * The searches run on the unmodified graph, so the result does not depend on the visiting order; a node's first
 * successor is never removed.  A row that lists a head twice (no DiGraph has one) gets the positional rule
 * literally: an earlier equal entry removes the later one only when R[w][w].
 * closure, when not NULL, receives R as n_nodes rows of ceil(n_nodes / 64) uint64 words: bit x of row u is bit
 * x & 63 of word x >> 6, bits at and above n_nodes are zero.
 * Every argument is checked on the host before anything is launched or written: OVL_E_ARG for null pointers, a
 * negative n_nodes, off[0] != 0 or an off that decreases; OVL_E_INDEX for a head outside [0, n_nodes); OVL_E_OOM
 * when the n_nodes^2 / 8-byte matrix cannot be allocated.  The matrix is closed by blocked Warshall over pivot
 * blocks of 64 nodes, 2 * ceil(n_nodes / 64) + 2 launches on one stream whatever the graph's diameter; the marking
 * holds a window of the rows' columns in registers and takes several passes over wider rows (OVL_REACH_WINDOW at
 * context creation lowers the window's bits, for tests).  With ovl_set_timing on, ovl_last_timing reports the
 * launches and the call.
 * ovl_reach_reduce_host: the same checks and results on one host thread (row-OR Warshall over the same bit
 * matrix), with no context and no GPU -- the small-graph path and the baseline the device call is measured against.
 * ovl_last_reach: the words per row, the pivot blocks and the marking window's bits of the last ovl_reach_reduce.
 */
int ovl_reach_reduce(ovl_ctx* ctx, const int64_t* off, const int32_t* head, int32_t n_nodes, uint8_t* reduced,
                     int64_t* n_reduced, uint64_t* closure);
int ovl_reach_reduce_host(const int64_t* off, const int32_t* head, int32_t n_nodes, uint8_t* reduced,
                          int64_t* n_reduced, uint64_t* closure);
int ovl_last_reach(const ovl_ctx* ctx, int32_t* words_per_row, int32_t* pivot_blocks, int32_t* window_bits);

/*
 * The selection step of the reference's read-depth coverage (plots.py:115-135, plot_reconstructed_coverage) on the
 * context's first device: every read against every contig.  Read r is reads[r_off[r] .. r_off[r+1]), contig c is
 * contigs[c_off[c] .. c_off[c+1]); repeated contigs are separate positions.  For each pair the rule is
 * align_read_or_contig_to_reference (aligners.py:170-202): a read with 0 < len < read_length is aligned to the
 * contig's last len bases (the whole contig when it is shorter), every other read to the whole contig, and a read
 * shorter than read_length has (contig length - len) added to its positions.  Per read, over the contigs in order:
 *   best_score[r]  the maximum score,
 *   first_best[r]  the smallest c that attains it (-1 when n_contigs == 0, with zeros elsewhere),
 *   n_best[r]      how many contigs attain it,
 *   best_start[r], best_end[r]  the start and end positions of the alignment to contig first_best[r], in that
 *                  contig's coordinates with the shift applied (local_alignment's start_pos and end_pos),
 *   tie_bits       (may be NULL) n_reads rows of ceil(n_contigs / 32) words: bit c & 31 of word c >> 5 of row r is
 *                  set iff contig c attains best_score[r],
 *   scores         (may be NULL; tests and small inputs) n_reads x n_contigs scores, row-major.
 * Every argument is checked before anything runs or is written: OVL_E_ARG for null pointers, negative counts or
 * read_length and offsets that decrease; OVL_E_UNSUPPORTED beyond ovl_local_align's limits (lengths < 2^20,
 * match * min(n, m) < 2^24) or when the contigs together reach 2^31 bases.
 * The scores come from a kernel in which one lane owns one read and a wavefront's 64 reads sweep a contig column by
 * column with the DP column in registers; it takes reads of up to 128 bases under scorings with mismatch <= 0,
 * indel <= 0, match < 65536 and at most 255 distinct symbols.  Every other (read, contig) pair goes through
 * ovl_local_align_batch inside the same call.  The scores' tile in device memory is bounded by a chunk of contigs
 * (OVL_READ_BEST_CHUNK at context creation sets the contigs per chunk, for tests) and folded into the per-read
 * results on the device.  The start positions come from a second pass of n_reads items through
 * ovl_local_align_batch, each read against its first best contig.  With ovl_set_timing on, ovl_last_timing reports
 * the score pass (the lane kernel's launches and their folds) and the call.
 * ovl_read_best_host: the same checks and results on one host thread, with no context and no GPU.
 * ovl_last_read_best: the pairs of the last ovl_read_best that took the lane kernel, those that took the existing
 * kernels, and the lane kernel's launches.
 */
int ovl_read_best(ovl_ctx* ctx, const uint8_t* reads, const int64_t* r_off, int32_t n_reads, const uint8_t* contigs,
                  const int64_t* c_off, int32_t n_contigs, int32_t read_length, int32_t match, int32_t mismatch,
                  int64_t indel, int32_t* best_score, int32_t* first_best, int32_t* n_best, int32_t* best_start,
                  int32_t* best_end, uint32_t* tie_bits, int32_t* scores);
int ovl_read_best_host(const uint8_t* reads, const int64_t* r_off, int32_t n_reads, const uint8_t* contigs,
                       const int64_t* c_off, int32_t n_contigs, int32_t read_length, int32_t match, int32_t mismatch,
                       int64_t indel, int32_t* best_score, int32_t* first_best, int32_t* n_best, int32_t* best_start,
                       int32_t* best_end, uint32_t* tie_bits, int32_t* scores);
int ovl_last_read_best(const ovl_ctx* ctx, int64_t* lane_pairs, int64_t* fallback_pairs, int32_t* launches);

/*
 * Consensus polishing on the context's first device: the reads vote on the bases of the contigs they are placed on.
 * Reads and contigs are given as for ovl_read_best (repeated contigs are separate positions); place[r] is the contig
 * position read r votes on, or -1 for none.  Read r is aligned to contig place[r] by
 * align_read_or_contig_to_reference (aligners.py:170-202: the same window, best cell and walk as ovl_read_best); a
 * read with score 0 casts no vote.  Every column below is the contig's own column, window start + window-relative
 * column, not the reference's shifted start / end.  The walk's ops vote, at the column of the cell they are taken at:
 *   diag   +1 in channel A, C, G or T of the column, by the read's byte (upper case); any other byte casts no vote
 *          and adds one to *n_other,
 *   left   +1 in channel gap of the column (a contig base with no read base),
 *   up     +1 in channel ins of the column at the left of the inserted read base.
 * counts (may be NULL) receives total_bases x 6 int32, row-major, channels A, C, G, T, gap, ins, where base b is
 * byte contigs[c_off[0] + b] and total_bases = c_off[n_contigs] - c_off[0].  called receives total_bases bytes: with
 * n = A + C + G + T < min_depth the contig's byte; else the byte of the largest of the four channels, a tie going to
 * the contig's own byte when it is among the tied and else to the first of A, C, G, T.  gap and ins never change a
 * base, so polished contigs keep their lengths.  *n_changed counts the bases where called differs from the contig.
 * aln (may be NULL) receives three int32 per read: the score, the first column and one past the last column of its
 * alignment; zeros for unplaced reads and reads with score 0.  The sums are integer, so the result does not depend
 * on the order of the reads.
 * Every argument is checked before anything is launched or written: OVL_E_ARG for null pointers, negative counts or
 * read_length, min_depth < 1 and offsets that decrease; OVL_E_INDEX for place[r] outside [-1, n_contigs);
 * OVL_E_UNSUPPORTED beyond ovl_local_align's limits (lengths < 2^20, match * min(n, m) < 2^24) for a placed read or
 * when the contigs together reach 2^31 bases.
 * The alignments run in the batch kernel of ovl_local_align_batch, one item per placed read, whose walks stay in
 * device memory; a second kernel piles them up (one wavefront per read, one int32 atomic add per op) and a third
 * votes (one thread per base).  Reads beyond the batch kernel's limits go through ovl_local_align one by one and
 * their votes are added before the vote kernel runs.  Reads are taken in chunks bounded by a 256 MiB budget of ops
 * (OVL_CONSENSUS_CHUNK at context creation caps the reads per chunk, for tests), so device memory is bounded by the
 * contigs (31 bytes per base) plus one chunk.  With ovl_set_timing on, ovl_last_timing reports the kernels and the
 * call.
 * ovl_consensus_host: the same checks and results on one host thread, with no context and no GPU.
 * ovl_last_consensus: the reads of the last ovl_consensus that took the batch kernel and the single-pair path, the
 * ops piled up and the batch kernel's launches.  ovl_last_consensus_timing (timing on): the kernel time by part, in
 * ms -- the alignment launches with their uploads, the pileup kernel, the vote kernel.
 */
int ovl_consensus(ovl_ctx* ctx, const uint8_t* reads, const int64_t* r_off, int32_t n_reads, const uint8_t* contigs,
                  const int64_t* c_off, int32_t n_contigs, const int32_t* place, int32_t read_length, int32_t match,
                  int32_t mismatch, int64_t indel, int32_t min_depth, int32_t* counts, uint8_t* called,
                  int64_t* n_changed, int64_t* n_other, int32_t* aln);
int ovl_consensus_host(const uint8_t* reads, const int64_t* r_off, int32_t n_reads, const uint8_t* contigs,
                       const int64_t* c_off, int32_t n_contigs, const int32_t* place, int32_t read_length,
                       int32_t match, int32_t mismatch, int64_t indel, int32_t min_depth, int32_t* counts,
                       uint8_t* called, int64_t* n_changed, int64_t* n_other, int32_t* aln);
int ovl_last_consensus(const ovl_ctx* ctx, int64_t* batch_reads, int64_t* single_reads, int64_t* ops,
                       int32_t* launches);
int ovl_last_consensus_timing(const ovl_ctx* ctx, double* align_ms, double* pileup_ms, double* vote_ms);

/*
 * Placed consensus: every read votes on its contig where a layout placed it (ovl_layout's contig[r] and offset[r]),
 * aligned only inside a band around the diagonal the placement names, with a weight (a distinct read's copy count),
 * for up to `rounds` rounds.
 *
 *   Inputs: reads (reads, r_off) and weight[r] (NULL: 1 for every read); contigs (contigs, c_off; a repeated contig is
 *   a separate position); contig[r] in [-1, n_contigs), -1 meaning no vote; offset[r], any int32; slack >= 0, match,
 *   mismatch, indel, min_vote_score >= 1, min_depth >= 1, rounds >= 1.
 *   A read r of length L > 0 with weight > 0, placed on contig c of length m, votes only if it passes every step:
 *   1. Window.  In int64, lo = max(0, offset - slack) and hi = min(m, offset + L + slack).  If hi <= lo the read casts
 *      no vote.  Otherwise t = contig[lo:hi), w = hi - lo, d = offset - lo.
 *   2. Band.  DP cell (i, j), 1 <= i <= L, 1 <= j <= w, is in the band iff |(j - i) - d| <= slack.  Row 0, column 0
 *      and every cell outside the band hold value 0 and code 0.
 *   3. Fill.  Every in-band cell is filled by local alignment's statement (aligners.py:106-137): dg, u and l from the
 *      three neighbours' values, an out-of-band neighbour counting as 0.  If dg >= u && dg >= l && dg >= 0 the cell
 *      takes diag (code 1); else if u >= l && u >= 0, up (code 2); else if l >= 0, left (code 3); else its value is 0.
 *      The code is stored only when the value is > 0.  The statement is total for any indel.
 *   4. Best cell.  The first strict maximum over the in-band cells in row-major order.  A best score below
 *      min_vote_score casts no vote and leaves the read's aln at zeros.
 *   5. Walk.  From the best cell along the codes (aligners.py:139-161); it stops at code 0.
 *   6. Votes.  The ops vote as in ovl_consensus, on the contig's own columns (lo + window column): diag in channel A,
 *      C, G or T by the read's byte, left in gap, up in ins at the column at the left of the inserted base; a byte
 *      outside ACGT on a diagonal goes to *n_other.  Every +1 is +weight[r], n_other included.  aln[r] is (score,
 *      lo + the column where the walk stops, lo + the best cell's column).
 *   7. Call.  Every base is called as in ovl_consensus (min_depth, majority, ties to the contig's own byte).
 *   8. Rounds.  Round k + 1 runs on the contigs as round k called them (lengths never change, so the placement stays
 *      valid); the loop stops after a round that changed nothing, or after `rounds` rounds.  counts, *n_changed,
 *      *n_other and aln are the last round's; called is the contigs after the last round; *total_changed counts the
 *      bases of called that differ from the input contigs; *rounds_done is the number of rounds that ran.
 *   With slack >= max(L, m), weight NULL, min_vote_score 1 and one round this is ovl_consensus with place = contig and
 *   read_length 0; `rounds` = R equals R calls with rounds = 1, each fed the call before's called bytes.
 *
 * counts and aln may be NULL.  Every argument is checked before anything is launched or written: OVL_E_ARG for null
 * pointers, negative counts, slack or weights, min_vote_score, min_depth or rounds below 1, and offsets that decrease;
 * OVL_E_INDEX for contig[r] outside [-1, n_contigs); OVL_E_UNSUPPORTED when the sum of weight * length over the placed
 * reads reaches 2^31 (below it no channel can overflow), when the contigs together reach 2^31 bases, and for a placed
 * read beyond ovl_local_align's limits (lengths < 2^20, match * min(L, m) < 2^24).  The device form also returns
 * OVL_E_UNSUPPORTED for slack > 15 and for a placed read with max(0, match, mismatch, indel) * (L + w) >= 2^30 (its
 * cells are int32); the host form takes any slack and scoring.
 * ovl_consensus_placed (the context's first device): one lane per read fills the band row by row in registers (9, 17
 * or 31 diagonals for slack <= 4, 8, 15), keeps a row's codes as one 64-bit word in device memory, walks its own
 * words back and adds its weight per op; ovl_consensus's vote kernel calls the bases, and between rounds the called
 * bytes become the contigs on the device: only the counters cross the link.  The call uploads its reads.  Reads are
 * taken in chunks under a 256 MiB budget of code words (OVL_CONSENSUS_CHUNK caps the reads per chunk, for tests).
 * ovl_last_consensus_placed: of the last ovl_consensus_placed, the reads that voted in the last round, the placed
 * reads without a window, the ops of the last round's walks, the band kernel's launches and the rounds that ran.
 * ovl_last_consensus_placed_timing (timing on): the band kernel's and the vote kernel's time over all rounds, in ms.
 */
int ovl_consensus_placed(ovl_ctx* ctx, const uint8_t* reads, const int64_t* r_off, int32_t n_reads,
                         const int32_t* weight, const uint8_t* contigs, const int64_t* c_off, int32_t n_contigs,
                         const int32_t* contig, const int32_t* offset, int32_t slack, int32_t match, int32_t mismatch,
                         int64_t indel, int32_t min_vote_score, int32_t min_depth, int32_t rounds, int32_t* counts,
                         uint8_t* called, int64_t* n_changed, int64_t* n_other, int64_t* total_changed,
                         int32_t* rounds_done, int32_t* aln);
int ovl_consensus_placed_host(const uint8_t* reads, const int64_t* r_off, int32_t n_reads, const int32_t* weight,
                              const uint8_t* contigs, const int64_t* c_off, int32_t n_contigs, const int32_t* contig,
                              const int32_t* offset, int32_t slack, int32_t match, int32_t mismatch, int64_t indel,
                              int32_t min_vote_score, int32_t min_depth, int32_t rounds, int32_t* counts,
                              uint8_t* called, int64_t* n_changed, int64_t* n_other, int64_t* total_changed,
                              int32_t* rounds_done, int32_t* aln);
int ovl_last_consensus_placed(const ovl_ctx* ctx, int64_t* voted_reads, int64_t* windowless_reads, int64_t* ops,
                              int32_t* launches, int32_t* rounds);
int ovl_last_consensus_placed_timing(const ovl_ctx* ctx, double* band_ms, double* vote_ms);

/*
 * Best-successor layout: contigs straight from the score columns, without a graph object.
 *
 *   Inputs: n reads with lengths len[r]; E pairs (a[p], b[p], score[p], end[p]) in list order; min_score and
 *   min_overlap.
 *   1. Eligible.  Pair p is eligible iff a[p] != b[p], score[p] >= min_score and min_overlap <= end[p] < len[b[p]].
 *      A link that adds no base is no link.
 *   2. Link.  link[a] is the eligible pair of a with the greatest score; ties go to the smallest p.
 *      succ[a] = b[link[a]].  A read without an eligible pair has link = succ = -1.
 *   3. Cycles.  succ is a functional graph.  Every cycle is cut at its pair with the least score; ties go to the
 *      greatest p.  The source of that pair gets link = succ = -1.  What remains is a forest of in-trees, each with
 *      one root (succ = -1).
 *   4. Span.  tail[root] = 0; otherwise tail[a] = tail[succ[a]] + len[succ[a]] - end[link[a]].
 *      span[a] = len[a] + tail[a] is the length of the contig spelled from a.
 *   5. Contigs.  One contig per root, in ascending root index.  Its head is the read of the tree with the greatest
 *      span; ties go to the smallest read index.  The contig is the head followed, along succ, by
 *      read[succ][end[link]:] (the reference's own concatenation, create_contig).  Its length is span[head].
 *   6. Placement.  Every read r gets contig[r], its tree's contig; offset[r] = span[head] - span[r], which for a read
 *      on the head's path is where its first base lies; and on_path[r].
 *   Everything is integer and independent of pair order, except the tie rules, which name p.
 *
 * The rule works on the reads it is given (the distinct reads of a read set: copies do not multiply contigs).
 * Outputs, each of which may be NULL: succ, link, contig, offset (n_reads int32 each), on_path (n_reads bytes, 0 or
 * 1), bases (the contigs' bytes one after the other: at most sum len bytes, since every read contributes at most its
 * length) and c_off (n_reads + 1 int64, of which *n_contigs + 1 are written: contig c is bases[c_off[c] ..
 * c_off[c+1])).  *n_contigs is always written.  No two-call protocol is needed.
 * Every argument is checked before anything is launched or written: OVL_E_ARG for null pointers (n_contigs; offsets
 * with reads; a column with pairs; seqs with bases to spell), negative counts, offsets that decrease and
 * min_overlap < 1; OVL_E_UNSUPPORTED for n_pairs >= 2^31 or sum len >= 2^31, and from the device forms when the
 * columns and tables do not fit the device's free memory; OVL_E_INDEX for a pair index outside [0, n_reads).
 *
 * ovl_layout_host: the rule on one host thread, with no context and no GPU.
 * ovl_layout: uploads the reads and the columns and runs the kernels of ovl_layout.hip on the context's first
 *   device: one lane per pair reduces the key (score biased by 2^31) << 32 | ~p into best[a] (runs of equal a inside
 *   a wavefront first, one 64-bit atomic max per run; an ungrouped list is as correct); pointer doubling over succ
 *   (ceil(log2 n) levels) finds every read's root or a node on a cycle, the minimum key around a cycle names the one
 *   link to cut, and the doubling is redone only when a cycle was found; tail is the same doubling with a sum; the
 *   head per root is a 64-bit atomic max of span << 32 | ~r; the head's path is marked from the highest level down
 *   through the kept jump tables; a wavefront per on-path read copies its successor's new bases.
 *   Device memory: 16 bytes per pair (the four columns) and 66 + 4 * (ceil(log2 n) + 1) bytes per read (the jump
 *   tables are (levels + 1) * n * 4 of them), plus the reads (sum len + 12 per read) and the contigs (sum len).
 * ovl_layout_candidates: the same on the resident reads and the resident candidate list (ovl_candidates or
 *   ovl_seed_candidates): the list is scored into device columns by the launches of ovl_score_device (same
 *   scoring arguments and limits) and the same kernels run on them; only the outputs cross the link, and the list
 *   stays as it was.  8 bytes per pair for the two columns beside the list's own 8, the per-read bytes as above.
 *   OVL_E_STATE without resident reads or without a candidate list.  A list whose columns do not fit the device is
 *   refused (OVL_E_UNSUPPORTED): it is not scored in chunks.
 * ovl_last_layout: of the last ovl_layout / ovl_layout_candidates of the context -- or, with ctx NULL, of the calling
 *   thread's last ovl_layout_host -- the links of the forest (after the cuts), the cycles cut, the doubling levels
 *   (0 from the host form, which walks) and the reads on contig paths.  ovl_last_layout_timing (timing on): device
 *   time in ms of the scoring launches (0 for ovl_layout), the link kernel, the forest kernels and the spelling.
 */
int ovl_layout_host(const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, const int32_t* a, const int32_t* b,
                    const int32_t* score, const int32_t* end, int64_t n_pairs, int32_t min_score, int32_t min_overlap,
                    int32_t* succ, int32_t* link, int32_t* contig, int32_t* offset, uint8_t* on_path, uint8_t* bases,
                    int64_t* c_off, int32_t* n_contigs);
int ovl_layout(ovl_ctx* ctx, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, const int32_t* a,
               const int32_t* b, const int32_t* score, const int32_t* end, int64_t n_pairs, int32_t min_score,
               int32_t min_overlap, int32_t* succ, int32_t* link, int32_t* contig, int32_t* offset, uint8_t* on_path,
               uint8_t* bases, int64_t* c_off, int32_t* n_contigs);
int ovl_layout_candidates(ovl_ctx* ctx, int32_t match, int32_t mismatch, int64_t indel, int32_t band,
                          int32_t min_score, int32_t min_overlap, int32_t* succ, int32_t* link, int32_t* contig,
                          int32_t* offset, uint8_t* on_path, uint8_t* bases, int64_t* c_off, int32_t* n_contigs);
int ovl_last_layout(const ovl_ctx* ctx, int64_t* links, int64_t* cycles, int32_t* levels, int64_t* on_path_reads);
int ovl_last_layout_timing(const ovl_ctx* ctx, double* score_ms, double* link_ms, double* forest_ms, double* spell_ms);

/*
 * k-mer spectrum read correction: the reads corrected against their own k-mer spectrum, before anything is scored.
 *
 *   Codes, keys and windows.  Codes are A = 0, C = 1, G = 2, T = 3, taken from the bytes ACGT; any other byte has no
 *   code.  k is in [1, 31].  The key of a window r[o:o+k] whose bytes all have codes is
 *   sum_j code(r[o+j]) << 2(k-1-j), a uint64 below 2^62, so key order is the k-mers' order as byte strings.  A window
 *   that holds a byte without a code has no key, and so has every window of a read shorter than k.
 *   Spectrum.  The distinct keys over all windows of all reads (reads counted as given, duplicates included) in
 *   ascending order, each with its number of occurrences as an int32.
 *   Threshold.  h[c] = the number of distinct keys with count c.  solid_threshold is the smallest c >= 1 with
 *   c >= max count or h[c+1] >= h[c] (the first valley of the histogram).  A key is solid when its count is >=
 *   min_count; a window without a key is never solid.
 *   Correction, one round.  Every decision reads the original reads only, so reads and positions are independent of
 *   each other and of the order in which they are handled.  For a read r of length L >= k and a position i the
 *   covering windows are the offsets o in [max(0, i-k+1), min(i, L-k)].  Position i is trusted when at least one
 *   covering window is solid, and stays.  An untrusted position whose byte has no code stays.  Otherwise, for each of
 *   the three other bases x, s(x) is the number of covering windows that are solid after r[i] alone is replaced by x;
 *   if the largest s(x) is >= 1 and strictly greater than the other two, r[i] becomes that x; on a tie, or when all
 *   are 0, r[i] stays.  Reads shorter than k are returned as they are.  Lengths never change.
 *
 * Read r is seqs[offsets[r] .. offsets[r+1]).  Every argument is checked before anything runs or is written:
 * OVL_E_ARG for null pointers (offsets; seqs with bytes to read; out_n_distinct; the output arrays with a capacity > 0;
 * out_stats; out_changed with reads; out_seqs with bytes), n_reads < 0, capacity < 0, min_count < 0, k outside [1, 31]
 * and offsets that decrease.
 *
 * ovl_kmer_spectrum: the spectrum into out_keys / out_counts (capacity entries each); *out_n_distinct receives the
 *   number of distinct keys.  With capacity too small it writes nothing but *out_n_distinct and returns OVL_E_RANGE,
 *   so a caller can size the buffers (capacity 0, both arrays NULL) and call again.
 * ovl_correct_reads: one round.  min_count >= 1, or 0 for the threshold rule.  out_seqs receives the corrected bytes in
 *   the input's layout (read r at out_seqs[offsets[r] ..); bytes outside [offsets[0], offsets[n_reads]) are not
 *   touched; it may be seqs itself: the decisions are made from keys formed before anything is written), out_changed the changed bases per read, and out_stats eight
 *   int64: {0 k-mers (windows with a key), 1 distinct keys, 2 solid windows, 3 untrusted positions, 4 changed bases,
 *   5 ties (untrusted positions whose largest s(x) is >= 1 and not alone), 6 the threshold used, 7 windows}.
 * The device forms run the kernels of ovl_spectrum.hip on the context's first device: a key pass (one wavefront per
 *   read, keys rolled), hipcub's radix sort over 2k + 1 bits (a window without a key is ~0 and sorts last), head flags,
 *   a scan and a scatter of (key, run length), then the correction pass over the spectrum in device memory.  Device
 *   memory: 40 bytes per window, the reads twice and 20 bytes per read.  Limits: reads of up to k + 8,191 bases (64 KiB
 *   of keys in LDS) and fewer than 2^31 windows; beyond either OVL_E_UNSUPPORTED, naming the read; the same when the
 *   tables do not fit the device's free memory.
 * ovl_kmer_spectrum_host / ovl_correct_reads_host: the rule on one host thread, with no context, no GPU and no limit
 *   on the reads (OVL_E_UNSUPPORTED only when one key occurs 2^31 times or more).
 * ovl_last_correct_timing (timing on): device time in ms of the key pass, the sort, the count pass (head flags, scan,
 *   scatter, run lengths; the host's wait for the number of distinct keys lies inside it) and the correction pass (0
 *   after ovl_kmer_spectrum) of the context's last call.
 */
int ovl_kmer_spectrum_host(const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, int32_t k, uint64_t* out_keys,
                           int32_t* out_counts, int64_t capacity, int64_t* out_n_distinct);
int ovl_correct_reads_host(const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, int32_t k, int32_t min_count,
                           uint8_t* out_seqs, int32_t* out_changed, int64_t* out_stats);
int ovl_kmer_spectrum(ovl_ctx* ctx, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, int32_t k,
                      uint64_t* out_keys, int32_t* out_counts, int64_t capacity, int64_t* out_n_distinct);
int ovl_correct_reads(ovl_ctx* ctx, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, int32_t k,
                      int32_t min_count, uint8_t* out_seqs, int32_t* out_changed, int64_t* out_stats);
int ovl_last_correct_timing(const ovl_ctx* ctx, double* keys_ms, double* sort_ms, double* count_ms,
                            double* correct_ms);

/*
 * The unitig pipeline from the score columns: construct_string_graph, transitive_reduction2 and find_unitigs
 * (overlapGraphs.py:332-412) without a graph object.
 *
 *   Inputs: the raw reads R[0 .. n_raw) as ids[j], the distinct read of R[j]; the n_reads distinct reads d, numbered by
 *   first occurrence (so ids[j] is at most one more than every id before it, and every distinct read occurs); the
 *   columns score / end over the n (n - 1) ordered pairs of distinct reads in ovl_candidates(k = 0) order, pair (x, y)
 *   at x (n - 1) + y - (y > x); and the self columns self_score[x] / self_end[x], the pair (x, x), read only for a
 *   read with at least two copies (both may be NULL when there is none).  first[x] is the first raw position of x,
 *   prev[j] the previous raw position holding ids[j], or -1.
 *   1. String graph.  Nodes are d in order.  The successor list of x is produced by j = first[x] + 1 .. n_raw - 1
 *      ascending: position j yields ids[j] iff prev[j] <= first[x] (j is that read's first occurrence after first[x])
 *      and score(x, ids[j]) > 0.  The edge carries weight = score and end_position = end.  That is the insertion order
 *      of the reference's loop over combinations(R, 2); a self-loop (x, x) appears when x has a second copy.
 *   2. Reduction.  ovl_reach_reduce's rule on that CSR.  The kept edges in CSR order are the reduced graph, added
 *      tail-major in node order (the predecessor order of DiGraph.copy()).
 *   3. Walk.  From every node not yet on a path, in node order, the path goes on while its last node has exactly one
 *      kept out-edge and one kept in-edge and that edge's head is on no earlier path; a head with several predecessors
 *      is still appended, and ends the path.  When the head is on the path itself -- a cycle of non-branching nodes,
 *      where the reference never returns -- the call returns OVL_UNITIGS_CYCLE (1, not an error) with the node in
 *      *cycle_node; only *n_edges, *n_kept and the kept edge columns are then valid.
 *   4. Spelling.  A path's contig is its first read followed by read[v][end_position:] for every further node v.
 *
 * Outputs, each of which may be NULL but n_contigs: path_off (n_reads + 1 int64, *n_contigs + 1 written), path_nodes
 * (n_reads int32: every node lies on exactly one path), bases (at most sum len bytes) with c_off (n_reads + 1 int64),
 * *n_edges (the string graph's edges), *n_kept, *cycle_node (-1 without a cycle).  The kept edge columns (tail, head,
 * weight, end_position; *n_kept int32 each, any may be NULL) are fetched by ovl_unitigs_edges_copy from the context's
 * last device call or, with ctx NULL, from the calling thread's last ovl_unitigs_host.
 * Every argument is checked before anything is launched or written: OVL_E_ARG for null pointers (n_contigs; offsets
 * with reads; ids with raw reads; a column with pairs; a self column with a repeated read; seqs with bases to spell),
 * negative counts, offsets that decrease, n_raw < n_reads and ids not numbered by first occurrence; OVL_E_INDEX for an
 * id outside [0, n_reads); OVL_E_UNSUPPORTED for n_reads^2 >= 2^31 or sum len >= 2^31, and from the device forms when
 * columns, CSR (sized for the most edges the raw list allows) and matrix do not fit the device's free memory: nothing
 * is chunked.
 *
 * ovl_unitigs_host: the rule on one host thread, with no context and no GPU.
 * ovl_unitigs: uploads ids and the columns and runs ovl_unitigs.hip on the context's first device: a wavefront per row
 *   counts the row's edges by ballot, a scan gives the offsets, the same walk writes the CSR in ascending j; then
 *   ovl_reach.hip's closure and marking on the resident CSR; then a lane per edge counts the kept in- and out-degrees
 *   and stores the sole successor, and a scan compacts the kept edges.  The walk and the spelling run on the host from
 *   16 bytes per node.  Device memory: 8 bytes per ordered pair, 41 per edge, 44 per node, 8 per raw read and the
 *   n x ceil(n / 64) x 8-byte matrix.
 * ovl_unitigs_candidates: the same on the resident reads and the resident ovl_candidates(k = 0) list, scored into
 *   device columns by the launches of ovl_score_device (the self pairs of repeated reads in a second short list); only
 *   ids, the per-node arrays and the outputs cross the link.  seqs: the resident reads' bytes, read 0 first, needed
 *   only to spell bases.  OVL_E_STATE without resident reads or without a candidate list; OVL_E_ARG when the list is
 *   not the k = 0 list of these reads (its length is not n (n - 1)).
 * ovl_unitigs_walk_host: step 3 alone over a CSR without repeated heads (ovl_reach_reduce's checks): the paths, or
 *   OVL_UNITIGS_CYCLE and *cycle_node.
 * ovl_last_unitigs: of the context's last device call -- or, with ctx NULL, the thread's last ovl_unitigs_host -- the
 *   edges, the kept edges, the paths and the matrix's words per row.  ovl_last_unitigs_timing (timing on): device time
 *   in ms of the scoring launches (0 for ovl_unitigs), the edge build (degrees, scan, CSR; the host's wait for the
 *   offsets lies inside it), the closure and marking, and the node facts with the kept edges.
 */
#define OVL_UNITIGS_CYCLE 1
int ovl_unitigs_host(const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, const int32_t* ids, int32_t n_raw,
                     const int32_t* score, const int32_t* end, const int32_t* self_score, const int32_t* self_end,
                     int64_t* path_off, int32_t* path_nodes, uint8_t* bases, int64_t* c_off, int32_t* n_contigs,
                     int64_t* n_edges, int64_t* n_kept, int32_t* cycle_node);
int ovl_unitigs(ovl_ctx* ctx, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, const int32_t* ids,
                int32_t n_raw, const int32_t* score, const int32_t* end, const int32_t* self_score,
                const int32_t* self_end, int64_t* path_off, int32_t* path_nodes, uint8_t* bases, int64_t* c_off,
                int32_t* n_contigs, int64_t* n_edges, int64_t* n_kept, int32_t* cycle_node);
int ovl_unitigs_candidates(ovl_ctx* ctx, const uint8_t* seqs, const int32_t* ids, int32_t n_raw, int32_t match,
                           int32_t mismatch, int64_t indel, int32_t band, int64_t* path_off, int32_t* path_nodes,
                           uint8_t* bases, int64_t* c_off, int32_t* n_contigs, int64_t* n_edges, int64_t* n_kept,
                           int32_t* cycle_node);
int ovl_unitigs_edges_copy(const ovl_ctx* ctx, int32_t* tail, int32_t* head, int32_t* weight, int32_t* end);
int ovl_unitigs_walk_host(const int64_t* off, const int32_t* head, int32_t n_nodes, int64_t* path_off,
                          int32_t* path_nodes, int32_t* n_paths, int32_t* cycle_node);
int ovl_last_unitigs(const ovl_ctx* ctx, int64_t* edges, int64_t* kept, int32_t* paths, int32_t* words_per_row);
int ovl_last_unitigs_timing(const ovl_ctx* ctx, double* score_ms, double* build_ms, double* reduce_ms,
                            double* facts_ms);

#ifdef __cplusplus
}
#endif

#endif /* OVL_H */
