// ovl_ctx.h — internal header of the C ABI of include/ovl.h on top of the gfx950 kernels: the context and
// per-device state, and the functions that cross the host files ovl_ctx.cpp (contexts, devices, pinned memory),
// ovl_plan.cpp (planner, kernel launch), ovl_pipeline.cpp (host-array pipeline), ovl_reads.cpp (read upload),
// ovl_cand.cpp (candidate lists, resident grid), ovl_local_api.cpp (single alignments), ovl_depth_api.cpp (read
// depth), ovl_consensus_api.cpp (read pileup and consensus), ovl_consensus_placed_api.cpp (consensus at the layout's
// placement), ovl_layout_api.cpp (best-successor layout),
// ovl_spectrum_api.cpp (k-mer spectrum read correction), ovl_unitigs_api.cpp (the unitig pipeline from the score
// columns) and the graph stages ovl_reduce_api.cpp / ovl_reach_api.cpp.  What the local-alignment stages share on the host is in ovl_local_host.h; what every stage's
// call, timing and device state share is in ovl_stage.h (included below, ahead of Dev).
//
// A context (ovl_ctx) drives one or more HIP devices from one host thread.  Each
// device (Dev) owns: a compute stream and two copy streams (H2D, D2H), its copy
// of the resident read store (codes + bit-plane layouts in HBM), scratch for
// host-array calls, pinned staging rings and the device error flag.  Host-array
// scoring calls shard the pair list over the devices (contiguous ranges balanced
// by sum n*m) and run a chunked pipeline per device (run_pipeline).
// The kernels read host pair lists and store results through host mappings:
// packed (2 bytes per pair, Call::pack) into staging slots that the host pool
// expands into the caller's int32 arrays while the next chunk scores, with a
// last share of the pairs stored as int32 straight into pinned arrays; otherwise
// as int32 into the caller's pinned arrays or staging slots.  Only the compact
// in-place pair list (encode_chunk) crosses by copy-engine transfer.
// Kernel choice per call (ovl_plan): the ungapped popcount kernel whenever gaps
// provably cannot win and the read store has a bit-plane layout, else a DP kernel.
// Never falls back to the CPU.
#pragma once

#include <hip/hip_runtime.h>

#include <emmintrin.h>
#include <immintrin.h>
#include <pthread.h>
#include <sched.h>
#include <sys/socket.h>
#include <sys/un.h>
#include <unistd.h>

#include <new>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "ovl.h"
#include "ovl_encode.h"
#include "ovl_scan.h"
#include "ovl_expand.h"
#include "ovl_pool.h"
#include "ovl_kernels.h"
#include "ovl_resident.h"
#include "ovl_worker.h"
#include "ovl_digest.h"
#include "ovl_score_range.h"
#include "ovl_pair_layout.h"

#define OVL_API extern "C" __attribute__((visibility("default")))

constexpr int32_t kFastMaxLen = 256;   // bit-plane layouts up to W = 8 words of 32 bases
constexpr int32_t kDpMaxLen = 8192;    // DP kernel: LDS row of the t read
constexpr int32_t kLaneMaxLen = 1024;  // lane-per-pair DP: hand-off column buffer per wavefront slot
constexpr int kSlots = 3;              // pipeline depth: staging slots / events per device
// Host memory that kernels store into and host code reads within one call (staging slots, the error
// flag): fine-grained, whose device stores snoop the CPU caches, so a line the host read in an earlier call
// is never returned stale.  (HIP's default for hipHostMalloc, with HIP_HOST_COHERENT unset, is the
// coarse-grained kind.)
constexpr unsigned kHostShared = hipHostMallocPortable | hipHostMallocCoherent;

// Device memory that goes with its owner: freed when the Dev (or whatever holds it) is deleted, unless it is a view.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool view = false;  // a part of another buffer (set_view): not freed, not grown
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p && !view) (void)hipFree(p);
    }
};

extern thread_local std::string g_err;  // ovl_last_error(NULL): this thread's last error (ovl_ctx.cpp)

// Test knobs, read from the environment once per context: they force a kernel form or a transport that the
// planner would otherwise pick by size or scoring, so the tests reach every form on small inputs.  (The A/B
// knobs of rounds 1-3 -- lane split, copy-engine transfers, spin waits, ordinary-store expansion, grid cap, heavy
// tiles, lane strip width and hand-off forms, read packing, pool spin, coarse-grained host memory -- are gone
// with the forms they measured; DESIGN.md records each measurement.  Round 5 merged the pairs of switches over one
// choice into one knob each -- OVL_DP_FORM, OVL_LANE_FORM, OVL_PAIRS_FORM -- and dropped the settled vector-width
// knobs of the host expansion and encoding: both run the widest form the CPU has.  The build macros of the A/B
// builds up to round 6 -- shift pairing and its word limit, the uniform and resident kernels' occupancies, the
// ablation modes, the lane kernels' mux profile, LDS hand-off, resident-slot grids, one-trip band loop and h2
// occupancy, the grid cap, the share wait and the dict builder's made-ahead dicts -- went the same way, each
// default folded into the code.)
struct Knobs {
    int32_t band_form = -1;       // OVL_BAND_FORM env (lane|diag|rows|fast|strip): band knob kernel (tests)
    // OVL_DP_FORM env, full-DP scoring (tests): auto (default: lane-per-pair from kLaneMinPairs pairs, else
    // dp_fast_kernel), lane (lane-per-pair forced), fast (dp_fast_kernel), classic (dp_kernel)
    int32_t dp_classic = 0;
    int32_t dp_lane = -1;         // -1 auto by list size, 0 off, 1 forced
    // OVL_LANE_FORM env, the lane kernels' inner form (tests), a bit mask, default 7: bit 0 scores by the byte
    // profile (else compare/select), bit 1 takes row symbols from the bit planes (else byte gathers), bit 2 lets
    // the full DP hold two pairs per lane as packed f16 cells (dp_lane_h2_kernel) where the scoring allows
    int32_t lane_prof = 1;
    int32_t lane_sfx = 1;
    int32_t lane_h2 = 1;
    int64_t pipe_chunk = 0;       // OVL_PIPE_CHUNK env: pairs per pipeline chunk (0 = automatic; tests)
    int32_t pack = 1;             // OVL_PACK: 0 host-array results cross the link as int32 pairs even when a packed
                                  // form holds; 1 (default) packed as 2 bytes per pair, expanded chunk by chunk
                                  // after each chunk's kernel, a last chunk stored as int32 meanwhile.  (Round 5's
                                  // streamed tile records, one launch whose records host threads expand while it
                                  // runs, were removed in round 6: target N = 1 / 2 / 8 0.144 / 0.081 / 0.050 ms
                                  // against 0.135 / 0.088 / 0.045, profiles/r05_stream_vs_packed_ab.json; its record
                                  // format lives on in the resident grid's ring)
    int64_t pack_min = 1 << 16;   // OVL_PACK_MIN: packed transport from this many pairs per call into pinned arrays
                                  // (64 K: a 250 K-pair shard -- N = 8 at the target point -- 0.057 -> 0.054 ms)
    int32_t pack_adapt = 1;       // the direct share follows the measured balance (pack_share); off when
                                  // OVL_PACK_DIRECT_PCT fixes it
    // OVL_PAIRS_FORM env, host pair lists over the link (tests): ix (default: the compact encoding, encode_chunk,
    // read in place by uniform_kernel as b16 + tile deltas where it can), decode (compact, always decoded into HBM
    // by the widen / runs kernels), plain (the caller's int32 arrays)
    int32_t compact = 1;
    int32_t pairs_ix = 1;
    // OVL_RESIDENT: scoring calls over the resident candidate list into host arrays go to the device's resident grid
    // (ovl_resident.h) -- 0 never (default: on the boxes measured it did not beat the launch pipeline, N = 1 or a
    // 1/8 shard -- profiles/r06_shard_steps.json), 1 from resident_min pairs up to resident_max, 2 at every size
    int32_t resident = 0;
    int64_t resident_min = 1;
    int64_t resident_max = int64_t(1) << 40;
    int32_t resident_blocks = 2;  // the grid's blocks of 256 threads per CU
    int32_t resident_pf = 1;      // its tiles software-pipelined (fewer, fatter wavefronts) or one at a time
    int32_t resident_sleep = 4;   // its non-lead blocks' pause between polls (~0.1 us units)
    int32_t resident_ring = 0;    // its ring's memory (ResidentGrid::ring_kind)
    int32_t local_batch_waves = 0; // OVL_LOCAL_BATCH_WAVES: cap on the wavefronts of ovl_local_align_batch's
                                  // kernel (0: none; tests reach slab reuse with a handful of queries)
    int32_t tr_window = 0;        // OVL_TR_WINDOW: entries of a node's out-row held in LDS per pass of
                                  // ovl_transitive_reduce (0: kReduceWindow; tests force several passes)
    int32_t read_best_chunk = 0;  // OVL_READ_BEST_CHUNK: contigs per launch of ovl_read_best's score pass (0: what
                                  // the tile budget allows; tests force several chunks)
    int32_t consensus_chunk = 0;  // OVL_CONSENSUS_CHUNK: reads per chunk of ovl_consensus (0: what the ops budget
                                  // allows; tests force several chunks)
    int32_t seed_keep = 1;        // OVL_SEED_GROUPS env (keep|search): ovl_seed_candidates' emit pass takes every
                                  // offset's group from HBM, where the count pass left it (default), or searches it
                                  // again: PhiX N = 50,000, k = 12, the emit kernel 69 us against 294 us, the whole
                                  // call 0.47 ms against 0.69 ms (profiles/seed_candidates.json; tests run both)
    int32_t reach_window = 0;     // OVL_REACH_WINDOW: columns (bits) of the reachability rows that ovl_reach_reduce's
                                  // marking holds in registers per pass (0: 16,384; tests force several passes)
    int32_t layout_runs = 1;      // OVL_LAYOUT_LINK env (runs|plain): the layout's link kernel reduces runs of equal a
                                  // inside the wavefront before its atomics (default), or issues one atomic per
                                  // eligible pair (the measurement: DESIGN.md 4.15; tests run both)
    int32_t spec_bins = 0;        // OVL_SPECTRUM_BINS: bins of the device histogram that ovl_correct_reads takes its
                                  // threshold from (0: 1,024, the most; at least 4).  A first valley past the exact
                                  // bins is taken from the counts themselves (tests reach that with 4 bins)
    int32_t spec_ballot = 0;      // OVL_SPECTRUM_VOTE env (atomic|ballot): ovl_correct_reads' correction pass counts a
                                  // solid work item with one LDS atomic (default) or by ballot, one add per segment:
                                  // PhiX N = 50,000, k = 12, the pass 0.617 ms against 0.613 ms, inside the spreads
                                  // (profiles/spectrum.json; tests run both)
    int32_t pack_direct_pct = 18; // OVL_PACK_DIRECT_PCT: packed calls into pinned arrays store this share of the
                                  // pairs (the last chunk) as int32 straight into them, over the link while the
                                  // host expands the packed chunks (tools/pack_ab.py, target point, six
                                  // processes: 0 % 0.16-0.26 ms, 10 % 0.16-0.25, 18 % 0.157-0.226, 25 % 0.175-0.209)
};

// Lane-per-pair DP kernels from this many pairs per launch (one 64-pair tile per SIMD); below, a wavefront per pair
constexpr int64_t kLaneMinPairs = 65536;
// uniform_kernel grid cap, blocks of 256 per CU: ~1 tile per wavefront at the target point, the dispatcher
// balances the tail (measured -2.3 % against 8 per CU; 16 / 32 / 64: 69.2 / 68.6 / 68.4 us)
constexpr int64_t kBlocksPerCu = 32;
// band knob: two lanes per pair (band_lane2_kernel) from this half-width.  Measured at cfg5 (tools/band_ab.py,
// profiles/r04_band_lane_ab.json, ms one lane / two lanes): 40: 6.07 / 6.99, 48: 7.13 / 8.04, 56: 8.29 / 9.09,
// 64: 10.50 / 10.17 -- two lanes only pay where one lane's 129 band cells leave one wavefront per SIMD.  With
// the row table built once per row (profiles/r04_band_table_ab.json): 48: 6.60 / 7.59, 64: 10.52 / 9.63
constexpr int32_t kBandLane2Min = 64;
// uniform_kernel's latency mode (two wavefronts per tile) up to this many 64-pair tiles per CU in a launch: a
// rank's shard at N = 4 / 8 (0.5 M / 0.25 M pairs) 0.068 -> 0.062 / 0.051 -> 0.047 ms per step, the whole list's
// 0.87 M-pair chunks unchanged in throughput mode, 64 tiles per CU (those chunks too) slower: 0.141 -> 0.153 ms
// (tools/gpu_r04_lat.sh, profiles/r04_lat_mode_ab.json).  Host-encoded lists keep 8: only throughput mode reads
// them in place.
constexpr int64_t kLatTiles = 32;
constexpr int64_t kLatTilesIx = 8;
// compact host pair lists from this many pairs per call
constexpr int64_t kCompactMin = int64_t(1) << 16;
// host expansion of packed results: pairs per pool part at least (finer parts than 64 K: the expansion of a
// 250 K-pair shard 22.7 -> 9.4 us, the N = 4 step 0.085 -> 0.075 ms; tools/pool_probe.cpp,
// profiles/r04_pool_ab_*.json)
constexpr size_t kExpandPart = size_t(1) << 14;

struct ovl_ctx;
struct Dev;

// ovl_last_score_form: the form the first scoring launch of the last scoring call took (launch_score_chunk records
// it while `open`, which the call's entry sets)
struct ScoreForm {
    bool open = false;
    int32_t kernel = OVL_KERNEL_NONE, key64 = 0, wide = 0;
    int32_t lane = 0, prof = 0, sfx = 0, ho = 0, h2 = 0;  // the lane-per-pair full DP and its arguments
    int32_t band_form = -1, split = 0;                    // the band knob's form (-1: none) and two lanes per pair
    int32_t rs_log2 = 0;                                  // the ungapped launch's rs_log2 (ungapped_rs_log2)
};

// The host side of a read-set upload in one pinned block (grown on demand, kept by the context): offsets,
// lengths, the length bitmap, the code table and the bytes (stage_reads).
struct ReadStage {
    char* p = nullptr;
    size_t bytes = 0;
    size_t o_off = 0, o_len = 0, o_full = 0, o_lut = 0, o_raw = 0, o_pk = 0;
};

// The host-side facts of a read set (prep_reads); kept by the context so that its arrays are reused, without
// fresh pages to fault in, by the next ovl_set_reads.
struct HostReads {
    std::vector<int64_t> off;
    std::vector<int32_t> len;
    std::vector<uint32_t> full;
    uint8_t lut[256];
    uint8_t inv[256];              // code -> byte (the layout spells contigs from the resident codes)
    const uint8_t* src = nullptr;  // the caller's bytes, then (stage_reads) their pinned copy
    int64_t total = 0;
    bool packed2 = false;          // every byte is A, C, G or T: the stage holds them 2-bit packed (o_pk)
    int32_t n_reads = 0, lmax = 0, planes = 2, wmax = 0, srow = 0, trow = 0;
};

struct ovl_ctx {
    std::vector<Dev*> devs;
    bool shared_slots = false;   // OVL_SHARE_DEVICES=1: a device listed more than once (tests); every call uses
                                 // every slot (no device cap, devices_for)
    ReadStage stage;             // pinned upload stage of ovl_set_reads
    HostReads hreads;            // ovl_set_reads' host arrays (reused)
    // the read set resident on every device after the last complete ovl_set_reads: its offsets relative to
    // offsets[0] and a digest of its bytes, so that a call with the same read set (a graph build per k over one read set,
    // the one-shot ovl_score_pairs per build) keeps it instead of uploading and packing it again
    std::vector<int64_t> res_off;
    int64_t res_total = 0;
    uint64_t res_hash[2] = {0, 0};  // reads_hash of its bytes
    bool res_valid = false;
    std::string err;
    std::vector<int32_t> h_len;  // read lengths (shard balance of host pair lists)
    int32_t timing = 0;          // ovl_set_timing
    double t_kernel_ms = 0.0, t_call_ms = 0.0;
    struct Launch {
        int32_t device, sink;
        int64_t pairs;
        double ms;
    };
    std::vector<Launch> t_launches;  // timing on: every scoring launch of the last host-array call
    int64_t x_link_bytes = 0, x_packed_pairs = 0;  // ovl_last_transfer
    int64_t x_res_bytes = 0, x_rec_pairs = 0, x_esc = 0;  // ovl_last_results
    int64_t x_ix_pairs = 0, x_dec_pairs = 0;       // ovl_last_pair_list
};

int fail(const ovl_ctx* c, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int fail(const Dev* d, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));

#define HIPCHK(ctx, expr)                                                                           \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail((ctx), e_ == hipErrorOutOfMemory ? OVL_E_OOM : OVL_E_HIP, "%s: %s", #expr, \
                        hipGetErrorString(e_));                                                     \
    } while (0)

inline hipError_t ensure(DevBuf& b, size_t bytes) {
    if (bytes < 16) bytes = 16;
    if (b.view) return hipErrorInvalidValue;
    if (b.bytes >= bytes) return hipSuccess;
    if (b.p) {
        hipError_t e = hipFree(b.p);
        b.p = nullptr;
        b.bytes = 0;
        if (e != hipSuccess) return e;
    }
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e == hipSuccess) b.bytes = bytes;
    return e;
}

inline void release(DevBuf& b) {
    if (b.p && !b.view) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
    b.view = false;
}

inline void set_view(DevBuf& v, DevBuf& whole, size_t offset, size_t bytes) {
    v.p = static_cast<char*>(whole.p) + offset;
    v.bytes = bytes;
    v.view = true;
}

template <typename T>
T* as(DevBuf& b) { return reinterpret_cast<T*>(b.p); }

// Restores the caller's current device when a public entry point returns.
struct DeviceGuard {
    int dev = -1;
    DeviceGuard() {
        if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    }
    ~DeviceGuard() {
        if (dev >= 0) (void)hipSetDevice(dev);
    }
};

void quiet(ovl_ctx* c);  // ovl_ctx.cpp

#include "ovl_stage.h"

// Per-device state.
struct Dev {
    ovl_ctx* owner = nullptr;
    int32_t device = 0;
    hipStream_t stream = nullptr;  // kernels
    hipStream_t s_in = nullptr;    // host-array calls: the pair list's copies and decodes, beside the kernels
    int32_t cu_count = 256;
    Knobs k;
    ScoreForm form;
    // resident reads
    int32_t n_reads = -1;
    int32_t lmax = 0;
    int32_t planes = 2;
    int32_t wmax = 0;  // 0: no bit-plane layout (reads longer than kFastMaxLen)
    int32_t srow = 0;  // sfx row stride (words)
    int32_t trow = 0;  // pfx row stride (words)
    DevBuf codes, off, len, sfx, pfx, lut, full;  // full: bit r set iff len[r] == lmax
    DevBuf raw;                                   // the uploaded read bytes (raw or 2-bit packed)
    DevBuf rd;  // ovl_set_reads' upload block, the stage's layout; off, len, full, lut and raw are views into it
    // scratch
    DevBuf a, b, score, end, tb, err_flag;
    DevBuf lane_col;      // lane-per-pair DP: per-wavefront strip hand-off columns
    DevBuf seed_s, seed_e;  // band knob: the ungapped seed (score, j*) of each pair
    hipEvent_t scratch_evt = nullptr;     // last launch that used lane_col / seed_* ...
    hipEvent_t ev_last = nullptr;         // packed calls into pinned arrays: after the last (direct) chunk
    double pack_pct = -1.0;               // live direct share of packed calls into pinned arrays (pack_share)
    double pack_pct_h = -1.0;             // the same for calls with a compact host pair list (the host also
                                          // encodes the list, so its balance point differs)
    hipStream_t scratch_stream = nullptr; // ... and its stream (launches on other streams wait for it)
    bool scratch_used = false;
    int64_t codes_bytes = 0;
    // device candidate enumeration (ovl_candidates): per-read keys / groups and the pair list
    DevBuf k_pre, k_suf, k_sorted, k_iota, k_order, k_lo, k_hi, k_cnt, k_offs, k_temp, cand_a, cand_b;
    int64_t cand_n = -1;  // -1: no candidate list for the resident reads
    bool cand_seed = false;  // the resident list came from ovl_seed_candidates (its offsets: sd.offs)
    // heavy tiles of the candidate list (tiles holding side pairs, scheduled first: uniform_kernel), built on
    // the first throughput-mode launch over the list (ensure_heavy)
    DevBuf tile_flags, heavy_ids;
    std::vector<int32_t> h_heavy;
    int64_t heavy_for = -1;  // cand_n the heavy tiles were built for (-1: none)
    int64_t cand_tail[2] = {0, 0};
    DevBuf sh_cum, sh_temp, sh_cuts;  // shard bounds (ovl_candidates_shards)
    // local alignment (ovl_local_align): query / reference bytes, carried rows, progress, traceback
    DevBuf l_q, l_r, l_row, l_tb, l_best;
    uint32_t l_epoch = 0;  // tags this launch's row hand-off words (l_row is zeroed when allocated)
    // pinned host copy of the part of the traceback table the walk can reach (grown on demand)
    int8_t* l_tb_host = nullptr;
    size_t l_tb_host_bytes = 0;
    // the stages, each with its buffers, its timer and what its last call reports (ovl_stage.h)
    SeedState sd;
    LocalBatchState lb;
    TransitiveState tr;
    ReachState rc;
    ReadBestState rb;
    ConsensusState cs;
    PlacedState pl;
    LayoutState ly;
    SpectrumState sp;
    UnitigsState ug;
    // host-array pipeline: events per slot and pinned staging (slots x cap pairs x {a, b} / {score, end})
    hipEvent_t ev_k[kSlots] = {};
    int32_t* st_in = nullptr;
    int32_t* st_out = nullptr;
    int32_t* st_in_dev = nullptr;   // device addresses of the staging rings (kernels read / store them)
    int32_t* st_out_dev = nullptr;
    int64_t st_cap = 0;
    uint32_t* h_flag = nullptr;      // pinned error flag of host-array calls (the kernels store into it)
    uint32_t* h_flag_dev = nullptr;  // its device address
    std::vector<hipEvent_t> t_ev;  // timing: kernel start/end per chunk (recorded on the stream around the launch)
    std::vector<hipEvent_t> k_ev;  // timing: the same recorded by an ungapped launch itself (kernel start / end)
    // compact host pair lists (encode_chunk): pinned encoding buffer (PairLayout::job_bytes), its device
    // address, a decode event per chunk, and the encoded bytes of the last call
    char* cp_host = nullptr;
    char* cp_dev = nullptr;
    size_t cp_bytes = 0;
    DevBuf cp_hbm;  // the in-place encoding's chunks copied into HBM (same layout as cp_host)
    std::vector<hipEvent_t> dec_ev;
    int64_t cp_link = 0;
    ResidentGrid res;  // the resident scoring grid (ovl_resident.h), launched by the first call that uses it
    std::unique_ptr<DevWorker> worker;  // multi-device contexts: this device's host thread (run_pipeline)
};

struct Plan {
    int kernel = OVL_KERNEL_NONE;
    bool key64 = false;
    bool wide = true;
    int32_t band = -1;       // OVL_KERNEL_BANDED: band half-width
    int seed_kernel = OVL_KERNEL_NONE;  // OVL_KERNEL_BANDED: how the seed end j* is computed
    bool seed_key64 = false;
    bool seed_wide = true;
};

// What a scoring launch takes (launch_score): the scores, the pair list and the result arrays as the device addresses
// them, and in LaunchIo everything else that differs between callers.  A default LaunchIo is a device call's: results
// into HBM, the device's own error flag, int32 pair arrays, no kernel timing.
struct Scoring { int32_t match = 0, mismatch = 0; int64_t indel = 0; };
struct PairList { const int32_t* a = nullptr; const int32_t* b = nullptr; int64_t n = 0; };
struct ScoreOut { int32_t* score = nullptr; int32_t* end = nullptr; };
struct LaunchIo {
    int32_t sink = 0;           // results (OvlUngappedArgs::host_out): 0 HBM, 1 host-mapped int32, 2 host-mapped packed
    uint32_t* flag = nullptr;   // the error flag the kernels write; null: the device's err_flag
    const uint16_t* ix_b16 = nullptr;  // non-null: the pair list in the host encoding, read in place instead of
    const uint8_t* ix_d8 = nullptr;    // PairList's arrays (OvlUngappedArgs::ix_*; only a launch that ix_launch admits)
    const int32_t* ix_base = nullptr;
    hipEvent_t kev_start = nullptr, kev_stop = nullptr;  // timing: uniform_kernel records these itself, once
    bool timed = false;         // out: it did (else the caller times the launch on the stream)
};

struct Call {
    const Plan* plan = nullptr;
    Scoring sc;
    const int32_t* h_a = nullptr;  // host pair list (global indexing), or null: device lists per job
    const int32_t* h_b = nullptr;
    bool in_pinned = false;
    int32_t* out_s = nullptr;      // host results; out_s[p - out_base] for global pair p
    int32_t* out_e = nullptr;
    int64_t out_base = 0;
    bool out_pinned = false;
    bool pack = false;             // results cross the link packed (2 bytes per pair) into the staging
                                   // slots and are expanded into the caller's arrays on the host (all chunks for
                                   // pageable arrays; for pinned ones all but a last direct chunk, Job::n_packed)
    bool compact = false;          // one device: the host pair list is encoded per chunk (encode_chunk)
                                   // and decoded into HBM by kernels reading it through the host mapping
    bool timing = false;
};

struct Job {
    Dev* d = nullptr;
    int64_t lo = 0, hi = 0;  // global pair range of this device
    int64_t chunk = 1;       // largest chunk (the staging slot capacity)
    std::vector<int64_t> cb; // chunk k: pairs [cb[k], cb[k + 1]) of the range (local indexing)
    int64_t nchunks = 0;
    int64_t n_packed = 0;    // C.pack: the first n_packed chunks are packed and staged
    const int32_t* dev_a = nullptr;  // device pair list (global indexing) when the call has no host list
    const int32_t* dev_b = nullptr;
    int32_t* ka = nullptr;  // device copies of the host list (local indexing)
    int32_t* kb = nullptr;
    const int32_t* za = nullptr;  // direct: device addresses of the caller's pinned pair arrays (local indexing)
    const int32_t* zb = nullptr;
    int32_t* d_score = nullptr;  // device results (local indexing)
    int32_t* d_end = nullptr;
    std::vector<uint8_t> ixk;    // C.compact: chunk k's list is read in place by uniform_kernel (encode_chunk)
    std::vector<uint8_t> kexact; // timing: chunk k's kernel recorded its own start / end (k_ev)
    int64_t drained = 0;         // chunks [0, drained) are drained (run_pipeline)
};

inline int32_t chunk_sink(const Job& J, int64_t k) { return k < J.n_packed ? 2 : 1; }  // LaunchIo::sink of chunk k
inline int chunk_slot(const Job&, int64_t k) { return (int)(k % kSlots); }              // its staging slot

// OVL_TRACE_PIPE=1 (diagnostics): one stderr line per host-array call with the microsecond offsets of its
// pipeline events (s setup, i<k> chunk k issued, w<k> its results ready on the host side, d<k> drained,
// y final synchronisation; streamed records: f<k> the calling thread's first record expanded, p<k> its part
// done, k<k> the chunk's kernel seen finished).
struct PipeTrace {
    bool on;
    std::chrono::steady_clock::time_point t0;
    std::string line;
    PipeTrace() : on(enabled()), t0(std::chrono::steady_clock::now()) {}
    static bool enabled() {
        static const bool e = [] {
            const char* v = getenv("OVL_TRACE_PIPE");
            return v && atoi(v) != 0;
        }();
        return e;
    }
    void mark(char what, int64_t k) {
        if (!on) return;
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        char buf[48];
        snprintf(buf, sizeof(buf), " %c%lld=%.1f", what, (long long)k, us);
        line += buf;
    }
    ~PipeTrace() {
        if (on) fprintf(stderr, "ovl_pipe:%s\n", line.c_str());
    }
};

// ovl_ctx.cpp
void free_staging(int32_t*& p);
hipError_t alloc_staging(int32_t*& p, int32_t*& p_dev, int64_t cap);
bool host_pinned(const void* p, size_t bytes);
// ovl_plan.cpp
int launch_score(Dev* c, const Plan& pl, const PairList& pairs, const Scoring& sc, const ScoreOut& out, LaunchIo& io,
                 hipStream_t s);
int ensure_heavy(Dev* c);
struct HeavyWindow {
    const int32_t* ids = nullptr;  // device address of the window's ascending tile ids
    int64_t count = 0, tile_base = 0;
};
HeavyWindow heavy_window(const Dev* c, int64_t lo, int64_t n_pairs);
bool ix_launch(const Dev* c, int64_t n_pairs);
int check_scoring_args(ovl_ctx* c, int32_t match, int32_t mismatch, int64_t indel, int32_t band, Plan* p);
// ovl_pipeline.cpp
void host_copy(void* dst, const void* src, size_t bytes);
int run_pipeline(ovl_ctx* c, const Call& C, std::vector<Job>& jobs);
Call make_call(ovl_ctx* c, const Plan& p, const Scoring& sc, const int32_t* h_a, const int32_t* h_b, int64_t n_pairs,
               int32_t* out_s, int32_t* out_e, int64_t out_base, int32_t* n_devices);
std::vector<Job> jobs_from_cuts(ovl_ctx* c, const std::vector<int64_t>& cuts, bool resident_list);
int device_cuts(Dev* d, int64_t lo, int64_t hi, int32_t shards, std::vector<int64_t>& cuts);
bool pack_ok(const ovl_ctx* c, const Plan& p, int64_t n_pairs, bool out_pinned, int32_t n_devices);
int32_t devices_for(const ovl_ctx* c, int64_t n_pairs);
int32_t devices_used(const ovl_ctx* c, int64_t n_pairs);
// ovl_reach_api.cpp: the closure and marking launches of ovl_reach.hip over a CSR that is in device memory (a->off,
// head, order, n_nodes, n_order, words and reduced set by the caller, reduced zeroed; the matrix and the pivot rows are
// the reach stage's own buffers, grown here), and the marking's column window in words (OVL_REACH_WINDOW)
int reach_launches(Dev* c, OvlReachArgs* a, bool closure, hipStream_t s);
int32_t reach_window_words(const Dev* c);
// ovl_reads.cpp
int set_reads(ovl_ctx* c, const uint8_t* seqs, const int64_t* offsets, int32_t n_reads, bool sync);
