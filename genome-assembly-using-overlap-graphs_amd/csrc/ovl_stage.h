// ovl_stage.h — what every stage of the library (seed candidates, batched local alignment, the two graph reductions,
// read depth, the two consensus forms, layout, read correction, the unitig pipeline) has on the host: a timer for its phases, the scope of
// one call, and its state on the device it runs on.  Host only and header only.  ovl_ctx.h includes it between the
// context, which the call scope writes, and Dev, which holds one member per state struct below.
//
// A new stage declares a struct here -- its DevBufs, a StageTimer<N> for N marks, and `last`, what its ovl_last_*
// getters report -- and one member of Dev.  For that its buffers and events are freed with the device (delete: nothing
// to add to destroy_dev), and its call is:
//     StageCall call(ctx);                       quiet, the caller's device kept, the wall clock
//     ... argument checks ...                    (a refused call leaves the last call's figures alone)
//     call.begin();  st.last = {};               from here the figures are this call's
//     HIPCHK(c, st.timer.arm(ctx->timing));
//     HIPCHK(c, st.timer.mark(0, s));  launch;  HIPCHK(c, st.timer.mark(1, s));  ... synchronise ...
//     return call.done(st.timer.ms(0, 1));
// Tables that share a buffer: one lay_*(Carve&, args) per block, run without a base to size it, then over the buffer.
// Copies from or into host memory: a StreamDrain declared after that memory, disarmed after the last synchronise.
#pragma once

// The events of a stage's phases.  Made by the first call that has timing on, destroyed with the device.  With timing
// off no member issues a HIP call.
template <int N>
struct StageTimer {
    hipEvent_t ev[N] = {};
    bool on = false;  // the call that armed it last records
    StageTimer() = default;
    StageTimer(const StageTimer&) = delete;
    StageTimer& operator=(const StageTimer&) = delete;
    ~StageTimer() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    // once per call, before its first mark
    hipError_t arm(bool timing) {
        on = timing;
        for (hipEvent_t& e : ev) {
            const hipError_t r = !on || e ? hipSuccess : hipEventCreate(&e);
            if (r != hipSuccess) return r;
        }
        return hipSuccess;
    }
    hipError_t mark(int i, hipStream_t s) { return on ? hipEventRecord(ev[i], s) : hipSuccess; }
    // after the stream is synchronised: the time from mark i to mark j; 0 with timing off or where it cannot be read
    double ms(int i, int j) const {
        float v = 0.f;
        return on && hipEventElapsedTime(&v, ev[i], ev[j]) == hipSuccess ? (double)v : 0.0;
    }
};

// One call of a stage, on the context's first device.  Construct it where the call starts, begin() where the stage
// zeroes its own figures (after the argument checks), done() at the successful return: ovl_last_timing's pair is
// zeroed and stored there.  Anything a stage does differently about the pair stands in the stage as a line of its own.
struct StageCall {
    ovl_ctx* ctx;
    Dev* dev;
    DeviceGuard guard;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit StageCall(ovl_ctx* c) : ctx(c), dev(c->devs[0]) { quiet(c); }
    void begin() { ctx->t_kernel_ms = ctx->t_call_ms = 0.0; }
    int done(double kernel_ms) {
        ctx->t_kernel_ms = kernel_ms;
        ctx->t_call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return OVL_OK;
    }
};

// Waits for the compute stream of every device of the context, whatever `rc` says; the first error is kept.  (A
// template only to stand here, ahead of Dev.)
template <typename Ctx>
int sync_devices(Ctx* ctx, int rc, const char* what) {
    for (auto* d : ctx->devs) {
        (void)hipSetDevice(d->device);
        const hipError_t e = hipStreamSynchronize(d->stream);
        if (rc == OVL_OK && e != hipSuccess) rc = fail(ctx, OVL_E_HIP, "%s: %s", what, hipGetErrorString(e));
    }
    return rc;
}

// From a call's first copy enqueued to its return: whichever way the call leaves, the stream is drained before the
// host memory its copies read or write (the call's own vectors, the caller's arrays) can go away.  Declared in the
// frame that owns that memory and after it, so it goes first; disarmed at the successful return, just after the call's
// own last synchronise.
struct StreamDrain {
    hipStream_t s;
    bool armed = true;
    explicit StreamDrain(hipStream_t stream) : s(stream) {}
    StreamDrain(const StreamDrain&) = delete;
    StreamDrain& operator=(const StreamDrain&) = delete;
    ~StreamDrain() {
        if (armed) (void)hipStreamSynchronize(s);
    }
};

inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

// A block of device tables laid out one after the other, each on a 256-byte boundary.  Without a base it sizes: take
// returns NULL and only `at`, the block's bytes so far, moves.  With a buffer's address it places.
struct Carve {
    char* base = nullptr;
    size_t at = 0;
    Carve() = default;
    explicit Carve(void* buffer) : base(static_cast<char*>(buffer)) {}
    template <typename T>
    T* take(size_t count) {
        const size_t o = at;
        at = al256(at + sizeof(T) * count);
        return base ? static_cast<T*>(static_cast<void*>(base + o)) : nullptr;
    }
    // where a placed table starts in the block
    size_t offset_of(const void* table) const { return (size_t)(static_cast<const char*>(table) - base); }
};

// A table the kernels only read (const in their argument struct), for the call that owns its block and fills it.
template <typename T>
T* writable(const T* p) { return const_cast<T*>(p); }

// OVL_E_UNSUPPORTED when `need` bytes of a stage's buffers exceed what the device has free plus what those buffers
// (`held`) hold already; `what` names the bytes in the message.
inline int check_fits(const Dev* c, const char* stage, const char* what, size_t need,
                      std::initializer_list<const DevBuf*> held) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    for (const DevBuf* b : held) free_b += b->bytes;
    if (need > free_b)
        return fail(c, OVL_E_UNSUPPORTED, "%s: %zu bytes of %s do not fit the device (%zu free)", stage, need, what,
                    free_b);
    return OVL_OK;
}

// ----------------------------------------------------------------------------- the stages' states

// seed candidates (ovl_cand.cpp): the offset of each pair of the resident list, and every offset's group (count pass
// -> emit pass).  Marks: before the keys, after them, the sort, the count + scan; around the emit
struct SeedState {
    DevBuf offs, glo, gn;
    StageTimer<6> timer;
    struct Last {
        double ms[4] = {};  // ovl_last_seed_timing
    } last;
};

// batched local alignment (ovl_local_api.cpp): the upload block (items, query bytes, reference), the two counters,
// per-wavefront rows / traceback slabs / op scratch, and the results (a record per query, packed ops).  Marks: around
// the batch kernel
struct LocalBatchState {
    DevBuf in, ctr, rows, slabs, wops, out, ops;
    StageTimer<2> timer;
    struct Last {
        int32_t batched = 0, single = 0, waves = 0;  // ovl_last_local_batch
    } last;
};

// transitive reduction (ovl_reduce_api.cpp): the CSR, the node order, the counter and the mask.  Marks: around the
// reduction kernel
struct TransitiveState {
    DevBuf off, edge, order, ctr, out;
    StageTimer<2> timer;
    struct Last {
        int32_t window = 0, passes = 0;  // ovl_last_transitive
        int64_t steps = 0;
    } last;
};

// reachability reduction (ovl_reach_api.cpp): the CSR, the node order, the bit matrix, the pivot rows, the mask.
// Marks: around all of a call's launches
struct ReachState {
    DevBuf off, head, order, matrix, pivot, out;
    StageTimer<2> timer;
    struct Last {
        int32_t words = 0, blocks = 0, window = 0;  // ovl_last_reach
    } last;
};

// read depth (ovl_depth_api.cpp): the upload block (padded reads, lengths, contigs, their offsets and lengths), a
// chunk's score / cell tile, the per-read results and the tie bits.  Marks: around the score pass and its folds
struct ReadBestState {
    DevBuf in, tile, res, bits;
    StageTimer<2> timer;
    struct Last {
        int64_t lane = 0, fallback = 0;  // ovl_last_read_best
        int32_t launches = 0;
    } last;
};

// consensus (ovl_consensus_api.cpp): the contigs' bytes, the vote counts (6 int32 per base), the called bytes, the
// counters {n_other, n_changed, bad ops}, and the flat count indices of the single-pair reads' votes.  Marks: a
// chunk's start, after its alignment launch, after its pileup; the vote
struct ConsensusState {
    DevBuf ref, counts, called, ctr, hits;
    StageTimer<4> timer;
    struct Last {
        int64_t batch = 0, single = 0, ops = 0;  // ovl_last_consensus
        int32_t launches = 0;
        double ms[3] = {};                       // ovl_last_consensus_timing
    } last;
};

// placed consensus (ovl_consensus_placed_api.cpp; the contigs, counts, called bytes and counters are ConsensusState's,
// Dev::cs): the upload block (items, the reads' bytes), a chunk's code words ([row][lane]) and three int32 per read.
// Marks: a round's start, after its band launches, after its vote
struct PlacedState {
    DevBuf in, slab, aln;
    StageTimer<3> timer;
    struct Last {
        int64_t voted = 0, windowless = 0, ops = 0;  // ovl_last_consensus_placed
        int32_t launches = 0, rounds = 0;
        double ms[2] = {};                           // ovl_last_consensus_placed_timing
    } last;
};

// layout (ovl_layout_api.cpp): the call's inputs (ovl_layout: lengths, offsets, bytes and the four columns;
// ovl_layout_candidates: the score and end columns and the code table), the per-read block (lay_layout_work), the
// contigs' bytes and the scan's scratch.  Marks: before and after the scoring launches, the link kernel, the forest,
// the spelling
struct LayoutState {
    DevBuf in, work, bases, temp;
    StageTimer<5> timer;
    struct Last {
        int64_t links = 0, cycles = 0, on_path = 0;  // ovl_last_layout
        int32_t levels = 0;
        double ms[4] = {};                           // ovl_last_layout_timing
    } last;
};

// read correction (ovl_spectrum_api.cpp): the call's upload (offsets, window offsets, bytes) and its tables
// (lay_spectrum_work: keys, sorted keys, head flags and their scan, run starts, counts, histogram, counters, outputs).
// Marks: before the keys, after them, the sort, the count pass; around the correction
struct SpectrumState {
    DevBuf in, work;
    StageTimer<6> timer;
    struct Last {
        double ms[4] = {};  // ovl_last_correct_timing
    } last;
};

// unitig pipeline from the score columns (ovl_unitigs_api.cpp; the matrix and the pivot rows are ReachState's,
// Dev::rc): the call's inputs (ids, first, prev, the self column's index and, per form, the uploaded or scored
// columns), the per-node block (degrees, offsets, the marking's order, the node facts), the per-edge block (the CSR's
// columns, the mask, the kept flags and their scan, the kept edges' columns) and the scans' scratch.  Marks: before and
// after the scoring launches, the edge build, the closure and marking, the node facts and the kept edges
struct UnitigsState {
    DevBuf in, node, edge, temp;
    int64_t kept = -1;  // kept edges in `edge` (ovl_unitigs_edges_copy), -1: none
    const int32_t* kept_at[4] = {};  // their columns, placed
    StageTimer<5> timer;
    struct Last {
        int64_t edges = 0, kept = 0;  // ovl_last_unitigs
        int32_t paths = 0, words = 0;
        double ms[4] = {};            // ovl_last_unitigs_timing
    } last;
};
