// stage_block_check.cpp — the carver of csrc/ovl_stage.h (Carve) and the device blocks that the layout, the read
// correction and the unitig pipeline lay out with it, as a stand-alone program for a sanitizer build on a machine
// without a GPU:
//
//     make -C genome-assembly-using-overlap-graphs_amd/csrc stage-block-check
//
// compiles this file and the three API files with -fsanitize=address,undefined (host side) and runs the result.  A
// block is carved twice, without a base (the sizing pass) and over a host buffer of exactly the sized bytes (the
// placing pass): both end at the same byte, the sizing pass hands out only NULL, every placed table starts on a
// 256-byte boundary inside the buffer and holds its bytes ahead of the next (each table is filled here, so a table
// that ran past the buffer would stop the program under AddressSanitizer).  The tables' bytes are restated here from
// the kernels' needs; nothing of the device calls runs: their launches, the scoring and the context helpers are stubs.
#include "host_check.h"
#include "ovl_layout.h"
#include "ovl_spectrum.h"
#include "ovl_unitigs.h"

#define STUB(name, ...) \
    extern "C" hipError_t name(__VA_ARGS__) { return hipErrorNotSupported; }
STUB(ovl_launch_layout_link, const OvlLayoutArgs*, int32_t, hipStream_t)
STUB(ovl_launch_layout_double, const OvlLayoutArgs*, int32_t, hipStream_t)
STUB(ovl_launch_layout_cut, const OvlLayoutArgs*, hipStream_t)
STUB(ovl_layout_scan_bytes, int32_t, size_t*)
STUB(ovl_launch_layout_place, const OvlLayoutArgs*, void*, size_t, hipStream_t)
STUB(ovl_launch_layout_spell, const OvlLayoutArgs*, int32_t, hipStream_t)
STUB(ovl_spectrum_temp_bytes, int64_t, int32_t, size_t*)
STUB(ovl_launch_spectrum_keys, const OvlSpectrumArgs*, hipStream_t)
STUB(ovl_launch_spectrum_sort, const OvlSpectrumArgs*, void*, size_t, hipStream_t)
STUB(ovl_launch_spectrum_heads, const OvlSpectrumArgs*, void*, size_t, hipStream_t)
STUB(ovl_launch_spectrum_counts, const OvlSpectrumArgs*, hipStream_t)
STUB(ovl_launch_spectrum_correct, const OvlSpectrumArgs*, int32_t, hipStream_t)
STUB(ovl_launch_unitigs_degree, const OvlUnitigArgs*, hipStream_t)
STUB(ovl_unitigs_scan_bytes, int64_t, size_t*)
STUB(ovl_launch_unitigs_offsets, const OvlUnitigArgs*, void*, size_t, hipStream_t)
STUB(ovl_launch_unitigs_fill, const OvlUnitigArgs*, hipStream_t)
STUB(ovl_launch_unitigs_facts, const OvlUnitigArgs*, hipStream_t)
STUB(ovl_launch_unitigs_kept, const OvlUnitigArgs*, void*, size_t, hipStream_t)
int reach_launches(Dev*, OvlReachArgs*, bool, hipStream_t) { return OVL_E_HIP; }
int launch_score(Dev*, const Plan&, const PairList&, const Scoring&, const ScoreOut&, LaunchIo&, hipStream_t) {
    return OVL_E_HIP;
}
int check_scoring_args(ovl_ctx*, int32_t, int32_t, int64_t, int32_t, Plan*) { return OVL_E_HIP; }

// the stages' own blocks (csrc/ovl_layout_api.cpp, ovl_spectrum_api.cpp, ovl_unitigs_api.cpp)
void lay_layout_work(Carve&, OvlLayoutArgs&, int32_t n, int32_t levels);
void lay_spectrum_in(Carve&, OvlSpectrumArgs&, int32_t n_reads, int64_t total);
void* lay_spectrum_work(Carve&, OvlSpectrumArgs&, int32_t n_reads, int64_t n_win, int64_t total, size_t temp_bytes,
                        bool correct);
int32_t* lay_unitigs_in(Carve&, OvlUnitigArgs&, int32_t n, int32_t n_raw, size_t n_sx, size_t n_self);
int32_t* lay_unitigs_node(Carve&, OvlUnitigArgs&, int32_t n);
void lay_unitigs_edge(Carve&, OvlUnitigArgs&, int64_t n_edges);

struct Table {
    const void* p;
    size_t bytes;
};

// One block: lay(carve) carves it and returns its tables in carving order with the bytes each must hold.
template <typename Lay>
static void check_block(Lay&& lay) {
    Carve size;
    for (const Table& t : lay(size)) EXPECT(t.p == nullptr);
    EXPECT(size.at % 256 == 0);
    const size_t bytes = std::max<size_t>(size.at, 256);
    char* buf = static_cast<char*>(aligned_alloc(256, bytes));
    Carve place(buf);
    const std::vector<Table> tables = lay(place);
    EXPECT(place.at == size.at);
    const char* prev_end = buf;
    for (const Table& t : tables) {
        const char* p = static_cast<const char*>(t.p);
        EXPECT(p != nullptr && (uintptr_t)p % 256 == 0);
        EXPECT(p >= prev_end && p + t.bytes <= buf + size.at);
        if (p < prev_end || p + t.bytes > buf + size.at) break;
        EXPECT(place.offset_of(p) == (size_t)(p - buf));
        memset(const_cast<char*>(p), 0x5A, t.bytes);
        prev_end = p + t.bytes;
    }
    free(buf);
}

int main() {
    // the carver alone: every element size, counts that end on and next to a boundary, and tables of no entries
    for (size_t k : {size_t(0), size_t(1), size_t(31), size_t(32), size_t(33), size_t(255), size_t(256), size_t(257)})
        check_block([k](Carve& c) {
            std::vector<Table> t;
            t.push_back({c.take<uint8_t>(k), k});
            t.push_back({c.take<int32_t>(0), 0});
            t.push_back({c.take<int64_t>(k + 1), 8 * (k + 1)});
            t.push_back({c.take<int32_t>(k), 4 * k});
            t.push_back({c.take<uint8_t>(0), 0});
            t.push_back({c.take<unsigned long long>(8), 64});
            return t;
        });
    {
        Carve none;  // nothing taken: no bytes
        EXPECT(none.at == 0 && none.take<int64_t>(0) == nullptr && none.at == 0);
        EXPECT(none.take<uint8_t>(1) == nullptr && none.at == 256);
    }

    for (int32_t n : {0, 1, 63, 64, 65}) {
        const size_t N = (size_t)std::max(n, 1);
        // layout: the per-read block
        const int32_t levels = ovl_layout_levels(n);
        check_block([&](Carve& c) {
            OvlLayoutArgs g{};
            lay_layout_work(c, g, n, levels);
            EXPECT((void*)g.scan_in == (void*)g.mk[0] && (void*)g.scan_out == (void*)g.mk[1]);
            return std::vector<Table>{{g.best, 8 * N},     {g.mk[0], 8 * N},   {g.mk[1], 8 * N},
                                      {g.headkey, 8 * N},  {g.c_off, 8 * (N + 1)}, {g.link, 4 * N},
                                      {g.succ, 4 * N},     {g.tail[0], 4 * N}, {g.tail[1], 4 * N},
                                      {g.contig, 4 * N},   {g.offset, 4 * N},  {g.jump, 4 * N * ((size_t)levels + 1)},
                                      {g.on_path, N},      {g.on_cycle, N},    {g.ctr, 64}};
        });
        // read correction: reads of 20 bases, k = 12 (9 windows each); with and without the correction's outputs
        const int64_t total = 20 * (int64_t)n, n_win = 9 * (int64_t)n;
        const size_t W = (size_t)std::max<int64_t>(n_win, 1), T = (size_t)std::max<int64_t>(total, 1);
        check_block([&](Carve& c) {
            OvlSpectrumArgs g{};
            lay_spectrum_in(c, g, n, total);
            return std::vector<Table>{{g.off, 8 * (N + 1)}, {g.woff, 8 * (N + 1)}, {g.seqs, T}};
        });
        for (bool correct : {false, true})
            for (size_t temp : {size_t(0), size_t(1000)})
                check_block([&](Carve& c) {
                    OvlSpectrumArgs g{};
                    const void* d_temp = lay_spectrum_work(c, g, n, n_win, total, temp, correct);
                    EXPECT(g.spec_keys == g.keys);
                    return std::vector<Table>{{g.keys, 8 * (W + 1)},
                                              {g.sorted, 8 * W},
                                              {g.flag, 4 * W},
                                              {g.pos, 4 * W},
                                              {g.starts, 4 * (W + 2)},
                                              {g.spec_counts, 4 * (W + 1)},
                                              {g.hist, 4 * (size_t)kSpecHistBins},
                                              {g.ctr, 64},
                                              {g.out, correct ? T : 1},
                                              {g.changed, correct ? 4 * N : 4},
                                              {d_temp, temp}};
                });
        // the unitig pipeline: the node block, the edge block without an edge and with the most a list without copies
        // can have, and the input block of either form (no self pairs; n / 2 reads with a second copy)
        const size_t Z = (size_t)n, P = Z > 0 ? Z * (Z - 1) : 0;
        check_block([&](Carve& c) {
            OvlUnitigArgs g{};
            const int32_t* order = lay_unitigs_node(c, g, n);
            return std::vector<Table>{{g.deg, 8 * (Z + 1)}, {g.off, 8 * (Z + 1)}, {order, 4 * Z},   {g.outdeg, 4 * Z},
                                      {g.indeg, 4 * Z},     {g.nxt, 4 * Z},       {g.nend, 4 * Z}};
        });
        for (int64_t edges : {int64_t(0), (int64_t)(P / 2)}) {
            const size_t E = (size_t)edges;
            check_block([&](Carve& c) {
                OvlUnitigArgs g{};
                lay_unitigs_edge(c, g, edges);
                return std::vector<Table>{{g.tail, 4 * E},     {g.head, 4 * E},       {g.weight, 4 * E},
                                          {g.eend, 4 * E},     {g.reduced, E},        {g.keep, 4 * (E + 1)},
                                          {g.pos, 4 * (E + 1)}, {g.k_tail, 4 * E},    {g.k_head, 4 * E},
                                          {g.k_weight, 4 * E}, {g.k_end, 4 * E}};
            });
        }
        const size_t M = Z / 2, R = Z + M;  // raw reads
        for (int form = 0; form < 3; ++form) {
            const size_t n_sx = form == 2 ? M : 0, n_self = form == 0 ? 0 : (form == 1 ? Z : M);
            check_block([&](Carve& c) {
                OvlUnitigArgs g{};
                const int32_t* sx = lay_unitigs_in(c, g, n, (int32_t)R, n_sx, n_self);
                return std::vector<Table>{{g.ids, 4 * R},   {g.prev, 4 * R},          {g.first, 4 * Z},
                                          {g.self_ix, 4 * Z}, {sx, 4 * n_sx},         {g.self_score, 4 * n_self},
                                          {g.self_end, 4 * n_self}, {g.score, 4 * P}, {g.end, 4 * P}};
            });
        }
    }
    if (g_failed) {
        fprintf(stderr, "stage_block_check: %d expectation(s) failed\n", g_failed);
        return 1;
    }
    printf("stage_block_check: ok\n");
    return 0;
}
