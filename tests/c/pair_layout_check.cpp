// pair_layout_check.cpp — the compact pair list's chunk layout (csrc/ovl_pair_layout.h) as a stand-alone host program
// (tests/test_pair_layout_cpu.py builds and runs it; `make pair-layout-check` runs it under the sanitizers).
//
// Over jobs cut the way ovl_pipeline.cpp's setup_job cuts them -- a packed share in equal 64-aligned steps, then direct
// chunks of the chunk size, the last one short -- at both index widths, every chunk's areas are compared for equality
// with the three expressions the layout replaced (written out below as they stood in setup_job, encode_chunk and
// issue_chunk), and checked to be 16-byte aligned, disjoint, and to end at or before the next chunk's base (the last
// chunk's within the job's buffer), in each of the three forms of the a area: like b, in place, and runs for
// R = 0, 1, the largest R that the rule 8 R + 4 < n * width admits, and the largest such R with R % 4 == 1 (the most
// padding between the values and the starts).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ovl_pair_layout.h"

static long g_failed = 0, g_chunks = 0;
#define EXPECT(cond)                                                                                        \
    do {                                                                                                    \
        if (!(cond) && ++g_failed <= 20)                                                                    \
            fprintf(stderr, "%s:%d: %s failed (off %lld k %lld n %lld width %d)\n", __FILE__, __LINE__, #cond, \
                    (long long)off, (long long)k, (long long)n, wd);                                        \
    } while (0)

// one chunk against the parent's expressions; `limit`: the next chunk's base, or the job's buffer size
static void check_chunk(int64_t off, int64_t k, int64_t n, int wd, size_t limit) {
    ++g_chunks;
    const PairLayout lay(off, k, n, wd);
    // encode_chunk / issue_chunk, as they stood
    const size_t base = (8 * (size_t)off + 32 * (size_t)k + 15) & ~size_t(15);
    const size_t b_bytes = ((size_t)n * wd + 15) & ~size_t(15);
    const size_t a = base + b_bytes;
    EXPECT(lay.base() == base);
    EXPECT(lay.b_bytes() == b_bytes);
    EXPECT(lay.a() == a);
    EXPECT(base % 16 == 0 && a % 16 == 0);
    EXPECT(base + (size_t)n * wd <= a);  // b ends before a starts
    // a like b
    EXPECT(lay.plain_end() == a + (size_t)n * wd);
    EXPECT(lay.plain_end() <= limit);
    EXPECT(lay.decoded_link(false, 0) == (int64_t)n * wd + (int64_t)n * wd);
    // in place: d8 at a, the tile bases behind it, and the bytes issue_chunk copied
    if (wd == 2) {
        const size_t tb = a + (((size_t)n + 15) & ~size_t(15));
        const size_t bytes = b_bytes + (((size_t)n + 15) & ~size_t(15)) + 4 * (size_t)((n + 63) / 64);
        EXPECT(lay.d8() == a);
        EXPECT(lay.tile_bases() == tb);
        EXPECT(tb % 16 == 0 && a + (size_t)n <= tb);
        EXPECT(lay.ix_bytes() == bytes);
        EXPECT(base + bytes == tb + 4 * lay.tiles() && base + bytes <= limit);
        EXPECT(lay.ix_link() == 3 * (int64_t)n + 4 * ((n + 63) / 64));
    }
    // runs: values at a, starts behind them on 16 bytes, R + 1 starts
    if (4 < n * wd) {
        const int64_t r_max = (n * wd - 5) / 8;  // the largest R with 8 R + 4 < n * width
        EXPECT(8 * r_max + 4 < n * wd && 8 * (r_max + 1) + 4 >= n * wd);
        int64_t r_pad = r_max;
        while (r_pad > 0 && r_pad % 4 != 1) --r_pad;
        for (const int64_t R : {int64_t(0), std::min<int64_t>(1, r_max), r_max, r_pad}) {
            const size_t starts = a + 4 * (size_t)((R + 3) & ~int64_t(3));
            EXPECT(lay.run_values() == a);
            EXPECT(lay.run_starts(R) == starts);
            EXPECT(starts % 16 == 0 && a + 4 * (size_t)R <= starts);
            EXPECT(lay.runs_end(R) == starts + 4 * (size_t)(R + 1));
            EXPECT(lay.runs_end(R) <= limit);
            EXPECT(lay.decoded_link(true, R) == (int64_t)n * wd + 8 * R + 4);
        }
    }
}

// setup_job's cuts of n pairs: chunk size `chunk`, `pct` percent direct (100: nothing packed; -1: no packed call)
static std::vector<int64_t> cuts(int64_t n, int64_t chunk, int pct) {
    std::vector<int64_t> cb(1, 0);
    if (pct >= 0) {
        int64_t packed = (n - n * pct / 100) & ~int64_t(63);
        if (packed >= n - 64) packed = n;
        const int64_t pieces = (packed + chunk - 1) / chunk;
        const int64_t step = pieces ? (((packed + pieces - 1) / pieces + 63) & ~int64_t(63)) : 0;
        for (int64_t o = step; o < packed; o += step) cb.push_back(o);
        if (packed > 0) cb.push_back(packed);
    }
    for (int64_t o = cb.back(); o < n;) {
        o = std::min(n, o + chunk);
        cb.push_back(o);
    }
    return cb;
}

static void check_job(int64_t total, int64_t chunk, int pct) {
    const std::vector<int64_t> cb = cuts(total, chunk, pct);
    const int64_t nchunks = (int64_t)cb.size() - 1;
    const size_t need = PairLayout::job_bytes(total, nchunks);
    {
        const int64_t off = 0, k = nchunks, n = total;
        const int wd = 0;
        EXPECT(need == 8 * (size_t)total + 32 * (size_t)nchunks + 64);  // setup_job, as it stood
        EXPECT(cb.back() == total);
    }
    for (const int wd : {2, 4})
        for (int64_t k = 0; k < nchunks; ++k) {
            const size_t limit = k + 1 < nchunks ? PairLayout(cb[(size_t)k + 1], k + 1, 1, wd).base() : need;
            check_chunk(cb[(size_t)k], k, cb[(size_t)k + 1] - cb[(size_t)k], wd, limit);
        }
}

int main() {
    std::vector<int64_t> sizes;
    for (int64_t n = 1; n <= 4200; ++n) sizes.push_back(n);
    for (const int64_t n : {int64_t(65535), int64_t(65537), int64_t(300007), int64_t(1048577), int64_t(16777259)})
        sizes.push_back(n);
    for (const int64_t n : sizes) {
        std::vector<int64_t> chunks = {n, 4096, 1000, 101};
        if (n <= 700) chunks.push_back(64);
        if (n > 100000) chunks = {n, int64_t(1) << 20, 4096, 100001};
        for (const int64_t chunk : chunks)
            for (const int pct : {-1, 0, 18, 36, 100}) check_job(n, chunk, pct);
    }
    printf("chunks %ld\n", g_chunks);
    if (g_failed) {
        fprintf(stderr, "%ld checks failed\n", g_failed);
        return 1;
    }
    printf("ok\n");
    return 0;
}
