// ovl_pair_layout.h — where a chunk of a compact host pair list lies in the pinned encoding buffer and its HBM copy
// (ovl_pipeline.cpp: setup_job sizes the buffer, encode_chunk fills it, issue_chunk copies in-place chunks).  Plain
// arithmetic without HIP, so tests/c/pair_layout_check.cpp checks it stand-alone.
//
// Chunk k of a job, pairs [off, off + n) at `width` bytes per index (2: uint16 when n_reads <= 65,535, else 4), from
// base() = align16(8 off + 32 k), every area on 16 bytes:
//   b area        n * width bytes
//   a area        one of
//     in place    d8: n bytes (a - its tile's first a), then the tile bases: int32 per 64 pairs   (width 2 only)
//     runs        R values int32, padded to a multiple of 4, then R + 1 starts int32 (when 8 R + 4 < n * width)
//     a like b    n * width bytes
// Every form ends at or before the next chunk's base, and the last chunk within job_bytes.
#pragma once

#include <cstddef>
#include <cstdint>

struct PairLayout {
    size_t n, width, at;

    PairLayout(int64_t off, int64_t k, int64_t n_pairs, int width_bytes)
        : n((size_t)n_pairs), width((size_t)width_bytes), at(align16(8 * (size_t)off + 32 * (size_t)k)) {}

    static size_t align16(size_t x) { return (x + 15) & ~size_t(15); }
    // the encoding buffer of a whole job
    static size_t job_bytes(int64_t n_pairs, int64_t chunks) { return 8 * (size_t)n_pairs + 32 * (size_t)chunks + 64; }

    size_t base() const { return at; }
    size_t b_bytes() const { return align16(n * width); }
    size_t a() const { return at + b_bytes(); }
    size_t plain_end() const { return a() + n * width; }
    // in place
    size_t tiles() const { return (n + 63) / 64; }
    size_t d8() const { return a(); }
    size_t tile_bases() const { return a() + align16(n); }
    size_t ix_bytes() const { return tile_bases() + 4 * tiles() - at; }      // what issue_chunk copies into HBM
    int64_t ix_link() const { return (int64_t)(3 * n + 4 * tiles()); }       // ... and ovl_last_transfer counts
    // runs
    size_t run_values() const { return a(); }
    size_t run_starts(int64_t R) const { return a() + 4 * (((size_t)R + 3) & ~size_t(3)); }
    size_t runs_end(int64_t R) const { return run_starts(R) + 4 * ((size_t)R + 1); }
    // a decoded chunk's bytes over the link: b, and a as R runs or like b
    int64_t decoded_link(bool runs, int64_t R) const {
        return (int64_t)(n * width) + (runs ? 8 * R + 4 : (int64_t)(n * width));
    }
};
