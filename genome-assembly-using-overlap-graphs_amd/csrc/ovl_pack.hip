// ovl_pack.hip — gfx950 (CDNA4) kernels that encode a read set for the overlap-scoring engine.
//
// Kernels
//   map_codes     bytes -> dense symbol codes (LUT), one lane per byte.
//   pack_planes   codes -> bit-plane words in two layouts (prefix / suffix),
//                 one lane per (read, word).  Byte work, run once per read set.
//
// Layouts (per read, W = ceil(lmax/32) words of 32 bases, P planes interleaved per
// word, rows padded to 16 bytes):
//   sfx[r][k*P + p], k < W:       read right-aligned: base i at position 32W - n + i
//   pfx[r][x*P + p], x < W:       read left-aligned: base i at position i (word W is implicitly zero)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ovl_kernels.h"

namespace ovl {

__global__ void map_codes_kernel(const uint8_t* __restrict__ raw, const uint8_t* __restrict__ lut,
                                 uint8_t* __restrict__ codes, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) codes[i] = lut[raw[i]];
}

// 2-bit packed ACGT bytes (host-packed by ovl_set_reads: base i at bits 2(i % 4) of byte i / 4, A C G T =
// 0 1 2 3) -> dense symbol codes through the read set's LUT (codes[i] = lut["ACGT"[code]]); one lane per 16
// packed bytes (64 bases: one 16-byte load, four 16-byte stores), a 4-entry table in registers.
__global__ void unpack2_kernel(const uint8_t* __restrict__ pk, const uint8_t* __restrict__ lut,
                               uint8_t* __restrict__ codes, int64_t n) {
    const uint32_t c0 = lut['A'], c1 = lut['C'], c2 = lut['G'], c3 = lut['T'];
    const int64_t groups = (n + 63) / 64;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const uint4 v = reinterpret_cast<const uint4*>(pk)[g];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t out[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t x = w[k >> 2] >> (8 * (k & 3));  // packed byte k: bases 4k .. 4k + 3
            uint32_t o = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t c = (x >> (2 * b)) & 3u;
                const uint32_t m = c == 0 ? c0 : (c == 1 ? c1 : (c == 2 ? c2 : c3));
                o |= m << (8 * b);
            }
            out[k] = o;
        }
        const int64_t base = g * 64;
        if (base + 64 <= n) {
            uint4* d = reinterpret_cast<uint4*>(codes + base);
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = make_uint4(out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]);
        } else {
            for (int64_t i = base; i < n; ++i) codes[i] = (uint8_t)(out[(i - base) >> 2] >> (8 * ((i - base) & 3)));
        }
    }
}

// One lane per (read, word); the lane of a row's last word also zeroes the row padding (words W*P ..
// row stride), so the rows need no clearing beforehand.
template <int P>
__global__ void pack_planes_kernel(const uint8_t* __restrict__ codes, const int64_t* __restrict__ off,
                                   const int32_t* __restrict__ len, int32_t n_reads, int32_t w,
                                   int32_t srow, int32_t trow, uint32_t* __restrict__ sfx,
                                   uint32_t* __restrict__ pfx) {
    int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)n_reads * w;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; gid < total; gid += stride) {
        const int32_t r = (int32_t)(gid / w);
        const int32_t k = (int32_t)(gid % w);
        const int32_t n = len[r];
        const uint8_t* s = codes + off[r];
        uint32_t pl[P], sl[P];
#pragma unroll
        for (int p = 0; p < P; ++p) { pl[p] = 0u; sl[p] = 0u; }
        const int32_t shift = 32 * w - n;  // suffix layout: base i sits at position shift + i
        for (int b = 0; b < 32; ++b) {
            const int32_t i = 32 * k + b;      // prefix layout
            if (i < n) {
                const uint32_t c = s[i];
#pragma unroll
                for (int p = 0; p < P; ++p) pl[p] |= ((c >> p) & 1u) << b;
            }
            const int32_t u = i - shift;       // suffix layout
            if (u >= 0 && u < n) {
                const uint32_t c = s[u];
#pragma unroll
                for (int p = 0; p < P; ++p) sl[p] |= ((c >> p) & 1u) << b;
            }
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            pfx[(int64_t)r * trow + k * P + p] = pl[p];
            sfx[(int64_t)r * srow + k * P + p] = sl[p];
        }
        if (k == w - 1) {
            for (int32_t q = w * P; q < trow; ++q) pfx[(int64_t)r * trow + q] = 0u;
            for (int32_t q = w * P; q < srow; ++q) sfx[(int64_t)r * srow + q] = 0u;
        }
    }
}

}  // namespace ovl

// ----------------------------------------------------------------------------- launchers

using namespace ovl;

extern "C" hipError_t ovl_launch_map_codes(const uint8_t* raw, const uint8_t* lut, uint8_t* codes, int64_t n,
                                           hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    map_codes_kernel<<<(unsigned)blocks, 256, 0, stream>>>(raw, lut, codes, n);
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_unpack2(const uint8_t* pk, const uint8_t* lut, uint8_t* codes, int64_t n,
                                         hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (reinterpret_cast<uintptr_t>(pk) & 15) return hipErrorInvalidValue;
    int64_t blocks = ((n + 63) / 64 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    unpack2_kernel<<<(unsigned)blocks, 256, 0, stream>>>(pk, lut, codes, n);
    return hipGetLastError();
}

extern "C" hipError_t ovl_launch_pack(int planes, const uint8_t* codes, const int64_t* off, const int32_t* len,
                                      int32_t n_reads, int32_t w, int32_t srow, int32_t trow, uint32_t* sfx,
                                      uint32_t* pfx, hipStream_t stream) {
    if (n_reads <= 0) return hipSuccess;
    const int64_t total = (int64_t)n_reads * w;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    switch (planes) {
        case 2: pack_planes_kernel<2><<<(unsigned)blocks, 256, 0, stream>>>(codes, off, len, n_reads, w, srow, trow, sfx, pfx); break;
        case 4: pack_planes_kernel<4><<<(unsigned)blocks, 256, 0, stream>>>(codes, off, len, n_reads, w, srow, trow, sfx, pfx); break;
        case 8: pack_planes_kernel<8><<<(unsigned)blocks, 256, 0, stream>>>(codes, off, len, n_reads, w, srow, trow, sfx, pfx); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
