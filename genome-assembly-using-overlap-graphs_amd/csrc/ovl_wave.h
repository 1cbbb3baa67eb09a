// ovl_wave.h — wavefront-level device helpers shared by the anti-diagonal DP kernels (ovl_dp.hip, ovl_local.hip,
// ovl_local_batch.hip), the ungapped scorer and the resident grid: one reviewed copy of each.  Device-only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace ovl_wave {

// lane L receives lane L-1's value (lane 0 gets 0): DPP wave_shr:1; the int64 form is two of them
template <typename Acc>
__device__ __forceinline__ Acc shr1(Acc v);

template <>
__device__ __forceinline__ int32_t shr1<int32_t>(int32_t v) {
    return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xF, 0xF, false);
}

template <>
__device__ __forceinline__ int64_t shr1<int64_t>(int64_t v) {
    const int32_t lo = shr1<int32_t>((int32_t)(uint32_t)(uint64_t)v);
    const int32_t hi = shr1<int32_t>((int32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// vec[L] = s: v_writelane_b32 with an inline-constant lane (one SGPR read: the constant-bus limit)
template <int L>
__device__ __forceinline__ int32_t writelane(int32_t vec, int32_t s) {
    asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(vec) : "s"(s), "n"(L));
    return vec;
}

// f(integral_constant<int, U>) for U = B .. E-1: a compile-time step index inside the unrolled loop
template <int B, int E, typename F>
__device__ __forceinline__ void unroll(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        unroll<B + 1, E>(f);
    }
}

// one chunk of traceback codes ([step][lane], 64 x 64 bytes in LDS) out to memory: four 16-byte stores per lane
__device__ __forceinline__ void flush_codes(const uint8_t* tbs, int8_t* dst_chunk, int lane) {
    const uint4* src = reinterpret_cast<const uint4*>(tbs);
    uint4* dst = reinterpret_cast<uint4*>(dst_chunk);
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[k * 64 + lane] = src[k * 64 + lane];
}

// retires this wavefront's outstanding vector memory operations
__device__ __forceinline__ void vm_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// every lane gets the wavefront's maximum, as a vector value.  ovl_dp_lane.hip keeps its own wave_max / wave_min
// pair: those end in v_readfirstlane (a scalar result), a different instruction sequence.
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

}  // namespace ovl_wave
