// What the two device entropy coders share (rans_coder.hip: "rans1", occ_coder.hip: "occ1"): the constants of the 32-bit rANS state,
// the per-stream status flags, the wave helpers that place the words of a step, the integer cost with its lane rule, and byte stores.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace {

constexpr int kMaxLanes = 64;
constexpr uint32_t kLow = 1u << 16;

// flags of the per-stream status word
constexpr int32_t kBadRow = 1, kCorrupt = 2, kBadShape = 4;

// lane of a thread in its wave (the rans1 kernels run one wave per workgroup, the occ1 kernels several)
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63u); }
__device__ __forceinline__ int prefix_rank(uint64_t mask) { return __popcll(mask & ((1ull << lane_id()) - 1ull)); }

__host__ __device__ __forceinline__ int32_t cost256(uint32_t f) {
    const int k = 31 - __builtin_clz(f);                                // floor(log2 f), f >= 1
    const uint32_t r = f - (1u << k);
    return 256 * (16 - k) - (int32_t)((r << 8) >> k);
}

// the largest power of two L <= 64 with 128 L <= est, at least 1
__host__ __device__ __forceinline__ int lane_rule(int64_t est) {
    int L = 1;
    while (L < kMaxLanes && 128 * (2 * L) <= est) L *= 2;
    return L;
}

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += (int64_t)__shfl_xor((long long)v, off);
    return v;
}

__device__ __forceinline__ int32_t wave_or(int32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v |= __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ void put16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
__device__ __forceinline__ void put32(uint8_t* p, uint32_t v) { put16(p, v); put16(p + 2, v >> 16); }
__device__ __forceinline__ uint32_t get16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

}  // namespace
