// Dropout masks of the readout (arch/mlp.py: nn.Dropout after each BatchNorm + ReLU) from a counter-based hash of
// (seed, element): the forward, the backward and the fused readout passes regenerate the same mask instead of storing it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mgv {

__device__ __forceinline__ uint32_t hash_u32(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return (uint32_t)x;
}
// inverted-dropout factor of element (row, col): 0 or 1/(1-p); the same counter-based stream is
// regenerated in the backward pass
__device__ __forceinline__ float drop_scale(uint64_t seed, int64_t elem, float p, float keep_scale) {
    if (p <= 0.f) return 1.0f;
    const uint32_t h = hash_u32(seed + 0x9E3779B97F4A7C15ULL * (uint64_t)(elem + 1));
    const float u = (h >> 8) * (1.0f / 16777216.0f);
    return u < p ? 0.f : keep_scale;
}

}  // namespace mgv
