// The stateless Gaussian generator of the VAE sampler (digvae_model.py:138-141 draws torch.randn_like): element i of the stream
// `seed` is a Box-Muller pair from two 64-bit counter hashes, so any kernel that knows (seed, i) draws the same noise — the
// reparameterisation kernels of losses.hip, and the fused variational head (var_head_x3.hip) in its forward and again in its backward.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mgv {

__device__ __forceinline__ uint32_t mix32(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return (uint32_t)x;
}
__device__ __forceinline__ float gauss_from_counter(uint64_t seed, uint64_t i) {
    const uint32_t a = mix32(seed * 0x9E3779B97F4A7C15ULL + 2 * i), b = mix32(seed * 0x9E3779B97F4A7C15ULL + 2 * i + 1);
    const float u1 = ((a >> 8) + 1.0f) * (1.0f / 16777216.0f), u2 = (b >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * __cosf(6.283185307179586f * u2);
}

}  // namespace mgv
