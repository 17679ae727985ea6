// The negative sampler's draw, stated once for every kernel that draws (k_neg_sample, k_np_draw): slot i of a call is a pure
// function of (seed, i, N, the positive out-lists).
#pragma once
#include "mgv_common.h"

namespace mgv {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// the pair of slot i: attempts 0..64 from the slot's counter until one is neither a self pair nor an edge of the CSR
__device__ __forceinline__ void neg_draw_slot(int64_t N, uint64_t seed, int64_t i, const int32_t* out_ptr, const int32_t* out_dst, int& s, int& d) {
    uint64_t ctr = seed ^ ((uint64_t)i * 0xD1342543DE82EF95ull);
    for (int attempt = 0;; ++attempt) {
        const uint64_t r = splitmix64(ctr + attempt);
        s = (int)(((r >> 32) * (uint64_t)N) >> 32);
        d = (int)(((r & 0xFFFFFFFFull) * (uint64_t)N) >> 32);
        bool ok = s != d;
        if (ok)
            for (int e = out_ptr[s]; e < out_ptr[s + 1]; ++e)
                if (out_dst[e] == d) { ok = false; break; }
        if (ok || attempt >= 64) break;      // 64 straight rejections: the graph is (nearly) complete; keep the pair
    }
}

}  // namespace mgv
