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

// ---- the local draw (k_np_draw<NpDrawLocal>, k_neg_draw_local): slot i is a pure function of (seed, i, N, R, graph_ptr, the positive lists).
// The first R slots are reversals of listed positive edges, the others a source uniform over the batch and a destination uniform over the
// source's own graph.  With graph_ptr = {0, N} and R = 0 it is neg_draw_slot, integer for integer.
constexpr int kNegGraphLds = 4096;     // graphs up to here: the drawing kernels keep the table in LDS (16 KB), above it they read it from memory

// graph_ptr[g] clamped into [0, N]: a wrong table gives wrong pairs, never an address outside the arrays
__device__ __forceinline__ int neg_graph_ptr(const int32_t* gp, int g, int N) {
    const int v = gp[g];
    return v < 0 ? 0 : (v > N ? N : v);
}

// gp: the table [G + 1], in LDS or in memory; (pin_src[e], pin_dst[e]): the Epos positive edges in any order (read by reversed slots only)
__device__ __forceinline__ void neg_draw_slot_local(int64_t N, uint64_t seed, int64_t i, const int32_t* out_ptr, const int32_t* out_dst, int64_t R,
                                                    int G, const int32_t* gp, int64_t Epos, const int32_t* pin_src, const int32_t* pin_dst,
                                                    int& s, int& d) {
    const uint64_t ctr = seed ^ ((uint64_t)i * 0xD1342543DE82EF95ull);
    const int last = (int)N - 1;
    for (int attempt = 0;; ++attempt) {
        const uint64_t r = splitmix64(ctr + attempt);
        const uint64_t hi = r >> 32, lo = r & 0xFFFFFFFFull;
        if (i < R) {
            const int64_t e = (int64_t)((hi * (uint64_t)Epos) >> 32);
            s = pin_dst[e]; d = pin_src[e];
            s = s < 0 ? 0 : (s > last ? last : s);      // (ids of a plan's lists lie in [0, N): the clamps never move one)
        } else {
            s = (int)((hi * (uint64_t)N) >> 32);
            int g = 0, z = G - 1;                       // the largest g < G with gp[g] <= s
            while (g < z) { const int mid = (g + z + 1) >> 1; if (neg_graph_ptr(gp, mid, (int)N) <= s) g = mid; else z = mid - 1; }
            const int a = neg_graph_ptr(gp, g, (int)N), n = neg_graph_ptr(gp, g + 1, (int)N) - a;
            d = a + (int)((lo * (uint64_t)(n > 0 ? n : 0)) >> 32);
        }
        d = d < 0 ? 0 : (d > last ? last : d);
        bool ok = s != d;
        if (ok)
            for (int e = out_ptr[s]; e < out_ptr[s + 1]; ++e)
                if (out_dst[e] == d) { ok = false; break; }
        if (ok || attempt >= 64) break;      // as neg_draw_slot: the pair of attempt 64 is kept whatever it is
    }
}

}  // namespace mgv
