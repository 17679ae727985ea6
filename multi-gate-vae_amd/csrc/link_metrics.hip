// Link-prediction ranking metrics on the device: ROC-AUC and average precision of the decoder's scores of P positive pairs
// against Q negative pairs (DG_VAE/deepgate/digvae_model.py:177-189 copies every score to the host and calls sklearn).
//   1. mgv_link_keys: the decoder's score of every pair (k_edge_dot's arithmetic) as an order-preserving 32-bit key;
//   2. mgv_sort_pairs (rocPRIM radix sort, csrc/radix_sort.hip): descending score order plus the permutation — element i of the
//      sorted array is a positive iff order[i] < P, so no label array exists;
//   3. mgv_link_rank: two streaming passes over the sorted array, one tile of 2048 elements per workgroup.  The first leaves
//      every tile's positive count and its last tie-group head, one workgroup scans those carries in tile order, the second
//      forms the terms at each tie group's LAST element:  U2 += p (2 Qbelow + q)  (an integer: one 64-bit partial per
//      workgroup, added by the last kernel — atomics on one address cost 0.8 ms at 17 M pairs) and  p TP / (TP + FP)  (double:
//      summed per workgroup in a fixed order, one slab row per workgroup, rows added in index order by k_slab_sum).  Tie
//      groups of any length cost the same: a group's head travels in the scan's carry, nothing walks a group.  Two runs give
//      the same bits.
#include "mgv_launch.h"
#include "mgv_slab.h"
#include "../../include/mgvae_hip.h"

namespace mgv {

// fp32 -> uint32 whose unsigned order is the float order (sign bit of non-negatives flipped, all bits of negatives), then
// complemented: an ASCENDING unsigned sort puts the highest score first
__device__ __forceinline__ uint32_t desc_key(float x) {
    const uint32_t u = __float_as_uint(x);
    return ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}

template <int H>
__global__ __launch_bounds__(kThreads) void k_link_keys(int64_t P, int64_t Q, const float* s, const float* t, int ld, const int64_t* psrc,
                                                        const int64_t* pdst, const int64_t* nsrc, const int64_t* ndst, uint32_t* keys,
                                                        float* scores, int32_t* status) {
    constexpr int LPR = H / 4, EPB = kThreads / LPR;
    const int lr = threadIdx.x % LPR, slot = threadIdx.x / LPR;
    const int64_t E = P + Q;
    int nans = 0;
    for (int64_t e0 = (int64_t)blockIdx.x * EPB; e0 < E; e0 += (int64_t)gridDim.x * EPB) {
        const int64_t e = e0 + slot;
        const bool ok = e < E;
        const bool pos = e < P;
        float4 a = zero4(), b = zero4();
        if (ok) {
            const int64_t u = pos ? psrc[e] : nsrc[e - P];
            const int64_t v = pos ? pdst[e] : ndst[e - P];
            a = ld4(s + u * ld + 4 * lr);
            b = ld4(t + v * ld + 4 * lr);
        }
        const float val = group_sum<LPR>(dot4(a, b));
        if (ok && lr == 0) {
            const float p = sigmoidf_(val);
            keys[e] = desc_key(p);
            if (scores) scores[e] = p;
            nans += (p != p);
        }
    }
    // one integer atomic per wave that met a NaN
    for (int d = 32; d > 0; d >>= 1) nans += __shfl_xor(nans, d, 64);
    if ((threadIdx.x & 63) == 0 && nans > 0) atomicAdd(status, nans);
}

// ------------------------------------------------------------------------------------------------ rank pass
constexpr int kRankItems = 8;                          // consecutive sorted elements per thread (two 16-byte loads per array)
constexpr int kRankTile = kThreads * kRankItems;       // 2048 elements per workgroup
constexpr int kCarryThreads = 1024;

// A tie group's head as one 64-bit word: (index of the group's first element) << 32 | positives before it.  Both halves grow
// with the position, so the LATEST head seen so far is the maximum; -1 = no head yet.
__device__ __forceinline__ long long pack_head(int start, int pref) { return ((long long)start << 32) | (unsigned int)pref; }

// exclusive scans across the NW waves of a workgroup (NW * 64 threads); `total` = the combination of all threads' values
template <int NW>
__device__ __forceinline__ int block_excl_sum(int v, int* red, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
    __syncthreads();
    if (lane == 63) red[w] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
    for (int k = 0; k < NW; ++k) { if (k < w) base += red[k]; total += red[k]; }
    return base + inc - v;
}
template <int NW>
__device__ __forceinline__ long long block_excl_max(long long v, long long* red, long long& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long inc = v;
    for (int d = 1; d < 64; d <<= 1) { const long long o = __shfl_up(inc, d, 64); if (lane >= d && o > inc) inc = o; }
    long long exc = __shfl_up(inc, 1, 64);
    if (lane == 0) exc = -1;
    __syncthreads();
    if (lane == 63) red[w] = inc;
    __syncthreads();
    total = -1;
    for (int k = 0; k < NW; ++k) { if (k < w && red[k] > exc) exc = red[k]; if (red[k] > total) total = red[k]; }
    return exc;
}

struct RankArgs {
    int64_t n, P;
    const uint32_t* keys;          // sorted, highest score first
    const int32_t* order;          // the sorting permutation: positive iff order[i] < P
    int32_t* cnt;                  // [tiles] positives of the tile
    int32_t* hstart;               // [tiles] index of the tile's last tie-group head, -1: the tile starts no group
    int32_t* hlocal;               // [tiles] positives of the tile in front of that head
    int32_t* base;                 // [tiles] positives in front of the tile                          (k_link_carry)
    int32_t* cstart;               // [tiles] head of the group that is open where the tile begins     (k_link_carry)
    int32_t* cpref;                // [tiles] positives in front of that head                          (k_link_carry)
    double* slab;                  // [tiles] the tile's sum of p TP / (TP + FP)
    unsigned long long* u2part;    // [tiles] the tile's sum of p (2 Qbelow + q)
    int32_t* groups;               // [tiles] tie groups that end in the tile
    unsigned long long* acc;       // the result's integer words: U2, P, Q, tie groups
};

// FINAL = false: the tile's carries;  FINAL = true: the terms of the tie groups that END in the tile
template <bool FINAL>
__global__ __launch_bounds__(kThreads) void k_link_tile(RankArgs a) {
    __shared__ int red_i[kThreads / 64];
    __shared__ long long red_l[kThreads / 64];
    __shared__ double red_d[kThreads];
    __shared__ unsigned long long red_u[kThreads / 64];
    __shared__ unsigned int red_g[kThreads / 64];
    const int64_t i0 = (int64_t)blockIdx.x * kRankTile + (int64_t)threadIdx.x * kRankItems;
    const int m = a.n - i0 >= kRankItems ? kRankItems : (a.n > i0 ? (int)(a.n - i0) : 0);     // this thread's elements
    uint32_t k[kRankItems + 2];        // k[0] = the element in front of the thread's, k[kRankItems + 1] = the one behind
    int pos[kRankItems];
    if (m == kRankItems) {
        const uint4 k0 = *reinterpret_cast<const uint4*>(a.keys + i0), k1 = *reinterpret_cast<const uint4*>(a.keys + i0 + 4);
        const int4 o0 = *reinterpret_cast<const int4*>(a.order + i0), o1 = *reinterpret_cast<const int4*>(a.order + i0 + 4);
        k[1] = k0.x; k[2] = k0.y; k[3] = k0.z; k[4] = k0.w; k[5] = k1.x; k[6] = k1.y; k[7] = k1.z; k[8] = k1.w;
        pos[0] = o0.x < a.P; pos[1] = o0.y < a.P; pos[2] = o0.z < a.P; pos[3] = o0.w < a.P;
        pos[4] = o1.x < a.P; pos[5] = o1.y < a.P; pos[6] = o1.z < a.P; pos[7] = o1.w < a.P;
    } else {
#pragma unroll
        for (int j = 0; j < kRankItems; ++j) {
            k[j + 1] = j < m ? a.keys[i0 + j] : 0u;
            pos[j] = j < m ? (a.order[i0 + j] < a.P) : 0;
        }
    }
    const bool first = i0 == 0;                                        // element 0 starts the first group
    k[0] = (m > 0 && !first) ? a.keys[i0 - 1] : 0u;
    const bool last = m > 0 && i0 + m == a.n;                          // element n - 1 ends the last group
    k[kRankItems + 1] = (FINAL && m == kRankItems && !last) ? a.keys[i0 + kRankItems] : 0u;

    // the thread's positives, and those in front of its last head
    int c = 0, lh = -1, ls = 0;
#pragma unroll
    for (int j = 0; j < kRankItems; ++j) {
        if (j < m) {
            const bool head = (j == 0 && first) || k[j + 1] != k[j];
            if (head) { lh = c; ls = j; }
            c += pos[j];
        }
    }
    int total;
    const int excl = block_excl_sum<kThreads / 64>(c, red_i, total);       // the tile's positives in front of the thread
    const long long mine = lh >= 0 ? pack_head((int)(i0 + ls), excl + lh) : -1;      // (positives counted from the tile's start)
    long long tile_head;
    const long long before = block_excl_max<kThreads / 64>(mine, red_l, tile_head);
    if (!FINAL) {
        if (threadIdx.x == 0) {
            a.cnt[blockIdx.x] = total;
            a.hstart[blockIdx.x] = tile_head >= 0 ? (int)(tile_head >> 32) : -1;
            a.hlocal[blockIdx.x] = tile_head >= 0 ? (int)(tile_head & 0xffffffffLL) : 0;
        }
        return;
    }
    const int tb = a.base[blockIdx.x];
    const int64_t Q = a.n - a.P;
    // the group that is open where this thread begins: a head of this tile, else the one the tile inherited
    int64_t gs = before >= 0 ? (before >> 32) : a.cstart[blockIdx.x];
    int64_t gp = before >= 0 ? tb + (before & 0xffffffffLL) : a.cpref[blockIdx.x];
    int64_t run = (int64_t)tb + excl;            // positives in front of the current element
    unsigned long long u2 = 0;
    unsigned int groups = 0;
    double ap = 0.0;
#pragma unroll
    for (int j = 0; j < kRankItems; ++j) {
        if (j < m) {
            const int64_t i = i0 + j;
            if ((j == 0 && first) || k[j + 1] != k[j]) { gs = i; gp = run; }
            run += pos[j];
            const bool end = (i == a.n - 1) || k[j + 2] != k[j + 1];
            if (end) {
                const int64_t TP = run, tot = i + 1, FP = tot - TP;
                const int64_t p = TP - gp, q = (tot - gs) - p;
                u2 += (unsigned long long)p * (unsigned long long)(2 * (Q - FP) + q);
                if (p > 0) ap += (double)p * ((double)TP / (double)tot);
                ++groups;
            }
        }
    }
    // integers: wave sums, then the workgroup's partial (integer addition does not depend on the order)
    for (int d = 32; d > 0; d >>= 1) {
        u2 += __shfl_xor(u2, d, 64);
        groups += __shfl_xor(groups, d, 64);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red_u[threadIdx.x >> 6] = u2; red_g[threadIdx.x >> 6] = groups; }
    red_d[threadIdx.x] = ap;
    __syncthreads();
    if (threadIdx.x == 0) {
        a.u2part[blockIdx.x] = red_u[0] + red_u[1] + red_u[2] + red_u[3];
        a.groups[blockIdx.x] = (int32_t)(red_g[0] + red_g[1] + red_g[2] + red_g[3]);
    }
    // doubles: a fixed tree over the workgroup, one slab row
    for (int sft = kThreads / 2; sft > 0; sft >>= 1) {
        if ((int)threadIdx.x < sft) red_d[threadIdx.x] += red_d[threadIdx.x + sft];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.slab[blockIdx.x] = red_d[0];
}

// One workgroup: tile carries in tile order (every thread a contiguous run of tiles), and the result words reset.
__global__ __launch_bounds__(kCarryThreads) void k_link_carry(int64_t tiles, RankArgs a, double* out) {
    __shared__ int red_i[kCarryThreads / 64];
    __shared__ long long red_l[kCarryThreads / 64];
    const int64_t seg = (tiles + kCarryThreads - 1) / kCarryThreads;
    const int64_t b0 = min(tiles, (int64_t)threadIdx.x * seg), b1 = min(tiles, b0 + seg);
    int sum = 0;
    for (int64_t b = b0; b < b1; ++b) sum += a.cnt[b];
    int total;
    int run = block_excl_sum<kCarryThreads / 64>(sum, red_i, total);
    long long mine = -1;
    for (int64_t b = b0; b < b1; ++b) {
        a.base[b] = run;
        if (a.hstart[b] >= 0) mine = pack_head(a.hstart[b], run + a.hlocal[b]);
        run += a.cnt[b];
    }
    long long all;
    long long cur = block_excl_max<kCarryThreads / 64>(mine, red_l, all);
    for (int64_t b = b0; b < b1; ++b) {
        a.cstart[b] = cur >= 0 ? (int)(cur >> 32) : 0;
        a.cpref[b] = cur >= 0 ? (int)(cur & 0xffffffffLL) : 0;
        if (a.hstart[b] >= 0) cur = pack_head(a.hstart[b], a.base[b] + a.hlocal[b]);
    }
    if (threadIdx.x == 0) {
        out[0] = 0.0; out[1] = 0.0;
        a.acc[0] = 0; a.acc[1] = (unsigned long long)a.P; a.acc[2] = (unsigned long long)(a.n - a.P); a.acc[3] = 0;
    }
}

// One workgroup: the integer partials of the tiles, then AUC and AP, each formed once in double (out[1] holds the sum of the slab rows)
__global__ __launch_bounds__(kCarryThreads) void k_link_final(int64_t tiles, RankArgs a, double* out) {
    __shared__ unsigned long long red_u[kCarryThreads / 64], red_g[kCarryThreads / 64];
    unsigned long long u2 = 0, groups = 0;
    for (int64_t b = threadIdx.x; b < tiles; b += kCarryThreads) { u2 += a.u2part[b]; groups += (unsigned long long)a.groups[b]; }
    for (int d = 32; d > 0; d >>= 1) {
        u2 += __shfl_xor(u2, d, 64);
        groups += __shfl_xor(groups, d, 64);
    }
    if ((threadIdx.x & 63) == 0) { red_u[threadIdx.x >> 6] = u2; red_g[threadIdx.x >> 6] = groups; }
    __syncthreads();
    if (threadIdx.x == 0) {
        u2 = 0; groups = 0;
        for (int k = 0; k < kCarryThreads / 64; ++k) { u2 += red_u[k]; groups += red_g[k]; }
        a.acc[0] = u2; a.acc[3] = groups;
        const double dp = (double)a.P, dq = (double)(a.n - a.P);
        out[0] = (double)u2 / (2.0 * dp * dq);
        out[1] = out[1] / dp;
    }
}

inline int64_t rank_tiles(int64_t n) { return (n + kRankTile - 1) / kRankTile; }

}  // namespace mgv

extern "C" int mgv_link_keys(int H, const float* s, const float* t, int ld, const int64_t* pos_src, const int64_t* pos_dst, int64_t P,
                             const int64_t* neg_src, const int64_t* neg_dst, int64_t Q, uint32_t* keys, float* scores, int32_t* status,
                             void* stream) {
    MGV_CHECK_ARG(P > 0 && Q > 0 && s && t && pos_src && pos_dst && neg_src && neg_dst && keys && status && ld >= H && ld % 4 == 0);
    if (P + Q >= (int64_t(1) << 31)) return MGV_EUNSUPPORTED;
    return mgv::launch_width(mgv::AllWidths{}, H, [&](auto w) {
        constexpr int HH = w, per_block = mgv::kThreads / (HH / 4);
        hipLaunchKernelGGL(mgv::k_link_keys<HH>, dim3(mgv::grid_for((P + Q + per_block - 1) / per_block, 8)), dim3(mgv::kThreads), 0,
                           static_cast<hipStream_t>(stream), P, Q, s, t, ld, pos_src, pos_dst, neg_src, neg_dst, keys, scores, status);
    });
}

extern "C" int mgv_link_rank_work_ints(int64_t n) {
    if (n < 1 || n >= (int64_t(1) << 31)) return -1;
    return (int)(11 * mgv::rank_tiles(n));         // per tile: a double slab row, a 64-bit integer partial, seven int32 words
}

extern "C" int mgv_link_rank(int64_t n, int64_t P, const uint32_t* sorted_keys, const int32_t* order, double* out, int32_t* work,
                             int64_t work_ints, void* stream) {
    MGV_CHECK_ARG(n > 0 && P > 0 && P < n && sorted_keys && order && out && work);
    if (n >= (int64_t(1) << 31)) return MGV_EUNSUPPORTED;
    MGV_CHECK_ARG(work_ints >= mgv_link_rank_work_ints(n));
    // 16-byte loads of the two arrays, doubles in the work array and the result
    MGV_CHECK_ARG((uintptr_t)sorted_keys % 16 == 0 && (uintptr_t)order % 16 == 0 && (uintptr_t)work % 8 == 0 && (uintptr_t)out % 8 == 0);
    const int64_t tiles = mgv::rank_tiles(n);
    mgv::RankArgs a{};
    a.n = n; a.P = P; a.keys = sorted_keys; a.order = order;
    a.slab = reinterpret_cast<double*>(work);
    a.u2part = reinterpret_cast<unsigned long long*>(work + 2 * tiles);
    int32_t* w = work + 4 * tiles;
    a.cnt = w; a.hstart = w + tiles; a.hlocal = w + 2 * tiles; a.base = w + 3 * tiles; a.cstart = w + 4 * tiles; a.cpref = w + 5 * tiles;
    a.groups = w + 6 * tiles;
    a.acc = reinterpret_cast<unsigned long long*>(out + 2);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL((mgv::k_link_tile<false>), dim3((unsigned)tiles), dim3(mgv::kThreads), 0, st, a);
    hipLaunchKernelGGL(mgv::k_link_carry, dim3(1), dim3(mgv::kCarryThreads), 0, st, tiles, a, out);
    hipLaunchKernelGGL((mgv::k_link_tile<true>), dim3((unsigned)tiles), dim3(mgv::kThreads), 0, st, a);
    mgv::launch_slab_sum<double, double>(a.slab, (int)tiles, 1, 1, out + 1, st);
    hipLaunchKernelGGL(mgv::k_link_final, dim3(1), dim3(mgv::kCarryThreads), 0, st, tiles, a, out);
    MGV_LAUNCH_RET();
}
