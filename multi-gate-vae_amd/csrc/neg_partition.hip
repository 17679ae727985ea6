// Negative edges drawn and bucketed by block partition: the same five arrays as mgv_neg_sample + mgv_neg_bucket + two
// mgv_sort_lists_i32, integer for integer, without a global atomic or a scattered store per pair and without a list sort of its own.
//
// s and d of a drawn pair are uniform over [0, N) whatever the graph, so a block of 2^shift consecutive node ids receives a
// near-constant number of pairs (Poisson around E 2^shift / N).  Three passes and one scan:
//   A  k_np_draw       one workgroup per chunk of kNpChunk slots: the draw of k_neg_sample (mgv_neg_draw.h), the pair stored as two
//                      int32, the chunk's pairs counted per source block and per destination block in LDS; one histogram row each.
//      scan            one flat exclusive scan over [side][block][chunk]: every (chunk, block) its base, every block its extent.
//   B  k_np_partition  one workgroup per chunk: the chunk ordered by block in LDS (LDS atomics: the order inside a block does not
//                      survive pass C), every block's run written contiguously at its base; by source (s, d), then by destination (d, s).
//   C  k_np_finish     one workgroup per node block and side: count per node, local scan + the block's base = ptr rows; the pairs
//                      placed per node in LDS, every node's entries sorted ascending, stored coalesced.  A block with more pairs
//                      than a trip holds (kNpCap) is finished in several trips over node sub-ranges; a single node above kNpCap is
//                      placed and sorted in its output rows directly.  No host read-back anywhere.
// mgv_neg_partition_local is the same three passes with the local draw in pass A (negatives inside each graph, a share of reversed
// links); mgv_neg_draw_local is that draw alone.
#include "mgv_launch.h"
#include "mgv_neg_draw.h"
#include "../../include/mgvae_hip.h"

namespace mgv {

constexpr int kNpChunk = 16384;        // slots per chunk (passes A and B)
constexpr int kNpDrawThreads = 512;    // pass A: 32 slots per thread
constexpr int kNpThreads = 1024;       // passes B and C
constexpr int kNpMaxBlocks = 2048;     // node blocks that passes A and B count in LDS
constexpr int kNpMaxShift = 12;        // nodes per block that pass C scans in LDS: 4,096
constexpr int kNpCap = 16384;          // pairs one finishing trip holds in LDS
constexpr int kNpShort = 32;           // lists up to here are sorted by one thread
constexpr int kNpScanInts = 17;        // np_exscan's wave totals and its carry
constexpr int64_t kNpMaxE = 1ll << 28; // the workspace (a little over 4 E ints) is sized by an int

// a[0 .. n) -> its exclusive prefix sums in place, a[n] = the total; LDS, all kNpThreads threads; s_w: kNpScanInts
__device__ __forceinline__ void np_exscan(int* a, int n, int* s_w) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_w[16] = 0;
    __syncthreads();
    for (int b0 = 0; b0 < n; b0 += kNpThreads) {
        const int i = b0 + threadIdx.x;
        const int t = i < n ? a[i] : 0;
        int inc = t;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int u = __shfl_up(inc, d, 64); if (lane >= d) inc += u; }
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        int woff = s_w[16];
        for (int k = 0; k < w; ++k) woff += s_w[k];
        if (i < n) a[i] = woff + inc - t;
        __syncthreads();
        if (threadIdx.x == kNpThreads - 1) s_w[16] = woff + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) a[n] = s_w[16];
    __syncthreads();
}

// a[0 .. n) ascending, any n, LDS or global, all threads of the workgroup: the bitonic network whose merges open with a flip, so
// that every exchange moves the smaller value down and the network padded to a power of two never touches its padding
__device__ __forceinline__ void np_sort_wide(int32_t* a, int n) {
    for (unsigned k = 2; (k >> 1) < (unsigned)n; k <<= 1) {
        for (unsigned i = threadIdx.x; i < (unsigned)n; i += blockDim.x) {
            const unsigned j = i ^ (k - 1);
            if (j > i && j < (unsigned)n) { const int x = a[i], y = a[j]; if (y < x) { a[i] = y; a[j] = x; } }
        }
        __syncthreads();
        for (unsigned h = k >> 2; h > 0; h >>= 1) {
            for (unsigned i = threadIdx.x; i < (unsigned)n; i += blockDim.x) {
                const unsigned j = i ^ h;
                if (j > i && j < (unsigned)n) { const int x = a[i], y = a[j]; if (y < x) { a[i] = y; a[j] = x; } }
            }
            __syncthreads();
        }
    }
}

// the draw of pass A, a compile-time policy: the batch-wide draw (neg_draw_slot: mgv_neg_partition) or the local one (neg_draw_slot_local:
// mgv_neg_partition_local).  With s uniform over the batch and d uniform inside s's graph every node is still a destination with
// probability 1 / N per slot, so the header's invariant holds for the local slots; reversed slots follow the positive degrees, and a
// hub's block or list that outgrows a trip takes pass C's several trips or its output-row path.
struct NpDrawBatch { static constexpr bool kLocal = false; };
struct NpDrawLocal {
    static constexpr bool kLocal = true;
    int64_t R, Epos;
    int G;
    const int32_t *graph_ptr, *in_src, *in_dst;
};

// the table of a local draw copied into LDS, clamped, where it fits (uniform over the workgroup; the caller's barrier follows)
__device__ __forceinline__ bool np_stage_graphs(const NpDrawLocal& p, int64_t N, int* s_gp) {
    if (p.G > kNegGraphLds) return false;
    for (int g = threadIdx.x; g <= p.G; g += blockDim.x) s_gp[g] = neg_graph_ptr(p.graph_ptr, g, (int)N);
    return true;
}

// the slots [c0, c1) of a chunk: slot(i, s, d) draws, the pair is stored and counted per source block and per destination block
template <class Slot>
__device__ __forceinline__ void np_draw_chunk(int64_t c0, int64_t c1, int shift, int nb, int32_t* ps, int32_t* pd, int* s_h, Slot slot) {
    for (int64_t i = c0 + threadIdx.x; i < c1; i += kNpDrawThreads) {
        int s, d;
        slot(i, s, d);
        ps[i] = s; pd[i] = d;
        atomicAdd(&s_h[s >> shift], 1);
        atomicAdd(&s_h[nb + (d >> shift)], 1);
    }
}

// ---- A: draw.  hist[(side * nb + block) * nchunks + chunk]
template <class Draw>
__global__ __launch_bounds__(kNpDrawThreads) void k_np_draw(int64_t N, int64_t E, uint64_t seed, const int32_t* pos_ptr, const int32_t* pos_dst,
                                                            int shift, int nb, int nchunks, int32_t* ps, int32_t* pd, int32_t* hist, Draw draw) {
    __shared__ int s_h[2 * kNpMaxBlocks];
    for (int b = threadIdx.x; b < 2 * nb; b += kNpDrawThreads) s_h[b] = 0;
    const int64_t c0 = (int64_t)blockIdx.x * kNpChunk;
    const int64_t c1 = c0 + kNpChunk < E ? c0 + kNpChunk : E;
    if constexpr (Draw::kLocal) {
        __shared__ int s_gp[kNegGraphLds + 1];
        const bool staged = np_stage_graphs(draw, N, s_gp);
        __syncthreads();
        if (staged)
            np_draw_chunk(c0, c1, shift, nb, ps, pd, s_h, [&](int64_t i, int& s, int& d) {
                neg_draw_slot_local(N, seed, i, pos_ptr, pos_dst, draw.R, draw.G, s_gp, draw.Epos, draw.in_src, draw.in_dst, s, d);
            });
        else
            np_draw_chunk(c0, c1, shift, nb, ps, pd, s_h, [&](int64_t i, int& s, int& d) {
                neg_draw_slot_local(N, seed, i, pos_ptr, pos_dst, draw.R, draw.G, draw.graph_ptr, draw.Epos, draw.in_src, draw.in_dst, s, d);
            });
    } else {
        __syncthreads();
        np_draw_chunk(c0, c1, shift, nb, ps, pd, s_h, [&](int64_t i, int& s, int& d) { neg_draw_slot(N, seed, i, pos_ptr, pos_dst, s, d); });
    }
    __syncthreads();
    for (int b = threadIdx.x; b < 2 * nb; b += kNpDrawThreads) hist[(int64_t)b * nchunks + blockIdx.x] = s_h[b];
}

// ---- the local draw alone, slot by slot: the pairs as int64, in slot order (the probe of the tests; the two-entry route of the host)
__global__ __launch_bounds__(kThreads) void k_neg_draw_local(int64_t N, int64_t E, uint64_t seed, const int32_t* pos_ptr, const int32_t* pos_dst,
                                                            NpDrawLocal draw, int64_t* neg_src, int64_t* neg_dst) {
    __shared__ int s_gp[kNegGraphLds + 1];
    const bool staged = np_stage_graphs(draw, N, s_gp);
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < E; i += (int64_t)gridDim.x * kThreads) {
        int s, d;
        if (staged) neg_draw_slot_local(N, seed, i, pos_ptr, pos_dst, draw.R, draw.G, s_gp, draw.Epos, draw.in_src, draw.in_dst, s, d);
        else neg_draw_slot_local(N, seed, i, pos_ptr, pos_dst, draw.R, draw.G, draw.graph_ptr, draw.Epos, draw.in_src, draw.in_dst, s, d);
        neg_src[i] = s; neg_dst[i] = d;
    }
}

// ---- B: partition.  base = the scan of hist (side 1 continues side 0's count: minus E)
__global__ __launch_bounds__(kNpThreads) void k_np_partition(int64_t E, int shift, int nb, int nchunks, const int32_t* ps, const int32_t* pd,
                                                             const int32_t* base, int2* part0, int2* part1) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];      // all of the kernel's LDS: the opt-in of allow_lds covers dynamic LDS only
    int2* s_pair = reinterpret_cast<int2*>(s_dyn);     // [kNpChunk]
    int* s_cur = s_dyn + 2 * kNpChunk;                 // [nb + 1]
    int* s_delta = s_cur + nb + 1;                     // [nb]
    int* s_w = s_delta + nb;                           // [kNpScanInts]
    constexpr int PT = kNpChunk / kNpThreads;
    const int64_t c0 = (int64_t)blockIdx.x * kNpChunk;
    const int m = (int)((c0 + kNpChunk < E ? c0 + kNpChunk : E) - c0);
    int rs[PT], rd[PT];
#pragma unroll
    for (int j = 0; j < PT; ++j) {
        const int i = j * kNpThreads + threadIdx.x;
        rs[j] = i < m ? ps[c0 + i] : 0;
        rd[j] = i < m ? pd[c0 + i] : 0;
    }
    for (int side = 0; side < 2; ++side) {
        for (int b = threadIdx.x; b < nb; b += kNpThreads) s_cur[b] = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PT; ++j)
            if (j * kNpThreads + (int)threadIdx.x < m) atomicAdd(&s_cur[(side ? rd[j] : rs[j]) >> shift], 1);
        __syncthreads();
        np_exscan(s_cur, nb, s_w);
        for (int b = threadIdx.x; b < nb; b += kNpThreads)
            s_delta[b] = base[((int64_t)side * nb + b) * nchunks + blockIdx.x] - (side ? (int)E : 0) - s_cur[b];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PT; ++j)
            if (j * kNpThreads + (int)threadIdx.x < m) {
                const int k = side ? rd[j] : rs[j], o = side ? rs[j] : rd[j];
                s_pair[atomicAdd(&s_cur[k >> shift], 1)] = make_int2(k, o);
            }
        __syncthreads();
        int2* part = side ? part1 : part0;
        for (int p = threadIdx.x; p < m; p += kNpThreads) {
            const int2 pr = s_pair[p];
            part[s_delta[pr.x >> shift] + p] = pr;
        }
        __syncthreads();
    }
}

// ---- C: finish.  grid (nb, 2): side 0 = by source (out_ptr, out_dst, both rows of edge_index), side 1 = by destination (in_ptr, in_src)
__global__ __launch_bounds__(kNpThreads) void k_np_finish(int64_t N, int64_t E, int shift, int nb, int nchunks, const int32_t* base,
                                                          const int2* part0, const int2* part1, int32_t* out_ptr, int32_t* out_dst,
                                                          int32_t* in_ptr, int32_t* in_src, int64_t* ei0, int64_t* ei1, int32_t* status) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];
    const int L = 1 << shift;
    int* s_val = s_dyn;                                // [kNpCap]
    int* s_ptr = s_dyn + kNpCap;                       // [L + 1]
    int* s_cur = s_ptr + L + 1;                        // [L + 1]
    int* s_w = s_cur + L + 1;                          // [kNpScanInts]
    int& s_n = s_w[kNpScanInts];                       // long lists of a trip / the cursor of an oversize node
    const int b = blockIdx.x, side = blockIdx.y, tid = threadIdx.x;
    const int2* part = side ? part1 : part0;
    int32_t* gptr = side ? in_ptr : out_ptr;
    int32_t* list = side ? in_src : out_dst;
    const int64_t hb = ((int64_t)side * nb + b) * nchunks;
    const int off = side ? (int)E : 0;
    const int start = base[hb] - off, n = base[hb + nchunks] - off - start;
    const int64_t node0 = (int64_t)b << shift;
    const int nodes = (int)(N - node0 < L ? N - node0 : L);
    part += start;

    for (int i = tid; i < nodes; i += kNpThreads) s_ptr[i] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kNpThreads) atomicAdd(&s_ptr[part[i].x - (int)node0], 1);
    __syncthreads();
    np_exscan(s_ptr, nodes, s_w);
    for (int i = tid; i < nodes; i += kNpThreads) gptr[node0 + i] = start + s_ptr[i];
    if (b == nb - 1 && tid == 0) gptr[N] = start + n;

    int trips = 0, wide = 0;
    for (int lo = 0; lo < nodes; ++trips) {
        const int p0 = s_ptr[lo];
        int hi = lo + 1;
        if (s_ptr[hi] - p0 > kNpCap) {
            // one node above a trip's capacity: placed in its output rows, sorted there
            const int len = s_ptr[hi] - p0;
            int32_t* row = list + start + p0;
            if (tid == 0) s_n = 0;
            __syncthreads();
            for (int i = tid; i < n; i += kNpThreads) {
                const int2 pr = part[i];
                if (pr.x - (int)node0 == lo) row[atomicAdd(&s_n, 1)] = pr.y;
            }
            __syncthreads();
            np_sort_wide(row, len);
            if (!side)
                for (int p = tid; p < len; p += kNpThreads) { ei0[start + p0 + p] = node0 + lo; ei1[start + p0 + p] = row[p]; }
            __syncthreads();
            ++wide;
        } else {
            int z = nodes;                              // the largest hi with at most kNpCap pairs in [lo, hi)
            while (hi < z) { const int mid = (hi + z + 1) >> 1; if (s_ptr[mid] - p0 <= kNpCap) hi = mid; else z = mid - 1; }
            const int m = s_ptr[hi] - p0;
            for (int i = lo + tid; i < hi; i += kNpThreads) s_cur[i] = s_ptr[i] - p0;
            if (tid == 0) s_n = 0;
            __syncthreads();
            for (int i = tid; i < n; i += kNpThreads) {
                const int2 pr = part[i];
                const int k = pr.x - (int)node0;
                if (k >= lo && k < hi) s_val[atomicAdd(&s_cur[k], 1)] = pr.y;
            }
            __syncthreads();
            // every node's entries ascending: short lists by their thread, the others queued (the cursors are dead by now)
            for (int i = lo + tid; i < hi; i += kNpThreads) {
                int* v = s_val + (s_ptr[i] - p0);
                const int len = s_ptr[i + 1] - s_ptr[i];
                if (len > kNpShort) { s_cur[atomicAdd(&s_n, 1)] = i; continue; }
                for (int a = 1; a < len; ++a) {
                    const int x = v[a];
                    int c = a;
                    for (; c > 0 && v[c - 1] > x; --c) v[c] = v[c - 1];
                    v[c] = x;
                }
            }
            __syncthreads();
            const int nlong = s_n;
            for (int q = 0; q < nlong; ++q) {
                const int i = s_cur[q];
                np_sort_wide(s_val + (s_ptr[i] - p0), s_ptr[i + 1] - s_ptr[i]);
            }
            for (int p = tid; p < m; p += kNpThreads) {
                const int v = s_val[p];
                const int64_t g = (int64_t)start + p0 + p;
                list[g] = v;
                if (!side) {
                    int a = lo, c = hi - 1;             // the node whose list holds position p0 + p
                    while (a < c) { const int mid = (a + c + 1) >> 1; if (s_ptr[mid] <= p0 + p) a = mid; else c = mid - 1; }
                    ei0[g] = node0 + a;
                    ei1[g] = v;
                }
            }
            __syncthreads();
        }
        lo = hi;
    }
    if (tid == 0) {
        if (b == 0 && side == 0) status[0] = nb;
        atomicMax(status + 1, n);
        atomicAdd(status + 2, trips);
        atomicAdd(status + 3, wide);
    }
}

struct NpLayout { int64_t status, hist, scan, scratch, part0, part1, total; };

// nb node blocks: the workspace is laid out for the blocks in use, and sized (mgv_neg_partition_ws_ints) for kNpMaxBlocks
static NpLayout np_layout(int64_t E, int64_t nb) {
    const int64_t nchunks = (E + kNpChunk - 1) / kNpChunk, nh = 2 * nb * nchunks;
    NpLayout w;
    w.status = 0;
    w.hist = 8;
    w.scan = w.hist + nh;
    w.scratch = w.scan + nh + 2;
    w.part0 = (w.scratch + nh / 2048 + 4 + 1) & ~1ll;      // int2 rows: 8-byte aligned
    w.part1 = w.part0 + 2 * E;
    w.total = w.part1 + 2 * E;
    return w;
}

}  // namespace mgv

using namespace mgv;

extern "C" int mgv_neg_partition_ws_ints(int64_t N, int64_t E) {
    if (N < 2 || N >= (1ll << 31) || E < 0 || E >= kNpMaxE) return -1;
    return (int)np_layout(E, kNpMaxBlocks).total;
}

// the three passes and the scan under one draw policy: what mgv_neg_partition and mgv_neg_partition_local share, refusals included
template <class Draw>
static int np_run(int64_t N, int64_t E, uint64_t seed, int shift, const int32_t* pos_out_ptr, const int32_t* pos_out_dst, int64_t* edge_index,
                  int32_t* out_ptr, int32_t* out_dst, int32_t* in_ptr, int32_t* in_src, int32_t* ws, int64_t ws_ints, void* stream, Draw draw) {
    MGV_CHECK_ARG(N >= 2 && N < (1ll << 31) && E >= 0 && E < kNpMaxE && pos_out_ptr && out_ptr && in_ptr && ws);
    MGV_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0 && ws_ints >= mgv_neg_partition_ws_ints(N, E));
    MGV_CHECK_ARG(E == 0 || (edge_index && out_dst && in_src));     // (the payload arrays of an empty draw have no address)
    if (shift < 0 || shift > kNpMaxShift) return MGV_EUNSUPPORTED;
    const int64_t L = 1ll << shift, nb64 = (N + L - 1) / L;
    if (nb64 > kNpMaxBlocks) return MGV_EUNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipMemsetAsync(ws, 0, 8 * sizeof(int32_t), st);
    if (E == 0) {                               // no slots: empty buckets
        hipMemsetAsync(out_ptr, 0, (N + 1) * sizeof(int32_t), st);
        hipMemsetAsync(in_ptr, 0, (N + 1) * sizeof(int32_t), st);
        MGV_LAUNCH_RET();
    }
    const int nb = (int)nb64, nchunks = (int)((E + kNpChunk - 1) / kNpChunk);
    const NpLayout w = np_layout(E, nb);
    int32_t* ps = reinterpret_cast<int32_t*>(edge_index);      // the drawn pairs rest in edge_index's own rows until pass C writes them
    int32_t* pd = ps + E;
    int2* part0 = reinterpret_cast<int2*>(ws + w.part0);
    int2* part1 = reinterpret_cast<int2*>(ws + w.part1);
    hipLaunchKernelGGL(k_np_draw<Draw>, dim3(nchunks), dim3(kNpDrawThreads), 0, st, N, E, seed, pos_out_ptr, pos_out_dst, shift, nb, nchunks, ps,
                       pd, ws + w.hist, draw);
    const int rc = mgv_scan_exclusive_i32(2ll * nb * nchunks, ws + w.hist, ws + w.scan, ws + w.scratch, stream);
    if (rc != MGV_OK) return rc;
    const size_t lds_b = (size_t)(2 * kNpChunk + 2 * nb + 1 + kNpScanInts) * sizeof(int);
    allow_lds<k_np_partition>();
    hipLaunchKernelGGL(k_np_partition, dim3(nchunks), dim3(kNpThreads), lds_b, st, E, shift, nb, nchunks, ps, pd, ws + w.scan, part0, part1);
    const size_t lds_c = (size_t)(kNpCap + 2 * ((int)L + 1) + kNpScanInts + 1) * sizeof(int);
    allow_lds<k_np_finish>();
    hipLaunchKernelGGL(k_np_finish, dim3(nb, 2), dim3(kNpThreads), lds_c, st, N, E, shift, nb, nchunks, ws + w.scan, part0, part1, out_ptr, out_dst,
                       in_ptr, in_src, edge_index, edge_index + E, ws + w.status);
    MGV_LAUNCH_RET();
}

extern "C" int mgv_neg_partition(int64_t N, int64_t E, uint64_t seed, int shift, const int32_t* pos_out_ptr, const int32_t* pos_out_dst,
                                 int64_t* edge_index, int32_t* out_ptr, int32_t* out_dst, int32_t* in_ptr, int32_t* in_src, int32_t* ws,
                                 int64_t ws_ints, void* stream) {
    return np_run(N, E, seed, shift, pos_out_ptr, pos_out_dst, edge_index, out_ptr, out_dst, in_ptr, in_src, ws, ws_ints, stream, NpDrawBatch{});
}

// what both local entries refuse before anything else, in this order
static int np_check_local(int64_t E, int64_t R, int G, const int32_t* graph_ptr, int64_t Epos, const int32_t* pos_in_src, const int32_t* pos_in_dst) {
    MGV_CHECK_ARG(G >= 1);
    MGV_CHECK_ARG(R >= 0 && R <= E);
    MGV_CHECK_ARG(R == 0 || (Epos >= 1 && Epos < (1ll << 31)));
    MGV_CHECK_ARG(graph_ptr);
    MGV_CHECK_ARG(R == 0 || (pos_in_src && pos_in_dst));
    return MGV_OK;
}

extern "C" int mgv_neg_draw_local(int64_t N, int64_t E, uint64_t seed, int64_t R, int G, const int32_t* graph_ptr, const int32_t* pos_out_ptr,
                                  const int32_t* pos_out_dst, int64_t Epos, const int32_t* pos_in_src, const int32_t* pos_in_dst,
                                  int64_t* neg_src, int64_t* neg_dst, void* stream) {
    const int rc = np_check_local(E, R, G, graph_ptr, Epos, pos_in_src, pos_in_dst);
    if (rc != MGV_OK) return rc;
    MGV_CHECK_ARG(N >= 2 && N < (1ll << 31) && E >= 0 && E < kNpMaxE && pos_out_ptr);
    if (E == 0) return MGV_OK;              // no slots: the pair arrays of an empty draw have no address
    MGV_CHECK_ARG(neg_src && neg_dst);
    const NpDrawLocal draw{R, Epos, G, graph_ptr, pos_in_src, pos_in_dst};
    hipLaunchKernelGGL(k_neg_draw_local, dim3(grid_for((E + kThreads - 1) / kThreads, 16)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), N, E,
                       seed, pos_out_ptr, pos_out_dst, draw, neg_src, neg_dst);
    MGV_LAUNCH_RET();
}

extern "C" int mgv_neg_partition_local(int64_t N, int64_t E, uint64_t seed, int shift, const int32_t* pos_out_ptr, const int32_t* pos_out_dst,
                                       int64_t R, int G, const int32_t* graph_ptr, int64_t Epos, const int32_t* pos_in_src,
                                       const int32_t* pos_in_dst, int64_t* edge_index, int32_t* out_ptr, int32_t* out_dst, int32_t* in_ptr,
                                       int32_t* in_src, int32_t* ws, int64_t ws_ints, void* stream) {
    const int rc = np_check_local(E, R, G, graph_ptr, Epos, pos_in_src, pos_in_dst);
    if (rc != MGV_OK) return rc;
    return np_run(N, E, seed, shift, pos_out_ptr, pos_out_dst, edge_index, out_ptr, out_dst, in_ptr, in_src, ws, ws_ints, stream,
                  NpDrawLocal{R, Epos, G, graph_ptr, pos_in_src, pos_in_dst});
}
