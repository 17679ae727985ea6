// Exact functional ordering accuracy (utils/utils.py:111-147 get_function_acc, on the `dis` of trainer.py:158-160): where the
// reference draws 100 comparisons of two listed truth-table pairs per circuit, EVERY unordered comparison {p, q}, p < q, of a circuit's
// listed pairs is counted, as integers.  With dd = gt[q] - gt[p] and de = pred[q] - pred[p] in float32 a comparison is
//     eligible at gap j   dd != 0 && fabsf(dd) >= gaps[j]           (the reference's two `continue`s negated; note the >=)
//     concordant          (dd > 0 && de > 0) || (dd < 0 && de < 0)
//     tied                de == 0
// and out[g][j] = {eligible, eligible and concordant, eligible and tied}.  A NaN in gt makes its comparisons ineligible (every compare
// with it is false); a NaN in pred leaves them eligible and neither concordant nor tied, the reference's `succ = False`.
//
// The walk.  Row tiles of kConcordTile = 256 listed pairs, one row per thread with its (gt, pred) in registers; the column tiles of
// the upper triangle — from the row tile's own (diagonal) tile to the last tile that holds a partner of one of its rows — pass
// through LDS as (gt, pred) pairs, and every lane reads the same address at a time: a broadcast, no bank conflict.  Row p's partners
// are the q with p < q < hi[p], hi[p] the end of p's own segment (a binary search of seg_ptr per row, clamped into [0, P] as
// row_ranges of pair_scores.hip clamps graph_ptr): a row block that straddles segments gives every row its own range, and no
// comparison crosses a boundary because q > p >= lo[p].  A column tile that lies behind the diagonal and in front of hi for every
// lane of a wave takes the loop without the range test (a wave-uniform branch); columns past P hold gt = NaN and are ineligible.
// grid.y workgroups share one row tile's column tiles (tile ct0 + y, ct0 + y + grid.y, ...) when there are too few row tiles to
// fill the device: one 65,536-node circuit lists 16,384 pairs, 64 row tiles.
//
// Counting.  The three kinds of one comparison travel as ONE word, w = 1 | concordant << 10 | tied << 20 (0 when dd == 0 or the
// column is no partner), and gap j adds it where fabsf(dd) >= gaps[j]: a compare, a select and an add per gap, the chain unrolled at
// compile time over NB in {1, 2, 4, 8} gaps padded with +inf (only an infinite fabsf(dd) passes a padding gap, and the counter it
// lands in is never read).  A tile has 256 columns, so a field holds at most 256 < 1024 before the lane unpacks the word into its
// int32 counters at the end of the tile (a row has fewer than 2^31 partners).  No register is indexed dynamically, and there is no
// LDS atomic in the tile loop.  kConcordTile is ops.CONCORD_TILE on the Python side.
//
// Reduction.  After the walk a segmented butterfly over each wave (shuffles on 64-bit values; rows of one segment are neighbours)
// leaves the sum of every run of rows of one segment in the run's first lane.  That lane adds it to a 64-bit LDS counter when the
// segment is the workgroup's first or last one, and the workgroup then issues ONE global 64-bit integer atomic add per non-zero
// (segment, gap, kind) of those two, as k_pair_hist does; a segment that lies wholly inside the tile (fewer than 256 pairs) adds
// directly, once per wave it touches.  Integer adds only: exact, and the same bytes from call to call whatever the order.
#include "mgv_launch.h"
#include "../../include/mgvae_hip.h"

#include <math.h>

namespace mgv {

constexpr int kConcordTile = 256;      // rows per workgroup (one per thread) and columns per LDS tile
constexpr int kConcordMaxGaps = 8;
constexpr int kConcordField = 10;      // bits per kind in the packed word
static_assert(kConcordTile == kThreads, "one row per thread");
static_assert(kConcordTile < (1 << kConcordField), "a tile's count of one kind must fit its field");

struct ConcordGaps { float g[kConcordMaxGaps]; };

// one column against the lane's row: the packed word of the comparison (0: not eligible at any gap)
__device__ __forceinline__ int concord_word(float rg, float rp, float cg, float cp) {
    const float dd = cg - rg, de = cp - rp;
    const int conc = ((dd > 0.f && de > 0.f) || (dd < 0.f && de < 0.f)) ? (1 << kConcordField) : 0;
    const int tied = de == 0.f ? (1 << (2 * kConcordField)) : 0;
    return dd != 0.f ? (1 | conc | tied) : 0;
}

template <int NB, bool CHECKED>
__device__ __forceinline__ void concord_tile(int (&acc)[NB], const float4* cl, const ConcordGaps& gaps, float rg, float rp, int jlo, int jhi) {
#pragma unroll 4
    for (int j2 = 0; j2 < kConcordTile / 2; ++j2) {
        const float4 c = cl[j2];                               // columns 2 j2 and 2 j2 + 1: (gt, pred, gt, pred), one address for all lanes
        int w0 = concord_word(rg, rp, c.x, c.y), w1 = concord_word(rg, rp, c.z, c.w);
        if constexpr (CHECKED) {
            w0 = (2 * j2 >= jlo && 2 * j2 < jhi) ? w0 : 0;
            w1 = (2 * j2 + 1 >= jlo && 2 * j2 + 1 < jhi) ? w1 : 0;
        }
        const float a0 = fabsf(c.x - rg), a1 = fabsf(c.z - rg);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            acc[b] += a0 >= gaps.g[b] ? w0 : 0;                // false for a NaN
            acc[b] += a1 >= gaps.g[b] ? w1 : 0;
        }
    }
}

template <int NB>
__global__ __launch_bounds__(kThreads) void k_concord(int64_t P, const float* gt, const float* pred, const int32_t* sp, int G,
                                                      ConcordGaps gaps, int B, unsigned long long* out) {
    __shared__ __attribute__((aligned(16))) float2 cl[kConcordTile];
    __shared__ unsigned long long lh[2 * 3 * NB];
    __shared__ int s_chi, s_gfirst, s_glast;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t u0 = (int64_t)blockIdx.x * kConcordTile, u = u0 + tid;       // u0 < P
    // the row's segment: partners are (u, hi)
    int64_t hi = 0;
    int gi = 0;
    float rg = NAN, rp = 0.f;
    if (u < P) {
        rg = gt[u]; rp = pred[u];
        if (sp == nullptr) { hi = P; }
        else {
            int a = 0, b = G;                                  // first segment whose end lies behind u
            while (a < b) { const int m = (a + b) >> 1; if ((int64_t)sp[m + 1] <= u) a = m + 1; else b = m; }
            if (a < G) {
                const int64_t lo = sp[a];
                hi = sp[a + 1];
                gi = a;
                hi = (lo > u) ? 0 : (hi > P ? P : hi);         // whatever the table holds, no column outside [0, P) is touched
            }
        }
    }
    if (tid == 0) { s_chi = 0; s_gfirst = gi; }
    const int64_t left = P - 1 - u0;
    if (tid == (left < kConcordTile - 1 ? (int)left : kConcordTile - 1)) s_glast = gi;   // the tile's last row inside P
    for (int i = tid; i < 2 * 3 * NB; i += kThreads) lh[i] = 0ull;
    __syncthreads();
    if (hi > u + 1) atomicMax(&s_chi, (int)hi);                // once per row, in front of the walk
    __syncthreads();
    const int64_t chi = s_chi;
    const int gfirst = s_gfirst, glast = s_glast;
    int elig[NB], conc[NB], tied[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) elig[b] = conc[b] = tied[b] = 0;
    const int64_t ct0 = (int64_t)blockIdx.x + blockIdx.y, ct1 = (chi + kConcordTile - 1) / kConcordTile;   // chi = 0: nothing to walk
    auto col_load = [&](int64_t ct) {
        const int64_t q = ct * kConcordTile + tid;
        return q < P ? make_float2(gt[q], pred[q]) : make_float2(NAN, 0.f);
    };
    float2 nxt = make_float2(NAN, 0.f);
    if (ct0 < ct1) nxt = col_load(ct0);
    for (int64_t ct = ct0; ct < ct1; ct += gridDim.y) {
        __syncthreads();
        cl[tid] = nxt;
        __syncthreads();
        if (ct + gridDim.y < ct1) nxt = col_load(ct + gridDim.y);
        const int64_t c0 = ct * kConcordTile;
        // the row's partners inside this tile: columns [jlo, jhi) of it
        const int64_t lo_ = u + 1 - c0, hi_ = hi - c0;
        const int jlo = lo_ < 0 ? 0 : (lo_ > kConcordTile ? kConcordTile : (int)lo_);
        const int jhi = hi_ < 0 ? 0 : (hi_ > kConcordTile ? kConcordTile : (int)hi_);
        if (__ballot(jlo < jhi) == 0ull) continue;             // no row of the wave has a partner here
        int acc[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = 0;
        const float4* c4 = reinterpret_cast<const float4*>(cl);
        if (__ballot(jlo != 0 || jhi != kConcordTile) == 0ull) concord_tile<NB, false>(acc, c4, gaps, rg, rp, jlo, jhi);
        else concord_tile<NB, true>(acc, c4, gaps, rg, rp, jlo, jhi);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            elig[b] += acc[b] & ((1 << kConcordField) - 1);
            conc[b] += (acc[b] >> kConcordField) & ((1 << kConcordField) - 1);
            tied[b] += acc[b] >> (2 * kConcordField);
        }
    }
    // runs of one segment inside the wave -> the run's first lane
    const int gprev = __shfl_up(gi, 1, 64);
    const bool head = lane == 0 || gprev != gi;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            unsigned long long v = (unsigned long long)(unsigned)(k == 0 ? elig[b] : k == 1 ? conc[b] : tied[b]);
#pragma unroll
            for (int d = 1; d < 64; d *= 2) {
                const unsigned long long o = __shfl_down(v, d, 64);
                const int og = __shfl_down(gi, d, 64);
                if (lane + d < 64 && og == gi) v += o;
            }
            if (head && v != 0ull && b < B) {
                if (gi == gfirst) atomicAdd(&lh[3 * b + k], v);
                else if (gi == glast) atomicAdd(&lh[3 * NB + 3 * b + k], v);
                else atomicAdd(&out[((int64_t)gi * B + b) * 3 + k], v);           // gi < max(G, 1), b < B
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < 2 * 3 * NB; i += kThreads) {
        const unsigned long long n = lh[i];
        const int s = i / (3 * NB), r = i % (3 * NB);          // r = 3 b + k
        if (n != 0ull && r < 3 * B) atomicAdd(&out[(int64_t)(s == 0 ? gfirst : glast) * B * 3 + r], n);
    }
}

}  // namespace mgv

extern "C" int mgv_concord_counts(int64_t P, const float* gt, const float* pred, const int32_t* seg_ptr, int G, const float* gaps_host, int B,
                                  int64_t* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    MGV_CHECK_ARG(P >= 0 && P <= 0x7fffffffLL);                            // pair ids are int32
    MGV_CHECK_ARG(G >= 0);
    MGV_CHECK_ARG(B >= 1 && B <= mgv::kConcordMaxGaps);
    MGV_CHECK_ARG(out != nullptr);
    MGV_CHECK_ARG(P == 0 || (gt != nullptr && pred != nullptr && gaps_host != nullptr));
    mgv::ConcordGaps gaps;
    for (int j = 0; j < mgv::kConcordMaxGaps; ++j) gaps.g[j] = INFINITY;
    if (gaps_host != nullptr) {
        for (int j = 0; j < B; ++j) {
            MGV_CHECK_ARG(gaps_host[j] >= 0.f);                            // false for a NaN
            gaps.g[j] = gaps_host[j];
        }
    }
    const int64_t rows = G > 1 ? G : 1;
    hipError_t err = hipMemsetAsync(out, 0, sizeof(int64_t) * (size_t)rows * (size_t)B * 3, st);
    if (err != hipSuccess) return (int)err;
    if (P == 0) return MGV_OK;
    const int64_t nrt = (P + mgv::kConcordTile - 1) / mgv::kConcordTile;   // <= 2^23
    int split = (int)(2048 / nrt);                                         // few row tiles: their column tiles are shared out
    split = split < 1 ? 1 : (split > 16 ? 16 : split);
    if ((int64_t)split > nrt) split = (int)nrt;
    unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
    const dim3 grid((unsigned)nrt, (unsigned)split);
    if (B == 1) hipLaunchKernelGGL(mgv::k_concord<1>, grid, dim3(mgv::kThreads), 0, st, P, gt, pred, seg_ptr, G, gaps, B, o);
    else if (B == 2) hipLaunchKernelGGL(mgv::k_concord<2>, grid, dim3(mgv::kThreads), 0, st, P, gt, pred, seg_ptr, G, gaps, B, o);
    else if (B <= 4) hipLaunchKernelGGL(mgv::k_concord<4>, grid, dim3(mgv::kThreads), 0, st, P, gt, pred, seg_ptr, G, gaps, B, o);
    else hipLaunchKernelGGL(mgv::k_concord<8>, grid, dim3(mgv::kThreads), 0, st, P, gt, pred, seg_ptr, G, gaps, B, o);
    MGV_LAUNCH_RET();
}
