// Negative edges of the reconstruction loss, sampled and bucketed on the device.
//
// The reference calls torch_geometric.utils.negative_sampling(pos + self loops, N) (dg_ae_model_aig.py:115-119):
// as many (src, dst) pairs as that edge set has, uniform over the pairs that are neither an edge nor a self loop.
// Here every output slot draws pairs from a counter-based generator until one passes the test (the edge test walks
// the source's out-list in the batch's CSR: no sorted key table, no compaction pass), and counts its two ends so
// that a second pass can bucket the pairs by source and by destination: the backward of the loss then gathers
// instead of adding 2 x 256 bytes per pair with memory-side float atomics.
#include "mgv_common.h"
#include "mgv_neg_draw.h"
#include "../../include/mgvae_hip.h"

namespace mgv {

__global__ __launch_bounds__(kThreads) void k_neg_sample(int64_t N, int64_t E, uint64_t seed, const int32_t* out_ptr, const int32_t* out_dst,
                                                        int64_t* neg_src, int64_t* neg_dst, int32_t* cnt_out, int32_t* cnt_in,
                                                        int32_t* rank_out, int32_t* rank_in) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < E; i += (int64_t)gridDim.x * kThreads) {
        int s, d;
        neg_draw_slot(N, seed, i, out_ptr, out_dst, s, d);
        neg_src[i] = s; neg_dst[i] = d;
        // the pair's place inside its source's and its destination's bucket: the count it found (the bucket pass then needs no atomics)
        rank_out[i] = atomicAdd(cnt_out + s, 1);
        rank_in[i] = atomicAdd(cnt_in + d, 1);
    }
}

// bucket pass: ptr arrays = exclusive scans of the counts, rank_* = the pairs' places inside their buckets (from the sampling pass)
__global__ __launch_bounds__(kThreads) void k_neg_bucket(int64_t E, const int64_t* neg_src, const int64_t* neg_dst, const int32_t* out_ptr,
                                                        const int32_t* in_ptr, const int32_t* rank_out, const int32_t* rank_in, int64_t* srt_src,
                                                        int64_t* srt_dst, int32_t* out_dst, int32_t* in_src) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < E; i += (int64_t)gridDim.x * kThreads) {
        const int s = (int)neg_src[i], d = (int)neg_dst[i];
        const int p = out_ptr[s] + rank_out[i];
        srt_src[p] = s; srt_dst[p] = d; out_dst[p] = d;
        in_src[in_ptr[d] + rank_in[i]] = s;
    }
}

}  // namespace mgv

extern "C" int mgv_neg_sample(int64_t N, int64_t E, uint64_t seed, const int32_t* pos_out_ptr, const int32_t* pos_out_dst,
                              int64_t* neg_src, int64_t* neg_dst, int32_t* cnt_out, int32_t* cnt_in, int32_t* rank_out, int32_t* rank_in,
                              void* stream) {
    MGV_CHECK_ARG(N >= 2 && N < (1ll << 31) && E >= 0 && pos_out_ptr && cnt_out && cnt_in && rank_out && rank_in);
    if (E == 0) return MGV_OK;              // no slots: the pair arrays of an empty draw have no address (as in mgv_neg_bucket)
    MGV_CHECK_ARG(neg_src && neg_dst);
    hipLaunchKernelGGL(mgv::k_neg_sample, dim3(mgv::grid_for((E + mgv::kThreads - 1) / mgv::kThreads, 16)), dim3(mgv::kThreads), 0,
                       static_cast<hipStream_t>(stream), N, E, seed, pos_out_ptr, pos_out_dst, neg_src, neg_dst, cnt_out, cnt_in, rank_out, rank_in);
    MGV_LAUNCH_RET();
}

extern "C" int mgv_neg_bucket(int64_t E, const int64_t* neg_src, const int64_t* neg_dst, const int32_t* out_ptr, const int32_t* in_ptr,
                              const int32_t* rank_out, const int32_t* rank_in, int64_t* srt_src, int64_t* srt_dst, int32_t* out_dst, int32_t* in_src,
                              void* stream) {
    MGV_CHECK_ARG(E >= 0 && out_ptr && in_ptr && rank_out && rank_in);
    if (E == 0) return MGV_OK;
    MGV_CHECK_ARG(neg_src && neg_dst && srt_src && srt_dst && out_dst && in_src);
    hipLaunchKernelGGL(mgv::k_neg_bucket, dim3(mgv::grid_for((E + mgv::kThreads - 1) / mgv::kThreads, 16)), dim3(mgv::kThreads), 0,
                       static_cast<hipStream_t>(stream), E, neg_src, neg_dst, out_ptr, in_ptr, rank_out, rank_in, srt_src, srt_dst, out_dst, in_src);
    MGV_LAUNCH_RET();
}
