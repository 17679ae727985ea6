// DiGAE baseline layer (DirectedGCNConv, reference DG_VAE/deepgate/digae_layer.py:73-114) for gfx950: the degree-normalised neighbour sum
//   out[i] = din(i)^-alpha * sum_{j in L(i)} dout(j)^-beta * y[j]        (+ the node's own term when the layer adds self loops)
// over a CSR of the lists L(i).  The layer's Linear runs before the sum, where the reference has it (y = lin(x), :95), on the project's
// linear kernels; here are the scaled sum in exact fp32, which is also its own backward pull, and the first layer on class rows, one
// byte per neighbour.  (A fused gather + bf16x3 product + store tile kernel was built and measured: it tied Linear + sum per layer and
// lost 3-5 % over the encoder, NOTEBOOK 2026-10-17, and was removed.)
// Every sum has a fixed order: no float atomics, cross-workgroup sums go through slab rows (mgv_slab.h).
#include "mgv_launch.h"
#include "mgv_slab.h"
#include "mgvae_hip.h"

namespace mgv {

constexpr int kDigcnHeavy = 64;          // lists longer than this go to the one-workgroup-per-node kernel (GraphPlan.HEAVY_ROW)
constexpr int kDigcnClasses = 8;         // class-table rows (digae_layer.MAX_FEATURE_CLASSES)

// d^-a, exact for a = 0 (1) and correctly rounded for a = 1; a node that sits in no list (d = 0, only without self loops) scales by 0
__device__ __forceinline__ float inv_pow(int d, float a) {
    if (d <= 0) return 0.f;
    if (a == 0.f) return 1.f;
    const float x = (float)d;
    if (a == 1.f) return 1.0f / x;
    if (a == 0.5f) return 1.0f / sqrtf(x);
    return powf(x, -a);
}

__global__ __launch_bounds__(kThreads) void k_digcn_scales(int64_t N, const int32_t* list_ptr, const int32_t* opp_ptr, float alpha, float beta,
                                                           int self_loops, float* r, float* c) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kThreads) {
        r[i] = inv_pow(list_ptr[i + 1] - list_ptr[i] + self_loops, alpha);
        c[i] = inv_pow(opp_ptr[i + 1] - opp_ptr[i] + self_loops, beta);
    }
}

// one neighbour's contribution: inner[j] * y[j], columns counted only where mask[j] > 0 (the ReLU of the layer whose gradient is pulled)
template <int H>
__device__ __forceinline__ float4 digcn_term(const float* y, const float* inner, const float* mask, int64_t j, int lr) {
    float4 v = scale4(inner[j], ld4(y + j * H + 4 * lr));
    if (mask) {
        const float4 m = ld4(mask + j * H + 4 * lr);
        v.x = m.x > 0.f ? v.x : 0.f; v.y = m.y > 0.f ? v.y : 0.f; v.z = m.z > 0.f ? v.z : 0.f; v.w = m.w > 0.f ? v.w : 0.f;
    }
    return v;
}

__device__ __forceinline__ float4 relu4(const float4& v) { return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)); }

// H/4 lanes per node, four neighbour rows in flight per lane; nodes in `heavy` territory are left to k_digcn_gather_heavy
template <int H>
__global__ __launch_bounds__(kThreads) void k_digcn_gather(int64_t N, const float* y, const int32_t* ptr, const int32_t* idx, const float* outer,
                                                           const float* inner, const float* mask, int self_loops, int relu, int skip_heavy,
                                                           float* out) {
    constexpr int LPR = H / 4;
    const int64_t stride = (int64_t)gridDim.x * kThreads / LPR;
    const int lr = threadIdx.x % LPR;
    for (int64_t node = ((int64_t)blockIdx.x * kThreads + threadIdx.x) / LPR; node < N; node += stride) {
        const int e0 = ptr[node], e1 = ptr[node + 1];
        if (skip_heavy && e1 - e0 > kDigcnHeavy) continue;
        float4 acc = self_loops ? digcn_term<H>(y, inner, mask, node, lr) : zero4();
        int e = e0;
        for (; e + 4 <= e1; e += 4) {
            const int j0 = idx[e], j1 = idx[e + 1], j2 = idx[e + 2], j3 = idx[e + 3];
            const float4 v0 = digcn_term<H>(y, inner, mask, j0, lr), v1 = digcn_term<H>(y, inner, mask, j1, lr);
            const float4 v2 = digcn_term<H>(y, inner, mask, j2, lr), v3 = digcn_term<H>(y, inner, mask, j3, lr);
            acc = add4(add4(add4(add4(acc, v0), v1), v2), v3);
        }
        for (; e < e1; ++e) acc = add4(acc, digcn_term<H>(y, inner, mask, idx[e], lr));
        acc = scale4(outer[node], acc);
        st4(out + node * H + 4 * lr, relu ? relu4(acc) : acc);
    }
}

// one workgroup per long list (a primary input or a clock-like net with thousands of consumers): the lane groups stride over the
// list, their partials meet in LDS and are added in group order
template <int H>
__global__ __launch_bounds__(kThreads) void k_digcn_gather_heavy(int K, const int32_t* nodes, const float* y, const int32_t* ptr, const int32_t* idx,
                                                                 const float* outer, const float* inner, const float* mask, int self_loops,
                                                                 int relu, float* out) {
    constexpr int LPR = H / 4, GROUPS = kThreads / LPR;
    __shared__ __attribute__((aligned(16))) float s_part[GROUPS * H];
    const int lr = threadIdx.x % LPR, g = threadIdx.x / LPR;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const int64_t node = nodes[k];
        const int e0 = ptr[node], e1 = ptr[node + 1];
        float4 acc = zero4();
        for (int e = e0 + g; e < e1; e += GROUPS) acc = add4(acc, digcn_term<H>(y, inner, mask, idx[e], lr));
        st4(s_part + g * H + 4 * lr, acc);
        __syncthreads();
        if (g == 0) {
            float4 s = self_loops ? digcn_term<H>(y, inner, mask, node, lr) : zero4();
            for (int p = 0; p < GROUPS; ++p) s = add4(s, ld4(s_part + p * H + 4 * lr));
            s = scale4(outer[node], s);
            st4(out + node * H + 4 * lr, relu ? relu4(s) : s);
        }
        __syncthreads();
    }
}

// w[k] = sum of inner[j] over the entries j of the node's list (and the node itself with self loops) whose class is k: the lanes of
// the node's group split the list (one byte and one float per entry) and all-reduce the eight sums
template <int LPR>
__device__ __forceinline__ void class_hist(int64_t node, int e0, int e1, const int32_t* idx, const uint8_t* xcls, const float* inner, int self_loops,
                                           int lr, float (&w)[kDigcnClasses]) {
#pragma unroll
    for (int k = 0; k < kDigcnClasses; ++k) w[k] = 0.f;
    for (int e = e0 + lr; e < e1; e += LPR) {
        const int j = idx[e];
        const int cls = xcls[j];
        const float cj = inner[j];
#pragma unroll
        for (int k = 0; k < kDigcnClasses; ++k) w[k] += cls == k ? cj : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kDigcnClasses; ++k) w[k] = group_sum<LPR>(w[k]);
    if (self_loops) {
        const int cls = xcls[node];
        const float cj = inner[node];
#pragma unroll
        for (int k = 0; k < kDigcnClasses; ++k) w[k] += cls == k ? cj : 0.f;
    }
}

// first layer on class rows: out[i] = act(outer[i] * sum_k w_i[k] T[k])
template <int H>
__global__ __launch_bounds__(kThreads) void k_digcn_class_fwd(int64_t N, const uint8_t* xcls, const float* T, int C, const int32_t* ptr,
                                                              const int32_t* idx, const float* outer, const float* inner, int self_loops, int relu,
                                                              float* out) {
    constexpr int LPR = H / 4;
    __shared__ __attribute__((aligned(16))) float s_T[kDigcnClasses * H];
    for (int i = threadIdx.x; i < kDigcnClasses * H; i += kThreads) s_T[i] = i < C * H ? T[i] : 0.f;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kThreads / LPR;
    const int lr = threadIdx.x % LPR;
    // (the lanes of a group share `node`, so a group enters and leaves this loop together: the all-reduce inside class_hist sees whole groups)
    for (int64_t node = ((int64_t)blockIdx.x * kThreads + threadIdx.x) / LPR; node < N; node += stride) {
        float w[kDigcnClasses];
        class_hist<LPR>(node, ptr[node], ptr[node + 1], idx, xcls, inner, self_loops, lr, w);
        float4 acc = zero4();
#pragma unroll
        for (int k = 0; k < kDigcnClasses; ++k) acc = fma4(w[k], ld4(s_T + k * H + 4 * lr), acc);
        acc = scale4(outer[node], acc);
        st4(out + node * H + 4 * lr, relu ? relu4(acc) : acc);
    }
}

// its backward: dT[k] = sum_i w_i[k] * outer[i] * [z_i > 0] dz_i — the same lists as the forward, no pull over the opposite CSR.
// Per-lane class sums in registers, lane groups combined through LDS in group order, one slab row per workgroup.
template <int H>
__global__ __launch_bounds__(kThreads) void k_digcn_class_bwd(int64_t N, const uint8_t* xcls, const int32_t* ptr, const int32_t* idx,
                                                              const float* outer, const float* inner, int self_loops, const float* z,
                                                              const float* dz, float* slab) {
    constexpr int LPR = H / 4, GROUPS = kThreads / LPR, W = kDigcnClasses * H;
    __shared__ __attribute__((aligned(16))) float s_red[GROUPS * W];          // 32 KiB at every H
    float4 racc[kDigcnClasses];
#pragma unroll
    for (int k = 0; k < kDigcnClasses; ++k) racc[k] = zero4();
    const int64_t stride = (int64_t)gridDim.x * kThreads / LPR;
    const int lr = threadIdx.x % LPR, g = threadIdx.x / LPR;
    for (int64_t node = ((int64_t)blockIdx.x * kThreads + threadIdx.x) / LPR; node < N; node += stride) {
        float w[kDigcnClasses];
        class_hist<LPR>(node, ptr[node], ptr[node + 1], idx, xcls, inner, self_loops, lr, w);
        float4 d = scale4(outer[node], ld4(dz + node * H + 4 * lr));
        if (z) {
            const float4 m = ld4(z + node * H + 4 * lr);
            d.x = m.x > 0.f ? d.x : 0.f; d.y = m.y > 0.f ? d.y : 0.f; d.z = m.z > 0.f ? d.z : 0.f; d.w = m.w > 0.f ? d.w : 0.f;
        }
#pragma unroll
        for (int k = 0; k < kDigcnClasses; ++k) racc[k] = fma4(w[k], d, racc[k]);
    }
#pragma unroll
    for (int k = 0; k < kDigcnClasses; ++k) st4(s_red + g * W + k * H + 4 * lr, racc[k]);
    __syncthreads();
    for (int i = threadIdx.x; i < W; i += kThreads) {
        float s = 0.f;
        for (int p = 0; p < GROUPS; ++p) s += s_red[p * W + i];
        slab[(int64_t)blockIdx.x * W + i] = s;
    }
}

inline int digcn_grid(int64_t N, int H, int per_cu) {
    const int64_t rows_per_block = kThreads / (H / 4);
    return grid_for((N + rows_per_block - 1) / rows_per_block, per_cu);
}

}  // namespace mgv

extern "C" int mgv_digcn_scales(int64_t N, const int32_t* list_ptr, const int32_t* opp_ptr, float alpha, float beta, int self_loops,
                                float* r, float* c, void* stream) {
    MGV_CHECK_ARG(N >= 0 && list_ptr && opp_ptr && r && c && alpha >= 0.f && beta >= 0.f);
    if (N == 0) return MGV_OK;
    hipLaunchKernelGGL(mgv::k_digcn_scales, dim3(mgv::grid_for((N + mgv::kThreads - 1) / mgv::kThreads, 8)), dim3(mgv::kThreads), 0,
                       static_cast<hipStream_t>(stream), N, list_ptr, opp_ptr, alpha, beta, self_loops ? 1 : 0, r, c);
    MGV_LAUNCH_RET();
}

extern "C" int mgv_digcn_gather(int H, int64_t N, const float* y, const int32_t* nbr_ptr, const int32_t* nbr_idx, const float* outer,
                                const float* inner, const float* mask, int self_loops, int relu, int heavy_n, const int32_t* heavy_nodes,
                                float* out, void* stream) {
    MGV_CHECK_ARG(N >= 0 && y && nbr_ptr && outer && inner && out && out != y && heavy_n >= 0 && (heavy_n == 0 || heavy_nodes));
    return mgv::dispatch_width(mgv::AllWidths{}, H, [&](auto w) {
        constexpr int HH = w;
        if (N == 0) return MGV_OK;
        MGV_CHECK_ARG(nbr_idx != nullptr);
        hipStream_t st = static_cast<hipStream_t>(stream);
        const int sl = self_loops ? 1 : 0, rl = relu ? 1 : 0;
        hipLaunchKernelGGL(mgv::k_digcn_gather<HH>, dim3(mgv::digcn_grid(N, HH, 16)), dim3(mgv::kThreads), 0, st, N, y, nbr_ptr, nbr_idx, outer, inner,
                           mask, sl, rl, heavy_n > 0 ? 1 : 0, out);
        if (heavy_n > 0) hipLaunchKernelGGL(mgv::k_digcn_gather_heavy<HH>, dim3(mgv::heavy_seg_grid(heavy_n)), dim3(mgv::kThreads), 0, st, heavy_n,
                                            heavy_nodes, y, nbr_ptr, nbr_idx, outer, inner, mask, sl, rl, out);
        MGV_LAUNCH_RET();
    });
}

extern "C" int mgv_digcn_class_fwd(int H, int64_t N, const uint8_t* xcls, const float* T, int C, const int32_t* nbr_ptr, const int32_t* nbr_idx,
                                   const float* outer, const float* inner, int self_loops, int relu, float* out, void* stream) {
    MGV_CHECK_ARG(N >= 0 && xcls && T && nbr_ptr && outer && inner && out && C >= 1 && C <= mgv::kDigcnClasses);
    return mgv::dispatch_width(mgv::AllWidths{}, H, [&](auto w) {
        constexpr int HH = w;
        if (N == 0) return MGV_OK;
        MGV_CHECK_ARG(nbr_idx != nullptr);
        hipLaunchKernelGGL(mgv::k_digcn_class_fwd<HH>, dim3(mgv::digcn_grid(N, HH, 16)), dim3(mgv::kThreads), 0, static_cast<hipStream_t>(stream),
                           N, xcls, T, C, nbr_ptr, nbr_idx, outer, inner, self_loops ? 1 : 0, relu ? 1 : 0, out);
        MGV_LAUNCH_RET();
    });
}

extern "C" int mgv_digcn_class_bwd_ws_floats(int H, int64_t N) {
    if (N <= 0 || !mgv::has_width(mgv::AllWidths{}, H)) return 0;
    return mgv::digcn_grid(N, H, 4) * mgv::kDigcnClasses * H;
}

extern "C" int mgv_digcn_class_bwd(int H, int64_t N, const uint8_t* xcls, int C, const int32_t* nbr_ptr, const int32_t* nbr_idx, const float* outer,
                                   const float* inner, int self_loops, const float* z, const float* dz, float* dT, float* workspace,
                                   int64_t workspace_floats, void* stream) {
    MGV_CHECK_ARG(N >= 0 && xcls && nbr_ptr && outer && inner && dz && dT && C >= 1 && C <= mgv::kDigcnClasses);
    return mgv::dispatch_width(mgv::AllWidths{}, H, [&](auto w) {
        constexpr int HH = w;
        if (N == 0) return MGV_OK;
        MGV_CHECK_ARG(nbr_idx && workspace && workspace_floats >= mgv_digcn_class_bwd_ws_floats(HH, N));
        hipStream_t st = static_cast<hipStream_t>(stream);
        const int grid = mgv::digcn_grid(N, HH, 4);
        hipLaunchKernelGGL(mgv::k_digcn_class_bwd<HH>, dim3(grid), dim3(mgv::kThreads), 0, st, N, xcls, nbr_ptr, nbr_idx, outer, inner,
                           self_loops ? 1 : 0, z, dz, workspace);
        // only the C rows the caller's table has are added (class ids >= C never occur: GraphPlan.xcls indexes the table's rows)
        mgv::launch_slab_sum<float, float>(workspace, grid, mgv::kDigcnClasses * HH, C * HH, dT, st);
        MGV_LAUNCH_RET();
    });
}
