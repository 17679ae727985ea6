// Training-mode readout MLP 64 -> 32 -> 32 -> 1 (arch/mlp.py MLP.forward, dg_ae_model_aig.py:102-106:
// Linear, BatchNorm1d + ReLU + Dropout, Linear, BatchNorm1d + ReLU + Dropout, Linear, clamp) as a few grid-stride passes
// that end only where BatchNorm needs a batch-wide sum.  Only hf [N,64], the pre-BN outputs y1, y2 [N,32], prob / dprob [N]
// and dhf [N,64] touch HBM; activations, dropout masks, the head and the BN gradients are recomputed in registers.
//   forward:  F1  hf -> y1 (+ column sums)      finalize 1 (mean, invstd, running buffers)
//             F2  y1 -> a1 -> y2 (+ sums)       finalize 2
//             F3  y2 -> a2 -> prob
//   backward: B1  y2, dprob -> head gradients, BN2 sums
//             B2  y1, y2, dprob -> BN1 sums                   (dy2 recomputed; dA1 = dy2 W2)
//             B3w y1, y2, dprob -> dW2, db2                   (on the <32, 32> weight-gradient grid)
//             B3  hf, y1, y2, dprob -> dW1, db1, dhf = dy1 W1
// The products are the bf16x3 ones of linear_x3.hip on the same fragment layout (F1 / F2 give y1 / y2 bit for bit as the
// per-layer kernels do); every cross-workgroup sum goes through a per-workgroup slab row added in a fixed order (mgv_slab.h).
#include "mgv_x3.h"
#include "mgv_slab.h"
#include "mgv_dropout.h"
#include "../../include/mgvae_hip.h"

namespace mgv {
namespace ro {

constexpr int D = 64;                                  // dim_in
constexpr int C = 32;                                  // dim_hidden
constexpr int LDD = D + 8, LDC = C + 8;                // bf16 plane rows (mgv_x3.h Plane)
constexpr int PD = kTileRows * LDD, PC = kTileRows * LDC;
constexpr int LSC = C + 4, LSD = D + 4;                // fp32 staging rows
// weight pack (bf16 elements): [W1 hi, lo][W2 hi, lo][W2^T hi, lo][W1^T hi, lo], each in fragment order (k_wpack_bf16x3)
constexpr int o_w1 = 0, o_w2 = 2 * C * D, o_w2t = o_w2 + 2 * C * C, o_w1t = o_w2t + 2 * C * C, pack_elems = o_w1t + 2 * C * D;
// gradient buffer (floats): [dW1 C*D][db1][dgamma1][dbeta1][dW2 C*C][db2][dgamma2][dbeta2][dw3 C][db3]
constexpr int g_w1 = 0, g_b1 = C * D, g_g1 = g_b1 + C, g_be1 = g_g1 + C, g_w2 = g_be1 + C, g_b2 = g_w2 + C * C, g_g2 = g_b2 + C,
              g_be2 = g_g2 + C, g_w3 = g_be2 + C, g_b3 = g_w3 + C, grad_floats = g_b3 + 1;
// slab rows (doubles) of the passes
constexpr int s_f = 2 * C;                             // F1, F2: sum y, sum y^2
constexpr int s_b1 = 3 * C + 1;                        // B1: dw3, db3, sum dz2, sum dz2 xhat2
constexpr int s_b2 = 2 * C;                            // B2: sum dz1, sum dz1 xhat1
// B3 / B3w: fp32 rows as k_linear_wgrad_x3 leaves them: dW1 + db1 per workgroup of B3, dW2 + db2 per workgroup of B3w
constexpr int s_b3 = C * D + C, s_b3w2 = C * C + C;

// Y[64][M] (+)= X[64][K] W^T + b from bf16 hi/lo planes, exactly as k_linear_fwd_x3 forms it (same wave split, same MFMA order)
template <int M, int K>
struct MmFwd {
    using S = WaveSplit<M>;
    static constexpr int KS = K / 32;
    bf16x8 wh[S::HCW][KS], wl[S::HCW][KS];
    float bias[S::HCW];
    __device__ __forceinline__ void load(const __bf16* wp, const float* bp) {
        const int lane = threadIdx.x & 63, wc = (threadIdx.x >> 6) % S::WPC;
#pragma unroll
        for (int j = 0; j < S::HCW; ++j) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int wo = (((wc * S::HCW + j) * KS) + ks) * 512 + lane * 8;
                wh[j][ks] = ldfrag(wp + wo); wl[j][ks] = ldfrag(wp + M * K + wo);
            }
            bias[j] = bp ? bp[(wc * S::HCW + j) * 16 + (lane & 15)] : 0.f;
        }
    }
    __device__ __forceinline__ void run(const __bf16* x_hi, const __bf16* x_lo, int ldp, float* s_y, int ldy) const {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
        const int wc = w % S::WPC, wr = w / S::WPC;
        f32x4 acc[S::RTW][S::HCW];
#pragma unroll
        for (int i = 0; i < S::RTW; ++i)
#pragma unroll
            for (int j = 0; j < S::HCW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int i = 0; i < S::RTW; ++i) {
                const int off = ((wr * S::RTW + i) * 16 + r) * ldp + 32 * ks + 8 * q;
                const bf16x8 xh = ldfrag(x_hi + off), xl = ldfrag(x_lo + off);
#pragma unroll
                for (int j = 0; j < S::HCW; ++j) mma_x3(acc[i][j], xh, xl, wh[j][ks], wl[j][ks]);
            }
#pragma unroll
        for (int i = 0; i < S::RTW; ++i)
#pragma unroll
            for (int j = 0; j < S::HCW; ++j) {
                const int col = (wc * S::HCW + j) * 16 + r;
#pragma unroll
                for (int e = 0; e < 4; ++e) s_y[((wr * S::RTW + i) * 16 + q * 4 + e) * ldy + col] = acc[i][j][e] + bias[j];
            }
    }
};

// dW[M][K] += G^T X over one 64-row tile, both operands read transposed from their row-major planes (k_linear_wgrad_x3 with
// 4 waves in a 2 x 2 grid over the output tiles); the partial stays in registers for the whole launch
template <int M, int K>
struct MmWgrad {
    static constexpr int ITW = M / 32, JTW = K / 32;
    f32x4 acc[ITW][JTW];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < ITW; ++i)
#pragma unroll
            for (int j = 0; j < JTW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __device__ __forceinline__ void run(const __bf16* g_hi, const __bf16* g_lo, int ldg, const __bf16* x_hi, const __bf16* x_lo, int ldx) {
        const int w = threadIdx.x >> 6, it0 = (w >> 1) * ITW, jt0 = (w & 1) * JTW;
#pragma unroll
        for (int ks = 0; ks < kTileRows / 32; ++ks) {
            bf16x8 bh[JTW], bl[JTW];
#pragma unroll
            for (int j = 0; j < JTW; ++j) {
                bh[j] = ldfrag_tr2(x_hi, ldx, 32 * ks, (jt0 + j) * 16);
                bl[j] = ldfrag_tr2(x_lo, ldx, 32 * ks, (jt0 + j) * 16);
            }
#pragma unroll
            for (int i = 0; i < ITW; ++i) {
                const bf16x8 ah = ldfrag_tr2(g_hi, ldg, 32 * ks, (it0 + i) * 16), al = ldfrag_tr2(g_lo, ldg, 32 * ks, (it0 + i) * 16);
#pragma unroll
                for (int j = 0; j < JTW; ++j) mma_x3(acc[i][j], ah, al, bh[j], bl[j]);
            }
        }
    }
    template <typename T>
    __device__ __forceinline__ void store(T* row) const {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4, it0 = (w >> 1) * ITW, jt0 = (w & 1) * JTW;
#pragma unroll
        for (int i = 0; i < ITW; ++i)
#pragma unroll
            for (int j = 0; j < JTW; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) row[((it0 + i) * 16 + q * 4 + e) * K + (jt0 + j) * 16 + r] = (T)acc[i][j][e];
    }
};

// per-column constants of one BatchNorm + ReLU + Dropout block for a thread's column quad c4..c4+3
struct BnQuad {
    float m[4], is[4], g[4], b[4];
    __device__ __forceinline__ void load(const float* stats, const float* gamma, const float* beta, int c4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { m[k] = stats[c4 + k]; is[k] = stats[C + c4 + k]; g[k] = gamma[c4 + k]; b[k] = beta[c4 + k]; }
    }
    // pre-ReLU value gamma * xhat + beta, as k_bn_act_fwd / k_bn_act_bwd form it
    __device__ __forceinline__ float pre(float y, int k, float& xhat) const {
        xhat = (y - m[k]) * is[k];
        return xhat * g[k] + b[k];
    }
};

// dY = gamma * invstd * (dZ - S1/N - xhat * S2/N): the per-column factors of k_bn_bwd_apply (batch statistics)
struct BnBwdQuad {
    float sc[4], a1[4], a2[4];
    __device__ __forceinline__ void load(const BnQuad& q, const double* sums, int64_t N, int c4) {
        const double invn = 1.0 / (double)N;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sc[k] = q.g[k] * q.is[k];
            a1[k] = (float)(sums[c4 + k] * invn);
            a2[k] = (float)(sums[C + c4 + k] * invn) * q.is[k];
        }
    }
    __device__ __forceinline__ float apply(float dz, float y, int k, const BnQuad& q) const { return sc[k] * (dz - a1[k] - (y - q.m[k]) * a2[k]); }
};

__device__ __forceinline__ void to4(const float4& v, float (&o)[4]) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }

// column sums of a workgroup: thread t holds columns 4 (t % 8) .. +3; the 32 threads of a column quad are added in thread order
__device__ __forceinline__ void quad_colsum(const double (&v)[4], double* red, double* out) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        __syncthreads();
        red[threadIdx.x] = v[k];
        __syncthreads();
        if (threadIdx.x < C / 4) {
            double a = 0;
            for (int rr = 0; rr < kThreads / (C / 4); ++rr) a += red[rr * (C / 4) + threadIdx.x];
            out[threadIdx.x * 4 + k] = a;
        }
    }
}

// a row quad's share of the head: dot4 as k_head compiles it (four products, added in order, no contraction)
__device__ __forceinline__ float head_dot(const float (&a)[4], const float (&w)[4]) {
#pragma clang fp contract(off)
    return a[0] * w[0] + a[1] * w[1] + a[2] * w[2] + a[3] * w[3];
}

// The backward's recomputation of one row quad: a2 = drop(relu(bn2(y2))), the head's clamp decision and dY2 (zero for rows >= N).
// The 8 lanes of a row are consecutive lanes, so the head's row sum is the same DPP tree k_head forms.
struct Dy2 {
    float dy2[4], dy;
};
__device__ __forceinline__ Dy2 recompute_dy2(const float (&y)[4], float dp, bool ok, int64_t i, int c4, const BnQuad& q2, const BnBwdQuad& bq2,
                                             const float (&w3)[4], float b3, int clamp01, float p, float ks, uint64_t seed) {
    Dy2 o;
    float xh[4], bn[4], ds[4], a2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        bn[k] = q2.pre(y[k], k, xh[k]);
        ds[k] = drop_scale(seed, i * C + c4 + k, p, ks);
        a2[k] = fmaxf(bn[k], 0.f) * ds[k];
    }
    float h = head_dot(a2, w3);
    h = group_sum<C / 4>(h);
    h += b3;
    o.dy = (ok && (!clamp01 || (h >= 0.f && h <= 1.f))) ? dp : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float dz = bn[k] > 0.f ? (o.dy * w3[k]) * ds[k] : 0.f;
        o.dy2[k] = ok ? bq2.apply(dz, y[k], k, q2) : 0.f;
    }
    return o;
}

// split4 of values formed in registers: the per-layer kernels split values they loaded from memory, so a product that formed
// one of them must not be contracted into the split's subtraction (it would round the lo half differently)
__device__ __forceinline__ void split_store(__bf16* hi_plane, __bf16* lo_plane, int off, const float (&v)[4]) {
#pragma clang fp contract(off)
    __bf16 h[4], l[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        h[k] = (__bf16)v[k];
        l[k] = (__bf16)(v[k] - (float)h[k]);
    }
    st_bf4(hi_plane + off, bf16x4{h[0], h[1], h[2], h[3]}); st_bf4(lo_plane + off, bf16x4{l[0], l[1], l[2], l[3]});
}

// ------------------------------------------------------------------------------------------------ forward
// F1 (FIRST) y1 = hf W1^T + b1 / F2 y2 = drop(relu(bn1(y1))) W2^T + b2; both leave the column sums of their output in the slab
template <bool FIRST>
__global__ __launch_bounds__(kThreads) void k_ro_fwd_lin(int64_t N, const float* X, const __bf16* wp, const float* bias, const float* stats,
                                                         const float* gamma, const float* beta, float p, uint64_t seed, float* Y, double* slab) {
    constexpr int K = FIRST ? D : C, LDP = K + 8, QPT = kTileRows * K / 4 / kThreads;
    __shared__ __attribute__((aligned(16))) __bf16 x_hi[kTileRows * LDP], x_lo[kTileRows * LDP];
    __shared__ __attribute__((aligned(16))) float s_y[kTileRows * LSC];
    __shared__ double red[kThreads];
    const int tid = threadIdx.x;
    MmFwd<C, K> mm;
    mm.load(wp, bias);
    BnQuad q;
    const float ks = p > 0.f ? 1.0f / (1.0f - p) : 1.0f;
    if (!FIRST) q.load(stats, gamma, beta, (tid % (C / 4)) * 4);
    double s[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    const int64_t ntiles = (N + kTileRows - 1) / kTileRows;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r0 = tile * kTileRows;
        float4 xv[QPT];
#pragma unroll
        for (int u = 0; u < QPT; ++u) {
            const int f = tid + u * kThreads, row = f / (K / 4), c4 = (f % (K / 4)) * 4;
            xv[u] = r0 + row < N ? ld4(X + (r0 + row) * K + c4) : zero4();
        }
#pragma unroll
        for (int u = 0; u < QPT; ++u) {
            const int f = tid + u * kThreads, row = f / (K / 4), c4 = (f % (K / 4)) * 4;
            float v[4];
            to4(xv[u], v);
            if (!FIRST) {
                const int64_t i = r0 + row;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float xh;
                    v[k] = fmaxf(q.pre(v[k], k, xh), 0.f) * drop_scale(seed, i * C + c4 + k, p, ks);
                }
            }
            split_store(x_hi, x_lo, row * LDP + c4, v);
        }
        lds_barrier();
        mm.run(x_hi, x_lo, LDP, s_y, LSC);
        lds_barrier();
#pragma unroll
        for (int u = 0; u < kTileRows * C / 4 / kThreads; ++u) {
            const int f = tid + u * kThreads, row = f / (C / 4), c4 = (f % (C / 4)) * 4;
            if (r0 + row < N) {
                const float4 v = ld4(s_y + row * LSC + c4);
                st4(Y + (r0 + row) * C + c4, v);
                s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
                s2[0] += (double)v.x * v.x; s2[1] += (double)v.y * v.y; s2[2] += (double)v.z * v.z; s2[3] += (double)v.w * v.w;
            }
        }
        // the planes are rewritten only after this tile's second barrier; s_y only after the next tile's first
    }
    double* row = slab + (int64_t)blockIdx.x * s_f;
    quad_colsum(s, red, row);
    quad_colsum(s2, red, row + C);
}

// mean / invstd of a block and the running-buffer update of nn.BatchNorm1d, with the operations and roundings of BnReluDropFn:
// double statistics, var = E[y^2] - mean^2 clamped at 0, running = running * (1 - momentum) + momentum * value in fp32 steps
__global__ void k_ro_bn_finalize(int64_t N, const double* sums, float momentum, float keep, float eps, float* running_mean,
                                 float* running_var, float* stats) {
#pragma clang fp contract(off)
    const int c = threadIdx.x;
    if (c >= C) return;
    const double dn = (double)N, inv = 1.0 / dn;          // torch divides a tensor by a scalar as a product with its reciprocal
    const double mean64 = __dmul_rn(sums[c], inv);
    double var64 = __dsub_rn(__dmul_rn(sums[C + c], inv), __dmul_rn(mean64, mean64));
    var64 = var64 < 0.0 ? 0.0 : var64;
    const float mean = (float)mean64, var = (float)var64;
    const float var_unbiased = (float)__dmul_rn(var64, dn / (double)(N > 1 ? N - 1 : 1));
    running_mean[c] = __fadd_rn(__fmul_rn(running_mean[c], keep), __fmul_rn(momentum, mean));
    running_var[c] = __fadd_rn(__fmul_rn(running_var[c], keep), __fmul_rn(momentum, var_unbiased));
    stats[c] = mean;
    stats[C + c] = (float)(1.0 / sqrt((double)__fadd_rn(var, eps)));      // torch.rsqrt's correctly rounded value
}

// F3: prob = clamp(drop(relu(bn2(y2))) w3 + b3); C/4 lanes per row, the row sum as k_head<false> forms it
__global__ __launch_bounds__(kThreads) void k_ro_head_fwd(int64_t N, const float* Y2, const float* stats, const float* gamma, const float* beta,
                                                          float p, uint64_t seed, const float* w3, const float* b3, int clamp01, float* prob) {
    constexpr int rows = kThreads / (C / 4);
    const int c4 = (threadIdx.x % (C / 4)) * 4, r0 = threadIdx.x / (C / 4);
    BnQuad q;
    q.load(stats, gamma, beta, c4);
    const float ks = p > 0.f ? 1.0f / (1.0f - p) : 1.0f;
    const float w[4] = {w3[c4], w3[c4 + 1], w3[c4 + 2], w3[c4 + 3]}, bias = b3[0];
    const int64_t nblk = (N + rows - 1) / rows;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t i = blk * rows + r0;
        const bool ok = i < N;
        float y[4] = {0.f, 0.f, 0.f, 0.f};
        if (ok) to4(ld4(Y2 + i * C + c4), y);
        float a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float xh;
            a[k] = fmaxf(q.pre(y[k], k, xh), 0.f) * drop_scale(seed, i * C + c4 + k, p, ks);
        }
        float h = head_dot(a, w);
        h = group_sum<C / 4>(h);
        h += bias;
        if (ok && c4 == 0) prob[i] = clamp01 ? fminf(fmaxf(h, 0.f), 1.f) : h;
    }
}

// ------------------------------------------------------------------------------------------------ backward
// The two Linear biases in front of a BatchNorm get db = colsum(dy) = 0 up to rounding: their gradients are pure rounding noise,
// which Adam (eps 1e-8) turns into steps of lr size.  So that a step computes what the per-layer path computes, the quantities that
// noise is made of are formed bit for bit as the per-layer kernels form them: the BatchNorm sums in k_bn_act_bwd's rows, grid and
// float grouping (B1, B2), dy in k_bn_bwd_apply's expression, and colsum(dy) in k_linear_wgrad_x3's threads, grid and order (B3).
// The products are per row (an MFMA output row depends on that row only), so any row grouping gives the same dA1 and dhf.

// a += v without contracting the product that formed v into the add (the per-layer kernels add values loaded from memory)
__device__ __forceinline__ void add_nc(float (&a)[4], const float (&v)[4]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = a[k] + v[k];
}

// k_bn_act_bwd's walk over the rows of [N, C]: C/4 lanes per row, 32 rows per block, U = 4 rows (one per stride) in flight whose
// sums meet in fp32 before they join the double totals
constexpr int kRowsPB = kThreads / (C / 4), kU = 4;

// B1: head gradients (dw3, db3) and the BN2 sums (sum dz2, sum dz2 xhat2); nothing [N, *] is written
__global__ __launch_bounds__(kThreads) void k_ro_b1(int64_t N, const float* Y2, const float* stats, const float* gamma, const float* beta,
                                                    float p, uint64_t seed, const float* w3, const float* b3, int clamp01, const float* dprob,
                                                    double* slab) {
    __shared__ double red[kThreads];
    const int c4 = (threadIdx.x % (C / 4)) * 4, r0 = threadIdx.x / (C / 4);
    BnQuad q;
    q.load(stats, gamma, beta, c4);
    const float ks = p > 0.f ? 1.0f / (1.0f - p) : 1.0f;
    const float w[4] = {w3[c4], w3[c4 + 1], w3[c4 + 2], w3[c4 + 3]}, bias = b3[0];
    float dw[4] = {0.f, 0.f, 0.f, 0.f}, db = 0.f;
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    const int64_t stride = (int64_t)gridDim.x * kRowsPB;
    for (int64_t base = (int64_t)blockIdx.x * kRowsPB; base < N; base += kU * stride) {
        float fs[4] = {0.f, 0.f, 0.f, 0.f}, fs2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t i = base + u * stride + r0;
            const bool ok = i < N;                  // uniform over the C/4 lanes of a row (the head's DPP sum stays inside them)
            float y[4] = {0.f, 0.f, 0.f, 0.f};
            float dp = 0.f;
            if (ok) { to4(ld4(Y2 + i * C + c4), y); dp = dprob[i]; }
            float a[4], xh[4], bn[4], ds[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bn[k] = q.pre(y[k], k, xh[k]);
                ds[k] = drop_scale(seed, i * C + c4 + k, p, ks);
                a[k] = fmaxf(bn[k], 0.f) * ds[k];
            }
            float h = head_dot(a, w);
            h = group_sum<C / 4>(h);
            h += bias;
            const float dy = (ok && (!clamp01 || (h >= 0.f && h <= 1.f))) ? dp : 0.f;
            if (ok) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float dd = dy * w[k];                         // k_head<true>'s dA
                    const float dz = bn[k] > 0.f ? dd * ds[k] : 0.f;
                    fs[k] += dz; fs2[k] += dz * xh[k];
                    dw[k] = fmaf(dy, a[k], dw[k]);
                }
                if (c4 == 0) db += dy;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { s1[k] += fs[k]; s2[k] += fs2[k]; }
    }
    double* row = slab + (int64_t)blockIdx.x * s_b1;
    {   // dw3, db3 as k_head<true> reduces them: shuffles inside a wave, then the waves in order, in fp32
        float* s_stage = reinterpret_cast<float*>(red);          // [4 waves][C + 1]
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        for (int mk = C / 4; mk < 64; mk <<= 1)
#pragma unroll
            for (int k = 0; k < 4; ++k) dw[k] += __shfl_xor(dw[k], mk, 64);
        db = wave_sum(db);
        if (lane < C / 4)
#pragma unroll
            for (int k = 0; k < 4; ++k) s_stage[wv * (C + 1) + 4 * lane + k] = dw[k];
        if (lane == 0) s_stage[wv * (C + 1) + C] = db;
        __syncthreads();
        if (threadIdx.x <= C) {
            float v = 0.f;
#pragma unroll
            for (int ww = 0; ww < kThreads / 64; ++ww) v += s_stage[ww * (C + 1) + threadIdx.x];
            row[threadIdx.x] = (double)v;
        }
    }
    quad_colsum(s1, red, row + C + 1);
    quad_colsum(s2, red, row + 2 * C + 1);
}

// B2: the BN1 sums of dz1 = drop1 * relu1'(.) * (dy2 W2), over B1's walk: per block iteration the U groups of 32 rows are 128
// plane rows, multiplied as two 64-row tiles
__global__ __launch_bounds__(kThreads) void k_ro_b2(int64_t N, const float* Y1, const float* Y2, const float* dprob, const float* stats,
                                                    const float* g1, const float* be1, const float* g2, const float* be2, float p1, float p2,
                                                    uint64_t seed1, uint64_t seed2, const float* w3, const float* b3, int clamp01,
                                                    const double* sums2, const __bf16* w2t, double* slab) {
    constexpr int R = kU * kRowsPB;                                   // 128 plane rows
    __shared__ __attribute__((aligned(16))) __bf16 g_hi[R * LDC], g_lo[R * LDC];
    __shared__ __attribute__((aligned(16))) float s_d[R * LSC];
    __shared__ double red[kThreads];
    const int tid = threadIdx.x, c4 = (tid % (C / 4)) * 4, r0 = tid / (C / 4);
    BnQuad q1, q2;
    q1.load(stats, g1, be1, c4);
    q2.load(stats + 2 * C, g2, be2, c4);
    BnBwdQuad bq2;
    bq2.load(q2, sums2, N, c4);
    const float ks1 = p1 > 0.f ? 1.0f / (1.0f - p1) : 1.0f, ks2 = p2 > 0.f ? 1.0f / (1.0f - p2) : 1.0f;
    const float w[4] = {w3[c4], w3[c4 + 1], w3[c4 + 2], w3[c4 + 3]}, bias = b3[0];
    MmFwd<C, C> mm;
    mm.load(w2t, nullptr);
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    const int64_t stride = (int64_t)gridDim.x * kRowsPB;
    for (int64_t base = (int64_t)blockIdx.x * kRowsPB; base < N; base += kU * stride) {
        float y1[kU][4];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t i = base + u * stride + r0;
            const bool ok = i < N;
            float y2[4];
            to4(ok ? ld4(Y1 + i * C + c4) : zero4(), y1[u]);
            to4(ok ? ld4(Y2 + i * C + c4) : zero4(), y2);
            const float dp = ok ? dprob[i] : 0.f;
            const int prow = u * kRowsPB + r0;
            const Dy2 d = recompute_dy2(y2, dp, ok, i, c4, q2, bq2, w, bias, clamp01, p2, ks2, seed2);
            split_store(g_hi, g_lo, prow * LDC + c4, d.dy2);
        }
        lds_barrier();
#pragma unroll
        for (int h = 0; h < R / kTileRows; ++h) {
            const int o = h * kTileRows * LDC;
            mm.run(g_hi + o, g_lo + o, LDC, s_d + h * kTileRows * LSC, LSC);        // dA1 = dy2 W2
        }
        lds_barrier();
        float fs[4] = {0.f, 0.f, 0.f, 0.f}, fs2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t i = base + u * stride + r0;
            if (i < N) {
                float da[4];
                to4(ld4(s_d + (u * kRowsPB + r0) * LSC + c4), da);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float xh;
                    const float bn = q1.pre(y1[u][k], k, xh);
                    const float dz = bn > 0.f ? da[k] * drop_scale(seed1, i * C + c4 + k, p1, ks1) : 0.f;
                    fs[k] += dz; fs2[k] += dz * xh;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { s1[k] += fs[k]; s2[k] += fs2[k]; }
        // the planes are rewritten only after the second barrier; s_d only after the next iteration's first
    }
    double* row = slab + (int64_t)blockIdx.x * s_b2;
    quad_colsum(s1, red, row);
    quad_colsum(s2, red, row + C);
}

// column sums of one workgroup of k_linear_wgrad_x3: thread t's float4 partial in s_part[t], the threads t = c4/4 (mod C/4) added in
// thread order in fp32
__device__ __forceinline__ void wgrad_colsum(const float4* s_part, int nthreads, float* out) {
    if (threadIdx.x < C) {
        const int q4 = threadIdx.x / 4, e = threadIdx.x % 4;
        float sum = 0.f;
        for (int t = q4; t < nthreads; t += C / 4) { const float4 v = s_part[t]; sum += e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
        out[threadIdx.x] = sum;
    }
}

// B3: dy1 = bn1'(dz1), dhf = dy1 W1, and dW1, db1 as the per-layer weight-gradient launch forms them: k_linear_wgrad_x3<32, 64>
// (this grid, min(tiles, 512); db1 from 512 threads, one row each per tile).  The MFMA partial of an output tile is the same chain
// of mma_x3 over the same tiles whichever wave holds it, and the workgroup rows are added in fp32 by the same k_slab_sum.
__global__ __launch_bounds__(kThreads) void k_ro_b3(int64_t N, const float* HF, const float* Y1, const float* Y2, const float* dprob,
                                                    const float* stats, const float* g1, const float* be1, const float* g2, const float* be2,
                                                    float p1, float p2, uint64_t seed1, uint64_t seed2, const float* w3, const float* b3,
                                                    int clamp01, const double* sums1, const double* sums2, const __bf16* w2t, const __bf16* w1t,
                                                    float* dHF, float* slab1) {
    __shared__ __attribute__((aligned(16))) __bf16 x_hi[PD], x_lo[PD], g_hi[PC], g_lo[PC];
    __shared__ __attribute__((aligned(16))) float s_o[kTileRows * LSD];     // dA1 [64][LSC], then dhf [64][LSD]; column-sum partials at the end
    const int tid = threadIdx.x, c4 = (tid % (C / 4)) * 4;
    BnQuad q1, q2;
    q1.load(stats, g1, be1, c4);
    q2.load(stats + 2 * C, g2, be2, c4);
    BnBwdQuad bq1, bq2;
    bq1.load(q1, sums1, N, c4);
    bq2.load(q2, sums2, N, c4);
    const float ks1 = p1 > 0.f ? 1.0f / (1.0f - p1) : 1.0f, ks2 = p2 > 0.f ? 1.0f / (1.0f - p2) : 1.0f;
    const float w[4] = {w3[c4], w3[c4 + 1], w3[c4 + 2], w3[c4 + 3]}, bias = b3[0];
    MmFwd<C, C> mm2;
    mm2.load(w2t, nullptr);
    MmFwd<D, C> mm1;
    mm1.load(w1t, nullptr);
    MmWgrad<C, D> wg;
    wg.zero();
    constexpr int U = kTileRows * C / 4 / kThreads, UX = kTileRows * D / 4 / kThreads;
    float db1[U][4] = {};                                 // db1[u]: the 512-thread launch's thread tid + 256 u
    const int64_t ntiles = (N + kTileRows - 1) / kTileRows;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r0 = tile * kTileRows;
        float4 xv[UX];
        float y1[U][4], y2[U][4], dp[U];
#pragma unroll
        for (int u = 0; u < UX; ++u) {
            const int f = tid + u * kThreads, row = f / (D / 4), xc = (f % (D / 4)) * 4;
            xv[u] = r0 + row < N ? ld4(HF + (r0 + row) * D + xc) : zero4();
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = r0 + (tid + u * kThreads) / (C / 4);
            const bool ok = i < N;
            to4(ok ? ld4(Y1 + i * C + c4) : zero4(), y1[u]);
            to4(ok ? ld4(Y2 + i * C + c4) : zero4(), y2[u]);
            dp[u] = ok ? dprob[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < UX; ++u) {
            const int f = tid + u * kThreads, row = f / (D / 4), xc = (f % (D / 4)) * 4;
            float v[4];
            to4(xv[u], v);
            split_store(x_hi, x_lo, row * LDD + xc, v);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int row = (tid + u * kThreads) / (C / 4);
            const int64_t i = r0 + row;
            const Dy2 d = recompute_dy2(y2[u], dp[u], i < N, i, c4, q2, bq2, w, bias, clamp01, p2, ks2, seed2);
            split_store(g_hi, g_lo, row * LDC + c4, d.dy2);
        }
        lds_barrier();
        mm2.run(g_hi, g_lo, LDC, s_o, LSC);                     // dA1 = dy2 W2
        lds_barrier();
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int row = (tid + u * kThreads) / (C / 4);
            const int64_t i = r0 + row;
            float da[4], dy1[4];
            to4(ld4(s_o + row * LSC + c4), da);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float xh;
                const float bn = q1.pre(y1[u][k], k, xh);
                const float dz = bn > 0.f ? da[k] * drop_scale(seed1, i * C + c4 + k, p1, ks1) : 0.f;
                dy1[k] = i < N ? bq1.apply(dz, y1[u][k], k, q1) : 0.f;
            }
            add_nc(db1[u], dy1);
            split_store(g_hi, g_lo, row * LDC + c4, dy1);
        }
        lds_barrier();
        wg.run(g_hi, g_lo, LDC, x_hi, x_lo, LDD);               // dW1 += dy1^T hf
        mm1.run(g_hi, g_lo, LDC, s_o, LSD);                     // dhf = dy1 W1
        lds_barrier();
#pragma unroll
        for (int u = 0; u < UX; ++u) {
            const int f = tid + u * kThreads, row = f / (D / 4), xc = (f % (D / 4)) * 4;
            if (r0 + row < N) st4(dHF + (r0 + row) * D + xc, ld4(s_o + row * LSD + xc));
        }
        // next tile: the planes are rewritten after the barrier above, s_o after the next tile's first barrier
    }
    float* row1 = slab1 + (int64_t)blockIdx.x * s_b3;
    wg.store(row1);
    float4* s_part = reinterpret_cast<float4*>(s_o);          // 512 float4 fit in s_o (64 x 68 floats)
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u) s_part[tid + u * kThreads] = make_float4(db1[u][0], db1[u][1], db1[u][2], db1[u][3]);
    __syncthreads();
    wgrad_colsum(s_part, U * kThreads, row1 + C * D);
}

// B3w: dW2 = dy2^T a1 and db2 = colsum(dy2) as k_linear_wgrad_x3<32, 32> forms them, on its grid (min(tiles, 1024)), 256 threads, rows r
// and r + 32 of a tile per thread: a pass of its own over y1, y2 and dprob, so that B3 keeps two waves per SIMD
__global__ __launch_bounds__(kThreads) void k_ro_b3w(int64_t N, const float* Y1, const float* Y2, const float* dprob, const float* stats,
                                                     const float* g1, const float* be1, const float* g2, const float* be2, float p1, float p2,
                                                     uint64_t seed1, uint64_t seed2, const float* w3, const float* b3, int clamp01,
                                                     const double* sums2, float* slab2) {
    __shared__ __attribute__((aligned(16))) __bf16 g_hi[PC], g_lo[PC], a_hi[PC], a_lo[PC];
    __shared__ float4 s_part[kThreads];
    const int tid = threadIdx.x, c4 = (tid % (C / 4)) * 4;
    BnQuad q1, q2;
    q1.load(stats, g1, be1, c4);
    q2.load(stats + 2 * C, g2, be2, c4);
    BnBwdQuad bq2;
    bq2.load(q2, sums2, N, c4);
    const float ks1 = p1 > 0.f ? 1.0f / (1.0f - p1) : 1.0f, ks2 = p2 > 0.f ? 1.0f / (1.0f - p2) : 1.0f;
    const float w[4] = {w3[c4], w3[c4 + 1], w3[c4 + 2], w3[c4 + 3]}, bias = b3[0];
    MmWgrad<C, C> wg2;
    wg2.zero();
    constexpr int U = kTileRows * C / 4 / kThreads;
    float db2[4] = {};
    const int64_t ntiles = (N + kTileRows - 1) / kTileRows;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r0 = tile * kTileRows;
        float y1[U][4], y2[U][4], dp[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = r0 + (tid + u * kThreads) / (C / 4);
            const bool ok = i < N;
            to4(ok ? ld4(Y1 + i * C + c4) : zero4(), y1[u]);
            to4(ok ? ld4(Y2 + i * C + c4) : zero4(), y2[u]);
            dp[u] = ok ? dprob[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int row = (tid + u * kThreads) / (C / 4);
            const int64_t i = r0 + row;
            const Dy2 d = recompute_dy2(y2[u], dp[u], i < N, i, c4, q2, bq2, w, bias, clamp01, p2, ks2, seed2);
            add_nc(db2, d.dy2);
            split_store(g_hi, g_lo, row * LDC + c4, d.dy2);
            float a1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float xh;
                a1[k] = i < N ? fmaxf(q1.pre(y1[u][k], k, xh), 0.f) * drop_scale(seed1, i * C + c4 + k, p1, ks1) : 0.f;
            }
            split_store(a_hi, a_lo, row * LDC + c4, a1);
        }
        lds_barrier();
        wg2.run(g_hi, g_lo, LDC, a_hi, a_lo, LDC);             // dW2 += dy2^T a1
        lds_barrier();
    }
    float* row2 = slab2 + (int64_t)blockIdx.x * s_b3w2;
    wg2.store(row2);
    s_part[tid] = make_float4(db2[0], db2[1], db2[2], db2[3]);
    __syncthreads();
    wgrad_colsum(s_part, kThreads, row2 + C * C);
}

// workgroups: the forward tile kernels 4 per CU; B3 min(tiles, 512) and B3w G2 = min(tiles, 1024), the grids of
// k_linear_wgrad_x3<32, 64> and <32, 32>; B1 and B2 take k_bn_act_bwd's grid (8 per CU)
constexpr int kGridF = 256 * 4, kGridB3 = 256 * 2, kGridDb2 = 256 * 4, kGridS = 256 * 8;
inline int grid_tiles(int64_t N, int cap) { return grid_for((N + kTileRows - 1) / kTileRows, cap / 256); }
inline int grid_rows(int64_t N) { return grid_for((N + kThreads / (C / 4) - 1) / (kThreads / (C / 4)), kGridS / 256); }

}  // namespace ro
}  // namespace mgv

extern "C" int mgv_readout_fused_pack_elems(void) { return mgv::ro::pack_elems; }
extern "C" int mgv_readout_fused_grad_floats(void) { return mgv::ro::grad_floats; }
namespace {
int64_t ws_doubles(int64_t N) {
    using namespace mgv::ro;
    int64_t m = (int64_t)grid_tiles(N, kGridF) * s_f;
    const int64_t b3 = ((int64_t)grid_tiles(N, kGridB3) * s_b3 + (int64_t)grid_tiles(N, kGridDb2) * s_b3w2 + 1) / 2;
    const int64_t c[3] = {(int64_t)grid_rows(N) * s_b1, (int64_t)grid_rows(N) * s_b2, b3};
    for (int k = 0; k < 3; ++k) m = c[k] > m ? c[k] : m;
    return m;
}
}  // namespace

extern "C" int mgv_readout_fused_ws_doubles(int64_t N) {
    const int64_t m = ws_doubles(N);
    return m > 0x7fffffff ? -1 : (int)m;
}

extern "C" int mgv_readout_fused_fwd(int64_t N, const float* hf, const void* wpack, const float* b1, const float* g1, const float* be1,
                                     float* rm1, float* rv1, const float* b2, const float* g2, const float* be2, float* rm2, float* rv2,
                                     const float* w3, const float* b3, float p1, float p2, uint64_t seed1, uint64_t seed2, float momentum,
                                     float keep, float eps, int clamp01, float* y1, float* y2, float* stats, double* sums, float* prob,
                                     double* workspace, int64_t workspace_doubles, void* stream) {
    using namespace mgv::ro;
    MGV_CHECK_ARG(N > 0 && hf && wpack && b1 && g1 && be1 && rm1 && rv1 && b2 && g2 && be2 && rm2 && rv2 && w3 && b3);
    MGV_CHECK_ARG(y1 && y2 && stats && sums && prob && p1 >= 0.f && p1 < 1.f && p2 >= 0.f && p2 < 1.f);
    MGV_CHECK_ARG(workspace && workspace_doubles >= ws_doubles(N));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const __bf16* wp = static_cast<const __bf16*>(wpack);
    const int gf = grid_tiles(N, kGridF);
    hipMemsetAsync(sums, 0, 4 * C * sizeof(double), st);
    hipLaunchKernelGGL((mgv::ro::k_ro_fwd_lin<true>), dim3(gf), dim3(mgv::kThreads), 0, st, N, hf, wp + o_w1, b1, nullptr, nullptr, nullptr,
                       0.f, (uint64_t)0, y1, workspace);
    mgv::launch_slab_sum<double, double>(workspace, gf, s_f, 2 * C, sums, st);
    hipLaunchKernelGGL(mgv::ro::k_ro_bn_finalize, dim3(1), dim3(64), 0, st, N, sums, momentum, keep, eps, rm1, rv1, stats);
    hipLaunchKernelGGL((mgv::ro::k_ro_fwd_lin<false>), dim3(gf), dim3(mgv::kThreads), 0, st, N, y1, wp + o_w2, b2, stats, g1, be1,
                       p1, seed1, y2, workspace);
    mgv::launch_slab_sum<double, double>(workspace, gf, s_f, 2 * C, sums + 2 * C, st);
    hipLaunchKernelGGL(mgv::ro::k_ro_bn_finalize, dim3(1), dim3(64), 0, st, N, sums + 2 * C, momentum, keep, eps, rm2, rv2, stats + 2 * C);
    hipLaunchKernelGGL(mgv::ro::k_ro_head_fwd, dim3(grid_rows(N)), dim3(mgv::kThreads), 0, st, N, y2, stats + 2 * C, g2, be2, p2, seed2,
                       w3, b3, clamp01, prob);
    MGV_LAUNCH_RET();
}

extern "C" int mgv_readout_fused_bwd(int64_t N, const float* hf, const float* y1, const float* y2, const float* stats, const float* dprob,
                                     const void* wpack, const float* g1, const float* be1, const float* g2, const float* be2, const float* w3,
                                     const float* b3, float p1, float p2, uint64_t seed1, uint64_t seed2, int clamp01, float* dhf,
                                     float* grads, double* sums, double* workspace, int64_t workspace_doubles, void* stream) {
    using namespace mgv::ro;
    MGV_CHECK_ARG(N > 0 && hf && y1 && y2 && stats && dprob && wpack && g1 && be1 && g2 && be2 && w3 && b3 && dhf && grads && sums);
    MGV_CHECK_ARG(p1 >= 0.f && p1 < 1.f && p2 >= 0.f && p2 < 1.f);
    MGV_CHECK_ARG(workspace && workspace_doubles >= ws_doubles(N));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const __bf16* wp = static_cast<const __bf16*>(wpack);
    double* sums1 = sums;              // [sum dz1][sum dz1 xhat1]
    double* sums2 = sums + 2 * C;      // [sum dz2][sum dz2 xhat2]
    hipMemsetAsync(sums, 0, 4 * C * sizeof(double), st);
    hipMemsetAsync(grads, 0, grad_floats * sizeof(float), st);
    const int gs = grid_rows(N);
    hipLaunchKernelGGL(mgv::ro::k_ro_b1, dim3(gs), dim3(mgv::kThreads), 0, st, N, y2, stats + 2 * C, g2, be2, p2, seed2, w3, b3, clamp01,
                       dprob, workspace);
    mgv::launch_slab_sum<double, float>(workspace, gs, s_b1, C + 1, grads + g_w3, st);
    mgv::launch_slab_sum<double, double>(workspace + C + 1, gs, s_b1, 2 * C, sums2, st);
    mgv::launch_slab_sum<double, float>(workspace + C + 1, gs, s_b1, C, grads + g_be2, st);
    mgv::launch_slab_sum<double, float>(workspace + 2 * C + 1, gs, s_b1, C, grads + g_g2, st);
    hipLaunchKernelGGL(mgv::ro::k_ro_b2, dim3(gs), dim3(mgv::kThreads), 0, st, N, y1, y2, dprob, stats, g1, be1, g2, be2, p1, p2, seed1, seed2,
                       w3, b3, clamp01, sums2, wp + o_w2t, workspace);
    mgv::launch_slab_sum<double, double>(workspace, gs, s_b2, 2 * C, sums1, st);
    mgv::launch_slab_sum<double, float>(workspace, gs, s_b2, C, grads + g_be1, st);
    mgv::launch_slab_sum<double, float>(workspace + C, gs, s_b2, C, grads + g_g1, st);
    const int g3n = grid_tiles(N, kGridB3), g2n = grid_tiles(N, kGridDb2);
    float* slab1 = reinterpret_cast<float*>(workspace);
    float* slab2 = slab1 + (int64_t)g3n * s_b3;
    hipLaunchKernelGGL(mgv::ro::k_ro_b3w, dim3(g2n), dim3(mgv::kThreads), 0, st, N, y1, y2, dprob, stats, g1, be1, g2, be2, p1, p2, seed1,
                       seed2, w3, b3, clamp01, sums2, slab2);
    hipLaunchKernelGGL(mgv::ro::k_ro_b3, dim3(g3n), dim3(mgv::kThreads), 0, st, N, hf, y1, y2, dprob, stats, g1, be1, g2, be2, p1, p2, seed1,
                       seed2, w3, b3, clamp01, sums1, sums2, wp + o_w2t, wp + o_w1t, dhf, slab1);
    // [dW1][db1] and [dW2][db2] are contiguous in grads, as in a slab row
    mgv::launch_slab_sum<float, float>(slab1, g3n, s_b3, C * D + C, grads + g_w1, st);
    mgv::launch_slab_sum<float, float>(slab2, g2n, s_b3w2, C * C + C, grads + g_w2, st);
    MGV_LAUNCH_RET();
}
