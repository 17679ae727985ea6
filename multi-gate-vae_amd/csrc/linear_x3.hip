// Linear layers over node rows on bf16x3 split-precision MFMA (mgv_x3.h): the hs_linear / hs_decompose / VAE
// heads / readout layers of dg_ae_model_aig.py:50-56,100-106 and their input- and weight-gradients.  The fp32
// kernels of dense.hip price these streaming layers at the fp32-MFMA rate (K=128, M=64: 69 GFLOP per pass);
// here they are HBM-bound: rows are split into bf16 hi/lo planes in LDS once, the forward keeps its weight
// fragments in registers for the whole launch, the weight gradient reads both operands transposed from the
// row-major planes, and the next tile's rows are in flight (registers) while the current tile is multiplied.  The whole backward
// of a layer (k_linear_bwd_x3) is the weight-gradient kernel with the input gradient formed from the dY planes it already holds.
#include "mgv_x3.h"
#include "mgv_launch.h"
#include "mgv_slab.h"
#include "../../include/mgvae_hip.h"

namespace mgv {

struct LinX3Args {
    int64_t N;
    const float* X1; int K1; int ld1;
    const float* X2; int K2; int ld2;
    const __bf16* wpack;    // forward: [2][M*K] = W_hi, W_lo in fragment order (blocks (row tile, k-step))
    const float* b;
    float* Y; int ldy;
    const float* R; int ldr;     // optional residual rows added to Y on the way out
    float* Y2; int ldy2;         // fused backward: dX1 -> Y (its residual R), dX2 -> Y2; wpack = the transposed pack of the whole W
    const float* dY; int lddy;
    float* dW; float* db;
    float* slab;            // weight gradient: [gridDim][M*K + M] per-workgroup partials (dW row-major, then db)
    // grouped mode (order != nullptr): the rows are the level sweep's tiles — row r of tile t is NODE order[tile_start[t] + r]
    // (r < tile_count[t]); X / Y / R / dY rows are indexed by node; the forward takes tile t's weights from the pack of slot
    // tile_slot[t] (g_wstride elements apart) and its bias from b + tile_slot[t] * M.  tile_list (nullable) names the tiles.
    const int32_t* order; const int32_t* tile_start; const int32_t* tile_count; const int32_t* tile_slot; const int32_t* tile_list;
    int64_t g_ntiles; int64_t g_wstride;
};

// the wave split of a 64-row tile over M output columns (mgv_common.h WaveSplit without its H <= 128 bound: M = 3H = 192 here)
template <int M>
struct LinSplit {
    static_assert(M % 16 == 0, "column tiles of 16");
    static constexpr int HC = M / 16;
    static constexpr int WPC = HC < 4 ? HC : 4;
    static constexpr int WPR = 4 / WPC;
    static constexpr int RTW = 4 / WPR;
    static constexpr int HCW = HC / WPC;
    static_assert(HCW * WPC == HC, "column tiles must split over the waves");
};

__device__ __forceinline__ float4 f4x(const f32x4& v) { return make_float4(v[0], v[1], v[2], v[3]); }

// ---------------------------------------------------------------------------------------------- forward
template <int M, int K>
struct LinFwdGeom {
    using S = LinSplit<M>;                                    // 4 waves
    static constexpr int KS = K / 32;
    static constexpr int LDP = K + 8;                         // bf16 plane row
    static constexpr int PB = kTileRows * LDP * 2;
    static constexpr int LDY = M + 4;
    static constexpr int o_y = 2 * PB;
    static constexpr int smem_bytes = o_y + kTileRows * LDY * 4;
    static constexpr int F4 = kTileRows * K / 4;              // float4 per tile
    static constexpr int PF = F4 / kThreads;
    static_assert(PF * kThreads == F4 && K % 32 == 0, "tile must split over the threads");
};

template <int M, int K, bool GROUPED = false>
__global__ __launch_bounds__(kThreads) void k_linear_fwd_x3(LinX3Args a) {
    using G = LinFwdGeom<M, K>;
    using S = typename G::S;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __bf16* x_hi = reinterpret_cast<__bf16*>(smem_raw);
    __bf16* x_lo = reinterpret_cast<__bf16*>(smem_raw + G::PB);
    float* s_y = reinterpret_cast<float*>(smem_raw + G::o_y);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
    const int wc = w % S::WPC, wr = w / S::WPC;
    // this wave's weight fragments: column tiles wc*HCW.., all k-steps, hi and lo (grouped mode: reloaded per tile, the tile's slot)
    bf16x8 wh[S::HCW][G::KS], wl[S::HCW][G::KS];
    float bias[S::HCW];
    constexpr bool grouped = GROUPED;          // (its own instantiation: the plain kernels carry none of this)
    auto load_weights = [&](const __bf16* wp, const float* bp) {
#pragma unroll
        for (int j = 0; j < S::HCW; ++j) {
#pragma unroll
            for (int ks = 0; ks < G::KS; ++ks) {
                const int wo = (((wc * S::HCW + j) * G::KS) + ks) * 512 + lane * 8;
                wh[j][ks] = ldfrag(wp + wo); wl[j][ks] = ldfrag(wp + M * K + wo);
            }
            bias[j] = bp ? bp[(wc * S::HCW + j) * 16 + r] : 0.f;
        }
    };
    if (!grouped) load_weights(a.wpack, a.b);
    const int64_t ntiles = grouped ? a.g_ntiles : (a.N + kTileRows - 1) / kTileRows;
    // rows of a tile -> node ids: plain tiles are 64 consecutive nodes; grouped tiles go through the sweep's order list
    auto tile_span = [&](int64_t tile, int64_t& first, int& cnt, int& slot) {
        if (grouped) {
            const int64_t t = a.tile_list ? (int64_t)a.tile_list[tile] : tile;
            first = a.tile_start[t]; cnt = a.tile_count[t]; slot = a.tile_slot ? a.tile_slot[t] : 0;
        } else {
            first = tile * kTileRows; cnt = (int)(a.N - first < kTileRows ? a.N - first : kTileRows); slot = 0;
        }
    };
    auto node_of = [&](int64_t first, int cnt, int row) -> int64_t { return row < cnt ? (grouped ? (int64_t)a.order[first + row] : first + row) : -1; };
    f32x4 pf[G::PF];
    auto prefetch = [&](int64_t tile) {
        int64_t first; int cnt, slot;
        tile_span(tile, first, cnt, slot);
#pragma unroll
        for (int u = 0; u < G::PF; ++u) {
            const int f = tid + u * kThreads;
            const int row = f / (K / 4), c4 = (f % (K / 4)) * 4;
            const int64_t node = node_of(first, cnt, row);
            if (node >= 0) pf[u] = *reinterpret_cast<const f32x4*>(c4 < a.K1 ? a.X1 + node * a.ld1 + c4 : a.X2 + node * a.ld2 + (c4 - a.K1));
            else pf[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    int64_t tile = blockIdx.x;
    if (tile < ntiles) prefetch(tile);
    for (; tile < ntiles; tile += gridDim.x) {
        int64_t first; int cnt, slot;
        tile_span(tile, first, cnt, slot);
        if (grouped) load_weights(a.wpack + (int64_t)slot * a.g_wstride, a.b ? a.b + (int64_t)slot * M : nullptr);
#pragma unroll
        for (int u = 0; u < G::PF; ++u) {
            const int f = tid + u * kThreads;
            const int row = f / (K / 4), c4 = (f % (K / 4)) * 4;
            bf16x4 hi, lo;
            split4(f4x(pf[u]), hi, lo);
            st_bf4(x_hi + row * G::LDP + c4, hi); st_bf4(x_lo + row * G::LDP + c4, lo);
        }
        lds_barrier();
        if (tile + gridDim.x < ntiles) prefetch(tile + gridDim.x);
        f32x4 acc[S::RTW][S::HCW];
#pragma unroll
        for (int i = 0; i < S::RTW; ++i)
#pragma unroll
            for (int j = 0; j < S::HCW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks)
#pragma unroll
            for (int i = 0; i < S::RTW; ++i) {
                const int off = ((wr * S::RTW + i) * 16 + r) * G::LDP + 32 * ks + 8 * q;
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
                for (int e = 0; e < 4; ++e) s_y[((wr * S::RTW + i) * 16 + q * 4 + e) * G::LDY + col] = acc[i][j][e] + bias[j];
            }
        lds_barrier();
        for (int i = tid; i < kTileRows * (M / 4); i += kThreads) {
            const int row = i / (M / 4), c4 = (i % (M / 4)) * 4;
            const int64_t node = node_of(first, cnt, row);
            if (node >= 0) {
                float4 v = ld4(s_y + row * G::LDY + c4);
                if (a.R) v = add4(v, ld4(a.R + node * a.ldr + c4));
                st4(a.Y + node * a.ldy + c4, v);
            }
        }
        // the planes are rewritten only after this barrier pair; s_y only after the next tile's first barrier
    }
}

// ---------------------------------------------------------------------------------------------- weight gradient
// dW[M][K] += dY^T [X1|X2], db[M] += colsum(dY).  NW waves in a WI x WJ grid over the (M/16) x (K/16) output tiles.
template <int M, int K, int NW, int WI>
struct LinWgGeom {
    static constexpr int NT = 64 * NW;
    static constexpr int TI = M / 16, TJ = K / 16, WJ = NW / WI;
    static constexpr int ITW = TI / WI, JTW = TJ / WJ;
    static_assert(ITW * WI == TI && JTW * WJ == TJ && ITW >= 1 && JTW >= 1, "wave grid must tile the output");
    static constexpr int LDG = M + 8, LDX = K + 8;
    static constexpr int GPB = kTileRows * LDG * 2, XPB = kTileRows * LDX * 2;
    static constexpr int F4G = kTileRows * M / 4, F4X = kTileRows * K / 4;
    static constexpr int PFG = (F4G + NT - 1) / NT, PFX = (F4X + NT - 1) / NT;
    static_assert(NT % (M / 4) == 0, "a thread must keep its dY column across its loads");
    static constexpr int o_db = 2 * GPB + 2 * XPB;
    static constexpr int smem_bytes = o_db + M * 4;
};

// The input gradient of the same tile, dX[64][K] = dY[64][M] W (fused backward): the forward kernel's product with the dY planes as
// its row-major operand, 4 row tiles x K/16 column tiles over the NW waves, one column tile per wave.
template <int M, int K, int NW>
struct LinDxGeom {
    static constexpr int KS = M / 32;
    static constexpr int WPC = K / 16, WPR = NW / WPC, RTW = 4 / WPR;
    static_assert(WPC * WPR == NW && RTW * WPR == 4, "one column tile per wave, the row tiles split over the rest");
    static constexpr int LDY = K + 4;                         // fp32 staging row, over the X planes
    static_assert(kTileRows * LDY * 4 <= 2 * kTileRows * (K + 8) * 2, "the staged tile must fit the X planes");
    static constexpr int PF = kTileRows * K / 4 / (64 * NW);  // float4 per thread in the store phase
    static_assert(PF * 64 * NW * 4 == kTileRows * K, "the output tile must split over the threads");
};

// DX: also the input gradient (k_linear_bwd_x3).
// KSR: the transposed weight fragments of k-steps < KSR live in registers for the whole launch, those of the other k-steps in LDS
// behind s_db (M = 128: four k-steps of both planes are 32 registers, which the 128 of two workgroups per CU do not leave).
template <int M, int K, int NW, int WI, bool GROUPED, bool DX, int KSR>
__device__ __forceinline__ void linear_wgrad_x3_body(const LinX3Args& a) {
    using G = LinWgGeom<M, K, NW, WI>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __bf16* g_hi = reinterpret_cast<__bf16*>(smem_raw);
    __bf16* g_lo = reinterpret_cast<__bf16*>(smem_raw + G::GPB);
    __bf16* x_hi = reinterpret_cast<__bf16*>(smem_raw + 2 * G::GPB);
    __bf16* x_lo = reinterpret_cast<__bf16*>(smem_raw + 2 * G::GPB + G::XPB);
    float* s_db = reinterpret_cast<float*>(smem_raw + G::o_db);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
    const int it0 = (w / G::WJ) * G::ITW, jt0 = (w % G::WJ) * G::JTW;
    for (int i = tid; i < M; i += G::NT) s_db[i] = 0.f;
    f32x4 acc[G::ITW][G::JTW];
#pragma unroll
    for (int i = 0; i < G::ITW; ++i)
#pragma unroll
        for (int j = 0; j < G::JTW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 dbs = zero4();            // column sums of dY over this thread's rows (its column quad is fixed)
    f32x4 pg[G::PFG], px[G::PFX];
    constexpr bool grouped = GROUPED;
    const int64_t ntiles = grouped ? a.g_ntiles : (a.N + kTileRows - 1) / kTileRows;
    auto prefetch = [&](int64_t tile) {
        int64_t first = tile * kTileRows;
        int cnt = (int)(a.N - first < kTileRows ? a.N - first : kTileRows);
        if (grouped) {
            const int64_t t = a.tile_list ? (int64_t)a.tile_list[tile] : tile;
            first = a.tile_start[t]; cnt = a.tile_count[t];
        }
#pragma unroll
        for (int u = 0; u < G::PFG; ++u) {
            const int f = tid + u * G::NT;
            const int row = f / (M / 4), c4 = (f % (M / 4)) * 4;
            const int64_t node = row < cnt ? (grouped ? (int64_t)a.order[first + row] : first + row) : -1;
            if (f < G::F4G && node >= 0) pg[u] = *reinterpret_cast<const f32x4*>(a.dY + node * a.lddy + c4);
            else pg[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < G::PFX; ++u) {
            const int f = tid + u * G::NT;
            const int row = f / (K / 4), c4 = (f % (K / 4)) * 4;
            const int64_t node = row < cnt ? (grouped ? (int64_t)a.order[first + row] : first + row) : -1;
            if (f < G::F4X && node >= 0) px[u] = *reinterpret_cast<const f32x4*>(c4 < a.K1 ? a.X1 + node * a.ld1 + c4 : a.X2 + node * a.ld2 + (c4 - a.K1));
            else px[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    // fused backward: this wave's column tile of W^T, hi and lo (without DX the geometry is a placeholder that satisfies its asserts)
    using D = LinDxGeom<DX ? M : 32, DX ? K : 16 * NW, NW>;
    const int dwc = w % D::WPC, dwr = w / D::WPC;
    bf16x8 th[KSR > 0 ? KSR : 1], tl[KSR > 0 ? KSR : 1];
    constexpr int KSL = DX ? D::KS - KSR : 0, WTL = (K / 16) * KSL * 512;      // k-steps and elements per plane in LDS
    __bf16* s_wt = reinterpret_cast<__bf16*>(smem_raw + G::smem_bytes);
    auto wt_lds = [&](int plane, int ks) { return ldfrag(s_wt + plane * WTL + (dwc * KSL + ks - KSR) * 512 + lane * 8); };
    if constexpr (DX) {
#pragma unroll
        for (int ks = 0; ks < KSR; ++ks) {
            const int wo = (dwc * D::KS + ks) * 512 + lane * 8;
            th[ks] = ldfrag(a.wpack + wo); tl[ks] = ldfrag(a.wpack + M * K + wo);
        }
        if constexpr (KSL > 0) for (int c = tid; c < 2 * WTL / 8; c += G::NT) {         // (the first tile barrier publishes it)
            const int plane = c / (WTL / 8), blk = (c % (WTL / 8)) / 64, ct = blk / KSL, ks = KSR + blk % KSL;
            *reinterpret_cast<bf16x8*>(s_wt + c * 8) = ldfrag(a.wpack + plane * M * K + (ct * D::KS + ks) * 512 + (c % 64) * 8);
        }
    }
    int64_t tile = blockIdx.x;
    if (tile < ntiles) prefetch(tile);
    for (; tile < ntiles; tile += gridDim.x) {
#pragma unroll
        for (int u = 0; u < G::PFG; ++u) {
            const int f = tid + u * G::NT;
            if (f < G::F4G) {
                const int row = f / (M / 4), c4 = (f % (M / 4)) * 4;
                const float4 v = f4x(pg[u]);
                dbs = add4(dbs, v);
                bf16x4 hi, lo;
                split4(v, hi, lo);
                st_bf4(g_hi + row * G::LDG + c4, hi); st_bf4(g_lo + row * G::LDG + c4, lo);
            }
        }
#pragma unroll
        for (int u = 0; u < G::PFX; ++u) {
            const int f = tid + u * G::NT;
            if (f < G::F4X) {
                const int row = f / (K / 4), c4 = (f % (K / 4)) * 4;
                bf16x4 hi, lo;
                split4(f4x(px[u]), hi, lo);
                st_bf4(x_hi + row * G::LDX + c4, hi); st_bf4(x_lo + row * G::LDX + c4, lo);
            }
        }
        lds_barrier();
        if (tile + gridDim.x < ntiles) prefetch(tile + gridDim.x);
#pragma unroll
        for (int ks = 0; ks < kTileRows / 32; ++ks) {
            bf16x8 bh[G::JTW], bl[G::JTW];
#pragma unroll
            for (int j = 0; j < G::JTW; ++j) {
                bh[j] = ldfrag_tr2(x_hi, G::LDX, 32 * ks, (jt0 + j) * 16);
                bl[j] = ldfrag_tr2(x_lo, G::LDX, 32 * ks, (jt0 + j) * 16);
            }
#pragma unroll
            for (int i = 0; i < G::ITW; ++i) {
                const bf16x8 ah = ldfrag_tr2(g_hi, G::LDG, 32 * ks, (it0 + i) * 16), al = ldfrag_tr2(g_lo, G::LDG, 32 * ks, (it0 + i) * 16);
#pragma unroll
                for (int j = 0; j < G::JTW; ++j) mma_x3(acc[i][j], ah, al, bh[j], bl[j]);
            }
        }
        lds_barrier();
        if constexpr (DX) {
            // dX = dY W as k_linear_fwd_x3 forms it (ks ascending, mma_x3, zero-initialised accumulators: the same bits), from the dY
            // planes still in LDS; the fp32 tile is staged over the X planes, which nobody reads after the barrier above
            float* s_y = reinterpret_cast<float*>(smem_raw + 2 * G::GPB);
            const int64_t first = tile * kTileRows;
            f32x4 dacc[D::RTW];
#pragma unroll
            for (int i = 0; i < D::RTW; ++i) dacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < D::KS; ++ks)
#pragma unroll
                for (int i = 0; i < D::RTW; ++i) {
                    const int off = ((dwr * D::RTW + i) * 16 + r) * G::LDG + 32 * ks + 8 * q;
                    const bf16x8 gh = ldfrag(g_hi + off), gl = ldfrag(g_lo + off);
                    if (ks < KSR) mma_x3(dacc[i], gh, gl, th[ks], tl[ks]);
                    else mma_x3(dacc[i], gh, gl, wt_lds(0, ks), wt_lds(1, ks));
                }
#pragma unroll
            for (int i = 0; i < D::RTW; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) s_y[((dwr * D::RTW + i) * 16 + q * 4 + e) * D::LDY + dwc * 16 + r] = dacc[i][e] + 0.f;   // (the forward's absent bias)
            lds_barrier();
#pragma unroll
            for (int u = 0; u < D::PF; ++u) {
                const int f = tid + u * G::NT;
                const int row = f / (K / 4), c4 = (f % (K / 4)) * 4;
                if (first + row < a.N) {
                    float4 v = ld4(s_y + row * D::LDY + c4);
                    if (c4 < a.K1) {
                        if (a.R) v = add4(v, ld4(a.R + (first + row) * a.ldr + c4));
                        st4(a.Y + (first + row) * a.ldy + c4, v);
                    } else {
                        st4(a.Y2 + (first + row) * a.ldy2 + (c4 - a.K1), v);
                    }
                }
            }
            lds_barrier();      // the next tile's X planes overwrite the staged rows
        }
    }
    // per-workgroup partials to this workgroup's slab row (plain stores); k_slab_sum adds the rows in a fixed order
    float* slab = a.slab + (int64_t)blockIdx.x * (M * K + M);
#pragma unroll
    for (int i = 0; i < G::ITW; ++i)
#pragma unroll
        for (int j = 0; j < G::JTW; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                slab[((it0 + i) * 16 + q * 4 + e) * K + (jt0 + j) * 16 + r] = acc[i][j][e];
    if (a.db) {
        // column sums of dY: one float4 per thread into the (dead) planes, then a fixed-order sum over the threads of a column quad
        float4* s_part = reinterpret_cast<float4*>(smem_raw);
        if (tid < G::F4G) s_part[tid] = dbs;
        __syncthreads();
        constexpr int QPR = M / 4;                       // column quads per row; thread t holds quad t % QPR
        if (tid < M) {
            const int c4 = tid / 4, e = tid % 4;
            float sum = 0.f;
            for (int t = c4; t < G::F4G && t < G::NT; t += QPR) { const float4 v = s_part[t]; sum += e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
            slab[M * K + tid] = sum;
        }
    }
}

template <int M, int K, int NW, int WI, bool GROUPED = false>
__global__ __launch_bounds__(64 * NW) void k_linear_wgrad_x3(LinX3Args a) {
    linear_wgrad_x3_body<M, K, NW, WI, GROUPED, false, 0>(a);
}

// dW, db as k_linear_wgrad_x3 (same grid, tile walk and slab rows) and dX1 | dX2 = dY W (+ R) in the same pass over dY
template <int M, int K, int NW, int WI, int KSR>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(4))) void k_linear_bwd_x3(LinX3Args a) {
    linear_wgrad_x3_body<M, K, NW, WI, false, true, KSR>(a);
}

// fp32 matrix -> bf16 hi/lo planes in MFMA fragment order: block (row tile, k-step) = 512 elements, lane 16q+r holds
// A[16 rt + r][32 ks + 8q .. +7] where A = W (R x K, leading dimension ldw) or its transpose view A[i][k] = W[k][i]
__global__ __launch_bounds__(256) void k_wpack_bf16x3(const float* W, int R, int K, int ldw, int transpose, __bf16* hi, __bf16* lo) {
    const int total = R * K, ksn = K / 32;
    for (int o = blockIdx.x * 256 + threadIdx.x; o < total; o += gridDim.x * 256) {
        const int blk = o >> 9, within = o & 511, lane = within >> 3, e = within & 7;
        const int rt = blk / ksn, ks = blk % ksn;
        const int row = rt * 16 + (lane & 15), k = ks * 32 + (lane >> 4) * 8 + e;
        const float v = transpose ? W[(int64_t)k * ldw + row] : W[(int64_t)row * ldw + k];
        __bf16 h, l;
        split_bf16(v, h, l);
        hi[o] = h; lo[o] = l;
    }
}

template <int M, int K, bool GROUPED = false>
int launch_linear_fwd_x3(const LinX3Args& a, hipStream_t st) {
    using G = LinFwdGeom<M, K>;
    allow_lds<k_linear_fwd_x3<M, K, GROUPED>>();
    const int64_t ntiles = a.order ? a.g_ntiles : (a.N + kTileRows - 1) / kTileRows;
    int per_cu = 160 * 1024 / G::smem_bytes;
    per_cu = per_cu > 4 ? 4 : per_cu;
    hipLaunchKernelGGL((k_linear_fwd_x3<M, K, GROUPED>), dim3(grid_for(ntiles, per_cu)), dim3(kThreads), G::smem_bytes, st, a);
    MGV_LAUNCH_RET();
}

template <int M, int K, int NW, int WI, bool GROUPED = false>
int launch_linear_wgrad_x3(const LinX3Args& a, int64_t ws_floats, hipStream_t st) {
    using G = LinWgGeom<M, K, NW, WI>;
    allow_lds<k_linear_wgrad_x3<M, K, NW, WI, GROUPED>>();
    const int64_t ntiles = a.order ? a.g_ntiles : (a.N + kTileRows - 1) / kTileRows;
    int per_cu = 160 * 1024 / G::smem_bytes;
    const int cap = 1024 / G::NT;                    // 16 waves per CU
    per_cu = per_cu > cap ? cap : per_cu;
    const int grid = grid_for(ntiles, per_cu);
    if (a.slab == nullptr || ws_floats < (int64_t)grid * (M * K + M)) return MGV_EINVAL;
    hipLaunchKernelGGL((k_linear_wgrad_x3<M, K, NW, WI, GROUPED>), dim3(grid), dim3(G::NT), G::smem_bytes, st, a);
    launch_slab_sum<float, float>(a.slab, grid, M * K + M, M * K, a.dW, st);
    if (a.db) launch_slab_sum<float, float>(a.slab + M * K, grid, M * K + M, M, a.db, st);
    MGV_LAUNCH_RET();
}

// the weight-gradient launch of the same shape with the input-gradient phase in its kernel: same grid, same slab rows, same sums
template <int M, int K, int NW, int WI, int KSR>
int launch_linear_bwd_x3(const LinX3Args& a, int64_t ws_floats, hipStream_t st) {
    using G = LinWgGeom<M, K, NW, WI>;
    allow_lds<k_linear_bwd_x3<M, K, NW, WI, KSR>>();
    const int64_t ntiles = (a.N + kTileRows - 1) / kTileRows;
    int per_cu = 160 * 1024 / G::smem_bytes;
    const int cap = 1024 / G::NT;
    per_cu = per_cu > cap ? cap : per_cu;
    const int grid = grid_for(ntiles, per_cu);
    if (a.slab == nullptr || ws_floats < (int64_t)grid * (M * K + M)) return MGV_EINVAL;
    constexpr int smem = G::smem_bytes + 2 * (K / 16) * (M / 32 - KSR) * 512 * 2;
    static_assert(2 * smem <= 160 * 1024, "two workgroups per CU, as the weight-gradient kernel runs");
    hipLaunchKernelGGL((k_linear_bwd_x3<M, K, NW, WI, KSR>), dim3(grid), dim3(G::NT), smem, st, a);
    launch_slab_sum<float, float>(a.slab, grid, M * K + M, M * K, a.dW, st);
    if (a.db) launch_slab_sum<float, float>(a.slab + M * K, grid, M * K + M, M, a.db, st);
    MGV_LAUNCH_RET();
}

// ---------------------------------------------------------------------------------------------- the hs seam (H = 64)
// hs = hs_linear([s|t]) and st = hs_decompose(hs) meet at hs: run as two Linears, hs is written and read straight back, and in the
// backward so is dhs.  The pair kernels make one pass each way: the forward forms st from the hs tile it still holds in LDS, the
// backward forms dhs = dst Wd + ghs per tile and feeds it to hs_linear's backward without a trip through memory.  Every product is
// the one the stand-alone kernels make (same planes, same k-step order, same mma_x3 chain), so the results carry the same bits.
struct LinPairArgs {
    int64_t N;
    const float* S; int lds;  const float* T; int ldt;      // the two 64-column inputs of hs_linear, row-strided
    const __bf16* wl; const float* bl;                       // forward: pack of Wl [64 x 128]; backward: of its [128 x 64] transposed view
    const __bf16* wd; const float* bd;                       // forward: pack of Wd [128 x 64]; backward: of its [64 x 128] transposed view
    float* HS; int ldhs; float* ST; int ldst;                // forward outputs
    const float* dST; int lddst; const float* gHS; int ldghs; const float* hs; int ldh;      // backward inputs (gHS nullable)
    float* dS; int ldds; float* dT; int lddt;
    float* slab_l; float* slab_d;                            // per-workgroup partials of (dWl, dbl) and (dWd, dbd)
    int want_dbl, want_dbd;
};

struct PairFwdGeom {
    using GL = LinFwdGeom<64, 128>;                          // hs = [s|t] Wl^T + bl
    using GD = LinFwdGeom<128, 64>;                          // st = hs Wd^T + bd
    // the hs planes lie over the head of the (dead) s|t planes; the staged st tile over their tail and the staged hs tile
    static constexpr int o_st = 2 * GD::PB;
    static constexpr int smem_bytes = GL::smem_bytes;
    static constexpr int NT = 512, PF = kTileRows * 128 / 4 / NT;
    static_assert(o_st + kTileRows * GD::LDY * 4 <= smem_bytes && o_st <= GL::o_y && o_st % 16 == 0, "the staged st tile must fit behind the hs planes");
};

// 8 waves: the hs product as 4 column tiles x 2 row halves, the st product as 8 column tiles (which wave forms an entry does not
// change its bits: every entry is one zero-initialised accumulator over ascending k-steps).  Two workgroups per CU.
__global__ __launch_bounds__(PairFwdGeom::NT) __attribute__((amdgpu_waves_per_eu(4))) void k_linear_pair_fwd_x3(LinPairArgs a) {
    using P = PairFwdGeom;
    using GL = P::GL;
    using GD = P::GD;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __bf16* x_hi = reinterpret_cast<__bf16*>(smem_raw);
    __bf16* x_lo = reinterpret_cast<__bf16*>(smem_raw + GL::PB);
    float* s_y = reinterpret_cast<float*>(smem_raw + GL::o_y);
    __bf16* h_hi = reinterpret_cast<__bf16*>(smem_raw);
    __bf16* h_lo = reinterpret_cast<__bf16*>(smem_raw + GD::PB);
    float* s_st = reinterpret_cast<float*>(smem_raw + P::o_st);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
    const int wc = w % 4, wr = w / 4;
    // this wave's weight fragments of both layers, for the whole launch
    bf16x8 lh[GL::KS], ll[GL::KS], dh[GD::KS], dl[GD::KS];
#pragma unroll
    for (int ks = 0; ks < GL::KS; ++ks) {
        const int wo = (wc * GL::KS + ks) * 512 + lane * 8;
        lh[ks] = ldfrag(a.wl + wo); ll[ks] = ldfrag(a.wl + 64 * 128 + wo);
    }
#pragma unroll
    for (int ks = 0; ks < GD::KS; ++ks) {
        const int wo = (w * GD::KS + ks) * 512 + lane * 8;
        dh[ks] = ldfrag(a.wd + wo); dl[ks] = ldfrag(a.wd + 128 * 64 + wo);
    }
    const float bias_l = a.bl ? a.bl[wc * 16 + r] : 0.f, bias_d = a.bd ? a.bd[w * 16 + r] : 0.f;
    const int64_t ntiles = (a.N + kTileRows - 1) / kTileRows;
    f32x4 pf[P::PF];
    auto prefetch = [&](int64_t tile) {
        const int64_t first = tile * kTileRows;
#pragma unroll
        for (int u = 0; u < P::PF; ++u) {
            const int f = tid + u * P::NT;
            const int row = f / 32, c4 = (f % 32) * 4;
            if (first + row < a.N) pf[u] = *reinterpret_cast<const f32x4*>(c4 < 64 ? a.S + (first + row) * a.lds + c4 : a.T + (first + row) * a.ldt + (c4 - 64));
            else pf[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    int64_t tile = blockIdx.x;
    if (tile < ntiles) prefetch(tile);
    for (; tile < ntiles; tile += gridDim.x) {
        const int64_t first = tile * kTileRows;
#pragma unroll
        for (int u = 0; u < P::PF; ++u) {
            const int f = tid + u * P::NT;
            const int row = f / 32, c4 = (f % 32) * 4;
            bf16x4 hi, lo;
            split4(f4x(pf[u]), hi, lo);
            st_bf4(x_hi + row * GL::LDP + c4, hi); st_bf4(x_lo + row * GL::LDP + c4, lo);
        }
        lds_barrier();
        if (tile + gridDim.x < ntiles) prefetch(tile + gridDim.x);
        {   // hs as k_linear_fwd_x3<64, 128> forms it
            f32x4 acc[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < GL::KS; ++ks)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int off = ((wr * 2 + i) * 16 + r) * GL::LDP + 32 * ks + 8 * q;
                    mma_x3(acc[i], ldfrag(x_hi + off), ldfrag(x_lo + off), lh[ks], ll[ks]);
                }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) s_y[((wr * 2 + i) * 16 + q * 4 + e) * GL::LDY + wc * 16 + r] = acc[i][e] + bias_l;
        }
        lds_barrier();      // the staged hs tile is whole; nobody reads the s|t planes any more
        // hs rows out, and the same fp32 values split into the planes the decompose product reads (what its own kernel makes of
        // the rows it loads back: the round trip through memory is exact)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int f = tid + u * P::NT;
            const int row = f / 16, c4 = (f % 16) * 4;
            const float4 v = ld4(s_y + row * GL::LDY + c4);
            bf16x4 hi, lo;
            split4(v, hi, lo);
            st_bf4(h_hi + row * GD::LDP + c4, hi); st_bf4(h_lo + row * GD::LDP + c4, lo);
            if (first + row < a.N) st4(a.HS + (first + row) * a.ldhs + c4, v);
        }
        lds_barrier();
        {   // st as k_linear_fwd_x3<128, 64> forms it
            f32x4 acc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < GD::KS; ++ks)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int off = (i * 16 + r) * GD::LDP + 32 * ks + 8 * q;
                    mma_x3(acc[i], ldfrag(h_hi + off), ldfrag(h_lo + off), dh[ks], dl[ks]);
                }
            // (the staged st tile lies clear of the hs planes; what it covers was last read before the two barriers above)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) s_st[(i * 16 + q * 4 + e) * GD::LDY + w * 16 + r] = acc[i][e] + bias_d;
        }
        lds_barrier();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int f = tid + u * P::NT;
            const int row = f / 32, c4 = (f % 32) * 4;
            if (first + row < a.N) st4(a.ST + (first + row) * a.ldst + c4, ld4(s_st + row * GD::LDY + c4));
        }
        lds_barrier();      // the next tile's s|t planes overwrite the staged st rows
    }
}

// Backward of the pair on the grid, tile walk and slab rows of k_linear_bwd_x3<64, 128, 8, 2, 2> (hs_linear's backward), per tile:
//   dWd += dst^T hs, dbd += colsum(dst)                 as k_linear_bwd_x3<128, 64, 8, 4, 1> accumulates them
//   dhs  = dst Wd + ghs                                  its DX phase with ghs as the residual, kept in LDS, split into planes
//   dWl += dhs^T [s|t], dbl += colsum(dhs), ds|dt = dhs Wl      as k_linear_bwd_x3<64, 128, 8, 2, 2> makes them from a dhs it loads
// ds|dt, dWl and dbl carry the bits of the two launches.  dWd and dbd are summed over THIS kernel's partition of the tiles over
// workgroups, which need not be the stand-alone decompose backward's: they may differ from it in rounding.
// LDS (bytes): R1 [0, 34816) the dst planes, then the staged dhs, then the s|t planes, then the staged ds|dt; R2 [34816, 53248) the
// hs planes, then the dhs planes; behind them the Wd^T fragments of k-steps >= 1 (k-step 0 and all of Wl^T live in registers).
// Loads in flight: dst and hs of the NEXT tile during the second half of a tile, s|t and ghs of THIS tile during its first half.
// One workgroup per CU at a time (amdgpu_waves_per_eu(2): 240 VGPRs, none spilled) on the two-per-CU grid whose slab rows it keeps:
// held to the 128 registers of two resident workgroups it spills 117 of them and takes 4.75 ms at N = 4,194,304 against 1.57 ms.
struct PairBwdGeom {
    static constexpr int NW = 8, NT = 64 * NW;
    using WL = LinWgGeom<64, 128, NW, 2>;                    // dWl: dY = dhs (LDG = 72), X = s|t (LDX = 136)
    using WD = LinWgGeom<128, 64, NW, 4>;                    // dWd: dY = dst (LDG = 136), X = hs (LDX = 72)
    using DL = LinDxGeom<64, 128, NW>;                       // ds|dt = dhs Wl
    using DD = LinDxGeom<128, 64, NW>;                       // dhs = dst Wd
    static constexpr int KSR = 1, KSL = DD::KS - KSR, WTL = DD::WPC * KSL * 512;
    static constexpr int o_r2 = 2 * WD::GPB, o_wt = o_r2 + 2 * WD::XPB;
    static constexpr int smem_bytes = o_wt + 2 * WTL * 2;
    static_assert(2 * WL::XPB == 2 * WD::GPB && 2 * WL::GPB == 2 * WD::XPB, "the two layers' planes share R1 and R2");
    static_assert(kTileRows * DD::LDY * 4 <= o_r2 && kTileRows * DL::LDY * 4 <= o_r2, "the staged tiles must fit R1");
    static_assert(2 * NT * 16 <= o_r2, "the column-sum partials must fit R1");
    static constexpr int slab_l = 64 * 128 + 64, slab_d = 128 * 64 + 128;
};

__global__ __launch_bounds__(PairBwdGeom::NT) __attribute__((amdgpu_waves_per_eu(2))) void k_linear_pair_bwd_x3(LinPairArgs a) {
    using P = PairBwdGeom;
    using WL = P::WL;
    using WD = P::WD;
    using DL = P::DL;
    using DD = P::DD;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    // R1
    __bf16* g_hi = reinterpret_cast<__bf16*>(smem_raw);                          // dst planes
    __bf16* g_lo = reinterpret_cast<__bf16*>(smem_raw + WD::GPB);
    float* s_dhs = reinterpret_cast<float*>(smem_raw);                           // staged dst Wd
    __bf16* x_hi = reinterpret_cast<__bf16*>(smem_raw);                          // s|t planes
    __bf16* x_lo = reinterpret_cast<__bf16*>(smem_raw + WL::XPB);
    float* s_dx = reinterpret_cast<float*>(smem_raw);                            // staged ds|dt
    // R2
    __bf16* h_hi = reinterpret_cast<__bf16*>(smem_raw + P::o_r2);                // hs planes
    __bf16* h_lo = reinterpret_cast<__bf16*>(smem_raw + P::o_r2 + WD::XPB);
    __bf16* e_hi = reinterpret_cast<__bf16*>(smem_raw + P::o_r2);                // dhs planes
    __bf16* e_lo = reinterpret_cast<__bf16*>(smem_raw + P::o_r2 + WL::GPB);
    __bf16* s_wt = reinterpret_cast<__bf16*>(smem_raw + P::o_wt);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
    const int it0l = (w / WL::WJ) * WL::ITW, jt0l = (w % WL::WJ) * WL::JTW;
    const int it0d = (w / WD::WJ) * WD::ITW, jt0d = (w % WD::WJ) * WD::JTW;
    const int dwc = w % DD::WPC, dwr = w / DD::WPC;          // dhs: column tile dwc, row tiles dwr * 2 ..; ds|dt: column tile w, all rows
    f32x4 accl[WL::ITW][WL::JTW], accd[WD::ITW][WD::JTW];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) { accl[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; accd[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    static_assert(WL::ITW == 2 && WL::JTW == 2 && WD::ITW == 2 && WD::JTW == 2, "2 x 2 output tiles per wave, both layers");
    float4 dbl = zero4(), dbd = zero4();
    // transposed weight fragments: Wl^T (both k-steps) and k-step 0 of Wd^T in registers, the rest of Wd^T in LDS
    bf16x8 th[DL::KS], tl[DL::KS];
#pragma unroll
    for (int ks = 0; ks < DL::KS; ++ks) {
        const int wo = (w * DL::KS + ks) * 512 + lane * 8;
        th[ks] = ldfrag(a.wl + wo); tl[ks] = ldfrag(a.wl + 64 * 128 + wo);
    }
    const bf16x8 uh = ldfrag(a.wd + (dwc * DD::KS) * 512 + lane * 8), ul = ldfrag(a.wd + 128 * 64 + (dwc * DD::KS) * 512 + lane * 8);
    for (int c = tid; c < 2 * P::WTL / 8; c += P::NT) {     // (the first tile barrier publishes it)
        const int plane = c / (P::WTL / 8), blk = (c % (P::WTL / 8)) / 64, ct = blk / P::KSL, ks = P::KSR + blk % P::KSL;
        *reinterpret_cast<bf16x8*>(s_wt + c * 8) = ldfrag(a.wd + plane * 128 * 64 + (ct * DD::KS + ks) * 512 + (c % 64) * 8);
    }
    auto wt_lds = [&](int plane, int ks) { return ldfrag(s_wt + plane * P::WTL + (dwc * P::KSL + ks - P::KSR) * 512 + lane * 8); };
    const int64_t ntiles = (a.N + kTileRows - 1) / kTileRows;
    f32x4 pa[4], pb[2];          // dst and hs of a tile, then its s|t and ghs
    auto fetch_gh = [&](int64_t tile) {
        const int64_t first = tile * kTileRows;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int f = tid + u * P::NT;
            const int64_t row = first + f / 32; const int c4 = (f % 32) * 4;
            pa[u] = row < a.N ? *reinterpret_cast<const f32x4*>(a.dST + row * a.lddst + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int f = tid + u * P::NT;
            const int64_t row = first + f / 16; const int c4 = (f % 16) * 4;
            pb[u] = row < a.N ? *reinterpret_cast<const f32x4*>(a.hs + row * a.ldh + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto fetch_xr = [&](int64_t tile) {
        const int64_t first = tile * kTileRows;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int f = tid + u * P::NT;
            const int64_t row = first + f / 32; const int c4 = (f % 32) * 4;
            pa[u] = row < a.N ? *reinterpret_cast<const f32x4*>(c4 < 64 ? a.S + row * a.lds + c4 : a.T + row * a.ldt + (c4 - 64)) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int f = tid + u * P::NT;
            const int64_t row = first + f / 16; const int c4 = (f % 16) * 4;
            pb[u] = (a.gHS && row < a.N) ? *reinterpret_cast<const f32x4*>(a.gHS + row * a.ldghs + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    int64_t tile = blockIdx.x;
    if (tile < ntiles) fetch_gh(tile);
    for (; tile < ntiles; tile += gridDim.x) {
        const int64_t first = tile * kTileRows;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int f = tid + u * P::NT;
            const int row = f / 32, c4 = (f % 32) * 4;
            const float4 v = f4x(pa[u]);
            dbd = add4(dbd, v);
            bf16x4 hi, lo;
            split4(v, hi, lo);
            st_bf4(g_hi + row * WD::LDG + c4, hi); st_bf4(g_lo + row * WD::LDG + c4, lo);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int f = tid + u * P::NT;
            const int row = f / 16, c4 = (f % 16) * 4;
            bf16x4 hi, lo;
            split4(f4x(pb[u]), hi, lo);
            st_bf4(h_hi + row * WD::LDX + c4, hi); st_bf4(h_lo + row * WD::LDX + c4, lo);
        }
        lds_barrier();
        fetch_xr(tile);
        // dWd += dst^T hs
#pragma unroll
        for (int ks = 0; ks < kTileRows / 32; ++ks) {
            bf16x8 bh[2], bl[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                bh[j] = ldfrag_tr2(h_hi, WD::LDX, 32 * ks, (jt0d + j) * 16);
                bl[j] = ldfrag_tr2(h_lo, WD::LDX, 32 * ks, (jt0d + j) * 16);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const bf16x8 ah = ldfrag_tr2(g_hi, WD::LDG, 32 * ks, (it0d + i) * 16), al = ldfrag_tr2(g_lo, WD::LDG, 32 * ks, (it0d + i) * 16);
#pragma unroll
                for (int j = 0; j < 2; ++j) mma_x3(accd[i][j], ah, al, bh[j], bl[j]);
            }
        }
        {   // dst Wd, as the DX phase of the decompose backward forms it
            f32x4 dacc[DD::RTW];
#pragma unroll
            for (int i = 0; i < DD::RTW; ++i) dacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < DD::KS; ++ks)
#pragma unroll
                for (int i = 0; i < DD::RTW; ++i) {
                    const int off = ((dwr * DD::RTW + i) * 16 + r) * WD::LDG + 32 * ks + 8 * q;
                    const bf16x8 gh = ldfrag(g_hi + off), gl = ldfrag(g_lo + off);
                    if (ks < P::KSR) mma_x3(dacc[i], gh, gl, uh, ul);
                    else mma_x3(dacc[i], gh, gl, wt_lds(0, ks), wt_lds(1, ks));
                }
            lds_barrier();      // nobody reads the dst and hs planes any more
#pragma unroll
            for (int i = 0; i < DD::RTW; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) s_dhs[((dwr * DD::RTW + i) * 16 + q * 4 + e) * DD::LDY + dwc * 16 + r] = dacc[i][e] + 0.f;
        }
        lds_barrier();
        // dhs = dst Wd + ghs in the stand-alone kernel's store-phase expression; the thread-to-entry map and the column sums are
        // those of hs_linear's backward loading dhs from memory
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int f = tid + u * P::NT;
            const int row = f / 16, c4 = (f % 16) * 4;
            float4 v = ld4(s_dhs + row * DD::LDY + c4);
            if (a.gHS) v = add4(v, f4x(pb[u]));
            dbl = add4(dbl, v);
            bf16x4 hi, lo;
            split4(v, hi, lo);
            st_bf4(e_hi + row * WL::LDG + c4, hi); st_bf4(e_lo + row * WL::LDG + c4, lo);
        }
        lds_barrier();          // the staged dhs is read; the s|t planes take its place
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int f = tid + u * P::NT;
            const int row = f / 32, c4 = (f % 32) * 4;
            bf16x4 hi, lo;
            split4(f4x(pa[u]), hi, lo);
            st_bf4(x_hi + row * WL::LDX + c4, hi); st_bf4(x_lo + row * WL::LDX + c4, lo);
        }
        lds_barrier();
        if (tile + gridDim.x < ntiles) fetch_gh(tile + gridDim.x);
        // dWl += dhs^T [s|t]
#pragma unroll
        for (int ks = 0; ks < kTileRows / 32; ++ks) {
            bf16x8 bh[2], bl[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                bh[j] = ldfrag_tr2(x_hi, WL::LDX, 32 * ks, (jt0l + j) * 16);
                bl[j] = ldfrag_tr2(x_lo, WL::LDX, 32 * ks, (jt0l + j) * 16);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const bf16x8 ah = ldfrag_tr2(e_hi, WL::LDG, 32 * ks, (it0l + i) * 16), al = ldfrag_tr2(e_lo, WL::LDG, 32 * ks, (it0l + i) * 16);
#pragma unroll
                for (int j = 0; j < 2; ++j) mma_x3(accl[i][j], ah, al, bh[j], bl[j]);
            }
        }
        {   // ds|dt = dhs Wl, as the DX phase of hs_linear's backward forms it
            f32x4 dacc[DL::RTW];
#pragma unroll
            for (int i = 0; i < DL::RTW; ++i) dacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < DL::KS; ++ks)
#pragma unroll
                for (int i = 0; i < DL::RTW; ++i) {
                    const int off = (i * 16 + r) * WL::LDG + 32 * ks + 8 * q;
                    mma_x3(dacc[i], ldfrag(e_hi + off), ldfrag(e_lo + off), th[ks], tl[ks]);
                }
            lds_barrier();      // nobody reads the s|t planes any more
#pragma unroll
            for (int i = 0; i < DL::RTW; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) s_dx[(i * 16 + q * 4 + e) * DL::LDY + w * 16 + r] = dacc[i][e] + 0.f;
        }
        lds_barrier();
#pragma unroll
        for (int u = 0; u < DL::PF; ++u) {
            const int f = tid + u * P::NT;
            const int row = f / 32, c4 = (f % 32) * 4;
            if (first + row < a.N) {
                const float4 v = ld4(s_dx + row * DL::LDY + c4);
                if (c4 < 64) st4(a.dS + (first + row) * a.ldds + c4, v);
                else st4(a.dT + (first + row) * a.lddt + (c4 - 64), v);
            }
        }
        lds_barrier();          // the next tile's dst planes overwrite the staged rows
    }
    // per-workgroup partials to this workgroup's slab rows (plain stores); k_slab_sum adds the rows in a fixed order
    float* sl = a.slab_l + (int64_t)blockIdx.x * P::slab_l;
    float* sd = a.slab_d + (int64_t)blockIdx.x * P::slab_d;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sl[((it0l + i) * 16 + q * 4 + e) * 128 + (jt0l + j) * 16 + r] = accl[i][j][e];
                sd[((it0d + i) * 16 + q * 4 + e) * 64 + (jt0d + j) * 16 + r] = accd[i][j][e];
            }
    // column sums: one float4 per thread into R1, then a fixed-order sum over the threads of a column quad (the stand-alone order)
    float4* s_part = reinterpret_cast<float4*>(smem_raw);
    s_part[tid] = dbl; s_part[P::NT + tid] = dbd;
    __syncthreads();
    if (a.want_dbl && tid < 64) {
        const int c4 = tid / 4, e = tid % 4;
        float sum = 0.f;
        for (int t = c4; t < P::NT; t += 16) { const float4 v = s_part[t]; sum += e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
        sl[64 * 128 + tid] = sum;
    }
    if (a.want_dbd && tid < 128) {
        const int c4 = tid / 4, e = tid % 4;
        float sum = 0.f;
        for (int t = c4; t < P::NT; t += 32) { const float4 v = s_part[P::NT + t]; sum += e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
        sd[128 * 64 + tid] = sum;
    }
}

inline int pair_bwd_grid(int64_t N) {      // the grid of hs_linear's backward (two workgroups of 8 waves per CU)
    return grid_for((N + kTileRows - 1) / kTileRows, 2);
}

}  // namespace mgv

extern "C" int mgv_linear_pair_fwd_x3(int64_t N, const float* S, int lds, const float* T, int ldt, const void* wlpack_bf16, const float* bl,
                                      const void* wdpack_bf16, const float* bd, float* HS, int ldhs, float* ST, int ldst, void* stream) {
    MGV_CHECK_ARG(N >= 0 && S && T && wlpack_bf16 && wdpack_bf16 && HS && ST);
    MGV_CHECK_ARG(lds >= 64 && lds % 4 == 0 && ldt >= 64 && ldt % 4 == 0 && ldhs >= 64 && ldhs % 4 == 0 && ldst >= 128 && ldst % 4 == 0);
    if (N == 0) return MGV_OK;
    mgv::LinPairArgs a{};
    a.N = N; a.S = S; a.lds = lds; a.T = T; a.ldt = ldt; a.wl = static_cast<const __bf16*>(wlpack_bf16); a.bl = bl;
    a.wd = static_cast<const __bf16*>(wdpack_bf16); a.bd = bd; a.HS = HS; a.ldhs = ldhs; a.ST = ST; a.ldst = ldst;
    using P = mgv::PairFwdGeom;
    mgv::allow_lds<mgv::k_linear_pair_fwd_x3>();
    const int grid = mgv::grid_for((N + mgv::kTileRows - 1) / mgv::kTileRows, 2);      // 16 waves per CU
    hipLaunchKernelGGL(mgv::k_linear_pair_fwd_x3, dim3(grid), dim3(P::NT), P::smem_bytes, static_cast<hipStream_t>(stream), a);
    MGV_LAUNCH_RET();
}

// floats of workspace mgv_linear_pair_bwd_x3 needs: per workgroup one row of (dWl, dbl) and one of (dWd, dbd) partials
extern "C" int mgv_linear_pair_bwd_x3_ws_floats(int64_t N) {
    if (N < 0) return 0;
    return mgv::pair_bwd_grid(N) * (mgv::PairBwdGeom::slab_l + mgv::PairBwdGeom::slab_d);
}

extern "C" int mgv_linear_pair_bwd_x3(int64_t N, const float* dST, int lddst, const float* gHS, int ldghs, const float* HS, int ldhs,
                                      const float* S, int lds, const float* T, int ldt, const void* wltpack_bf16, const void* wdtpack_bf16,
                                      float* dS, int ldds, float* dT, int lddt, float* dWl, float* dbl, float* dWd, float* dbd,
                                      float* workspace, int64_t workspace_floats, void* stream) {
    MGV_CHECK_ARG(N >= 0 && dST && HS && S && T && wltpack_bf16 && wdtpack_bf16 && dS && dT && dWl && dWd);
    MGV_CHECK_ARG(lddst >= 128 && lddst % 4 == 0 && (gHS == nullptr || (ldghs >= 64 && ldghs % 4 == 0)) && ldhs >= 64 && ldhs % 4 == 0);
    MGV_CHECK_ARG(lds >= 64 && lds % 4 == 0 && ldt >= 64 && ldt % 4 == 0 && ldds >= 64 && ldds % 4 == 0 && lddt >= 64 && lddt % 4 == 0);
    if (N == 0) return MGV_OK;
    using P = mgv::PairBwdGeom;
    const int grid = mgv::pair_bwd_grid(N);
    if (workspace == nullptr || workspace_floats < (int64_t)grid * (P::slab_l + P::slab_d)) return MGV_EINVAL;
    mgv::LinPairArgs a{};
    a.N = N; a.dST = dST; a.lddst = lddst; a.gHS = gHS; a.ldghs = ldghs; a.hs = HS; a.ldh = ldhs; a.S = S; a.lds = lds; a.T = T; a.ldt = ldt;
    a.wl = static_cast<const __bf16*>(wltpack_bf16); a.wd = static_cast<const __bf16*>(wdtpack_bf16);
    a.dS = dS; a.ldds = ldds; a.dT = dT; a.lddt = lddt;
    a.slab_l = workspace; a.slab_d = workspace + (int64_t)grid * P::slab_l; a.want_dbl = dbl != nullptr; a.want_dbd = dbd != nullptr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    mgv::allow_lds<mgv::k_linear_pair_bwd_x3>();
    hipLaunchKernelGGL(mgv::k_linear_pair_bwd_x3, dim3(grid), dim3(P::NT), P::smem_bytes, st, a);
    mgv::launch_slab_sum<float, float>(a.slab_l, grid, P::slab_l, 64 * 128, dWl, st);
    if (dbl) mgv::launch_slab_sum<float, float>(a.slab_l + 64 * 128, grid, P::slab_l, 64, dbl, st);
    mgv::launch_slab_sum<float, float>(a.slab_d, grid, P::slab_d, 128 * 64, dWd, st);
    if (dbd) mgv::launch_slab_sum<float, float>(a.slab_d + 128 * 64, grid, P::slab_d, 128, dbd, st);
    MGV_LAUNCH_RET();
}

extern "C" int mgv_linear_x3_supported(int M, int K) {
    return (M == 64 && K == 128) || (M == 128 && K == 64) || (M == 64 && K == 64) || (M == 64 && K == 32) || (M == 32 && K == 64) ||
           (M == 32 && K == 32);
}

static int linear_fwd_x3_impl(int64_t N, const float* X1, int K1, int ld1, const float* X2, int K2, int ld2, const void* wpack_bf16,
                              const float* b, int M, const float* R, int ldr, float* Y, int ldy, void* stream) {
    MGV_CHECK_ARG(N >= 0 && X1 && wpack_bf16 && Y && K1 > 0 && K2 >= 0 && (K2 == 0 || X2));
    MGV_CHECK_ARG(K1 % 4 == 0 && K2 % 4 == 0 && ld1 >= K1 && ld1 % 4 == 0 && (K2 == 0 || (ld2 >= K2 && ld2 % 4 == 0)) && ldy >= M && ldy % 4 == 0);
    MGV_CHECK_ARG(R == nullptr || (ldr >= M && ldr % 4 == 0));
    if (N == 0) return MGV_OK;
    mgv::LinX3Args a{};
    a.N = N; a.X1 = X1; a.K1 = K1; a.ld1 = ld1; a.X2 = X2; a.K2 = K2; a.ld2 = ld2; a.wpack = static_cast<const __bf16*>(wpack_bf16);
    a.b = b; a.Y = Y; a.ldy = ldy; a.R = R; a.ldr = ldr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int K = K1 + K2;
#define MGV_LF(MM, KK) if (M == MM && K == KK) return mgv::launch_linear_fwd_x3<MM, KK>(a, st);
    MGV_LF(64, 128) MGV_LF(128, 64) MGV_LF(64, 64) MGV_LF(64, 32) MGV_LF(32, 64) MGV_LF(32, 32)
#undef MGV_LF
    return MGV_EUNSUPPORTED;
}

extern "C" int mgv_linear_fwd_x3(int64_t N, const float* X1, int K1, int ld1, const float* X2, int K2, int ld2,
                                 const void* wpack_bf16, const float* b, int M, float* Y, int ldy, void* stream) {
    return linear_fwd_x3_impl(N, X1, K1, ld1, X2, K2, ld2, wpack_bf16, b, M, nullptr, 0, Y, ldy, stream);
}

extern "C" int mgv_linear_fwd_x3_res(int64_t N, const float* X1, int K1, int ld1, const float* X2, int K2, int ld2,
                                     const void* wpack_bf16, const float* b, int M, const float* R, int ldr, float* Y, int ldy,
                                     void* stream) {
    MGV_CHECK_ARG(R != nullptr);
    return linear_fwd_x3_impl(N, X1, K1, ld1, X2, K2, ld2, wpack_bf16, b, M, R, ldr, Y, ldy, stream);
}

// floats of workspace mgv_linear_wgrad_x3 needs: one row of M*K + M partials per workgroup (at most 4 workgroups per CU)
extern "C" int mgv_linear_wgrad_x3_ws_floats(int M, int K, int64_t N) {
    if (M <= 0 || K <= 0 || N < 0) return 0;
    const int64_t ntiles = (N + mgv::kTileRows - 1) / mgv::kTileRows;
    return mgv::grid_for(ntiles, 4) * (M * K + M);
}

extern "C" int mgv_linear_wgrad_x3(int64_t N, const float* X1, int K1, int ld1, const float* X2, int K2, int ld2,
                                   const float* dY, int lddy, int M, float* dW, float* db, float* workspace,
                                   int64_t workspace_floats, void* stream) {
    MGV_CHECK_ARG(N >= 0 && X1 && dY && dW && K1 > 0 && K2 >= 0 && (K2 == 0 || X2));
    MGV_CHECK_ARG(K1 % 4 == 0 && K2 % 4 == 0 && ld1 >= K1 && ld1 % 4 == 0 && (K2 == 0 || (ld2 >= K2 && ld2 % 4 == 0)) && lddy % 4 == 0 && lddy >= M);
    if (N == 0) return MGV_OK;
    mgv::LinX3Args a{};
    a.N = N; a.X1 = X1; a.K1 = K1; a.ld1 = ld1; a.X2 = X2; a.K2 = K2; a.ld2 = ld2; a.dY = dY; a.lddy = lddy; a.dW = dW; a.db = db; a.slab = workspace;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int K = K1 + K2;
#define MGV_WGX(MM, KK, NW, WI) if (M == MM && K == KK) return mgv::launch_linear_wgrad_x3<MM, KK, NW, WI>(a, workspace_floats, st);
    MGV_WGX(64, 128, 8, 2) MGV_WGX(128, 64, 8, 4) MGV_WGX(64, 64, 8, 2) MGV_WGX(64, 32, 8, 4) MGV_WGX(32, 64, 8, 2) MGV_WGX(32, 32, 4, 2)
#undef MGV_WGX
    return MGV_EUNSUPPORTED;
}

extern "C" int mgv_linear_bwd_x3_supported(int M, int K) { return (M == 64 && K == 128) || (M == 128 && K == 64) || (M == 64 && K == 64); }

extern "C" int mgv_linear_bwd_x3(int64_t N, const float* X1, int K1, int ld1, const float* X2, int K2, int ld2, const float* dY, int lddy,
                                 int M, const void* wtpack_bf16, float* dW, float* db, float* dX1, int ldx1, float* dX2, int ldx2,
                                 const float* R, int ldr, float* workspace, int64_t workspace_floats, void* stream) {
    if (!mgv_linear_bwd_x3_supported(M, K1 + K2)) return MGV_EUNSUPPORTED;
    MGV_CHECK_ARG(N >= 0 && X1 && dY && dW && wtpack_bf16 && dX1 && K1 > 0 && K2 >= 0 && (K2 == 0) == (X2 == nullptr) && (X2 == nullptr) == (dX2 == nullptr));
    MGV_CHECK_ARG(K1 % 4 == 0 && K2 % 4 == 0 && ld1 >= K1 && ld1 % 4 == 0 && (K2 == 0 || (ld2 >= K2 && ld2 % 4 == 0)) && lddy % 4 == 0 && lddy >= M);
    MGV_CHECK_ARG(ldx1 >= K1 && ldx1 % 4 == 0 && (K2 == 0 || (ldx2 >= K2 && ldx2 % 4 == 0)) && (R == nullptr || (ldr >= K1 && ldr % 4 == 0)));
    if (N == 0) return MGV_OK;
    mgv::LinX3Args a{};
    a.N = N; a.X1 = X1; a.K1 = K1; a.ld1 = ld1; a.X2 = X2; a.K2 = K2; a.ld2 = ld2; a.dY = dY; a.lddy = lddy; a.dW = dW; a.db = db; a.slab = workspace;
    a.wpack = static_cast<const __bf16*>(wtpack_bf16); a.Y = dX1; a.ldy = ldx1; a.Y2 = dX2; a.ldy2 = ldx2; a.R = R; a.ldr = ldr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int K = K1 + K2;
    if (M == 64 && K == 128) return mgv::launch_linear_bwd_x3<64, 128, 8, 2, 2>(a, workspace_floats, st);
    if (M == 128 && K == 64) return mgv::launch_linear_bwd_x3<128, 64, 8, 4, 1>(a, workspace_floats, st);
    return mgv::launch_linear_bwd_x3<64, 64, 8, 2, 2>(a, workspace_floats, st);
}

extern "C" int mgv_wpack_bf16x3(const float* W, int R, int K, int ldw, int transpose, void* hi, void* lo, void* stream) {
    MGV_CHECK_ARG(W && hi && lo && R > 0 && K > 0 && R % 16 == 0 && K % 32 == 0 && ldw >= (transpose ? R : K));
    const int total = R * K;
    hipLaunchKernelGGL(mgv::k_wpack_bf16x3, dim3((total + 255) / 256 > 1024 ? 1024 : (total + 255) / 256), dim3(256), 0,
                       static_cast<hipStream_t>(stream), W, R, K, ldw, transpose, static_cast<__bf16*>(hi), static_cast<__bf16*>(lo));
    MGV_LAUNCH_RET();
}

/* ---- grouped Linear over the level sweep's tiles (num_rounds > 1: gh = W_hh[slot] h_prev + b_hh[slot] per updated gate with its OWN
 * aggregator's GRU weights, dg_ae_model_aig.py:88-94; one launch instead of an index_select / three Linears / index_copy per gate type).
 * H = 64 shapes: (M, K) = (192, 64) forward, (64, 192) input gradient, (192, 64) weight gradient of ONE slot's tile list. */
extern "C" int mgv_grouped_linear_supported(int M, int K) { return (M == 192 && K == 64) || (M == 64 && K == 192); }

extern "C" int mgv_grouped_linear_fwd_x3(int64_t ntiles, const int32_t* tile_list, const int32_t* order, const int32_t* tile_start,
                                         const int32_t* tile_count, const int32_t* tile_slot, const float* X, int K, int ldx,
                                         const void* wpack_bf16, const float* b, int M, const float* R, int ldr, float* Y, int ldy, void* stream) {
    MGV_CHECK_ARG(ntiles >= 0 && order && tile_start && tile_count && tile_slot && X && wpack_bf16 && Y);
    MGV_CHECK_ARG(K % 4 == 0 && ldx >= K && ldx % 4 == 0 && ldy >= M && ldy % 4 == 0 && (R == nullptr || (ldr >= M && ldr % 4 == 0)));
    if (ntiles == 0) return MGV_OK;
    mgv::LinX3Args a{};
    a.N = 0; a.X1 = X; a.K1 = K; a.ld1 = ldx; a.wpack = static_cast<const __bf16*>(wpack_bf16); a.b = b; a.Y = Y; a.ldy = ldy; a.R = R; a.ldr = ldr;
    a.order = order; a.tile_start = tile_start; a.tile_count = tile_count; a.tile_slot = tile_slot; a.tile_list = tile_list;
    a.g_ntiles = ntiles; a.g_wstride = (int64_t)2 * M * K;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (M == 192 && K == 64) return mgv::launch_linear_fwd_x3<192, 64, true>(a, st);
    if (M == 64 && K == 192) return mgv::launch_linear_fwd_x3<64, 192, true>(a, st);
    return MGV_EUNSUPPORTED;
}

extern "C" int mgv_grouped_linear_wgrad_x3_ws_floats(int M, int K, int64_t ntiles) {
    if (M <= 0 || K <= 0 || ntiles < 0) return 0;
    return mgv::grid_for(ntiles, 4) * (M * K + M);
}

extern "C" int mgv_grouped_linear_wgrad_x3(int64_t ntiles, const int32_t* tile_list, const int32_t* order, const int32_t* tile_start,
                                           const int32_t* tile_count, const float* X, int K, int ldx, const float* dY, int lddy, int M,
                                           float* dW, float* db, float* workspace, int64_t workspace_floats, void* stream) {
    MGV_CHECK_ARG(ntiles >= 0 && order && tile_start && tile_count && X && dY && dW && K % 4 == 0 && ldx >= K && ldx % 4 == 0 && lddy % 4 == 0 && lddy >= M);
    if (ntiles == 0) return MGV_OK;
    mgv::LinX3Args a{};
    a.N = 0; a.X1 = X; a.K1 = K; a.ld1 = ldx; a.dY = dY; a.lddy = lddy; a.dW = dW; a.db = db; a.slab = workspace;
    a.order = order; a.tile_start = tile_start; a.tile_count = tile_count; a.tile_list = tile_list; a.g_ntiles = ntiles;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (M == 192 && K == 64) return mgv::launch_linear_wgrad_x3<192, 64, 6, 3, true>(a, workspace_floats, st);
    return MGV_EUNSUPPORTED;
}
