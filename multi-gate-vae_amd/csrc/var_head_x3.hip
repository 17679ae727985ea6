// The variational link heads as ONE pass over st = hs_decompose(hs), forward and backward (digvae_model.py:134-142, trainer.py:145-148):
// per column half h of st (s = st[:, :H], t = st[:, H:]) the two Linears fc_h_mu / fc_h_logstd are one (2H, H) bf16x3 product
// P = X_h Wp_h^T + bp_h = [mu | logstd] (the tuned (128, 64) shape of linear_x3.hip at H = 64), then z = mu + exp(logstd) eps and the
// KL terms 1 + 2 logstd - mu^2 - exp(logstd)^2 while the tile is still in LDS.  The backward recomputes P and eps from st and the seed
// (nothing but st is kept from the forward), forms dP = [dmu | dlogstd] in LDS and does what k_linear_bwd_x3 does with a dY it was
// handed: dWp += dP^T X, dbp += colsum(dP), dX = dP Wp in the same pass.  Chained, the same function is four Linear launches, two
// reparameterisation launches and their six backwards with mu, logstd and eps held in between.
// Workgroup b serves half b & 1 and walks the tiles b >> 1, b >> 1 + gridDim / 2, ...: its weight fragments stay in registers for the
// whole launch, and every row of st is read once.  Sums across workgroups go through slab rows added in a fixed order (mgv_slab.h).
#include "mgv_x3.h"
#include "mgv_launch.h"
#include "mgv_slab.h"
#include "mgv_gauss.h"
#include "../../include/mgvae_hip.h"

namespace mgv {

struct VarHeadArgs {
    int64_t N;
    const float* ST; int ldst;
    const __bf16* wpack[2];     // per half: [2][2H*H] = Wp_hi, Wp_lo in fragment order (rows: fc_mu.weight, then fc_logstd.weight)
    const __bf16* wtpack[2];    // backward: the transposed packs ([H x 2H] view)
    const float* b[2];          // per half: [2H] = fc_mu.bias, fc_logstd.bias
    const float* eps; int ldeps;
    uint64_t seed; int sample;
    float* Z; int ldz;
    float* ML; int ldml;
    double* klslab;             // forward: [gridDim / 2][2] per-workgroup KL sums
    const float* gZ; int ldg;
    const float* gkl;
    float* dST; int lddst;
    float* slab;                // backward: [gridDim / 2][2][2H*H + 2H] per-workgroup partials (dWp row-major, then dbp)
};

__device__ __forceinline__ float4 vh_f4(const f32x4& v) { return make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ float vh_get(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// eps of elements (node, c4 .. c4 + 3) of half `half`: the given rows [eps_s | eps_t], or the generator at element node * H + c
template <int H>
__device__ __forceinline__ float4 vh_eps(const VarHeadArgs& a, int half, int64_t node, int c4) {
    if (a.eps) return ld4(a.eps + node * a.ldeps + half * H + c4);
    const uint64_t i = (uint64_t)node * H + c4, sd = a.seed + (uint64_t)half;
    return make_float4(gauss_from_counter(sd, i), gauss_from_counter(sd, i + 1), gauss_from_counter(sd, i + 2), gauss_from_counter(sd, i + 3));
}

// ---------------------------------------------------------------------------------------------- forward
template <int H>
struct VarFwdGeom {
    static constexpr int M = 2 * H, K = H;
    static constexpr int HC = M / 16, WPC = 4, HCW = HC / WPC, RTW = 4;       // 4 waves across the column tiles, all four row tiles each
    static constexpr int KS = K / 32;
    static constexpr int LDP = K + 8;
    static constexpr int PB = kTileRows * LDP * 2;
    static constexpr int LDY = M + 4;
    static constexpr int o_y = 2 * PB;
    static constexpr int o_red = o_y + kTileRows * LDY * 4;
    static constexpr int smem_bytes = o_red + kThreads * 8;
    static constexpr int PF = kTileRows * K / 4 / kThreads;                   // float4 per thread and tile
    static constexpr int per_cu = 160 * 1024 / smem_bytes > 4 ? 4 : 160 * 1024 / smem_bytes;
    static_assert(PF * kThreads * 4 == kTileRows * K && HCW * WPC == HC && o_red % 8 == 0, "tile must split over the threads");
};

template <int H>
__global__ __launch_bounds__(kThreads) void k_var_head_fwd_x3(VarHeadArgs a) {
    using G = VarFwdGeom<H>;
    constexpr int M = G::M, K = G::K;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __bf16* x_hi = reinterpret_cast<__bf16*>(smem_raw);
    __bf16* x_lo = reinterpret_cast<__bf16*>(smem_raw + G::PB);
    float* s_y = reinterpret_cast<float*>(smem_raw + G::o_y);
    double* s_red = reinterpret_cast<double*>(smem_raw + G::o_red);
    const int tid = threadIdx.x, lane = tid & 63, wc = tid >> 6, r = lane & 15, q = lane >> 4;
    const int half = blockIdx.x & 1, wgi = blockIdx.x >> 1, nwg = gridDim.x >> 1;
    const float* X = a.ST + half * H;
    bf16x8 wh[G::HCW][G::KS], wl[G::HCW][G::KS];
    float bias[G::HCW];
#pragma unroll
    for (int j = 0; j < G::HCW; ++j) {
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks) {
            const int wo = (((wc * G::HCW + j) * G::KS) + ks) * 512 + lane * 8;
            wh[j][ks] = ldfrag(a.wpack[half] + wo); wl[j][ks] = ldfrag(a.wpack[half] + M * K + wo);
        }
        bias[j] = a.b[half][(wc * G::HCW + j) * 16 + r];
    }
    const int64_t ntiles = (a.N + kTileRows - 1) / kTileRows;
    f32x4 pf[G::PF];
    auto prefetch = [&](int64_t tile) {
        const int64_t first = tile * kTileRows;
#pragma unroll
        for (int u = 0; u < G::PF; ++u) {
            const int f = tid + u * kThreads;
            const int row = f / (K / 4), c4 = (f % (K / 4)) * 4;
            if (first + row < a.N) pf[u] = *reinterpret_cast<const f32x4*>(X + (first + row) * a.ldst + c4);
            else pf[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    double kl = 0;
    int64_t tile = wgi;
    if (tile < ntiles) prefetch(tile);
    for (; tile < ntiles; tile += nwg) {
        const int64_t first = tile * kTileRows;
#pragma unroll
        for (int u = 0; u < G::PF; ++u) {
            const int f = tid + u * kThreads;
            const int row = f / (K / 4), c4 = (f % (K / 4)) * 4;
            bf16x4 hi, lo;
            split4(vh_f4(pf[u]), hi, lo);
            st_bf4(x_hi + row * G::LDP + c4, hi); st_bf4(x_lo + row * G::LDP + c4, lo);
        }
        lds_barrier();
        if (tile + nwg < ntiles) prefetch(tile + nwg);
        // P = X Wp^T + bp as k_linear_fwd_x3 forms it at (2H, H): ks ascending, mma_x3, zero-initialised accumulators
        f32x4 acc[G::RTW][G::HCW];
#pragma unroll
        for (int i = 0; i < G::RTW; ++i)
#pragma unroll
            for (int j = 0; j < G::HCW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks)
#pragma unroll
            for (int i = 0; i < G::RTW; ++i) {
                const int off = (i * 16 + r) * G::LDP + 32 * ks + 8 * q;
                const bf16x8 xh = ldfrag(x_hi + off), xl = ldfrag(x_lo + off);
#pragma unroll
                for (int j = 0; j < G::HCW; ++j) mma_x3(acc[i][j], xh, xl, wh[j][ks], wl[j][ks]);
            }
#pragma unroll
        for (int i = 0; i < G::RTW; ++i)
#pragma unroll
            for (int j = 0; j < G::HCW; ++j) {
                const int col = (wc * G::HCW + j) * 16 + r;
#pragma unroll
                for (int e = 0; e < 4; ++e) s_y[(i * 16 + q * 4 + e) * G::LDY + col] = acc[i][j][e] + bias[j];
            }
        lds_barrier();
        // the head: one column quad of (mu, logstd) per thread and step
        for (int i = tid; i < kTileRows * (H / 4); i += kThreads) {
            const int row = i / (H / 4), c4 = (i % (H / 4)) * 4;
            const int64_t node = first + row;
            if (node < a.N) {
                const float4 mu = ld4(s_y + row * G::LDY + c4), ls = ld4(s_y + row * G::LDY + H + c4);
                const float4 sd = make_float4(expf(ls.x), expf(ls.y), expf(ls.z), expf(ls.w));
                float4 z = mu;
                if (a.sample) {
                    const float4 e = vh_eps<H>(a, half, node, c4);
                    z = make_float4(mu.x + sd.x * e.x, mu.y + sd.y * e.y, mu.z + sd.z * e.z, mu.w + sd.w * e.w);
                }
                st4(a.Z + node * a.ldz + half * H + c4, z);
                if (a.ML) {
                    st4(a.ML + node * a.ldml + half * M + c4, mu);
                    st4(a.ML + node * a.ldml + half * M + H + c4, ls);
                }
                kl += (double)(1.0f + 2.0f * ls.x - mu.x * mu.x - sd.x * sd.x);
                kl += (double)(1.0f + 2.0f * ls.y - mu.y * mu.y - sd.y * sd.y);
                kl += (double)(1.0f + 2.0f * ls.z - mu.z * mu.z - sd.z * sd.z);
                kl += (double)(1.0f + 2.0f * ls.w - mu.w * mu.w - sd.w * sd.w);
            }
        }
        // the planes are rewritten only after this barrier pair; s_y only after the next tile's first barrier
    }
    // this workgroup's KL sum: the threads' sums added in thread order, a plain store to its slab row
    s_red[tid] = kl;
    __syncthreads();
    if (tid == 0) {
        double s = 0;
        for (int t = 0; t < kThreads; ++t) s += s_red[t];
        a.klslab[(int64_t)wgi * 2 + half] = s;
    }
}

// klsum[h] = the slab rows of half h added in index order (OVERWRITES: the forward's sums are not accumulated across calls)
__global__ __launch_bounds__(64) void k_var_head_klsum(const double* slab, int nwg, double* klsum) {
    const int h = threadIdx.x;
    if (h < 2) {
        double s = 0;
        for (int g = 0; g < nwg; ++g) s += slab[(int64_t)g * 2 + h];
        klsum[h] = s;
    }
}

// ---------------------------------------------------------------------------------------------- backward
// 8 waves.  Per tile: X planes -> P (forward product, 4 x 2 waves) -> dP planes -> dWp += dP^T X (transposed reads of both planes,
// WI x WJ waves over the (2H/16) x (H/16) output tiles) -> dX = dP Wp (one column tile per wave) staged over the X planes.
template <int H>
struct VarBwdGeom {
    static constexpr int M = 2 * H, K = H, NW = 8, NT = 64 * NW;
    // forward product
    static constexpr int FHC = M / 16, FWPC = 4, FWPR = NW / FWPC, FRTW = 4 / FWPR, FHCW = FHC / FWPC, FKS = K / 32;
    // weight gradient
    static constexpr int TI = M / 16, TJ = K / 16, WI = 4, WJ = NW / WI;
    static constexpr int ITW = TI / WI, JTW = TJ / WJ;
    static_assert(ITW * WI == TI && JTW * WJ == TJ && FHCW * FWPC == FHC, "wave grids must tile the outputs");
    // input gradient: K-steps over the 2H columns of dP
    static constexpr int DKS = M / 32, DWPC = K / 16, DWPR = NW / DWPC, DRTW = 4 / DWPR;
    static_assert(DWPC * DWPR == NW && DRTW * DWPR == 4, "one column tile per wave");
    static constexpr int KSR = 1, KSL = DKS - KSR;                // transposed weight k-steps in registers / in LDS
    static constexpr int WTL = (K / 16) * KSL * 512;              // elements per plane in LDS
    static constexpr int LDG = M + 8, LDX = K + 8;
    static constexpr int GPB = kTileRows * LDG * 2, XPB = kTileRows * LDX * 2;
    static constexpr int LDPF = M + 4;                            // fp32 P rows, staged over the dP planes
    static_assert(kTileRows * LDPF * 4 <= 2 * GPB, "P must fit the dP planes");
    static constexpr int LDY = K + 4;                             // fp32 dX rows, staged over the X planes
    static_assert(kTileRows * LDY * 4 <= 2 * XPB, "dX must fit the X planes");
    static_assert(NT * 32 <= 2 * GPB, "the column-sum partials must fit the dP planes");
    static constexpr int PFX = kTileRows * K / 4 / NT;            // float4 of X (and of gZ, and quads of the head) per thread and tile
    static_assert(PFX * NT * 4 == kTileRows * K && NT % (K / 4) == 0, "a thread keeps its column quad across its rows");
    static constexpr int o_x = 2 * GPB, o_wt = o_x + 2 * XPB;
    static constexpr int smem_bytes = o_wt + 2 * WTL * 2;
    // resident workgroups per CU: the LDS would hold two at either width, the registers do not at H = 64 (216 VGPRs x 8 waves)
    static constexpr int per_cu = H == 64 ? 1 : 2;
    static_assert(per_cu * smem_bytes <= 160 * 1024, "LDS of the resident workgroups");
    static constexpr int slab_row = M * K + M;
};

template <int H>
__global__ __launch_bounds__(512) void k_var_head_bwd_x3(VarHeadArgs a) {
    using G = VarBwdGeom<H>;
    constexpr int M = G::M, K = G::K;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __bf16* g_hi = reinterpret_cast<__bf16*>(smem_raw);
    __bf16* g_lo = reinterpret_cast<__bf16*>(smem_raw + G::GPB);
    float* s_p = reinterpret_cast<float*>(smem_raw);                        // P, before the dP planes are written
    __bf16* x_hi = reinterpret_cast<__bf16*>(smem_raw + G::o_x);
    __bf16* x_lo = reinterpret_cast<__bf16*>(smem_raw + G::o_x + G::XPB);
    float* s_y = reinterpret_cast<float*>(smem_raw + G::o_x);               // dX, after the X planes are dead
    __bf16* s_wt = reinterpret_cast<__bf16*>(smem_raw + G::o_wt);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
    const int half = blockIdx.x & 1, wgi = blockIdx.x >> 1, nwg = gridDim.x >> 1;
    const float* X = a.ST + half * H;
    const float gk = a.gkl ? a.gkl[half] : 0.f;
    const bool want_eps = a.sample && a.gZ;
    // forward weight fragments of this wave's column tiles
    const int fwc = w % G::FWPC, fwr = w / G::FWPC;
    bf16x8 wh[G::FHCW][G::FKS], wl[G::FHCW][G::FKS];
    float bias[G::FHCW];
#pragma unroll
    for (int j = 0; j < G::FHCW; ++j) {
#pragma unroll
        for (int ks = 0; ks < G::FKS; ++ks) {
            const int wo = (((fwc * G::FHCW + j) * G::FKS) + ks) * 512 + lane * 8;
            wh[j][ks] = ldfrag(a.wpack[half] + wo); wl[j][ks] = ldfrag(a.wpack[half] + M * K + wo);
        }
        bias[j] = a.b[half][(fwc * G::FHCW + j) * 16 + r];
    }
    // transposed weight fragments of this wave's dX column tile: k-steps < KSR in registers, the others in LDS
    const int dwc = w % G::DWPC, dwr = w / G::DWPC;
    bf16x8 th[G::KSR], tl[G::KSR];
#pragma unroll
    for (int ks = 0; ks < G::KSR; ++ks) {
        const int wo = (dwc * G::DKS + ks) * 512 + lane * 8;
        th[ks] = ldfrag(a.wtpack[half] + wo); tl[ks] = ldfrag(a.wtpack[half] + M * K + wo);
    }
    for (int c = tid; c < 2 * G::WTL / 8; c += G::NT) {                     // (the first tile barrier publishes it)
        const int plane = c / (G::WTL / 8), blk = (c % (G::WTL / 8)) / 64, ct = blk / G::KSL, ks = G::KSR + blk % G::KSL;
        *reinterpret_cast<bf16x8*>(s_wt + c * 8) = ldfrag(a.wtpack[half] + plane * M * K + (ct * G::DKS + ks) * 512 + (c % 64) * 8);
    }
    auto wt_lds = [&](int plane, int ks) { return ldfrag(s_wt + plane * G::WTL + (dwc * G::KSL + ks - G::KSR) * 512 + lane * 8); };
    const int it0 = (w / G::WJ) * G::ITW, jt0 = (w % G::WJ) * G::JTW;
    f32x4 acc[G::ITW][G::JTW];
#pragma unroll
    for (int i = 0; i < G::ITW; ++i)
#pragma unroll
        for (int j = 0; j < G::JTW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 db_mu = zero4(), db_ls = zero4();       // column sums of dP over this thread's rows (its column quad is fixed)
    const int64_t ntiles = (a.N + kTileRows - 1) / kTileRows;
    f32x4 px[G::PFX], pg[G::PFX];
    auto prefetch_x = [&](int64_t tile) {
        const int64_t first = tile * kTileRows;
#pragma unroll
        for (int u = 0; u < G::PFX; ++u) {
            const int f = tid + u * G::NT;
            const int row = f / (K / 4), c4 = (f % (K / 4)) * 4;
            if (first + row < a.N) px[u] = *reinterpret_cast<const f32x4*>(X + (first + row) * a.ldst + c4);
            else px[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto prefetch_g = [&](int64_t tile) {
        const int64_t first = tile * kTileRows;
#pragma unroll
        for (int u = 0; u < G::PFX; ++u) {
            const int f = tid + u * G::NT;
            const int row = f / (K / 4), c4 = (f % (K / 4)) * 4;
            if (a.gZ && first + row < a.N) pg[u] = *reinterpret_cast<const f32x4*>(a.gZ + (first + row) * a.ldg + half * H + c4);
            else pg[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    int64_t tile = wgi;
    if (tile < ntiles) { prefetch_x(tile); prefetch_g(tile); }
    for (; tile < ntiles; tile += nwg) {
        const int64_t first = tile * kTileRows;
#pragma unroll
        for (int u = 0; u < G::PFX; ++u) {
            const int f = tid + u * G::NT;
            const int row = f / (K / 4), c4 = (f % (K / 4)) * 4;
            bf16x4 hi, lo;
            split4(vh_f4(px[u]), hi, lo);
            st_bf4(x_hi + row * G::LDX + c4, hi); st_bf4(x_lo + row * G::LDX + c4, lo);
        }
        lds_barrier();
        if (tile + nwg < ntiles) prefetch_x(tile + nwg);
        {   // P = X Wp^T + bp exactly as the forward formed it (ks ascending, mma_x3, zero-initialised accumulators: the same bits)
            f32x4 pacc[G::FRTW][G::FHCW];
#pragma unroll
            for (int i = 0; i < G::FRTW; ++i)
#pragma unroll
                for (int j = 0; j < G::FHCW; ++j) pacc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < G::FKS; ++ks)
#pragma unroll
                for (int i = 0; i < G::FRTW; ++i) {
                    const int off = ((fwr * G::FRTW + i) * 16 + r) * G::LDX + 32 * ks + 8 * q;
                    const bf16x8 xh = ldfrag(x_hi + off), xl = ldfrag(x_lo + off);
#pragma unroll
                    for (int j = 0; j < G::FHCW; ++j) mma_x3(pacc[i][j], xh, xl, wh[j][ks], wl[j][ks]);
                }
#pragma unroll
            for (int i = 0; i < G::FRTW; ++i)
#pragma unroll
                for (int j = 0; j < G::FHCW; ++j) {
                    const int col = (fwc * G::FHCW + j) * 16 + r;
#pragma unroll
                    for (int e = 0; e < 4; ++e) s_p[((fwr * G::FRTW + i) * 16 + q * 4 + e) * G::LDPF + col] = pacc[i][j][e] + bias[j];
                }
        }
        lds_barrier();
        // the head's backward: dP = [dmu | dlogstd] of this thread's quads; P is read out of the planes' bytes before any are written
        float4 mu[G::PFX], ls[G::PFX];
#pragma unroll
        for (int u = 0; u < G::PFX; ++u) {
            const int f = tid + u * G::NT;
            const int row = f / (K / 4), c4 = (f % (K / 4)) * 4;
            mu[u] = ld4(s_p + row * G::LDPF + c4); ls[u] = ld4(s_p + row * G::LDPF + H + c4);
        }
        lds_barrier();
#pragma unroll
        for (int u = 0; u < G::PFX; ++u) {
            const int f = tid + u * G::NT;
            const int row = f / (K / 4), c4 = (f % (K / 4)) * 4;
            const int64_t node = first + row;
            float4 dmu = zero4(), dls = zero4();
            if (node < a.N) {
                const float4 g = vh_f4(pg[u]);
                const float4 sd = make_float4(expf(ls[u].x), expf(ls[u].y), expf(ls[u].z), expf(ls[u].w));
                float4 e = zero4();
                if (want_eps) e = vh_eps<H>(a, half, node, c4);
                dmu = make_float4(g.x + gk * (-2.0f * mu[u].x), g.y + gk * (-2.0f * mu[u].y), g.z + gk * (-2.0f * mu[u].z), g.w + gk * (-2.0f * mu[u].w));
                dls = make_float4(g.x * e.x * sd.x + gk * (2.0f - 2.0f * sd.x * sd.x), g.y * e.y * sd.y + gk * (2.0f - 2.0f * sd.y * sd.y),
                                  g.z * e.z * sd.z + gk * (2.0f - 2.0f * sd.z * sd.z), g.w * e.w * sd.w + gk * (2.0f - 2.0f * sd.w * sd.w));
            }
            db_mu = add4(db_mu, dmu); db_ls = add4(db_ls, dls);
            bf16x4 hi, lo;
            split4(dmu, hi, lo);
            st_bf4(g_hi + row * G::LDG + c4, hi); st_bf4(g_lo + row * G::LDG + c4, lo);
            split4(dls, hi, lo);
            st_bf4(g_hi + row * G::LDG + H + c4, hi); st_bf4(g_lo + row * G::LDG + H + c4, lo);
        }
        lds_barrier();
        if (tile + nwg < ntiles) prefetch_g(tile + nwg);
        // dWp += dP^T X as k_linear_wgrad_x3 does it
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
        // dX = dP Wp from the dP planes still in LDS; the fp32 tile is staged over the X planes, which nobody reads after the barrier above
        f32x4 dacc[G::DRTW];
#pragma unroll
        for (int i = 0; i < G::DRTW; ++i) dacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < G::DKS; ++ks)
#pragma unroll
            for (int i = 0; i < G::DRTW; ++i) {
                const int off = ((dwr * G::DRTW + i) * 16 + r) * G::LDG + 32 * ks + 8 * q;
                const bf16x8 gh = ldfrag(g_hi + off), gl = ldfrag(g_lo + off);
                if (ks < G::KSR) mma_x3(dacc[i], gh, gl, th[ks], tl[ks]);
                else mma_x3(dacc[i], gh, gl, wt_lds(0, ks), wt_lds(1, ks));
            }
#pragma unroll
        for (int i = 0; i < G::DRTW; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) s_y[((dwr * G::DRTW + i) * 16 + q * 4 + e) * G::LDY + dwc * 16 + r] = dacc[i][e];
        lds_barrier();
#pragma unroll
        for (int u = 0; u < G::PFX; ++u) {
            const int f = tid + u * G::NT;
            const int row = f / (K / 4), c4 = (f % (K / 4)) * 4;
            if (first + row < a.N) st4(a.dST + (first + row) * a.lddst + half * H + c4, ld4(s_y + row * G::LDY + c4));
        }
        lds_barrier();      // the next tile's X planes overwrite the staged rows
    }
    // per-workgroup partials to this workgroup's slab row (plain stores); k_slab_sum adds the rows in a fixed order
    float* slab = a.slab + ((int64_t)wgi * 2 + half) * G::slab_row;
#pragma unroll
    for (int i = 0; i < G::ITW; ++i)
#pragma unroll
        for (int j = 0; j < G::JTW; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                slab[((it0 + i) * 16 + q * 4 + e) * K + (jt0 + j) * 16 + r] = acc[i][j][e];
    // column sums of dP: two float4 per thread into the (dead) planes, then a fixed-order sum over the threads of a column quad
    float4* s_part = reinterpret_cast<float4*>(smem_raw);
    s_part[2 * tid] = db_mu; s_part[2 * tid + 1] = db_ls;
    __syncthreads();
    if (tid < M) {
        const int which = tid / H, c = tid % H, quad = c / 4, e = c % 4;
        float sum = 0.f;
        for (int t = quad; t < G::NT; t += K / 4) sum += vh_get(s_part[2 * t + which], e);
        slab[M * K + tid] = sum;
    }
}

// workgroups per half: one per tile up to 128 per resident workgroup of a CU (the two halves together fill the 256 CUs)
inline int var_head_nwg(int64_t N, int per_cu) {
    const int64_t ntiles = (N + kTileRows - 1) / kTileRows, cap = 128LL * per_cu;
    return (int)(ntiles < 1 ? 1 : ntiles < cap ? ntiles : cap);
}
template <int H> inline int var_fwd_nwg(int64_t N) { return var_head_nwg(N, VarFwdGeom<H>::per_cu); }
template <int H> inline int var_bwd_nwg(int64_t N) { return var_head_nwg(N, VarBwdGeom<H>::per_cu); }

}  // namespace mgv

// workgroups per half: one per tile of 64 rows up to 128 per resident workgroup of a CU (the two halves fill the 256 CUs)
extern "C" int mgv_var_head_x3_ws_floats(int H, int64_t N, int backward) {
    if (N < 0) return 0;
    int n = 0;
    mgv::dispatch_width(mgv::X3Widths{}, H, [&](auto w) {
        constexpr int W = decltype(w)::value;
        n = backward ? mgv::var_bwd_nwg<W>(N) * 2 * mgv::VarBwdGeom<W>::slab_row : mgv::var_fwd_nwg<W>(N) * 4;    // (2 doubles per workgroup pair)
        return MGV_OK;
    });
    return n;
}

extern "C" int mgv_var_head_fwd_x3(int H, int64_t N, const float* ST, int ldst, const void* wpack_s, const void* wpack_t, const float* b_s,
                                   const float* b_t, const float* eps, int ldeps, uint64_t seed, int sample, float* Z, int ldz, float* ML,
                                   int ldml, double* klsum, float* workspace, int64_t workspace_floats, void* stream) {
    if (!mgv::has_width(mgv::X3Widths{}, H)) return MGV_EUNSUPPORTED;
    MGV_CHECK_ARG(N >= 0 && ST && wpack_s && wpack_t && b_s && b_t && Z && klsum && workspace);
    MGV_CHECK_ARG(ldst >= 2 * H && ldst % 4 == 0 && ldz >= 2 * H && ldz % 4 == 0 && (eps == nullptr || (ldeps >= 2 * H && ldeps % 4 == 0)) &&
                  (ML == nullptr || (ldml >= 4 * H && ldml % 4 == 0)) && (sample == 0 || sample == 1));
    MGV_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 8 == 0 && workspace_floats >= mgv_var_head_x3_ws_floats(H, N, 0));
    if (N == 0) return MGV_OK;
    mgv::VarHeadArgs a{};
    a.N = N; a.ST = ST; a.ldst = ldst; a.wpack[0] = static_cast<const __bf16*>(wpack_s); a.wpack[1] = static_cast<const __bf16*>(wpack_t);
    a.b[0] = b_s; a.b[1] = b_t; a.eps = eps; a.ldeps = ldeps; a.seed = seed; a.sample = sample; a.Z = Z; a.ldz = ldz; a.ML = ML; a.ldml = ldml;
    a.klslab = reinterpret_cast<double*>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return mgv::launch_width(mgv::X3Widths{}, H, [&](auto w) {
        constexpr int W = decltype(w)::value;
        using G = mgv::VarFwdGeom<W>;
        const int nwg = mgv::var_fwd_nwg<W>(N);
        mgv::allow_lds<mgv::k_var_head_fwd_x3<W>>();
        hipLaunchKernelGGL((mgv::k_var_head_fwd_x3<W>), dim3(2 * nwg), dim3(mgv::kThreads), G::smem_bytes, st, a);
        hipLaunchKernelGGL(mgv::k_var_head_klsum, dim3(1), dim3(64), 0, st, a.klslab, nwg, klsum);
    });
}

extern "C" int mgv_var_head_bwd_x3(int H, int64_t N, const float* ST, int ldst, const void* wpack_s, const void* wpack_t,
                                   const void* wtpack_s, const void* wtpack_t, const float* b_s, const float* b_t, const float* eps, int ldeps,
                                   uint64_t seed, int sample, const float* gZ, int ldg, const float* gkl, float* dST, int lddst, float* dWp_s,
                                   float* dWp_t, float* dbp_s, float* dbp_t, float* workspace, int64_t workspace_floats, void* stream) {
    if (!mgv::has_width(mgv::X3Widths{}, H)) return MGV_EUNSUPPORTED;
    MGV_CHECK_ARG(N >= 0 && ST && wpack_s && wpack_t && wtpack_s && wtpack_t && b_s && b_t && dST && dWp_s && dWp_t && dbp_s && dbp_t && workspace);
    MGV_CHECK_ARG(ldst >= 2 * H && ldst % 4 == 0 && lddst >= 2 * H && lddst % 4 == 0 && (eps == nullptr || (ldeps >= 2 * H && ldeps % 4 == 0)) &&
                  (gZ == nullptr || (ldg >= 2 * H && ldg % 4 == 0)) && (sample == 0 || sample == 1));
    MGV_CHECK_ARG(workspace_floats >= mgv_var_head_x3_ws_floats(H, N, 1));
    if (N == 0) return MGV_OK;
    mgv::VarHeadArgs a{};
    a.N = N; a.ST = ST; a.ldst = ldst; a.wpack[0] = static_cast<const __bf16*>(wpack_s); a.wpack[1] = static_cast<const __bf16*>(wpack_t);
    a.wtpack[0] = static_cast<const __bf16*>(wtpack_s); a.wtpack[1] = static_cast<const __bf16*>(wtpack_t);
    a.b[0] = b_s; a.b[1] = b_t; a.eps = eps; a.ldeps = ldeps; a.seed = seed; a.sample = sample; a.gZ = gZ; a.ldg = ldg; a.gkl = gkl;
    a.dST = dST; a.lddst = lddst; a.slab = workspace;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return mgv::launch_width(mgv::X3Widths{}, H, [&](auto w) {
        constexpr int W = decltype(w)::value;
        using G = mgv::VarBwdGeom<W>;
        constexpr int M = G::M, K = G::K;
        const int nwg = mgv::var_bwd_nwg<W>(N);
        mgv::allow_lds<mgv::k_var_head_bwd_x3<W>>();
        hipLaunchKernelGGL((mgv::k_var_head_bwd_x3<W>), dim3(2 * nwg), dim3(G::NT), G::smem_bytes, st, a);
        float* const dW[2] = {dWp_s, dWp_t};
        float* const db[2] = {dbp_s, dbp_t};
        for (int h = 0; h < 2; ++h) {
            mgv::launch_slab_sum<float, float>(workspace + (int64_t)h * G::slab_row, nwg, 2 * G::slab_row, M * K, dW[h], st);
            mgv::launch_slab_sum<float, float>(workspace + (int64_t)h * G::slab_row + M * K, nwg, 2 * G::slab_row, M, db[h], st);
        }
    });
}
