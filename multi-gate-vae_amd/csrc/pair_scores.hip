// All-pairs side of the inner-product decoder (digae_layer.py:26-33 forward_all, digae_model.py:118-122): dense scores with their
// backward, scores of listed pairs, and the streaming top-k / count consumer that never writes an N x N array.
//
// ONE arithmetic for every entry: exact fp32 on v_mfma_f32_16x16x4_f32 with k in plain ascending order 0 .. H-1 (k-step kk feeds
// k = 4 kk + q from lane quarter q; no in-block permutation as in mma_kblock), i.e. for every pair the chain
//     acc = 0;  for k = 0 .. H-1: acc = fmaf(s[i][k], t[j][k], acc)
// which k_pair_at restates with scalar fmaf.  The dense tile code (tile_scores) is shared by the dense forward and the top-k kernel,
// so a score reported by one is the other's bit for bit; these are decisions at a threshold and ranks, like k_edge_dot's.
// The same entries on unit rows (k_row_unit) are the cosine search on hf, the inference side of the functional loss (trainer.py:158-160);
// its thresholded pairs come from the symmetric form of the selection walk (k_pair_select<.., SYM>).
// The classes of that relation come from the same walk with a union-find in place of the lists (k_sim_union, mgv_unionfind.h).
// The rank of a true link among all candidates of its node comes from the same walk with a list of thresholds per row (k_pair_rank).
// The same consumers on the rows of ANOTHER graph of the batch (k_cross_*) are matching across circuits.
//
// What decides a result exists ONCE in the file: a row's graph and the clamp of its range (row_graph, graph_rows), who is a candidate
// (candidate<SYM>), and each consumer — the sorted lists (topk_*), the count / fill (select_*), the bins (HistRun), the unions
// (unite_bits).  An own-graph kernel and its cross twin are two prologues and two tile ranges around the same consumer, so the same
// bits meet the same `>` in both, and a fix to an insertion order, a fill cursor or a run merge is made and proved once.
// Three things stand in a kernel and in its twin all the same, each for a reason the compiler gave (stated where they stand): the
// five lines of the tile loop, the selection's one-line decision `candidate<SYM>(...) && rep > threshold`, and the histogram's flush
// of a finished run (six lines that add to arrays the kernel declares; it decides no bin and no count).
#include "mgv_launch.h"
#include "mgv_unionfind.h"
#include "../../include/mgvae_hip.h"

#include <limits.h>

#include <vector>

namespace mgv {

constexpr int kPairTile = 64;          // output tile: 64 x 64, wave w owns rows 16 w .. 16 w + 15 and all 64 columns
constexpr int kPairChunk = 16;         // column tiles one workgroup of the dense forward walks with its s fragments in registers
constexpr int kTopkMax = 32;

template <int H>
struct PairCfg {
    static_assert(H == 16 || H == 32 || H == 64 || H == 128, "H must be 16, 32, 64 or 128");
    static constexpr int KS = H / 4;                      // MFMA k-steps
    static constexpr int LDT = H + 4;                     // forward t tile [column][k]: lane (r, q) reads bank 4 r + q (+ const)
    static constexpr int VPT = H / 16;                    // float4s a thread moves per 64-row operand tile
    static constexpr int LDB = H % 64 == 0 ? H + 16 : 48; // backward operand tile [walked row][k]: lane (r, q) reads bank 16 q + r
};

// LDS traffic of ONE wave in program order: the lanes of a wave exchange data through LDS without a workgroup barrier
__device__ __forceinline__ void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// the wave's 16 rows of s as A fragments: lane (r = lane & 15, q = lane >> 4) holds s[row0 + r][4 kk + q]; rows past M are zeros
template <int H>
__device__ __forceinline__ void load_row_frags(float (&a)[H / 4], const float* s, int lds, int64_t row, bool ok, int q) {
    const float* p = s + (ok ? row : 0) * (int64_t)lds + q;
#pragma unroll
    for (int kk = 0; kk < H / 4; ++kk) a[kk] = ok ? p[4 * kk] : 0.f;
}

// rows c0 .. c0 + 63 of a row-major operand (zeros past n) as H / 16 float4s per thread, and their place in an LDS tile of stride LD
template <int H>
__device__ __forceinline__ void tile_load(float4 (&v)[H / 16], const float* x, int ldx, int64_t c0, int64_t n) {
#pragma unroll
    for (int i = 0; i < H / 16; ++i) {
        const int e = threadIdx.x + kThreads * i, jj = e / (H / 4), c4 = e % (H / 4);
        v[i] = c0 + jj < n ? ld4(x + (c0 + jj) * (int64_t)ldx + 4 * c4) : zero4();
    }
}
template <int H, int LD>
__device__ __forceinline__ void tile_store(float* tl, const float4 (&v)[H / 16]) {
#pragma unroll
    for (int i = 0; i < H / 16; ++i) {
        const int e = threadIdx.x + kThreads * i, jj = e / (H / 4), c4 = e % (H / 4);
        st4(tl + jj * LD + 4 * c4, v[i]);
    }
}

// acc[c] = the wave's 16 rows x columns 16 c .. 16 c + 15 of the tile; lane holds column (lane & 15), rows 4 (lane >> 4) + reg
template <int H>
__device__ __forceinline__ void tile_scores(f32x4 (&acc)[4], const float (&a)[H / 4], const float* tl, int r, int q) {
    constexpr int LDT = PairCfg<H>::LDT;
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < H / 4; ++kk) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = mfma16(a[kk], tl[(16 * c + r) * LDT + 4 * kk + q], acc[c]);
    }
}

// ---------------------------------------------------------------------------------- the walk every all-pairs kernel is a consumer of
// Its loop over the column tiles ct0 .. ct1 - 1 stands in every consumer as the same five lines — barrier (every wave is done with the
// previous tile), tile_store of the prefetched tile, barrier, tile_load of the next one (in flight under the MFMAs), tile_scores — with
// the consumer behind them.  As a function (a step the loop calls, or the loop with the consumer as a callable) the compiler allocates
// and branches differently around it: a wave less in k_pair_fwd<32>, k_pair_topk<16> and k_sim_union<16>, 2 - 5 % on the general count
// (NOTEBOOK 2026-10-19, eighth entry).  What decides — the rows' ranges, the tile range, who is a candidate — exists once, below.

// The graph of row u: the first whose end lies behind u; -1 for a row past N or behind the last graph.
__device__ __forceinline__ int row_graph(int64_t N, int64_t u, const int32_t* gp, int G) {
    if (u >= N) return -1;
    int a = 0, b = G;
    while (a < b) { const int m = (a + b) >> 1; if ((int64_t)gp[m + 1] <= u) a = m + 1; else b = m; }
    return a < G ? a : -1;
}

// The rows [lo, hi) of graph g, nothing for a g outside the table: whatever the table holds, no column outside [0, N) is touched.
__device__ __forceinline__ void graph_rows(int64_t N, const int32_t* gp, int G, int g, int64_t& lo, int64_t& hi) {
    lo = 0; hi = 0;
    if (g >= 0 && g < G) { lo = gp[g]; hi = gp[g + 1]; }
    lo = lo < 0 ? 0 : (lo > N ? N : lo);
    hi = hi < lo ? lo : (hi > N ? N : hi);
}

// The candidate columns [rlo[i], rhi[i]) of row u0 + i, i < 64: the row's own graph (the whole batch without a table, nothing for a row
// past N), and in rgi — only where the caller keeps that table (GI) — the graph's index.  The caller's barrier publishes the tables.
template <bool GI = false>
__device__ __forceinline__ void row_ranges(int64_t N, int64_t u0, const int32_t* gp, int G, int* rlo, int* rhi, int* rgi = nullptr) {
    if (threadIdx.x >= kPairTile) return;
    const int64_t u = u0 + threadIdx.x;
    const int g = gp != nullptr ? row_graph(N, u, gp, G) : -1;
    int64_t lo = 0, hi = u < N ? N : 0;
    if (gp != nullptr) graph_rows(N, gp, G, g, lo, hi);
    rlo[threadIdx.x] = (int)lo; rhi[threadIdx.x] = (int)hi;
    if constexpr (GI) rgi[threadIdx.x] = g < 0 ? 0 : g;    // < max(G, 1)
}

// The same tables where the candidates of a row of graph g are ALL rows of graph peer[g] (the k_cross_* kernels): nothing for a row
// past N, a row behind the last graph, peer = -1 or a peer outside the table.  rgi stays the ROW's graph.
template <bool GI = false>
__device__ __forceinline__ void cross_ranges(int64_t N, int64_t u0, const int32_t* gp, int G, const int32_t* peer, int* rlo, int* rhi,
                                             int* rgi = nullptr) {
    if (threadIdx.x >= kPairTile) return;
    const int g = row_graph(N, u0 + threadIdx.x, gp, G);
    int64_t lo, hi;
    graph_rows(N, gp, G, g < 0 ? -1 : peer[g], lo, hi);
    rlo[threadIdx.x] = (int)lo; rhi[threadIdx.x] = (int)hi;
    if constexpr (GI) rgi[threadIdx.x] = g < 0 ? 0 : g;
}

// The columns [clo, chi) that hold a candidate of any of the 64 rows (clo >= chi: none, nothing to walk).
__device__ __forceinline__ void col_span(int64_t N, const int* rlo, const int* rhi, int64_t& clo, int64_t& chi) {
    clo = N; chi = 0;
    for (int i = 0; i < kPairTile; ++i) {
        if (rlo[i] < rhi[i]) { clo = rlo[i] < clo ? rlo[i] : clo; chi = rhi[i] > chi ? rhi[i] : chi; }
    }
}

// The column tiles [ct0, ct1) that cover [clo, chi), asked only behind `clo < chi`, as each kernel had it: with the tile range computed
// in front of that branch k_pair_topk<16> takes 62 - 67 VGPRs for 60 and loses a wave, and every symmetric kernel changes by some
// hundred instructions (NOTEBOOK 2026-10-19, eighth entry).  SYM (s = t, the score matrix symmetric in bits, row u takes only v > u):
// from the row tile's own column tile on — row and column tiles are both 64 wide, so the diagonal tile of workgroup b is column tile
// b, and it starts inside t because u0 < N.
template <bool SYM>
__device__ __forceinline__ void tile_span(int64_t clo, int64_t chi, int64_t& ct0, int64_t& ct1) {
    ct0 = clo / kPairTile;
    ct1 = (chi + kPairTile - 1) / kPairTile;
    if constexpr (SYM) ct0 = ct0 > (int64_t)blockIdx.x ? ct0 : (int64_t)blockIdx.x;
}

// WHO is a candidate of row `row` and WHAT score is reported for it: the one statement behind every list, count, class and bin.
//   general: a column of the row's graph [lo, hi), without the row itself when skip_self; the sigmoid of the dot product when asked for.
//   SYM    : col > row (>= the graph's start) below hi; the raw score; `lo`, `skip_self` and `sigmoid` are not looked at.
// A NaN score is nobody's candidate.
// The symmetric form is stated as text (MGV_CAND_SYM) because k_sim_union needs it in one flat chain with its `> threshold`: behind
// the function the chain reaches the back end in another order (`(a ? b : false) & gt` for `a ? (b & gt) : false`), its 16 float
// compares per tile go through VCC one after the other, and mgv_sim_union ran 1.6 - 4.9 % slower (NOTEBOOK 2026-10-19, eighth entry).
// The function's arguments come by reference on purpose: by value they are `noundef`, the compiler turns the `&&` chain into plain ands,
// and where `> threshold` follows, its SLP vectoriser packs them into 4-wide 64-bit compares (seen in k_sim_union: a wave less at H = 128).
#define MGV_CAND_SYM(v, col, row, hi) ((col) > (row) && (col) < (hi) && (v) == (v))
template <bool SYM>
__device__ __forceinline__ bool candidate(const float& v, const int64_t& col, const int64_t& row, const int& lo, const int& hi,
                                          const int& skip_self, const int& sigmoid, float& rep) {
    if constexpr (SYM) {
        rep = v;
        return MGV_CAND_SYM(v, col, row, hi);
    } else {
        rep = sigmoid ? sigmoidf_(v) : v;
        return col >= lo && col < hi && !(skip_self && col == row) && v == v;
    }
}

// ---------------------------------------------------------------------------------- dense forward
// grid (row tiles, chunks of kPairChunk column tiles): no cap, every tile has its workgroup position
template <int H>
__global__ __launch_bounds__(kThreads) void k_pair_fwd(int64_t M, int64_t N, const float* s, int lds, const float* t, int ldt,
                                                       int sigmoid, float* out, int64_t ldo) {
    __shared__ __attribute__((aligned(16))) float tl[kPairTile * PairCfg<H>::LDT];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * kPairTile + 16 * w;
    float a[H / 4];
    load_row_frags<H>(a, s, lds, row0 + r, row0 + r < M, q);
    const int64_t nct = (N + kPairTile - 1) / kPairTile;
    const int64_t ct0 = (int64_t)blockIdx.y * kPairChunk, ct1 = ct0 + kPairChunk < nct ? ct0 + kPairChunk : nct;
    float4 nxt[H / 16];
    tile_load<H>(nxt, t, ldt, ct0 * kPairTile, N);
    for (int64_t ct = ct0; ct < ct1; ++ct) {
        __syncthreads();                                   // every wave is done with the previous tile
        tile_store<H, PairCfg<H>::LDT>(tl, nxt);
        __syncthreads();
        if (ct + 1 < ct1) tile_load<H>(nxt, t, ldt, (ct + 1) * kPairTile, N);   // in flight under the MFMAs
        f32x4 acc[4];
        tile_scores<H>(acc, a, tl, r, q);
        const int64_t col0 = ct * kPairTile;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t col = col0 + 16 * c + r;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int64_t row = row0 + 4 * q + g;
                if (row < M && col < N) out[row * ldo + col] = sigmoid ? sigmoidf_(acc[c][g]) : acc[c][g];
            }
        }
    }
}

// ---------------------------------------------------------------------------------- listed pairs
// the same chain with scalar fmaf: one thread per pair
template <int H>
__global__ __launch_bounds__(kThreads) void k_pair_at(int64_t E, const float* s, int lds, const float* t, int ldt, const int64_t* src,
                                                      const int64_t* dst, int sigmoid, float* out) {
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < E; e += (int64_t)gridDim.x * kThreads) {
        const float* a = s + src[e] * (int64_t)lds;
        const float* b = t + dst[e] * (int64_t)ldt;
        float acc = 0.f;
#pragma unroll
        for (int k4 = 0; k4 < H / 4; ++k4) {
            const float4 x = ld4(a + 4 * k4), y = ld4(b + 4 * k4);
            acc = fmaf(x.x, y.x, acc);
            acc = fmaf(x.y, y.y, acc);
            acc = fmaf(x.z, y.z, acc);
            acc = fmaf(x.w, y.w, acc);
        }
        out[e] = sigmoid ? sigmoidf_(acc) : acc;
    }
}

// ---------------------------------------------------------------------------------- dense backward
// d[a][k] = sum_b G(a, b) x[b][k]: one workgroup per 64 rows a, which walks b in tile order; every entry is ONE fmaf chain over
// b = 0 .. 64 ceil(B / 64) - 1 (zeros past B), so nothing meets in atomics and two runs give the same bits.
// TRANS = false: ds (a = row i of the score matrix, b = column j, x = t); TRANS = true: dt (a = column j, b = row i, x = s).
template <int H, bool TRANS>
__global__ __launch_bounds__(kThreads) void k_pair_bwd(int64_t A, int64_t B, const float* x, int ldx, int sigmoid, const float* p,
                                                       int64_t ldp, const float* g, int64_t ldg, float* d, int ldd) {
    constexpr int LDB = PairCfg<H>::LDB, HC = H / 16;
    __shared__ __attribute__((aligned(16))) float xl[kPairTile * LDB];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int64_t a0 = (int64_t)blockIdx.x * kPairTile + 16 * w, arow = a0 + r;
    f32x4 acc[HC];
#pragma unroll
    for (int c = 0; c < HC; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t b0 = 0; b0 < B; b0 += kPairTile) {
        float gf[16];
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            const int64_t b = b0 + 4 * st + q;
            float v = 0.f;
            if (arow < A && b < B) {
                v = g[TRANS ? b * ldg + arow : arow * ldg + b];
                if (sigmoid) { const float pp = p[TRANS ? b * ldp + arow : arow * ldp + b]; v *= pp * (1.0f - pp); }
            }
            gf[st] = v;
        }
        float4 xv[H / 16];
        tile_load<H>(xv, x, ldx, b0, B);
        __syncthreads();
        tile_store<H, LDB>(xl, xv);
        __syncthreads();
#pragma unroll
        for (int st = 0; st < 16; ++st) {
#pragma unroll
            for (int c = 0; c < HC; ++c) acc[c] = mfma16(gf[st], xl[(4 * st + q) * LDB + 16 * c + r], acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < HC; ++c) {
#pragma unroll
        for (int gI = 0; gI < 4; ++gI) {
            const int64_t row = a0 + 4 * q + gI;
            if (row < A) d[row * (int64_t)ldd + 16 * c + r] = acc[c][gI];
        }
    }
}

// ---------------------------------------------------------------------------------- streaming top-k and counts
// order of the lists: raw dot product descending, ties by ascending node id
__device__ __forceinline__ bool pair_better(float v, int i, float kv, int ki) { return v > kv || (v == kv && i < ki); }

// The top-k consumer.  Each wave leaves its 16 x 16 score blocks in LDS (sc), where 4 lanes per row — lane (lane >> 2, sub = lane & 3)
// scans for row srow = 16 w + (lane >> 2) of the tile — scan them in ascending column order against the row's k-th best and insert
// into the row's sorted list (lv / li, LDS).  A row only ever sees the columns of its range [mylo, myhi).
// Three functions of scalars by reference and plain pointers to the LDS arrays, the lane's indices among them: the kernels that call
// them have the registers and waves they had with this text in place (NOTEBOOK 2026-10-20, tenth entry).
constexpr int kTopkScLd = 17;          // row stride of sc

// the lists of the wave's rows start empty, initialised by their own wave
__device__ __forceinline__ void topk_init(float* lv, int* li, const int& srow, const int& sub) {
    for (int j = sub; j < kTopkMax; j += 4) { lv[srow * kTopkMax + j] = -INFINITY; li[srow * kTopkMax + j] = INT_MAX; }
}

// the wave's block of columns cb .. cb + 15: counted against the threshold (cnt) and offered to the lists of row su
__device__ __forceinline__ void topk_block(const f32x4& acc, const int64_t& cb, const int64_t& su, const int& mylo, const int& myhi,
                                           const int& k, const int& sigmoid, const float& threshold, const int& skip_self, float* sc,
                                           float* lv, int* li, int& cnt, const int& w, const int& r, const int& q, const int& srow,
                                           const int& sub) {
    wave_lds_fence();                              // the previous block's reads are done
#pragma unroll
    for (int g = 0; g < 4; ++g) sc[(16 * w + 4 * q + g) * kTopkScLd + r] = acc[g];
    wave_lds_fence();
    for (int st = 0; st < 4; ++st) {
        const int64_t col = cb + 4 * st + sub;
        const float v = sc[srow * kTopkScLd + 4 * st + sub];
        float rep;
        const bool valid = candidate<false>(v, col, su, mylo, myhi, skip_self, sigmoid, rep);
        cnt += (valid && rep > threshold) ? 1 : 0;
        const bool pass = valid && pair_better(v, (int)col, lv[srow * kTopkMax + k - 1], li[srow * kTopkMax + k - 1]);
        if (__ballot(pass) == 0ull) continue;
        for (int turn = 0; turn < 4; ++turn) {      // the row's four lanes insert one after the other, lowest column first
            if (pass && sub == turn) {
                float* L = lv + srow * kTopkMax;
                int* I = li + srow * kTopkMax;
                if (pair_better(v, (int)col, L[k - 1], I[k - 1])) {
                    int pos = k - 1;
                    while (pos > 0 && pair_better(v, (int)col, L[pos - 1], I[pos - 1])) {
                        L[pos] = L[pos - 1]; I[pos] = I[pos - 1]; --pos;
                    }
                    L[pos] = v; I[pos] = (int)col;
                }
            }
            wave_lds_fence();
        }
    }
}

// after the walk: the row's four counts meet, and row su < N writes n_above and its k entries (-1 / -inf where the list is short).
// The loop is kept rolled: unrolled inside this function it costs k_cross_topk<16> 12 VGPRs and a wave.
__device__ __forceinline__ void topk_write(const int64_t& N, const int64_t& su, const int& k, const int& sigmoid, int& cnt, const float* lv,
                                           const int* li, int32_t* idx, float* score, int32_t* n_above, const int& srow, const int& sub) {
    wave_lds_fence();
    cnt += __shfl_xor(cnt, 1, 64);
    cnt += __shfl_xor(cnt, 2, 64);
    if (su < N) {
        if (sub == 0) n_above[su] = cnt;
#pragma unroll 1
        for (int j = sub; j < k; j += 4) {
            const int id = li[srow * kTopkMax + j];
            const float v = lv[srow * kTopkMax + j];
            idx[su * k + j] = id == INT_MAX ? -1 : id;
            score[su * k + j] = id == INT_MAX ? -INFINITY : (sigmoid ? sigmoidf_(v) : v);
        }
    }
}

// One workgroup per 64 rows u; it walks the column tiles that meet the rows' graphs.
template <int H>
__global__ __launch_bounds__(kThreads) void k_pair_topk(int64_t N, const float* s, int lds, const float* t, int ldt, const int32_t* gp,
                                                        int G, int k, int sigmoid, float threshold, int skip_self, int32_t* idx,
                                                        float* score, int32_t* n_above) {
    __shared__ __attribute__((aligned(16))) float tl[kPairTile * PairCfg<H>::LDT];
    __shared__ float sc[kPairTile * kTopkScLd];
    __shared__ float lv[kPairTile * kTopkMax];
    __shared__ int li[kPairTile * kTopkMax];
    __shared__ int rlo[kPairTile], rhi[kPairTile];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int64_t u0 = (int64_t)blockIdx.x * kPairTile;
    row_ranges(N, u0, gp, G, rlo, rhi);
    const int srow = 16 * w + (lane >> 2), sub = lane & 3;
    topk_init(lv, li, srow, sub);
    __syncthreads();
    int64_t clo, chi;
    col_span(N, rlo, rhi, clo, chi);
    const int64_t su = u0 + srow;                          // the row this lane scans for
    const int mylo = rlo[srow], myhi = rhi[srow];
    const int64_t row0 = u0 + 16 * w;
    float a[H / 4];
    load_row_frags<H>(a, s, lds, row0 + r, row0 + r < N, q);
    int cnt = 0;
    if (clo < chi) {
        int64_t ct0, ct1;
        tile_span<false>(clo, chi, ct0, ct1);
        float4 nxt[H / 16];
        tile_load<H>(nxt, t, ldt, ct0 * kPairTile, N);
        for (int64_t ct = ct0; ct < ct1; ++ct) {
            __syncthreads();
            tile_store<H, PairCfg<H>::LDT>(tl, nxt);
            __syncthreads();
            if (ct + 1 < ct1) tile_load<H>(nxt, t, ldt, (ct + 1) * kPairTile, N);
            f32x4 acc[4];
            tile_scores<H>(acc, a, tl, r, q);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t cb = ct * kPairTile + 16 * c;
                topk_block(acc[c], cb, su, mylo, myhi, k, sigmoid, threshold, skip_self, sc, lv, li, cnt, w, r, q, srow, sub);
            }
        }
    }
    topk_write(N, su, k, sigmoid, cnt, lv, li, idx, score, n_above, srow, sub);
}

// ---------------------------------------------------------------------------------- fan-ins by arity: a legal circuit from the walk
// The walk of k_pair_topk with the rows as TARGETS v (the caller passes t as the row operand and s as the column operand; every product
// commutes and k keeps its order, so a score is the bits of mgv_pair_scores_at for (u, v)) and two differences in its consumer:
//   who is a candidate — a column u of v's graph whose order key is BELOW v's (fanin_candidate): never v itself, and every decoded edge
//                        runs from a smaller key to a larger one, so the result is acyclic whatever the scores are;
//   how many a row keeps — its own kk = min(max(want[v], 0), K), not one k for all rows: the list_insert of the top-k lists on lists of
//                        kFaninLd entries per row.
// A row that wants nothing has NO candidates (its range is empty, n_cand = 0): col_span then leaves a tile whose rows want nothing
// without a walk, and what a tile walks depends only on its rows that want something.  The column keys of a tile travel through LDS
// with the tile (kl, prefetched with it; INT_MAX past N: below no key).
// Tile skip: tile_min[ct] is the least key of column tile ct (k_tile_min, launched in front on the same stream).  No column of a tile
// whose least key is not below kmax — the greatest key among the tile's rows that want something — is anybody's candidate, so the
// workgroup steps over it (a scalar compare, uniform per workgroup) and the output keeps its bytes.  With keys that ascend with the
// id inside a graph (a levelised netlist in topological order) that is every tile behind the row tile's own: half the walk.
// LDS at H = 128: score tile 33,792 B + sc 4,352 B + lists 2 x 2,304 B + five row tables 1,280 B = 44,032 B (k_pair_topk: 55,040 B).
constexpr int kFaninMax = 8;
constexpr int kFaninLd = kFaninMax + 1;    // row stride of the lists: the 16 rows of a wave lie in 16 banks

// WHO is a candidate of target row v: a column of v's graph [lo, hi) whose key is strictly below v's; a NaN score is nobody's candidate.
__device__ __forceinline__ bool fanin_candidate(const float& v, const int64_t& col, const int& lo, const int& hi, const int& ckey,
                                                const int& rkey) {
    return col >= lo && col < hi && ckey < rkey && v == v;
}

// topk_block's sorted-list insert on a list of k >= 1 entries L / I, by one lane of the row at a time: (v, col) goes where it is better
// than the k-th.  Restated here: with the text taken out of topk_block into a function the two top-k kernels compile to other
// instructions at every width (NOTEBOOK 2026-10-21).
__device__ __forceinline__ void list_insert(float* L, int* I, const int& k, const float& v, const int64_t& col) {
    if (pair_better(v, (int)col, L[k - 1], I[k - 1])) {
        int pos = k - 1;
        while (pos > 0 && pair_better(v, (int)col, L[pos - 1], I[pos - 1])) {
            L[pos] = L[pos - 1]; I[pos] = I[pos - 1]; --pos;
        }
        L[pos] = v; I[pos] = (int)col;
    }
}

// tile_min[ct] = min key[64 ct .. 64 ct + 63] over the columns below N: one wave per column tile
__global__ __launch_bounds__(kThreads) void k_tile_min(int64_t N, const int32_t* key, int32_t* tile_min) {
    const int lane = threadIdx.x & 63;
    const int64_t ct = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), c = ct * kPairTile + lane;
    if (ct * kPairTile >= N) return;                       // the whole wave leaves
    int m = c < N ? key[c] : INT_MAX;
    for (int d = 32; d > 0; d >>= 1) { const int o = __shfl_xor(m, d, 64); m = o < m ? o : m; }
    if (lane == 0) tile_min[ct] = m;
}

// the keys of columns c0 .. c0 + 63 beside tile_load / tile_store: one per thread of the first wave
__device__ __forceinline__ int key_load(const int32_t* key, int64_t c0, int64_t n) {
    return (threadIdx.x < kPairTile && c0 + threadIdx.x < n) ? key[c0 + threadIdx.x] : INT_MAX;
}

// the wave's block of columns cb .. cb + 15 (keys kb[0 .. 15]): its candidates counted (cnt) and offered to the list of row srow
__device__ __forceinline__ void fanin_block(const f32x4& acc, const int64_t& cb, const int* kb, const int& mylo, const int& myhi,
                                            const int& mykey, const int& myk, float* sc, float* lv, int* li, int& cnt, const int& w,
                                            const int& r, const int& q, const int& srow, const int& sub) {
    wave_lds_fence();                              // the previous block's reads are done
#pragma unroll
    for (int g = 0; g < 4; ++g) sc[(16 * w + 4 * q + g) * kTopkScLd + r] = acc[g];
    wave_lds_fence();
    float* L = lv + srow * kFaninLd;
    int* I = li + srow * kFaninLd;
    const int last = myk > 0 ? myk - 1 : 0;        // myk = 0: an empty range, nothing is valid
    for (int st = 0; st < 4; ++st) {
        const int64_t col = cb + 4 * st + sub;
        const float v = sc[srow * kTopkScLd + 4 * st + sub];
        const bool valid = fanin_candidate(v, col, mylo, myhi, kb[4 * st + sub], mykey);
        cnt += valid ? 1 : 0;
        const bool pass = valid && pair_better(v, (int)col, L[last], I[last]);
        if (__ballot(pass) == 0ull) continue;
        for (int turn = 0; turn < 4; ++turn) {      // the row's four lanes insert one after the other, lowest column first
            if (pass && sub == turn) list_insert(L, I, myk, v, col);
            wave_lds_fence();
        }
    }
}

template <int H>
__global__ __launch_bounds__(kThreads) void k_fanin_decode(int64_t N, const float* x, int ldx, const float* y, int ldy, const int32_t* gp,
                                                           int G, const int32_t* key, const int32_t* want, int K, const int32_t* tile_min,
                                                           int32_t* idx, float* score, int32_t* n_cand) {
    __shared__ __attribute__((aligned(16))) float tl[kPairTile * PairCfg<H>::LDT];
    __shared__ float sc[kPairTile * kTopkScLd];
    __shared__ float lv[kPairTile * kFaninLd];
    __shared__ int li[kPairTile * kFaninLd];
    __shared__ int rlo[kPairTile], rhi[kPairTile], rkey[kPairTile], rk[kPairTile], kl[kPairTile];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int64_t u0 = (int64_t)blockIdx.x * kPairTile;
    row_ranges(N, u0, gp, G, rlo, rhi);
    if (threadIdx.x < kPairTile) {                         // the row's key and how many it keeps; a row that wants nothing: no candidates
        const int64_t u = u0 + threadIdx.x;
        int kk = u < N ? want[u] : 0;
        kk = kk < 0 ? 0 : (kk > K ? K : kk);
        rkey[threadIdx.x] = u < N ? key[u] : INT_MIN;
        rk[threadIdx.x] = kk;
        if (kk == 0) rhi[threadIdx.x] = rlo[threadIdx.x];  // (row_ranges wrote both from this thread)
    }
    const int srow = 16 * w + (lane >> 2), sub = lane & 3;
    for (int j = sub; j < kFaninMax; j += 4) { lv[srow * kFaninLd + j] = -INFINITY; li[srow * kFaninLd + j] = INT_MAX; }
    __syncthreads();
    int64_t clo, chi;
    col_span(N, rlo, rhi, clo, chi);
    int kmax = INT_MIN;                                    // the greatest key among the rows that want something
    for (int i = 0; i < kPairTile; ++i) kmax = (rlo[i] < rhi[i] && rkey[i] > kmax) ? rkey[i] : kmax;
    const int64_t su = u0 + srow;                          // the row this lane scans for
    const int mylo = rlo[srow], myhi = rhi[srow], mykey = rkey[srow], myk = rk[srow];
    const int64_t row0 = u0 + 16 * w;
    float a[H / 4];
    load_row_frags<H>(a, x, ldx, row0 + r, row0 + r < N, q);
    int cnt = 0;
    if (clo < chi) {
        int64_t ct0, ct1;
        tile_span<false>(clo, chi, ct0, ct1);
        // the next tile from `ct` on that can hold a candidate (without tile_min: ct itself)
        auto next_tile = [&](int64_t ct) {
            if (tile_min != nullptr) { while (ct < ct1 && tile_min[ct] >= kmax) ++ct; }
            return ct;
        };
        int64_t ct = next_tile(ct0);
        float4 nxt[H / 16];
        int nkey = INT_MAX;
        if (ct < ct1) { tile_load<H>(nxt, y, ldy, ct * kPairTile, N); nkey = key_load(key, ct * kPairTile, N); }
        while (ct < ct1) {
            __syncthreads();
            tile_store<H, PairCfg<H>::LDT>(tl, nxt);
            if (threadIdx.x < kPairTile) kl[threadIdx.x] = nkey;
            __syncthreads();
            const int64_t nct = next_tile(ct + 1);
            if (nct < ct1) { tile_load<H>(nxt, y, ldy, nct * kPairTile, N); nkey = key_load(key, nct * kPairTile, N); }
            f32x4 acc[4];
            tile_scores<H>(acc, a, tl, r, q);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t cb = ct * kPairTile + 16 * c;
                fanin_block(acc[c], cb, kl + 16 * c, mylo, myhi, mykey, myk, sc, lv, li, cnt, w, r, q, srow, sub);
            }
            ct = nct;
        }
    }
    wave_lds_fence();
    cnt += __shfl_xor(cnt, 1, 64);
    cnt += __shfl_xor(cnt, 2, 64);
    if (su < N) {                                          // every row below N writes its count and all K entries
        if (sub == 0) n_cand[su] = cnt;
#pragma unroll 1
        for (int j = sub; j < K; j += 4) {
            const int id = li[srow * kFaninLd + j];
            idx[su * K + j] = id == INT_MAX ? -1 : id;
            score[su * K + j] = id == INT_MAX ? -INFINITY : lv[srow * kFaninLd + j];
        }
    }
}

// ---------------------------------------------------------------------------------- thresholded links as per-row lists
// The walk of k_pair_topk without its lists: one workgroup per 64 rows u, the rows' s fragments in registers, the t tiles through
// LDS with the next one prefetched.  Nothing leaves the accumulators: lane (r, q) holds column 16 c + r of rows 4 q + g, so the 16
// lanes of quarter q are one row's 16-column block in ascending column order, and the decision `candidate and reported score >
// threshold` (the expression behind k_pair_topk's n_above) is taken where the score lies.
//   FILL = false: every lane counts its own columns; the 16 lanes of a quarter add up at the end -> n_sel[u].
//   FILL = true : a ballot per (c, g) gives the block's 16 decisions to all of the row's lanes; a lane's slot is the row's cursor plus
//                 the popcount of the lower columns, and the cursor (the same number in the row's 16 lanes) moves on by the block's
//                 popcount through the whole walk.  Ascending columns, no atomics, the same bytes from call to call.  A row writes
//                 only slots in [row_ptr[u], min(row_ptr[u+1], cap)) that are >= 0; what has no room is dropped.
//   SYM = true  : s = t = unit rows (mgv_sim_select_*; trainer.py:158-160 in the arithmetic of digae_layer.py:31-33): row u lists only
//                 v > u, on half the tiles (tile_span<true>, candidate<true>).
//
// The selection consumer: the lane's four rows 4 q + g of its wave — candidate range, slots, cursor (select_rows) — what a decided
// entry of a tile does with them (select_entry), and the counts at the end (select_counts).  The entry is the unit, with its row's
// state as scalars by reference: a function of the whole tile that takes the five arrays (as arguments, or as members of a struct)
// keeps them in memory until after it is inlined, and the general forms of k_pair_select then need 24 - 53 VGPRs more and lose a wave
// in four.  The decision itself — `candidate<SYM>(...) && rep > threshold`, one line on the one statement of `candidate` — stands in
// the kernels' loops over (c, g), as the unions' chains do: behind the call the 16 float compares of a tile of the general forms go
// into VCC one after the other (v_cmp_lt_f32_e32 for _e64), the form that cost k_sim_union 1.6 - 4.9 % (NOTEBOOK 2026-10-19, eighth
// entry; 2026-10-20, tenth entry).
template <bool FILL>
__device__ __forceinline__ void select_rows(const int64_t& N, const int64_t& u0, const int* rlo, const int* rhi, const int64_t* row_ptr,
                                            const int64_t& cap, int (&lo)[4], int (&hi)[4], int (&cnt)[4], int64_t (&base)[4],
                                            uint64_t (&room)[4]) {
    const int w = threadIdx.x >> 6, q = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int lr = 16 * w + 4 * q + g;
        lo[g] = rlo[lr]; hi[g] = rhi[lr]; cnt[g] = 0;
        base[g] = 0; room[g] = 0;
        if (FILL && u0 + lr < N) {
            const int64_t b = row_ptr[u0 + lr], e0 = row_ptr[u0 + lr + 1], e = e0 < cap ? e0 : cap;
            base[g] = b;
            room[g] = e > b ? (uint64_t)e - (uint64_t)b : 0ull;     // exact for any b < e
        }
    }
}

// one decided entry of the tile where it lies: the count or the fill of its row (cnt: the row's count or cursor)
template <bool FILL>
__device__ __forceinline__ void select_entry(const bool& pass, const float& rep, const int64_t& col, int& cnt,
                                             const int64_t& base, const uint64_t& room, int32_t* col_out, float* score_out) {
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    if constexpr (!FILL) {
        cnt += pass ? 1 : 0;
    } else {
        const unsigned bits = (unsigned)(__ballot(pass) >> (16 * q)) & 0xffffu;    // the row's block, bit = column
        const uint64_t i = (uint64_t)(unsigned)cnt + (uint64_t)__popc(bits & ((1u << r) - 1u));
        cnt += __popc(bits);
        if (pass && i < room) {                     // i < room: base + i < min(row_ptr[u+1], cap), no overflow
            const int64_t pos = base + (int64_t)i;
            if (pos >= 0) {
                col_out[pos] = (int32_t)col;
                if (score_out != nullptr) score_out[pos] = rep;
            }
        }
    }
}

// the counts of a row's 16 lanes add up -> n_sel[u]
__device__ __forceinline__ void select_counts(const int64_t& N, const int64_t& row0, const int (&cnt)[4], int32_t* n_sel) {
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        int n = cnt[g];
        n += __shfl_xor(n, 1, 64);
        n += __shfl_xor(n, 2, 64);
        n += __shfl_xor(n, 4, 64);
        n += __shfl_xor(n, 8, 64);
        const int64_t u = row0 + 4 * q + g;
        if (r == 0 && u < N) n_sel[u] = n;
    }
}

template <int H, bool FILL, bool SYM = false>
__global__ __launch_bounds__(kThreads) void k_pair_select(int64_t N, const float* s, int lds, const float* t, int ldt, const int32_t* gp,
                                                          int G, int sigmoid, float threshold, int skip_self, int32_t* n_sel,
                                                          const int64_t* row_ptr, int64_t cap, int32_t* col_out, float* score_out) {
    __shared__ __attribute__((aligned(16))) float tl[kPairTile * PairCfg<H>::LDT];
    __shared__ int rlo[kPairTile], rhi[kPairTile];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int64_t u0 = (int64_t)blockIdx.x * kPairTile;
    row_ranges(N, u0, gp, G, rlo, rhi);
    __syncthreads();
    int64_t clo, chi;
    col_span(N, rlo, rhi, clo, chi);
    const int64_t row0 = u0 + 16 * w;
    int mylo[4], myhi[4], cnt[4];
    int64_t base[4];
    uint64_t room[4];
    select_rows<FILL>(N, u0, rlo, rhi, row_ptr, cap, mylo, myhi, cnt, base, room);
    float a[H / 4];
    load_row_frags<H>(a, s, lds, row0 + r, row0 + r < N, q);
    if (clo < chi) {
        int64_t ct0, ct1;
        tile_span<SYM>(clo, chi, ct0, ct1);
        float4 nxt[H / 16];
        tile_load<H>(nxt, t, ldt, ct0 * kPairTile, N);
        for (int64_t ct = ct0; ct < ct1; ++ct) {
            __syncthreads();
            tile_store<H, PairCfg<H>::LDT>(tl, nxt);
            __syncthreads();
            if (ct + 1 < ct1) tile_load<H>(nxt, t, ldt, (ct + 1) * kPairTile, N);
            f32x4 acc[4];
            tile_scores<H>(acc, a, tl, r, q);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t col = ct * kPairTile + 16 * c + r;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float rep;
                    const bool pass = candidate<SYM>(acc[c][g], col, row0 + 4 * q + g, mylo[g], myhi[g], skip_self, sigmoid, rep) &&
                                      rep > threshold;
                    select_entry<FILL>(pass, rep, col, cnt[g], base[g], room[g], col_out, score_out);
                }
            }
        }
    }
    if (!FILL) select_counts(N, row0, cnt, n_sel);
}

// ---------------------------------------------------------------------------------- classes straight from the walk
// The symmetric walk of k_pair_select<H, ., true> — the same tiles, candidate<true> and `> threshold` — with a union-find as its
// consumer.  Where the fill would store column `col` of row `row`, the pair is united in `parent` (mgv_unionfind.h: every access an
// agent-scope atomic, the smaller root wins, bounded retries).  A cosine is the same bits whichever kernel computes it, so the components
// are exactly those of the list mgv_sim_select_fill writes.  Outside the MFMA section: a lane first decides its 16 entries of the tile
// into a bit mask, then unites the set bits; uf_unite starts with the two finds and leaves when the roots agree, which at a low
// threshold is nearly always.

// The lane's decisions of column tile ct as a mask — bit 4 c + g: the entry (row row0 + 4 q + g, column 16 c + r) — united one set bit
// after the other.  DIAG: an entry may be a row's own column (the cross walk under a self-peer), which unites nothing.
template <bool DIAG>
__device__ __forceinline__ void unite_bits(unsigned bits, const int64_t& row0, const int64_t& ct, int32_t* parent, int32_t* status) {
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    while (bits != 0) {
        const int b = __ffs(bits) - 1;
        bits &= bits - 1;
        const int u = (int)(row0 + 4 * q + (b & 3)), v = (int)(ct * kPairTile + 16 * (b >> 2) + r);
        if (!DIAG || u != v) uf_unite(parent, u, v, status);
    }
}

template <int H>
__global__ __launch_bounds__(kThreads) void k_sim_union(int64_t N, const float* y, int ldy, const int32_t* gp, int G, float threshold,
                                                        int32_t* parent, int32_t* status) {
    __shared__ __attribute__((aligned(16))) float tl[kPairTile * PairCfg<H>::LDT];
    __shared__ int rlo[kPairTile], rhi[kPairTile];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int64_t u0 = (int64_t)blockIdx.x * kPairTile;
    row_ranges(N, u0, gp, G, rlo, rhi);
    __syncthreads();
    int64_t clo, chi;
    col_span(N, rlo, rhi, clo, chi);
    const int64_t row0 = u0 + 16 * w;
    int myhi[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) myhi[g] = rhi[16 * w + 4 * q + g];      // 0 for a row past N: it decides nothing
    float a[H / 4];
    load_row_frags<H>(a, y, ldy, row0 + r, row0 + r < N, q);
    if (clo < chi) {
        int64_t ct0, ct1;
        tile_span<true>(clo, chi, ct0, ct1);
        float4 nxt[H / 16];
        tile_load<H>(nxt, y, ldy, ct0 * kPairTile, N);
        for (int64_t ct = ct0; ct < ct1; ++ct) {
            __syncthreads();
            tile_store<H, PairCfg<H>::LDT>(tl, nxt);
            __syncthreads();
            if (ct + 1 < ct1) tile_load<H>(nxt, y, ldy, (ct + 1) * kPairTile, N);
            f32x4 acc[4];
            tile_scores<H>(acc, a, tl, r, q);
            unsigned bits = 0;                                  // bit 4 c + g: the lane's entry (row 4 q + g, column 16 c + r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t col = ct * kPairTile + 16 * c + r;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float v = acc[c][g];                  // candidate<true>'s statement; the raw score is what is reported
                    const bool pass = MGV_CAND_SYM(v, col, row0 + 4 * q + g, myhi[g]) && v > threshold;
                    bits |= pass ? 1u << (4 * c + g) : 0u;
                }
            }
            unite_bits<false>(bits, row0, ct, parent, status);  // row < col < myhi <= N: both ids inside parent
        }
    }
}

// ---------------------------------------------------------------------------------- the distribution of all-pair scores
// The walk of k_pair_select<H, false, SYM> — the same tiles and candidate<SYM> — with a histogram as its consumer.  Where the count adds
// `rep > threshold`, a candidate is binned by bin = #{j : rep > edges[j]}: a branch-free binary search over the table in LDS, padded
// with +inf (nothing passes it) to 2^p - 1 entries, 2^p the first power of two above B, so that p steps
// `pos += rep > el[pos + step - 1] ? step : 0` from step = 2^(p-1) down to 1 count the edges below rep.  The same `>` on the same bits
// as the count entry: sum(hist[g][j+1:]) IS its total at edges[j].
//
// Accumulation.  A tile's 64 rows are consecutive nodes, so of the graphs they belong to only the first and the last can reach beyond
// the tile; every graph between them lies inside it and has at most 62 nodes.  The first and the last graph get an LDS histogram each
// (kHistSlots), filled with ds atomics and flushed at the end with one global integer atomic per non-zero (graph, bin); the graphs
// between them add straight to hist, at most 62^2 candidates per workgroup in all.  A lane merges consecutive candidates of one
// (graph, bin) in registers through the whole walk before it issues an atomic (run_*), which takes the same-address contention of a
// peaked distribution out of the tile loop.  Integer adds only: exact, and the same bits whatever the order.
// Counters.  One workgroup sees up to 64 (2^31 - 1) candidates, past 32 bits, and a periodic flush would put a barrier and a pass
// over the slots into the tile loop; 64-bit LDS counters (ds_add_u64) cost 2 x 257 x 8 = 4112 B instead.  A lane's run counts at most
// 16 candidates per tile over at most 2^25 tiles: int32.
// LDS at H = 128: score tile 33,792 B + row tables 768 B + edges 2,048 B + counters 4,112 B = 40,720 B against 34,304 B of
// k_pair_select: four workgroups (one wave per SIMD each) would still fit the 160 KB of a CU, 4 x 40,720 = 162,880 <= 163,840.  The
// bound is the registers, as it is for k_pair_select: 154 - 162 VGPRs + 16 AGPRs at H = 128 give 2 waves per SIMD (two workgroups
// per CU, 81 KB of LDS, fit either way), 117 - 121 at H = 64 give 3 (24,336 B each), so the histogram costs no occupancy at any width.
constexpr int kHistMaxEdges = 256;
constexpr int kHistTable = 512;        // >= 2^p - 1 for every B <= kHistMaxEdges
constexpr int kHistSlots = 2;          // the tile's first and last graph

// The histogram consumer: the two tables in LDS, the hist rows of the tile's first and last graph, and the lane's run.  Scalars only,
// so it lives in registers (no scratch in any kernel); the ranges and graphs of the lane's four rows stay arrays of the kernel and
// come to row() one row at a time, for the reason given at select_entry.  What a finished run does — flush: one add to the LDS
// counters of the first or the last graph, or to hist — is a lambda of the kernel that declares those arrays, handed to row() and
// finish(): as a member on pointers kept in the struct, the three adds are generic when the compiler merges them into ONE flat atomic
// on a selected address, LDS counters included (2.4 - 3.0 % on mgv_cross_hist at 64 and 256 edges, NOTEBOOK 2026-10-20, tenth entry).
struct HistRun {
    int B, B1, top, gfirst, glast;
    int run_gi = 0, run_bin = 0, run_n = 0;   // run_n candidates of bin run_bin of graph run_gi that no atomic has seen yet

    // the caller's barrier publishes both tables
    static __device__ __forceinline__ void tables(float* el, unsigned long long* lh, const float* edges, int B) {
        for (int i = threadIdx.x; i < kHistTable; i += kThreads) el[i] = i < B ? edges[i] : INFINITY;
        for (int i = threadIdx.x; i < kHistSlots * (B + 1); i += kThreads) lh[i] = 0ull;
    }

    // behind that barrier; rgi: the graph of each of the tile's rows
    __device__ __forceinline__ HistRun(int B_, int top_, int64_t N, int64_t u0, const int* rgi) : B(B_), B1(B_ + 1), top(top_) {
        const int64_t left = N - 1 - u0;                   // u0 < N: the tile's last row inside N
        gfirst = rgi[0]; glast = rgi[left < kPairTile - 1 ? (int)left : kPairTile - 1];
    }

    // the lane's four entries acc[c][g] of row u in column tile ct (columns 16 c + r); [lo, hi) and gi: the row's candidates and its graph.
    // Row by row: a run lasts as long as the row's scores stay in one bin.
    template <bool SYM, typename Flush>
    __device__ __forceinline__ void row(const f32x4 (&acc)[4], const int& g, const int64_t& ct, const int64_t& u, const int& lo,
                                        const int& hi, const int& gi, const int& skip_self, const int& sigmoid, const float* el,
                                        const Flush& flush) {
        const int r = threadIdx.x & 15;
        bool valid[4], any = false;
        float rep[4];
        int pos[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            valid[c] = candidate<SYM>(acc[c][g], ct * kPairTile + 16 * c + r, u, lo, hi, skip_self, sigmoid, rep[c]);
            any = any || valid[c];
            pos[c] = 0;
        }
        if (__ballot(any) == 0ull) return;                 // the wave has no candidate in these rows of this tile
        for (int step = top; step > 0; step >>= 1) {
#pragma unroll
            for (int c = 0; c < 4; ++c) pos[c] += rep[c] > el[pos[c] + step - 1] ? step : 0;   // <= 2 top - 2 < kHistTable
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!valid[c]) continue;
            const int bin = pos[c] < B ? pos[c] : B;       // an ascending table never gives more; nothing else is indexed
            if (run_n > 0 && run_gi == gi && run_bin == bin) { ++run_n; continue; }
            flush();
            run_gi = gi; run_bin = bin; run_n = 1;
        }
    }

    // after the walk, by every thread of the workgroup: the last run, then one global add per non-zero LDS counter
    template <typename Flush>
    __device__ __forceinline__ void finish(unsigned long long* lh, unsigned long long* hist, const Flush& flush) {
        flush();
        __syncthreads();
        for (int i = threadIdx.x; i < kHistSlots * B1; i += kThreads) {
            const unsigned long long n = lh[i];
            if (n != 0ull) atomicAdd(&hist[(int64_t)(i < B1 ? gfirst : glast) * B1 + (i < B1 ? i : i - B1)], n);
        }
    }
};

template <int H, bool SYM>
__global__ __launch_bounds__(kThreads) void k_pair_hist(int64_t N, const float* s, int lds, const float* t, int ldt, const int32_t* gp,
                                                        int G, int sigmoid, int skip_self, const float* edges, int B, int top,
                                                        unsigned long long* hist) {
    __shared__ __attribute__((aligned(16))) float tl[kPairTile * PairCfg<H>::LDT];
    __shared__ int rlo[kPairTile], rhi[kPairTile], rgi[kPairTile];
    __shared__ float el[kHistTable];
    __shared__ unsigned long long lh[kHistSlots * (kHistMaxEdges + 1)];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int64_t u0 = (int64_t)blockIdx.x * kPairTile;
    row_ranges<true>(N, u0, gp, G, rlo, rhi, rgi);         // rgi: a row of hist
    HistRun::tables(el, lh, edges, B);
    __syncthreads();
    int64_t clo, chi;
    col_span(N, rlo, rhi, clo, chi);
    const int64_t row0 = u0 + 16 * w;
    HistRun run(B, top, N, u0, rgi);
    auto flush = [&]() {
        if (run.run_n > 0) {
            if (run.run_gi == run.gfirst) atomicAdd(&lh[run.run_bin], (unsigned long long)run.run_n);
            else if (run.run_gi == run.glast) atomicAdd(&lh[run.B1 + run.run_bin], (unsigned long long)run.run_n);
            else atomicAdd(&hist[(int64_t)run.run_gi * run.B1 + run.run_bin], (unsigned long long)run.run_n);
        }
    };
    int mylo[4], myhi[4], mygi[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int lr = 16 * w + 4 * q + g;
        mylo[g] = rlo[lr]; myhi[g] = rhi[lr]; mygi[g] = rgi[lr];
    }
    float a[H / 4];
    load_row_frags<H>(a, s, lds, row0 + r, row0 + r < N, q);
    if (clo < chi) {
        int64_t ct0, ct1;
        tile_span<SYM>(clo, chi, ct0, ct1);
        float4 nxt[H / 16];
        tile_load<H>(nxt, t, ldt, ct0 * kPairTile, N);
        for (int64_t ct = ct0; ct < ct1; ++ct) {
            __syncthreads();
            tile_store<H, PairCfg<H>::LDT>(tl, nxt);
            __syncthreads();
            if (ct + 1 < ct1) tile_load<H>(nxt, t, ldt, (ct + 1) * kPairTile, N);
            f32x4 acc[4];
            tile_scores<H>(acc, a, tl, r, q);
#pragma unroll
            for (int g = 0; g < 4; ++g)
                run.template row<SYM>(acc, g, ct, row0 + 4 * q + g, mylo[g], myhi[g], mygi[g], skip_self, sigmoid, el, flush);
        }
    }
    run.finish(lh, hist, flush);
}

// ---------------------------------------------------------------------------------- ranks: counts against each row's own thresholds
// The walk of k_pair_select<H, false> — the same tiles and candidate<false> on the raw score — where the count compares with one scalar
// for everybody, a row compares with ITS list thr[thr_ptr[u] .. thr_ptr[u+1]) (ascending, NaNs last: the entry's contract) and every
// listed j gets n_gt[j] = #{candidates > thr[j]} and n_eq[j] = #{candidates == thr[j]}: the rank of a true link among all candidates of
// its node, as integers, when thr holds mgv_pair_scores_at of the row's links (the same bits the walk compares).
// Passes.  A list is taken kRankPass = 32 entries at a time: in pass p row i holds entries [32 p, 32 p + 32) of its list in tb (LDS,
// padded with +inf) and the tile repeats its column walk until its longest list is done; a tile whose rows list nothing walks nothing.
// Counting.  A score first meets the row's smallest threshold of the pass (rmin, in registers; NaN for an empty list: nothing passes) —
// a trained decoder scores true links high, so nearly every candidate leaves there.  The rest take a branch-free binary search,
// pos = #{entries of the pass < v} in 0 .. 32 (six dependent LDS reads; a row that lists at most two entries in the pass — a gate's
// fan-ins — answers from two registers instead: 1.60 -> 1.25 times the count walk on a fitted 65,536-node AIG, 2.91 -> 1.63 on random
// rows, NOTEBOOK 2026-10-19, ninth entry), and add 1 to cgt[row][pos] (pos = 0 says nothing: v is above none) and, where
// tb[row][pos] == v, to ceq[row][pos] — the first of the entries equal to v.  int32 ds atomics: exact in any order, and a row has fewer
// than 2^31 candidates.  After the walk entry k of a row reads n_gt = sum of cgt[row][b] over b > k (ascending: v > thr_k exactly when
// pos > k) and n_eq = sum of ceq[row][b] over the b of the pass with tb[b] == tb[k] (duplicates share the first one's counter), and
// WRITES both with plain stores; a NaN threshold writes (0, 0).  Every listed j has one owner (its row's workgroup, its pass): no
// global atomics, nothing to zero beforehand, the same bytes from call to call.
// Whatever thr_ptr holds, a row's range is clamped into [0, T) as row_ranges clamps graph_ptr, and a list that does not ascend only
// makes its own counts meaningless: pos stays in 0 .. 32.
// LDS: score tile + 2 x 64 x 33 counters (16,896 B) + 64 x 33 thresholds (8,448 B) + 1,024 B of row tables = 60,160 B at H = 128
// (two workgroups per CU), 43,776 B at H = 64, 35,584 B at H = 32, 31,488 B at H = 16.  Waves per SIMD: 2 at H = 128 (229 VGPRs + 20
// AGPRs, as k_pair_select<128>) and at H = 64 (163 + 20), 3 at H = 32 (139 + 20) and H = 16 (125 + 20); registers bound it, not LDS.
constexpr int kRankPass = 32;
constexpr int kRankLd = kRankPass + 1;     // row stride of tb / cgt / ceq: bin 32 exists, and the four rows of a lane lie in four banks

template <int H>
__global__ __launch_bounds__(kThreads) void k_pair_rank(int64_t N, const float* s, int lds, const float* t, int ldt, const int32_t* gp,
                                                        int G, int skip_self, const int32_t* thr_ptr, int T, const float* thr,
                                                        int32_t* n_gt, int32_t* n_eq) {
    __shared__ __attribute__((aligned(16))) float tl[kPairTile * PairCfg<H>::LDT];
    __shared__ int rlo[kPairTile], rhi[kPairTile], lb[kPairTile], ln[kPairTile];
    __shared__ float tb[kPairTile * kRankLd];
    __shared__ int cgt[kPairTile * kRankLd], ceq[kPairTile * kRankLd];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int64_t u0 = (int64_t)blockIdx.x * kPairTile;
    row_ranges(N, u0, gp, G, rlo, rhi);
    if (threadIdx.x < kPairTile) {                         // the row's list [lb, lb + ln): inside [0, T) whatever thr_ptr holds
        const int64_t u = u0 + threadIdx.x;
        int b = 0, e = 0;
        if (u < N) {
            b = thr_ptr[u]; e = thr_ptr[u + 1];
            b = b < 0 ? 0 : (b > T ? T : b);
            e = e < b ? b : (e > T ? T : e);
        }
        lb[threadIdx.x] = b; ln[threadIdx.x] = e - b;
    }
    __syncthreads();
    int64_t clo, chi;
    col_span(N, rlo, rhi, clo, chi);
    int longest = 0;
    for (int i = 0; i < kPairTile; ++i) longest = ln[i] > longest ? ln[i] : longest;
    const int64_t row0 = u0 + 16 * w;
    const int sigmoid = 0;                                 // ranks are by the raw score, the order of k_pair_topk
    int mylo[4], myhi[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) { mylo[g] = rlo[16 * w + 4 * q + g]; myhi[g] = rhi[16 * w + 4 * q + g]; }
    float a[H / 4];
    load_row_frags<H>(a, s, lds, row0 + r, row0 + r < N, q);
    for (int p0 = 0; p0 < longest; p0 += kRankPass) {
        __syncthreads();                                   // the previous pass has read its counters
        for (int e = threadIdx.x; e < kPairTile * kRankLd; e += kThreads) {
            const int i = e / kRankLd, k = e % kRankLd;
            tb[e] = (k < kRankPass && p0 + k < ln[i]) ? thr[lb[i] + p0 + k] : INFINITY;
            cgt[e] = 0; ceq[e] = 0;
        }
        __syncthreads();
        float rmin[4], rsec[4];                            // a list of one or two (a gate's fan-ins) is searched in registers
        bool two[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int lr = 16 * w + 4 * q + g;
            rmin[g] = p0 < ln[lr] ? tb[lr * kRankLd] : NAN;
            rsec[g] = tb[lr * kRankLd + 1];
            two[g] = ln[lr] - p0 <= 2;
        }
        if (clo < chi) {
            int64_t ct0, ct1;
            tile_span<false>(clo, chi, ct0, ct1);
            float4 nxt[H / 16];
            tile_load<H>(nxt, t, ldt, ct0 * kPairTile, N);
            for (int64_t ct = ct0; ct < ct1; ++ct) {
                __syncthreads();
                tile_store<H, PairCfg<H>::LDT>(tl, nxt);
                __syncthreads();
                if (ct + 1 < ct1) tile_load<H>(nxt, t, ldt, (ct + 1) * kPairTile, N);
                f32x4 acc[4];
                tile_scores<H>(acc, a, tl, r, q);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int64_t col = ct * kPairTile + 16 * c + r;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        float v;
                        if (!(candidate<false>(acc[c][g], col, row0 + 4 * q + g, mylo[g], myhi[g], skip_self, sigmoid, v) && v >= rmin[g]))
                            continue;
                        const int base = (16 * w + 4 * q + g) * kRankLd;
                        int pos = 0;
                        float at;                              // tb[pos]
                        if (two[g]) {                          // entries 2 .. of the pass are +inf
                            pos = (rmin[g] < v ? 1 : 0) + (rsec[g] < v ? 1 : 0);
                            at = pos == 0 ? rmin[g] : (pos == 1 ? rsec[g] : INFINITY);
                        } else {
#pragma unroll
                            for (int step = kRankPass / 2; step > 0; step >>= 1) pos += tb[base + pos + step - 1] < v ? step : 0;   // <= 31
                            pos += tb[base + pos] < v ? 1 : 0; // <= 32: column 32 of tb is +inf and is never below v
                            at = tb[base + pos];
                        }
                        if (pos > 0) atomicAdd(&cgt[base + pos], 1);
                        if (at == v) atomicAdd(&ceq[base + pos], 1);     // (bin 32, the padding, is never read back)
                    }
                }
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < kPairTile * kRankPass; e += kThreads) {
            const int i = e / kRankPass, k = e % kRankPass;
            if (p0 + k >= ln[i]) continue;
            const float x = tb[i * kRankLd + k];
            int gt = 0, eq = 0;
            for (int b = 0; b <= kRankPass; ++b) {
                gt += b > k ? cgt[i * kRankLd + b] : 0;
                eq += (b < kRankPass && tb[i * kRankLd + b] == x) ? ceq[i * kRankLd + b] : 0;
            }
            const int j = lb[i] + p0 + k;                  // < T
            n_gt[j] = x == x ? gt : 0;
            n_eq[j] = eq;                                  // NaN == anything is false: 0
        }
    }
}

// ---------------------------------------------------------------------------------- candidates in ANOTHER graph: matching across circuits
// The walk of k_pair_topk / k_pair_select on unit rows (s = t = y, the raw score) where the candidates of a row of graph g are ALL rows
// of graph peer[g] (peer[g] = -1: none; peer[g] = g: the row's own graph, itself included).  hf depends only on a circuit's own
// structure, so rows of two graphs of one batch are comparable as they stand: a golden design against its revision.
// What differs from the walk above is only WHERE the candidates lie: a row tile's rows may belong to several graphs whose peers lie
// far apart, so the column tiles are not one range but a few.  cross_spans leaves them in LDS as ascending disjoint spans of column
// tiles, and the tile loop — the same five lines — stands once inside a loop over the spans; a column tile that holds no candidate of
// any of the 64 rows is never loaded or scored.  With one span (two large graphs) the loop is the one k_pair_topk runs.
// Each kernel below is cross_ranges and cross_spans, that loop, and the CONSUMER of its own-graph twin — topk_*, select_*, HistRun,
// unite_bits, with candidate<false> on the raw score and no skip_self — called, not restated (NOTEBOOK 2026-10-20, tenth entry).

// The column tiles that hold a candidate of any of the 64 rows: *ns ascending, disjoint, non-adjacent spans [ta[j], tb[j]).  Wave 0
// does it behind the barrier that publishes the ranges; the caller's next barrier publishes the spans.  Rows of one graph follow each
// other, so a range counts once, at its first row (at most 64 ranges): each lane ranks its range among them by first tile (a rank sort
// over a ballot of the first rows), then lane 0 merges the sorted ranges that overlap or touch.
__device__ __forceinline__ void cross_spans(const int* rlo, const int* rhi, int* ta, int* tb, int* ns) {
    if (threadIdx.x >= kPairTile) return;
    const int i = threadIdx.x, lo = rlo[i], hi = rhi[i];
    const bool first = lo < hi && (i == 0 || lo != rlo[i - 1] || hi != rhi[i - 1]);
    const int t0 = lo / kPairTile, t1 = (hi + kPairTile - 1) / kPairTile;
    const uint64_t firsts = __ballot(first);
    int rank = 0;
    for (uint64_t m = firsts; m != 0ull; m &= m - 1) {
        const int j = __ffsll((unsigned long long)m) - 1, tj = rlo[j] / kPairTile;
        rank += (tj < t0 || (tj == t0 && j < i)) ? 1 : 0;
    }
    if (first) { ta[rank] = t0; tb[rank] = t1; }
    wave_lds_fence();
    if (i == 0) {
        const int n = __popcll(firsts);
        int out = 0, end = 0;
        for (int j = 0; j < n; ++j) {
            const int a = ta[j], b = tb[j];                // read before slot out <= j is written
            if (out > 0 && a <= end) { end = b > end ? b : end; }
            else { ta[out] = a; end = b; ++out; }
            tb[out - 1] = end;
        }
        *ns = out;
    }
}

// k_pair_topk's consumer — the blocks through LDS, four lanes per row, the sorted list per row — on the spans of cross_spans.
template <int H>
__global__ __launch_bounds__(kThreads) void k_cross_topk(int64_t N, const float* y, int ldy, const int32_t* gp, int G, const int32_t* peer,
                                                         int k, float threshold, int32_t* idx, float* score, int32_t* n_above) {
    __shared__ __attribute__((aligned(16))) float tl[kPairTile * PairCfg<H>::LDT];
    __shared__ float sc[kPairTile * kTopkScLd];
    __shared__ float lv[kPairTile * kTopkMax];
    __shared__ int li[kPairTile * kTopkMax];
    __shared__ int rlo[kPairTile], rhi[kPairTile], ta[kPairTile], tb[kPairTile], ns;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int64_t u0 = (int64_t)blockIdx.x * kPairTile;
    cross_ranges(N, u0, gp, G, peer, rlo, rhi);
    const int srow = 16 * w + (lane >> 2), sub = lane & 3;
    topk_init(lv, li, srow, sub);
    __syncthreads();
    cross_spans(rlo, rhi, ta, tb, &ns);
    __syncthreads();
    const int64_t su = u0 + srow;                          // the row this lane scans for
    const int mylo = rlo[srow], myhi = rhi[srow], spans = ns;
    const int no = 0;                                      // no skip_self, no sigmoid: a row of a self-peer is its own candidate
    const int64_t row0 = u0 + 16 * w;
    float a[H / 4];
    load_row_frags<H>(a, y, ldy, row0 + r, row0 + r < N, q);
    int cnt = 0;
    for (int sp = 0; sp < spans; ++sp) {
        const int64_t ct0 = ta[sp], ct1 = tb[sp];
        float4 nxt[H / 16];
        tile_load<H>(nxt, y, ldy, ct0 * kPairTile, N);
        for (int64_t ct = ct0; ct < ct1; ++ct) {
            __syncthreads();
            tile_store<H, PairCfg<H>::LDT>(tl, nxt);
            __syncthreads();
            if (ct + 1 < ct1) tile_load<H>(nxt, y, ldy, (ct + 1) * kPairTile, N);
            f32x4 acc[4];
            tile_scores<H>(acc, a, tl, r, q);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t cb = ct * kPairTile + 16 * c;
                topk_block(acc[c], cb, su, mylo, myhi, k, no, threshold, no, sc, lv, li, cnt, w, r, q, srow, sub);
            }
        }
    }
    topk_write(N, su, k, no, cnt, lv, li, idx, score, n_above, srow, sub);
}

// k_pair_select's consumer — the decision where the score lies, FILL = false: counts, FILL = true: ballot, prefix popcount and the row's
// cursor — on the spans of cross_spans.  The spans ascend and a row's candidates lie in one of them: ascending ids, no atomics.
template <int H, bool FILL>
__global__ __launch_bounds__(kThreads) void k_cross_select(int64_t N, const float* y, int ldy, const int32_t* gp, int G, const int32_t* peer,
                                                           float threshold, int32_t* n_sel, const int64_t* row_ptr, int64_t cap,
                                                           int32_t* col_out, float* score_out) {
    __shared__ __attribute__((aligned(16))) float tl[kPairTile * PairCfg<H>::LDT];
    __shared__ int rlo[kPairTile], rhi[kPairTile], ta[kPairTile], tb[kPairTile], ns;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int64_t u0 = (int64_t)blockIdx.x * kPairTile;
    cross_ranges(N, u0, gp, G, peer, rlo, rhi);
    __syncthreads();
    cross_spans(rlo, rhi, ta, tb, &ns);
    __syncthreads();
    const int64_t row0 = u0 + 16 * w;
    const int spans = ns, no = 0;
    int mylo[4], myhi[4], cnt[4];
    int64_t base[4];
    uint64_t room[4];
    select_rows<FILL>(N, u0, rlo, rhi, row_ptr, cap, mylo, myhi, cnt, base, room);
    float a[H / 4];
    load_row_frags<H>(a, y, ldy, row0 + r, row0 + r < N, q);
    for (int sp = 0; sp < spans; ++sp) {
        const int64_t ct0 = ta[sp], ct1 = tb[sp];
        float4 nxt[H / 16];
        tile_load<H>(nxt, y, ldy, ct0 * kPairTile, N);
        for (int64_t ct = ct0; ct < ct1; ++ct) {
            __syncthreads();
            tile_store<H, PairCfg<H>::LDT>(tl, nxt);
            __syncthreads();
            if (ct + 1 < ct1) tile_load<H>(nxt, y, ldy, (ct + 1) * kPairTile, N);
            f32x4 acc[4];
            tile_scores<H>(acc, a, tl, r, q);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t col = ct * kPairTile + 16 * c + r;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float rep;
                    const bool pass = candidate<false>(acc[c][g], col, row0 + 4 * q + g, mylo[g], myhi[g], no, no, rep) && rep > threshold;
                    select_entry<FILL>(pass, rep, col, cnt[g], base[g], room[g], col_out, score_out);
                }
            }
        }
    }
    if (!FILL) select_counts(N, row0, cnt, n_sel);
}

// ---------------------------------------------------------------------------------- cross classes straight from the walk
// The walk of k_cross_select<H, true> — the same spans, tiles, candidate<false> on the raw cosine and `> threshold` — with k_sim_union's
// consumer: where the fill would store column `col` in row `row`'s list, the pair is united in `parent` (mgv_unionfind.h).  A lane
// decides its 16 entries of the tile into a bit mask and unites the set bits outside the MFMA section.  A cosine is the same bits
// whichever kernel computes it and a root is only hooked under a smaller root, so the components are exactly those of the list
// mgv_cross_select_fill writes.  row == col (a row of a self-peer) unites nothing, as in mgv_cc_union_pairs.
// Ids: a row decides something only when its range is not empty, which cross_ranges grants only to a row below N, and a column passes
// only inside [rlo, rhi), clamped into [0, N]: both ids lie inside parent whatever graph_ptr and peer hold.
// With an involutive peer every pair is met from both sides; the second meeting is two finds and an exit.  The rows of the higher
// graph of such a couple are NOT skipped: a row tile holds rows of several graphs, so the skip saves tiles only where a whole tile
// belongs to one skipped graph, and it would make the kernel's spans differ from the fill's (NOTEBOOK 2026-10-20).
// LDS: score tile + 1,028 B of tables = 34,820 B at H = 128, 18,436 B at H = 64, 10,244 B at H = 32, 6,148 B at H = 16.  The
// compiler's resource report: 159 VGPRs + 16 AGPRs and 2 waves per SIMD at H = 128, 109 + 16 and 4 at H = 64, 92 + 16 and 4 at
// H = 32, 72 + 8 and 6 at H = 16, nothing spilled: at least the waves of k_cross_select<H, false> at every width.
template <int H>
__global__ __launch_bounds__(kThreads) void k_cross_union(int64_t N, const float* y, int ldy, const int32_t* gp, int G, const int32_t* peer,
                                                          float threshold, int32_t* parent, int32_t* status) {
    __shared__ __attribute__((aligned(16))) float tl[kPairTile * PairCfg<H>::LDT];
    __shared__ int rlo[kPairTile], rhi[kPairTile], ta[kPairTile], tb[kPairTile], ns;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int64_t u0 = (int64_t)blockIdx.x * kPairTile;
    cross_ranges(N, u0, gp, G, peer, rlo, rhi);
    __syncthreads();
    cross_spans(rlo, rhi, ta, tb, &ns);
    __syncthreads();
    const int64_t row0 = u0 + 16 * w;
    const int spans = ns, no = 0;
    int mylo[4], myhi[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) { mylo[g] = rlo[16 * w + 4 * q + g]; myhi[g] = rhi[16 * w + 4 * q + g]; }   // empty for a row past N
    float a[H / 4];
    load_row_frags<H>(a, y, ldy, row0 + r, row0 + r < N, q);
    for (int sp = 0; sp < spans; ++sp) {
        const int64_t ct0 = ta[sp], ct1 = tb[sp];
        float4 nxt[H / 16];
        tile_load<H>(nxt, y, ldy, ct0 * kPairTile, N);
        for (int64_t ct = ct0; ct < ct1; ++ct) {
            __syncthreads();
            tile_store<H, PairCfg<H>::LDT>(tl, nxt);
            __syncthreads();
            if (ct + 1 < ct1) tile_load<H>(nxt, y, ldy, (ct + 1) * kPairTile, N);
            f32x4 acc[4];
            tile_scores<H>(acc, a, tl, r, q);
            unsigned bits = 0;                                  // bit 4 c + g: the lane's entry (row 4 q + g, column 16 c + r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t col = ct * kPairTile + 16 * c + r;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float rep;
                    const bool pass = candidate<false>(acc[c][g], col, row0 + 4 * q + g, mylo[g], myhi[g], no, no, rep) && rep > threshold;
                    bits |= pass ? 1u << (4 * c + g) : 0u;
                }
            }
            unite_bits<true>(bits, row0, ct, parent, status);   // row < N and mylo <= col < myhi <= N: both ids inside parent
        }
    }
}

// ---------------------------------------------------------------------------------- the distribution of cross scores
// The walk of k_cross_select<H, false> — the same spans, tiles and candidate<false> on the raw cosine — with k_pair_hist's consumer:
// a candidate of a row of graph g is binned by bin = #{j : cos > edges[j]} into hist[g] (the ROW's graph, not the peer's), with the
// branch-free binary search over the +inf-padded table in LDS, the 64-bit LDS counters for the tile's first and last row graph, direct
// 64-bit integer adds for the graphs between them and the per-lane run merge, all as described there.  What differs is how much a graph
// between the first and the last can add directly: it has at most 62 rows, but each of them has all rows of the peer as candidates,
// not 62; the run merge (a lane's consecutive candidates of one (graph, bin) are one add) is what bounds those adds.
// Integer atomics only: exact, the same bytes from call to call.  A lane's run counts at most 16 candidates per tile: int32.
// LDS at H = 128: score tile 33,792 B + three row tables 768 B + two span tables and their count 516 B + edges 2,048 B + counters
// 4,112 B = 41,240 B with the counters' alignment; 24,856 B at H = 64, 16,664 B at H = 32, 12,568 B at H = 16.  Registers and waves
// per SIMD as the compiler's resource report has them (-Rpass-analysis=kernel-resource-usage): H = 128: 153 VGPRs + 16 AGPRs, 2 waves;
// H = 64: 111 + 16, 4 waves; H = 32: 88 + 16, 4 waves; H = 16: 77 + 16, 5 waves — against 2 / 3 / 4 / 5 of k_cross_select<H, false>
// (176, 116, 85 and 69 VGPRs + 16): the histogram costs the count walk no occupancy at any width.  Registers bound it, not LDS: the
// waves the registers allow are at most five workgroups per CU, 5 x 12,568 B at H = 16 and 2 x 41,240 B at H = 128 of its 160 KB.
template <int H>
__global__ __launch_bounds__(kThreads) void k_cross_hist(int64_t N, const float* y, int ldy, const int32_t* gp, int G, const int32_t* peer,
                                                         const float* edges, int B, int top, unsigned long long* hist) {
    __shared__ __attribute__((aligned(16))) float tl[kPairTile * PairCfg<H>::LDT];
    __shared__ int rlo[kPairTile], rhi[kPairTile], rgi[kPairTile], ta[kPairTile], tb[kPairTile], ns;
    __shared__ float el[kHistTable];
    __shared__ unsigned long long lh[kHistSlots * (kHistMaxEdges + 1)];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int64_t u0 = (int64_t)blockIdx.x * kPairTile;
    cross_ranges<true>(N, u0, gp, G, peer, rlo, rhi, rgi); // rgi: a row of hist
    HistRun::tables(el, lh, edges, B);
    __syncthreads();
    cross_spans(rlo, rhi, ta, tb, &ns);
    __syncthreads();
    const int64_t row0 = u0 + 16 * w;
    const int spans = ns, no = 0;
    HistRun run(B, top, N, u0, rgi);
    auto flush = [&]() {
        if (run.run_n > 0) {
            if (run.run_gi == run.gfirst) atomicAdd(&lh[run.run_bin], (unsigned long long)run.run_n);
            else if (run.run_gi == run.glast) atomicAdd(&lh[run.B1 + run.run_bin], (unsigned long long)run.run_n);
            else atomicAdd(&hist[(int64_t)run.run_gi * run.B1 + run.run_bin], (unsigned long long)run.run_n);
        }
    };
    int mylo[4], myhi[4], mygi[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int lr = 16 * w + 4 * q + g;
        mylo[g] = rlo[lr]; myhi[g] = rhi[lr]; mygi[g] = rgi[lr];
    }
    float a[H / 4];
    load_row_frags<H>(a, y, ldy, row0 + r, row0 + r < N, q);
    for (int sp = 0; sp < spans; ++sp) {
        const int64_t ct0 = ta[sp], ct1 = tb[sp];
        float4 nxt[H / 16];
        tile_load<H>(nxt, y, ldy, ct0 * kPairTile, N);
        for (int64_t ct = ct0; ct < ct1; ++ct) {
            __syncthreads();
            tile_store<H, PairCfg<H>::LDT>(tl, nxt);
            __syncthreads();
            if (ct + 1 < ct1) tile_load<H>(nxt, y, ldy, (ct + 1) * kPairTile, N);
            f32x4 acc[4];
            tile_scores<H>(acc, a, tl, r, q);
#pragma unroll
            for (int g = 0; g < 4; ++g)
                run.template row<false>(acc, g, ct, row0 + 4 * q + g, mylo[g], myhi[g], mygi[g], no, no, el, flush);
        }
    }
    run.finish(lh, hist, flush);
}

// ---------------------------------------------------------------------------------- unit rows
// y[i] = x[i] / max(|x[i]|, eps), the per-row clamp of torch.cosine_similarity (trainer.py:158-160) and of k_func_dist.  H / 4 lanes per
// row, one float4 each; the sum of squares meets in the row's lanes in float32.  A NaN norm is kept (NaN < eps is false): the whole
// row comes out NaN.  A row is read in full before any of it is written, so y may be x.
template <int H>
__global__ __launch_bounds__(kThreads) void k_row_unit(int64_t N, const float* x, int ldx, float eps, float* y, int ldy, float* norm) {
    constexpr int LPR = H / 4, RPB = kThreads / LPR;
    const int lr = threadIdx.x % LPR;
    for (int64_t i = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR; i < N; i += (int64_t)gridDim.x * RPB) {
        const float4 v = ld4(x + i * (int64_t)ldx + 4 * lr);
        const float n = sqrtf(group_sum<LPR>(dot4(v, v)));
        const float d = n < eps ? eps : n;
        st4(y + i * (int64_t)ldy + 4 * lr, make_float4(v.x / d, v.y / d, v.z / d, v.w / d));
        if (norm != nullptr && lr == 0) norm[i] = n;
    }
}

inline bool pair_h_ok(int H) { return has_width(AllWidths{}, H); }
inline bool pair_rows_ok(const float* x, int ld, int H) { return x != nullptr && ld >= H && ld % 4 == 0 && ((uintptr_t)x & 15) == 0; }

}  // namespace mgv

using mgv::dispatch_width;
using mgv::launch_width;

extern "C" int mgv_pair_scores_fwd(int H, int64_t M, int64_t N, const float* s, int lds, const float* t, int ldt, int sigmoid,
                                   float* out, int64_t ldo, void* stream) {
    if (!mgv::pair_h_ok(H)) return MGV_EUNSUPPORTED;
    MGV_CHECK_ARG(M >= 0 && N >= 0);
    if (M == 0 || N == 0) return MGV_OK;
    MGV_CHECK_ARG(mgv::pair_rows_ok(s, lds, H) && mgv::pair_rows_ok(t, ldt, H) && out != nullptr && ldo >= N);
    const int64_t nrt = (M + mgv::kPairTile - 1) / mgv::kPairTile, nct = (N + mgv::kPairTile - 1) / mgv::kPairTile;
    const int64_t chunks = (nct + mgv::kPairChunk - 1) / mgv::kPairChunk;
    if (nrt > 0x7fffffffLL || chunks > 65535) return MGV_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    return launch_width(mgv::AllWidths{}, H, [&](auto w) {
        hipLaunchKernelGGL(mgv::k_pair_fwd<w>, dim3((unsigned)nrt, (unsigned)chunks), dim3(mgv::kThreads), 0, st, M, N, s, lds, t, ldt, sigmoid, out, ldo);
    });
}

extern "C" int mgv_pair_scores_bwd(int H, int64_t M, int64_t N, const float* s, int lds, const float* t, int ldt, int sigmoid,
                                   const float* out, int64_t ldo, const float* gout, int64_t ldg, float* ds, int ldds, float* dt,
                                   int lddt, void* stream) {
    if (!mgv::pair_h_ok(H)) return MGV_EUNSUPPORTED;
    MGV_CHECK_ARG(M >= 0 && N >= 0);
    MGV_CHECK_ARG(ds == nullptr || ldds >= H);
    MGV_CHECK_ARG(dt == nullptr || lddt >= H);
    const bool want_ds = ds != nullptr && M > 0, want_dt = dt != nullptr && N > 0;
    if (!want_ds && !want_dt) return MGV_OK;
    if (M > 0 && N > 0) {
        MGV_CHECK_ARG(gout != nullptr && ldg >= N && (!sigmoid || (out != nullptr && ldo >= N)));
        MGV_CHECK_ARG(!want_ds || mgv::pair_rows_ok(t, ldt, H));
        MGV_CHECK_ARG(!want_dt || mgv::pair_rows_ok(s, lds, H));
    }
    const int64_t bs = (M + mgv::kPairTile - 1) / mgv::kPairTile, bt = (N + mgv::kPairTile - 1) / mgv::kPairTile;
    if (bs > 0x7fffffffLL || bt > 0x7fffffffLL) return MGV_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    return dispatch_width(mgv::AllWidths{}, H, [&](auto w) {
        if (want_ds) {      // an empty walked dimension leaves zeros
            hipLaunchKernelGGL((mgv::k_pair_bwd<w, false>), dim3((unsigned)bs), dim3(mgv::kThreads), 0, st, M, N, t, ldt, sigmoid, out, ldo, gout, ldg, ds, ldds);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return (int)e;
        }
        if (want_dt) hipLaunchKernelGGL((mgv::k_pair_bwd<w, true>), dim3((unsigned)bt), dim3(mgv::kThreads), 0, st, N, M, s, lds, sigmoid, out, ldo, gout, ldg, dt, lddt);
        MGV_LAUNCH_RET();
    });
}

extern "C" int mgv_pair_scores_at(int H, int64_t E, const float* s, int lds, const float* t, int ldt, const int64_t* src,
                                  const int64_t* dst, int sigmoid, float* out, void* stream) {
    if (!mgv::pair_h_ok(H)) return MGV_EUNSUPPORTED;
    MGV_CHECK_ARG(E >= 0);
    if (E == 0) return MGV_OK;
    MGV_CHECK_ARG(mgv::pair_rows_ok(s, lds, H) && mgv::pair_rows_ok(t, ldt, H) && src != nullptr && dst != nullptr && out != nullptr);
    hipStream_t st = (hipStream_t)stream;
    const int grid = mgv::grid_for((E + mgv::kThreads - 1) / mgv::kThreads, 8);
    return launch_width(mgv::AllWidths{}, H, [&](auto w) {
        hipLaunchKernelGGL(mgv::k_pair_at<w>, dim3(grid), dim3(mgv::kThreads), 0, st, E, s, lds, t, ldt, src, dst, sigmoid, out);
    });
}

// the arguments every walk entry shares, checked in this order by all of them; *launch = false: nothing to walk
static int pair_walk_args(int H, int64_t N, const float* s, int lds, const float* t, int ldt, const int32_t* graph_ptr, int G,
                          hipStream_t st, bool* launch) {
    *launch = false;
    if (!mgv::pair_h_ok(H)) return MGV_EUNSUPPORTED;
    MGV_CHECK_ARG(N >= 0 && N <= 0x7fffffffLL);                           // node ids are int32
    MGV_CHECK_ARG(graph_ptr == nullptr || G >= 0);
    if (graph_ptr != nullptr) {
        // the table must start at 0 and end at N: its two ends are read back (the only blocking step; NULL skips it)
        int32_t ends[2] = {0, 0};
        hipError_t e = hipMemcpyAsync(&ends[0], graph_ptr, sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&ends[1], graph_ptr + G, sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return (int)e;
        MGV_CHECK_ARG(ends[0] == 0 && (int64_t)ends[1] == N);
    }
    if (N == 0) return MGV_OK;
    MGV_CHECK_ARG(mgv::pair_rows_ok(s, lds, H) && mgv::pair_rows_ok(t, ldt, H));
    *launch = true;
    return MGV_OK;
}

// a walk kernel's launch: one workgroup per 64 rows
template <typename K, typename... A>
static void launch_row_tiles(K kernel, int64_t N, hipStream_t st, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((N + mgv::kPairTile - 1) / mgv::kPairTile)), dim3(mgv::kThreads), 0, st, args...);
}

// the arguments the cross entries share, in the order of the walk entries: the width, both tables present, pair_walk_args on (y, y),
// then every entry of peer in [-1, G) — the table is read back whole (G int32s, one more small blocking copy beside graph_ptr's ends)
static int cross_walk_args(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, const int32_t* peer, hipStream_t st,
                           bool* launch) {
    *launch = false;
    if (!mgv::pair_h_ok(H)) return MGV_EUNSUPPORTED;
    MGV_CHECK_ARG(graph_ptr != nullptr && peer != nullptr && G >= 0);
    const int rc = pair_walk_args(H, N, y, ldy, y, ldy, graph_ptr, G, st, launch);
    if (rc != MGV_OK) return rc;
    if (G > 0) {
        std::vector<int32_t> p((size_t)G);
        hipError_t e = hipMemcpyAsync(p.data(), peer, sizeof(int32_t) * (size_t)G, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return (int)e;
        for (int g = 0; g < G; ++g) MGV_CHECK_ARG(p[g] >= -1 && p[g] < G);
    }
    return MGV_OK;
}

// What the entries of one walk share, in its three forms.  general: rows s against rows t, each row's candidates its own graph (the
// whole batch without a table).  sym: s = t = unit rows, row u takes only v > u; `sigmoid` and `skip_self` are 0.  cross: s = t = unit
// rows, the candidates of a row of graph g are the rows of graph peer[g]; `sigmoid` and `skip_self` are 0.
// The form selects the argument check and the kernel; every check sequence behind it exists once, in the *_run helpers below.
enum class Walk { general, sym, cross };
struct WalkIn {
    Walk form;
    int H;
    int64_t N;
    const float* s;
    int lds;
    const float* t;
    int ldt;
    const int32_t* graph_ptr;
    int G;
    const int32_t* peer;               // cross only
    int sigmoid, skip_self;
    hipStream_t st;
};

static WalkIn pair_walk(int H, int64_t N, const float* s, int lds, const float* t, int ldt, const int32_t* graph_ptr, int G, int sigmoid,
                        int skip_self, void* stream) {
    return {Walk::general, H, N, s, lds, t, ldt, graph_ptr, G, nullptr, sigmoid, skip_self, (hipStream_t)stream};
}

static WalkIn sym_walk(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, void* stream) {
    return {Walk::sym, H, N, y, ldy, y, ldy, graph_ptr, G, nullptr, 0, 0, (hipStream_t)stream};
}

static WalkIn cross_walk(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, const int32_t* peer, void* stream) {
    return {Walk::cross, H, N, y, ldy, y, ldy, graph_ptr, G, peer, 0, 0, (hipStream_t)stream};
}

static int walk_args(const WalkIn& in, bool* launch) {
    if (in.form == Walk::cross) return cross_walk_args(in.H, in.N, in.s, in.lds, in.graph_ptr, in.G, in.peer, in.st, launch);
    return pair_walk_args(in.H, in.N, in.s, in.lds, in.t, in.ldt, in.graph_ptr, in.G, in.st, launch);
}

static int topk_run(const WalkIn& in, int k, float threshold, int32_t* idx, float* score, int32_t* n_above) {
    if (!mgv::pair_h_ok(in.H)) return MGV_EUNSUPPORTED;
    MGV_CHECK_ARG(k >= 1 && k <= mgv::kTopkMax);
    MGV_CHECK_ARG(in.N >= 0 && in.N <= 0x7fffffffLL / mgv::kTopkMax);    // node ids and idx offsets are int32 on the host side
    bool launch;
    const int rc = walk_args(in, &launch);
    if (rc != MGV_OK || !launch) return rc;
    MGV_CHECK_ARG(idx != nullptr && score != nullptr && n_above != nullptr);
    return launch_width(mgv::AllWidths{}, in.H, [&](auto w) {
        if (in.form == Walk::cross) {
            launch_row_tiles(mgv::k_cross_topk<w>, in.N, in.st, in.N, in.s, in.lds, in.graph_ptr, in.G, in.peer, k, threshold, idx, score,
                             n_above);
        } else {
            launch_row_tiles(mgv::k_pair_topk<w>, in.N, in.st, in.N, in.s, in.lds, in.t, in.ldt, in.graph_ptr, in.G, k, in.sigmoid, threshold,
                             in.skip_self, idx, score, n_above);
        }
    });
}

// the selection kernel of a form: FILL = false counts into n_sel, FILL = true fills col / score
template <int W, bool FILL>
static void launch_select(const WalkIn& in, float threshold, int32_t* n_sel, const int64_t* row_ptr, int64_t cap, int32_t* col,
                          float* score) {
    auto own = [&](auto sym) {
        launch_row_tiles(mgv::k_pair_select<W, FILL, sym>, in.N, in.st, in.N, in.s, in.lds, in.t, in.ldt, in.graph_ptr, in.G, in.sigmoid,
                         threshold, in.skip_self, n_sel, row_ptr, cap, col, score);
    };
    if (in.form == Walk::cross) {
        launch_row_tiles(mgv::k_cross_select<W, FILL>, in.N, in.st, in.N, in.s, in.lds, in.graph_ptr, in.G, in.peer, threshold, n_sel,
                         row_ptr, cap, col, score);
    } else if (in.form == Walk::sym) {
        own(std::true_type{});
    } else {
        own(std::false_type{});
    }
}

// the three count entries
static int select_count_run(const WalkIn& in, float threshold, int32_t* n_sel) {
    bool launch;
    const int rc = walk_args(in, &launch);
    if (rc != MGV_OK || !launch) return rc;
    MGV_CHECK_ARG(n_sel != nullptr);
    return launch_width(mgv::AllWidths{}, in.H,
                        [&](auto w) { launch_select<w, false>(in, threshold, n_sel, nullptr, 0, nullptr, nullptr); });
}

// the three fill entries
static int select_fill_run(const WalkIn& in, float threshold, const int64_t* row_ptr, int64_t cap, int32_t* col, float* score) {
    if (!mgv::pair_h_ok(in.H)) return MGV_EUNSUPPORTED;
    MGV_CHECK_ARG(cap >= 0);
    bool launch;
    const int rc = walk_args(in, &launch);
    if (rc != MGV_OK || !launch) return rc;
    if (cap == 0) return MGV_OK;                                          // no slot: nothing can be written
    MGV_CHECK_ARG(row_ptr != nullptr && col != nullptr);
    return launch_width(mgv::AllWidths{}, in.H, [&](auto w) { launch_select<w, true>(in, threshold, nullptr, row_ptr, cap, col, score); });
}

extern "C" int mgv_pair_topk(int H, int64_t N, const float* s, int lds, const float* t, int ldt, const int32_t* graph_ptr, int G, int k,
                             int sigmoid, float threshold, int skip_self, int32_t* idx, float* score, int32_t* n_above, void* stream) {
    return topk_run(pair_walk(H, N, s, lds, t, ldt, graph_ptr, G, sigmoid, skip_self, stream), k, threshold, idx, score, n_above);
}

extern "C" int mgv_fanin_decode(int H, int64_t N, const float* x, int ldx, const float* y, int ldy, const int32_t* graph_ptr, int G,
                                const int32_t* key, const int32_t* want, int K, int32_t* tile_min, int32_t* idx, float* score,
                                int32_t* n_cand, void* stream) {
    if (!mgv::pair_h_ok(H)) return MGV_EUNSUPPORTED;
    MGV_CHECK_ARG(K >= 1 && K <= mgv::kFaninMax);
    MGV_CHECK_ARG(N >= 0 && N <= 0x7fffffffLL / mgv::kFaninMax);         // node ids and idx offsets are int32 on the host side
    hipStream_t st = (hipStream_t)stream;
    bool launch;
    const int rc = pair_walk_args(H, N, x, ldx, y, ldy, graph_ptr, G, st, &launch);
    if (rc != MGV_OK || !launch) return rc;
    MGV_CHECK_ARG(key != nullptr && want != nullptr && idx != nullptr && score != nullptr && n_cand != nullptr);
    if (tile_min != nullptr) {
        const int64_t nct = (N + mgv::kPairTile - 1) / mgv::kPairTile, per = mgv::kThreads / 64;
        hipLaunchKernelGGL(mgv::k_tile_min, dim3((unsigned)((nct + per - 1) / per)), dim3(mgv::kThreads), 0, st, N, key, tile_min);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return launch_width(mgv::AllWidths{}, H, [&](auto w) {
        launch_row_tiles(mgv::k_fanin_decode<w>, N, st, N, x, ldx, y, ldy, graph_ptr, G, key, want, K, (const int32_t*)tile_min, idx, score,
                         n_cand);
    });
}

extern "C" int mgv_pair_select_count(int H, int64_t N, const float* s, int lds, const float* t, int ldt, const int32_t* graph_ptr, int G,
                                     int sigmoid, float threshold, int skip_self, int32_t* n_sel, void* stream) {
    return select_count_run(pair_walk(H, N, s, lds, t, ldt, graph_ptr, G, sigmoid, skip_self, stream), threshold, n_sel);
}

extern "C" int mgv_pair_select_fill(int H, int64_t N, const float* s, int lds, const float* t, int ldt, const int32_t* graph_ptr, int G,
                                    int sigmoid, float threshold, int skip_self, const int64_t* row_ptr, int64_t cap, int32_t* col,
                                    float* score, void* stream) {
    return select_fill_run(pair_walk(H, N, s, lds, t, ldt, graph_ptr, G, sigmoid, skip_self, stream), threshold, row_ptr, cap, col, score);
}

extern "C" int mgv_row_unit(int H, int64_t N, const float* x, int ldx, float eps, float* y, int ldy, float* norm, void* stream) {
    if (!mgv::pair_h_ok(H)) return MGV_EUNSUPPORTED;
    MGV_CHECK_ARG(N >= 0);
    if (N == 0) return MGV_OK;
    MGV_CHECK_ARG(mgv::pair_rows_ok(x, ldx, H) && mgv::pair_rows_ok(y, ldy, H));
    hipStream_t st = (hipStream_t)stream;
    return launch_width(mgv::AllWidths{}, H, [&](auto w) {
        constexpr int HH = w, rows = mgv::kThreads / (HH / 4);
        hipLaunchKernelGGL(mgv::k_row_unit<HH>, dim3(mgv::grid_for((N + rows - 1) / rows, 8)), dim3(mgv::kThreads), 0, st, N, x, ldx, eps, y, ldy, norm);
    });
}

extern "C" int mgv_sim_select_count(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, float threshold,
                                    int32_t* n_sel, void* stream) {
    return select_count_run(sym_walk(H, N, y, ldy, graph_ptr, G, stream), threshold, n_sel);
}

extern "C" int mgv_sim_select_fill(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, float threshold,
                                   const int64_t* row_ptr, int64_t cap, int32_t* col, float* score, void* stream) {
    return select_fill_run(sym_walk(H, N, y, ldy, graph_ptr, G, stream), threshold, row_ptr, cap, col, score);
}

extern "C" int mgv_cross_topk(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, const int32_t* peer, int k,
                              float threshold, int32_t* idx, float* score, int32_t* n_above, void* stream) {
    return topk_run(cross_walk(H, N, y, ldy, graph_ptr, G, peer, stream), k, threshold, idx, score, n_above);
}

extern "C" int mgv_cross_select_count(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, const int32_t* peer,
                                      float threshold, int32_t* n_sel, void* stream) {
    return select_count_run(cross_walk(H, N, y, ldy, graph_ptr, G, peer, stream), threshold, n_sel);
}

extern "C" int mgv_cross_select_fill(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, const int32_t* peer,
                                     float threshold, const int64_t* row_ptr, int64_t cap, int32_t* col, float* score, void* stream) {
    return select_fill_run(cross_walk(H, N, y, ldy, graph_ptr, G, peer, stream), threshold, row_ptr, cap, col, score);
}

// the two class entries (sym or cross): the walk unites in `parent` what the fill of that form would list
static int union_run(const WalkIn& in, float threshold, int32_t* parent, int32_t* status) {
    bool launch;
    const int rc = walk_args(in, &launch);
    if (rc != MGV_OK) return rc;
    MGV_CHECK_ARG(status != nullptr && (in.N == 0 || parent != nullptr));
    if (!launch) return MGV_OK;
    return launch_width(mgv::AllWidths{}, in.H, [&](auto w) {
        if (in.form == Walk::cross) {
            launch_row_tiles(mgv::k_cross_union<w>, in.N, in.st, in.N, in.s, in.lds, in.graph_ptr, in.G, in.peer, threshold, parent, status);
        } else {
            launch_row_tiles(mgv::k_sim_union<w>, in.N, in.st, in.N, in.s, in.lds, in.graph_ptr, in.G, threshold, parent, status);
        }
    });
}

extern "C" int mgv_sim_union(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, float threshold, int32_t* parent,
                             int32_t* status, void* stream) {
    return union_run(sym_walk(H, N, y, ldy, graph_ptr, G, stream), threshold, parent, status);
}

extern "C" int mgv_cross_union(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, const int32_t* peer,
                               float threshold, int32_t* parent, int32_t* status, void* stream) {
    return union_run(cross_walk(H, N, y, ldy, graph_ptr, G, peer, stream), threshold, parent, status);
}

// the table of a profile entry (1 <= B <= kHistMaxEdges, edges not NULL) must ascend strictly and hold no NaN: it is read back, like the
// two ends of graph_ptr (one small blocking copy)
static int hist_edges_check(const float* edges, int B, hipStream_t st) {
    float e[mgv::kHistMaxEdges];
    hipError_t err = hipMemcpyAsync(e, edges, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err != hipSuccess) return (int)err;
    MGV_CHECK_ARG(e[0] == e[0]);
    for (int j = 1; j < B; ++j) MGV_CHECK_ARG(e[j] > e[j - 1]);           // false for a NaN on either side
    return MGV_OK;
}

// half the first power of two above B: the first step of the kernels' binary search
static int hist_top(int B) {
    int top = 1;
    while (2 * top <= B) top *= 2;
    return top;
}

// the three profile entries: checks in the order of the selection entries, then the table; *launch = false: hist is zero and nothing is
// left to do.  hist has a row per graph and one row without a table; the cross form, whose table is never NULL, has none at G = 0.
static int hist_run(const WalkIn& in, const float* edges, int B, int64_t* hist) {
    if (!mgv::pair_h_ok(in.H)) return MGV_EUNSUPPORTED;
    MGV_CHECK_ARG(B >= 1 && B <= mgv::kHistMaxEdges && edges != nullptr && hist != nullptr);
    bool launch;
    const int rc = walk_args(in, &launch);
    if (rc != MGV_OK) return rc;
    const int ok = hist_edges_check(edges, B, in.st);
    if (ok != MGV_OK) return ok;
    const int64_t rows = in.form == Walk::cross ? in.G : (in.G > 1 ? in.G : 1);
    if (rows > 0) {
        hipError_t err = hipMemsetAsync(hist, 0, sizeof(int64_t) * (size_t)rows * (size_t)(B + 1), in.st);
        if (err != hipSuccess) return (int)err;
    }
    if (!launch) return MGV_OK;
    const int top = hist_top(B);
    unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
    return launch_width(mgv::AllWidths{}, in.H, [&](auto w) {
        auto own = [&](auto sym) {
            launch_row_tiles(mgv::k_pair_hist<w, sym>, in.N, in.st, in.N, in.s, in.lds, in.t, in.ldt, in.graph_ptr, in.G, in.sigmoid,
                             in.skip_self, edges, B, top, h);
        };
        if (in.form == Walk::cross) {
            launch_row_tiles(mgv::k_cross_hist<w>, in.N, in.st, in.N, in.s, in.lds, in.graph_ptr, in.G, in.peer, edges, B, top, h);
        } else if (in.form == Walk::sym) {
            own(std::true_type{});
        } else {
            own(std::false_type{});
        }
    });
}

extern "C" int mgv_pair_hist(int H, int64_t N, const float* s, int lds, const float* t, int ldt, const int32_t* graph_ptr, int G, int sigmoid,
                             int skip_self, const float* edges, int B, int64_t* hist, void* stream) {
    return hist_run(pair_walk(H, N, s, lds, t, ldt, graph_ptr, G, sigmoid, skip_self, stream), edges, B, hist);
}

extern "C" int mgv_sim_hist(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, const float* edges, int B,
                            int64_t* hist, void* stream) {
    return hist_run(sym_walk(H, N, y, ldy, graph_ptr, G, stream), edges, B, hist);
}

extern "C" int mgv_cross_hist(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, const int32_t* peer,
                              const float* edges, int B, int64_t* hist, void* stream) {
    return hist_run(cross_walk(H, N, y, ldy, graph_ptr, G, peer, stream), edges, B, hist);
}

extern "C" int mgv_pair_rank_counts(int H, int64_t N, const float* s, int lds, const float* t, int ldt, const int32_t* graph_ptr, int G,
                                    int skip_self, const int32_t* thr_ptr, const float* thr, int32_t* n_gt, int32_t* n_eq, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!mgv::pair_h_ok(H)) return MGV_EUNSUPPORTED;
    MGV_CHECK_ARG(N >= 0 && N <= 0x7fffffffLL);                           // node ids are int32
    MGV_CHECK_ARG(graph_ptr == nullptr || G >= 0);
    MGV_CHECK_ARG(thr_ptr != nullptr);
    // the two ends of both tables in one blocking step: graph_ptr from 0 to N (as pair_walk_args reads it), thr_ptr from 0 to T
    int32_t ends[4] = {0, (int32_t)N, 0, 0};
    hipError_t e = hipMemcpyAsync(&ends[2], thr_ptr, sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&ends[3], thr_ptr + N, sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && graph_ptr != nullptr) e = hipMemcpyAsync(&ends[0], graph_ptr, sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && graph_ptr != nullptr) e = hipMemcpyAsync(&ends[1], graph_ptr + G, sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    MGV_CHECK_ARG(ends[0] == 0 && (int64_t)ends[1] == N);
    MGV_CHECK_ARG(ends[2] == 0 && ends[3] >= 0);                          // T = thr_ptr[N] is an int32: below 2^31
    const int T = ends[3];
    if (N == 0) return MGV_OK;
    MGV_CHECK_ARG(mgv::pair_rows_ok(s, lds, H) && mgv::pair_rows_ok(t, ldt, H));
    if (T == 0) return MGV_OK;                                            // nothing is listed: nothing to write
    MGV_CHECK_ARG(thr != nullptr && n_gt != nullptr && n_eq != nullptr);
    return launch_width(mgv::AllWidths{}, H, [&](auto w) {
        launch_row_tiles(mgv::k_pair_rank<w>, N, st, N, s, lds, t, ldt, graph_ptr, G, skip_self, thr_ptr, T, thr, n_gt, n_eq);
    });
}
