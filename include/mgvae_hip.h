/* mgvae_hip.h — C ABI of libmgvae_hip.so: the MI355X (gfx950) kernels behind the DG_AE hot path.
 *
 * The reference (959AI994/Multi-Gate-VAE) has no FFI of its own: its hot path is Python calling
 * ATen / PyG operators.  Each entry point below names the reference operator(s) it replaces
 * (file:line under /root/reference/DG_VAE/deepgate/) — these are the calls a maintainer would bind
 * (ctypes stub: INTEGRATION.md).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless said otherwise; the library allocates nothing, keeps
 *     no state between calls and only enqueues work on `stream` (a hipStream_t passed as void*);
 *   - return value: 0 = enqueued, MGV_EINVAL (-1) = bad argument, MGV_EUNSUPPORTED (-2) = unsupported
 *     size, > 0 = hipError_t of the failed launch.  The hidden widths H an entry serves are one of four sets, stated with
 *     the entry (csrc/mgv_launch.h names them): {16, 32, 64, 128} the float4-per-lane gather / reduction kernels, {16, 32, 64}
 *     the one-float-per-lane and the exact-fp32 stage / level kernels, {32, 64} the bf16x3 stage / level kernels,
 *     {32, 64, 128} the attention pool.  Any other H is MGV_EUNSUPPORTED; where in the order of an entry's refusals
 *     (before or after its MGV_EINVAL checks and its MGV_OK for an empty problem) is stated with the entry;
 *   - matrices are row-major fp32, node indices int32, all "gradient accumulator" outputs (dW..,
 *     db..) are ADDED to: the caller zeroes them.  On the default path (H = 64, bf16x3) the sums go through per-workgroup
 *     slabs and a fixed-order reduction kernel (bit-identical from run to run); the exact-fp32 family, H = 32 and the
 *     first bf16x3 backward use float atomics;
 *   - N = nodes in the batch, E = edges, H = dim_hidden, gate column blocks are ordered r,z,n like
 *     torch.nn.GRU.
 */
#ifndef MGVAE_HIP_H
#define MGVAE_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#ifndef MGV_OK
#define MGV_OK 0
#define MGV_EINVAL (-1)
#define MGV_EUNSUPPORTED (-2)
#endif

int mgv_abi_version(void);

/* ---- structural encoder half round: AggConv -> GRU -> LayerNorm
 * replaces digae_layer.py:267-270 (forward edges) / :272-275 (reversed edges) with
 * arch/gcn_conv.py:30-45, torch.nn.GRU (seq_len 1) and torch.nn.LayerNorm.
 *   nbr_ptr[N+1], nbr_idx[E] : CSR of the nodes each node sums over (in-neighbours for the forward
 *                               half, out-neighbours for the reversed half)
 *   xcls[N], xtab[C][3H]      : feature-row class per node and W_ih[:,H:] x_c + b_ih per class
 *   Wc[3H][H], bc[3H]         : W_ih[:,:H] Wm and W_ih[:,:H] bm (message Linear folded into the GRU)
 *   ln_w/ln_b                 : NULL,NULL = no LayerNorm */
int mgv_struct_stage_fwd(int H, int64_t N, const float* h_in, const int32_t* nbr_ptr, const int32_t* nbr_idx,
                         const uint8_t* xcls, const float* xtab, int C, const float* Wc, const float* bc,
                         const float* Whh, const float* bhh, const float* ln_w, const float* ln_b, float ln_eps,
                         float* h_out, void* stream);
/* backward of the above (what autograd does for the same lines).  The incoming gradient is
 * dY[i] = gy_direct[i] + sum_{j in nbr(i)} gy_agg[j]  (gy_agg may be NULL): consecutive half rounds
 * use opposite CSRs, so the scatter of the NEXT stage's aggregate gradient is this stage's gather.
 * Outputs: g_direct_out = dL/dh_in through the GRU's hidden path, g_agg_out = dL/d(sum of neighbour
 * rows) (both NULL when h_in is a constant); WcT/WhhT are the [H][3H] transposes. */
int mgv_struct_stage_bwd(int H, int64_t N, const float* h_in, const int32_t* nbr_ptr, const int32_t* nbr_idx,
                         const uint8_t* xcls, const float* xtab, int C, const float* Wc, const float* WcT,
                         const float* bc, const float* Whh, const float* WhhT, const float* bhh,
                         const float* ln_w, const float* ln_b, float ln_eps, const float* gy_direct,
                         const float* gy_agg, float* g_direct_out, float* g_agg_out, float* dWc, float* dbc,
                         float* dWhh, float* dbhh, float* dxtab, float* dln_w, float* dln_b, void* stream);
/* general node features (digae_layer.py:257-277 accepts any x [N, F]; the reference Models only ever feed one-hot rows): the same half
 * round with the GRU's feature term per NODE, xrow[N][3H] = W_ih[:, H:] x_i + b_ih (formed with mgv_linear_fwd), instead of the class
 * table.  Exact-fp32 kernels, H in {16, 32, 64}.  Backward: d_xrow[N][3H] is ADDED to (the caller sums it over the stages that
 * share the weights and carries it to W_ih[:, H:], b_ih and x through mgv_linear_*). */
int mgv_struct_stage_rows_fwd(int H, int64_t N, const float* h_in, const int32_t* nbr_ptr, const int32_t* nbr_idx,
                              const float* xrow, const float* Wc, const float* bc, const float* Whh, const float* bhh,
                              const float* ln_w, const float* ln_b, float ln_eps, float* h_out, void* stream);
int mgv_struct_stage_rows_bwd(int H, int64_t N, const float* h_in, const int32_t* nbr_ptr, const int32_t* nbr_idx,
                              const float* xrow, const float* Wc, const float* WcT, const float* bc, const float* Whh,
                              const float* WhhT, const float* bhh, const float* ln_w, const float* ln_b, float ln_eps,
                              const float* gy_direct, const float* gy_agg, float* g_direct_out, float* g_agg_out,
                              float* dWc, float* dbc, float* dWhh, float* dbhh, float* d_xrow, float* dln_w, float* dln_b,
                              void* stream);

/* ---- the same half round on bf16x3 split-precision MFMA (hi/lo bf16 planes, three products, fp32
 * accumulate; H in {32, 64}).  wpack_bf16 = eight bf16 blocks of 3H*H elements each:
 * Wc_hi, Wc_lo, Whh_hi, Whh_lo ([3H][H]) then WcT_hi, WcT_lo, WhhT_hi, WhhT_lo ([H][3H]);
 * hi = bf16(W), lo = bf16(W - hi).  All other arguments as for the fp32 entry points.
 * heavy_n / heavy_nodes / heavy_ws (0 / NULL / NULL when there are none): the nodes with more than 64 neighbours in this CSR
 * (a clock- or reset-like net), ascending, and 2 * heavy_n * H floats of scratch: their neighbour sums are formed by a pre-pass
 * with one workgroup per node instead of by one lane group inside the tile kernel (100,000 consumers: 38 ms per launch there).
 * The pre-pass sums are read only where a tile takes the per-row path (its lists hold more than 504 entries together, or it is the
 * partial last tile); a listed node in any other tile is summed by the tile, and a long list that is not named here is walked in place:
 * the result is the same with and without the list.
 * table_own_idx (NULL = off): TABLE MODE for the half round that follows the (degree, class)-table one — h_in is the C-row table,
 * a node's own row is h_in[table_own_idx[node]], every nbr_idx entry carries its neighbour's table row in the top byte
 * (entry = node | row << 24, N < 2^24): the N x H expansion of the table is never gathered.  nbr_tagged = 0 with a table_own_idx:
 * the entries are plain rows of h_in and only the own rows go through the index (the quotient stages, GraphPlan.quotient: h_in is the
 * previous stage's colour table, a representative's own row is its previous colour's, its list names previous colours).
 * ln_stats_out (forward) / ln_stats (bwd2) [N][2], NULL = off: {mean, rstd} of every row's pre-LayerNorm state, kept by the forward
 * so that the backward's recompute needs two cross-lane row sums instead of four and no four-way combination of the column waves'
 * partial statistics (-3 % per backward launch); ignored when ln_w is NULL.
 * mgv_struct_stage_bwd_x3 (the first backward) serves H = 32 only: with valid arguments it returns MGV_EUNSUPPORTED at H = 64, whose
 * backward is mgv_struct_stage_bwd2_x3 below. */
int mgv_struct_stage_fwd_x3(int H, int64_t N, const float* h_in, const int32_t* nbr_ptr, const int32_t* nbr_idx,
                            const uint8_t* xcls, const float* xtab, int C, const void* wpack_bf16, const float* bc,
                            const float* bhh, const float* ln_w, const float* ln_b, float ln_eps, float* h_out,
                            int heavy_n, const int32_t* heavy_nodes, float* heavy_ws, const int32_t* table_own_idx,
                            int nbr_tagged, float* ln_stats_out, void* stream);
int mgv_struct_stage_bwd_x3(int H, int64_t N, const float* h_in, const int32_t* nbr_ptr, const int32_t* nbr_idx,
                            const uint8_t* xcls, const float* xtab, int C, const void* wpack_bf16, const float* bc,
                            const float* bhh, const float* ln_w, const float* ln_b, float ln_eps,
                            const float* gy_direct, const float* gy_agg, float* g_direct_out, float* g_agg_out,
                            float* dWc, float* dbc, float* dWhh, float* dbhh, float* dxtab, float* dln_w,
                            float* dln_b, int heavy_n, const int32_t* heavy_nodes, float* heavy_ws, const int32_t* table_own_idx,
                            int nbr_tagged, void* stream);

/* Second decomposition of the bf16x3 backward (H = 64 only): all weight fragments register-resident, transposed
 * products, one dgrad+wgrad phase per tile, and NO float atomics: parameter gradients leave through per-workgroup
 * slabs in `workspace` (mgv_struct_stage_bwd2_ws_floats(H, N) floats, device memory, contents irrelevant before and
 * after) and a fixed-order reduction, so two identical calls give bit-identical gradients.  Same reference lines and
 * argument meaning as mgv_struct_stage_bwd_x3 (digae_layer.py:266-275 under autograd). */
int mgv_struct_stage_bwd2_ws_floats(int H, int64_t N);   /* a size, not a status */
int mgv_struct_stage_bwd2_x3(int H, int64_t N, const float* h_in, const int32_t* nbr_ptr, const int32_t* nbr_idx,
                             const uint8_t* xcls, const float* xtab, int C, const void* wpack_bf16, const float* bc,
                             const float* bhh, const float* ln_w, const float* ln_b, float ln_eps,
                             const float* gy_direct, const float* gy_agg, float* g_direct_out, float* g_agg_out,
                             float* dWc, float* dbc, float* dWhh, float* dbhh, float* dxtab, float* dln_w,
                             float* dln_b, float* workspace, int64_t workspace_floats, int heavy_n,
                             const int32_t* heavy_nodes, float* heavy_ws, const int32_t* table_own_idx,
                             int nbr_tagged, const float* ln_stats, void* stream);

/* ---- Linear over node rows (hs_linear dg_ae_model_aig.py:64, hs_decompose :109, fc_{s,t}_{mu,logstd}
 * digvae_model.py:135-136, readout Linear layers mlp.py:29,38; also the dgrad with W^T):
 *   Y[N][M] = [X1 | X2] W^T + b     (X2/K2 = NULL/0 unless a torch.cat of two inputs is fused, :64)
 * K1+K2 multiple of 16 (<= 256), K1 and K2 multiples of 4, M in {16,32,64,128}; ld* = row strides in floats, multiples of 4, ld1 >= K1,
 * ld2 >= K2, ldy >= M (columns of a row beyond its M or K are neither read nor written).  N = 0 returns MGV_OK and launches nothing. */
int mgv_linear_fwd(int64_t N, const float* X1, int K1, int ld1, const float* X2, int K2, int ld2,
                   const float* W, const float* b, int M, float* Y, int ldy, void* stream);
/* dW[M][K1+K2] += dY^T [X1|X2],  db[M] += column sums of dY (db may be NULL).  dW and db ACCUMULATE: the caller zeroes them (or keeps
 * an earlier sum in them).  (M, K1+K2) in {16,32}x{16,32}, (32,64), (64,16), (64,32), (64,64), (64,128), (128,64); the same stride rules as
 * the forward (ld1 >= K1, ld2 >= K2, lddy >= M, multiples of 4).  The workgroups' partial sums meet in float atomics: not bit-reproducible. */
int mgv_linear_wgrad(int64_t N, const float* X1, int K1, int ld1, const float* X2, int K2, int ld2,
                     const float* dY, int lddy, int M, float* dW, float* db, void* stream);
/* the same layers on bf16x3 split-precision MFMA (see mgv_struct_stage_fwd_x3): HBM-bound instead of fp32-MFMA-bound.
 * (M, K = K1 + K2) must be one of the shapes mgv_linear_x3_supported() accepts (the model's layer shapes at H=64/32);
 * forward weights arrive as wpack_bf16[2][M*K] = {W_hi, W_lo} in MFMA fragment order (see mgv_func_sweep_fwd_x3). */
int mgv_linear_x3_supported(int M, int K);
/* fragment-order bf16 hi/lo planes (R*K elements each) of the fp32 matrix A = W [R][K] (transpose = 0) or of the
 * transposed view A[i][k] = W[k][i] (transpose = 1; W is then [K][R]); ldw = leading dimension of W */
int mgv_wpack_bf16x3(const float* W, int R, int K, int ldw, int transpose, void* hi, void* lo, void* stream);
int mgv_linear_fwd_x3(int64_t N, const float* X1, int K1, int ld1, const float* X2, int K2, int ld2,
                      const void* wpack_bf16, const float* b, int M, float* Y, int ldy, void* stream);
/* grouped Linear over the level sweep's tiles (num_rounds > 1, dg_ae_model_aig.py:70,88-94: every updated gate's GRU adds W_hh h_prev + b_hh
 * with its OWN aggregator's weights — here one launch over all tiles instead of an index_select / Linear / index_copy per gate type).
 * Row r of tile t is NODE order[tile_start[t] + r] (r < tile_count[t]); X / Y / R / dY rows are indexed by node.  fwd: tile t multiplies by
 * the pack of slot tile_slot[t] (wpack_bf16[T][2][M*K], fragment order as mgv_wpack_bf16x3 writes it) and adds b[tile_slot[t]][M];
 * tile_list (nullable) names the tiles to visit (ntiles entries; NULL: tiles 0 .. ntiles-1); a tile with tile_count[t] = 0 is allowed and
 * contributes / writes nothing; rows of Y no listed tile names are not touched; b may be NULL (no bias); ntiles = 0 returns MGV_OK.
 * wgrad: dW[M][K] += dY^T X, db[M] += colsum(dY) (both ACCUMULATE, fixed order: bit-identical from call to call; ldx >= K)
 * over the rows of the listed tiles (ONE slot's list: GraphPlan.slot_tiles).  Shapes at H = 64: (M, K) = (192, 64) and (64, 192) forward,
 * (192, 64) weight gradient. */
int mgv_grouped_linear_supported(int M, int K);
int mgv_grouped_linear_fwd_x3(int64_t ntiles, const int32_t* tile_list, const int32_t* order, const int32_t* tile_start,
                              const int32_t* tile_count, const int32_t* tile_slot, const float* X, int K, int ldx,
                              const void* wpack_bf16, const float* b, int M, const float* R, int ldr, float* Y, int ldy, void* stream);
int mgv_grouped_linear_wgrad_x3_ws_floats(int M, int K, int64_t ntiles);                            /* a size */
int mgv_grouped_linear_wgrad_x3(int64_t ntiles, const int32_t* tile_list, const int32_t* order, const int32_t* tile_start,
                                const int32_t* tile_count, const float* X, int K, int ldx, const float* dY, int lddy, int M,
                                float* dW, float* db, float* workspace, int64_t workspace_floats, void* stream);
/* the same with residual rows: Y = [X1 | X2] W^T + b + R (R [N][ldr >= M]).  Used as the input gradient of a Linear whose input has a
 * second consumer (hs: hs_decompose and the level sweep, dg_ae_model_aig.py:64-70,109): the other consumer's gradient rides in as R
 * instead of meeting this one in a separate N x M add */
int mgv_linear_fwd_x3_res(int64_t N, const float* X1, int K1, int ld1, const float* X2, int K2, int ld2,
                          const void* wpack_bf16, const float* b, int M, const float* R, int ldr, float* Y, int ldy,
                          void* stream);
/* dW[M][K1+K2] += dY^T [X1 | X2], db[M] += column sums of dY (db nullable).  Deterministic: every workgroup leaves its partial in
 * its own row of `workspace` (at least mgv_linear_wgrad_x3_ws_floats(M, K1+K2, N) floats) and a second launch adds the rows in a
 * fixed order — no float atomics, bit-identical from call to call.  dW and db ACCUMULATE (+=); strides as the forward takes them
 * (ld1 >= K1, ld2 >= K2, lddy >= M, multiples of 4); a workspace shorter than the size below is refused with MGV_EINVAL */
int mgv_linear_wgrad_x3_ws_floats(int M, int K, int64_t N);
int mgv_linear_wgrad_x3(int64_t N, const float* X1, int K1, int ld1, const float* X2, int K2, int ld2,
                        const float* dY, int lddy, int M, float* dW, float* db, float* workspace, int64_t workspace_floats,
                        void* stream);
/* The whole backward of one Linear in ONE pass over dY: dW and db as mgv_linear_wgrad_x3 (same arguments, same workspace size, same
 * bits), and the input gradients dX1[N][K1] = dY W[:, :K1] (+ R, nullable, [N][ldr >= K1]: a second consumer's gradient),
 * dX2[N][K2] = dY W[:, K1:] — bit for bit what mgv_linear_fwd_x3(_res) gives on the transposed packs of the two column blocks.
 * wtpack_bf16 = mgv_wpack_bf16x3(W, K1+K2, M, ldw, transpose = 1): the [K x M] view of the whole W.  X2, K2 = 0 and dX2 are NULL / 0
 * together; dX1 is required.  (M, K1+K2) in {(64,128), (128,64), (64,64)} (mgv_linear_bwd_x3_supported), any other shape returns
 * MGV_EUNSUPPORTED; N = 0 returns MGV_OK; both launch nothing. */
int mgv_linear_bwd_x3_supported(int M, int K);
int mgv_linear_bwd_x3(int64_t N, const float* X1, int K1, int ld1, const float* X2, int K2, int ld2, const float* dY, int lddy,
                      int M, const void* wtpack_bf16, float* dW, float* db, float* dX1, int ldx1, float* dX2, int ldx2,
                      const float* R, int ldr, float* workspace, int64_t workspace_floats, void* stream);
/* The hs seam at H = 64 in one pass each way.  Forward: HS[N][64] = [S | T] Wl^T + bl and ST[N][128] = HS Wd^T + bd, bit for bit
 * what mgv_linear_fwd_x3 gives for the two layers (wlpack = mgv_wpack_bf16x3(Wl, 64, 128, 128, 0), wdpack = mgv_wpack_bf16x3(Wd, 128,
 * 64, 64, 0); bl, bd nullable; S, T row-strided, lds, ldt >= 64, ldhs >= 64, ldst >= 128, multiples of 4).
 * Backward: dhs = dST Wd + gHS (gHS nullable: the gradient of hs's other consumers) is formed per tile and never written; dS | dT =
 * dhs Wl, dWl += dhs^T [S | T], dbl += colsum(dhs) carry the bits of mgv_linear_bwd_x3 on (64, 128) fed that dhs by
 * mgv_linear_bwd_x3 on (128, 64) with R = gHS.  dWd += dST^T HS and dbd += colsum(dST) are summed over this kernel's partition of the
 * tiles over workgroups and may differ from the stand-alone launch in rounding.  dbl, dbd nullable; all four ACCUMULATE.
 * wltpack = mgv_wpack_bf16x3(Wl, 128, 64, 128, 1), wdtpack = mgv_wpack_bf16x3(Wd, 64, 128, 64, 1).  workspace: at least
 * mgv_linear_pair_bwd_x3_ws_floats(N) floats, a shorter one is refused with MGV_EINVAL; N = 0 returns MGV_OK; both launch nothing. */
int mgv_linear_pair_fwd_x3(int64_t N, const float* S, int lds, const float* T, int ldt, const void* wlpack_bf16, const float* bl,
                           const void* wdpack_bf16, const float* bd, float* HS, int ldhs, float* ST, int ldst, void* stream);
int mgv_linear_pair_bwd_x3_ws_floats(int64_t N);
int mgv_linear_pair_bwd_x3(int64_t N, const float* dST, int lddst, const float* gHS, int ldghs, const float* HS, int ldhs,
                           const float* S, int lds, const float* T, int ldt, const void* wltpack_bf16, const void* wdtpack_bf16,
                           float* dS, int ldds, float* dT, int lddt, float* dWl, float* dbl, float* dWd, float* dbd,
                           float* workspace, int64_t workspace_floats, void* stream);
/* agg[i] = sum_{j in nbr(i)} h[j] added in list order, deg[i] = |nbr(i)| (deg may be NULL): the scatter-add half of
 * MessagePassing.propagate as used by AggConv called on its own (gcn_conv.py:34).  H in {16, 32, 64, 128} here and in the
 * row-sum entries below; any other H (0 and other non-multiples of 4 included) returns MGV_EUNSUPPORTED before anything is computed. */
int mgv_gather_sum(int H, int64_t N, const float* h, const int32_t* nbr_ptr, const int32_t* nbr_idx,
                   float* agg, float* deg, void* stream);

/* First half round of an encoder (digae_layer.py:260 starts every node from ones): an output row depends only on
 * the node's (degree, feature class) pair, class_id[N] numbers the pairs 0..C-1.
 * expand: out[i] = table[class_id[i]]; pull_sum: out[c] += sum over nodes of class c of
 * (gy_direct[i] + sum_{j in nbr(i)} gy_agg[j]) (gy_agg may be NULL); C * H * 20 <= 160 KiB.  pull_sum is deterministic for
 * C <= 8: per-workgroup rows in `workspace` (>= mgv_class_pull_sum_ws_floats(H, N, C) floats; 0 for an unsupported H), added in a fixed
 * order; C > 8 meets in LDS float atomics inside a workgroup.  `out` ACCUMULATES (+=) in both forms. */
int mgv_class_expand(int H, int64_t N, const float* table, const int32_t* class_id, float* out, void* stream);
/* Segmented row sums in list order (one lane group per segment, no atomics): out[s][H] = sum over m in [seg_ptr[s], seg_ptr[s+1]) of
 * v(item(m)), item(m) = items ? items[m] : m, v(i) = direct[i] + (agg ? sum of agg[nbr_idx[e]] over i's nbr list : 0).  The per-class
 * sums of an incoming gradient for the quotient stages of the structural encoder (rows that are identical by construction are
 * computed once: digae_layer.py:260 starts every node from ones, so early half rounds have few distinct rows): level 1 sums runs of
 * <= 64 class members with the stage backward's neighbour pull fused, the next levels sum the partial rows.  out_row (NULL: segment s
 * writes row s): the row of `out` each segment writes — a class that fits one segment writes its final row at once, only the classes
 * with more members than that leave partial rows behind the C final ones for the next level (most colours have a few members). */
int mgv_seg_sum(int H, int64_t n_seg, const int32_t* seg_ptr, const int32_t* items, const float* direct, const float* agg,
                const int32_t* nbr_ptr, const int32_t* nbr_idx, const int32_t* out_row, float* out, void* stream);
/* The same sums over a flat entry list, bit for bit (the additions of mgv_seg_sum in its order: a member's own row, + its pulled rows left
 * to right, then the member into the segment's sum, members in list order, from zero): seg_ptr[n_seg + 1] counts ENTRIES; entry >= 0 is row
 * `entry` of direct and starts a new member, entry < 0 is row ~entry of agg and continues the member (mgv_seg_entries writes such a list once
 * per plan; an items-only table is one as it stands).  entries NULL: the identity list (entry p = row p of direct: the levels above the
 * first); agg may be NULL when no entry is negative, and needs a list.  A lane group loads 8 entries at a time (4 at H = 16) and has their
 * rows in flight together; entry positions are int and a batch is formed as p + 8, so seg_ptr[n_seg] <= 2^31 - 9 (the caller's to keep:
 * mgv_seg_entries writes no longer list).  Refusals in this order: H outside {16, 32, 64, 128} MGV_EUNSUPPORTED; n_seg < 0, NULL seg_ptr / direct / out, or
 * agg without entries MGV_EINVAL; n_seg == 0 MGV_OK with nothing launched. */
int mgv_seg_sum_entries(int H, int64_t n_seg, const int32_t* seg_ptr, const int32_t* entries, const float* direct, const float* agg,
                        const int32_t* out_row, float* out, void* stream);

int mgv_class_pull_sum_ws_floats(int H, int64_t N, int C);
int mgv_class_pull_sum(int H, int64_t N, const float* gy_direct, const float* gy_agg, const int32_t* nbr_ptr,
                       const int32_t* nbr_idx, const int32_t* class_id, int C, float* out, float* workspace,
                       int64_t workspace_floats, void* stream);

/* ---- levelised functional sweep (dg_ae_model_aig.py:70-97 and mig/xag/xmg siblings; arch/tfmlp.py:38-46;
 * utils/dag_utils.py:91-105 is replaced by the tile tables).  T gate types ("slots"), per slot:
 *   attn_u[T][2H] = Wk^T w_attn[H:],  Wvc[T][3H][2H] = W_ih Wv,  bvc[T][3H] = W_ih bv,  bih/bhh[T][3H].
 * order/tile_* : updated nodes sorted by (level, slot) cut into <=64-node single-slot tiles;
 * level_tile_ptr_host: HOST array [num_levels+1] of tile offsets.
 * Round 1 (gh, h_prev and, backward, d_gh, g_hprev all NULL): hf must be zero on entry (every node is updated from h0 = 0).
 * Rounds r >= 2 (dg_ae_model_aig.py:70 with num_rounds > 1; all four set): every updated gate's GRU starts from its state of the
 * previous round.  hf holds the previous round's rows on entry (updated rows are rewritten), gh[N][3H] = W_hh h_prev + b_hh of each
 * node's own aggregator (r, z, n blocks; formed by the caller with mgv_linear_*), h_prev[N][H], bhh[T][3H] zeros (b_hh is inside
 * gh); backward: d_gh[N][3H] and g_hprev[N][H] = dh * z (rows of updated nodes written; the caller zeroes both), and the dbhh
 * accumulator receives nothing meaningful (its gradient comes from the caller's linear kernels). */
int mgv_func_sweep_fwd(int H, int64_t N, int T, int num_levels, const int32_t* level_tile_ptr_host,
                       const int32_t* order, const int32_t* tile_start, const int32_t* tile_count,
                       const int32_t* tile_slot, const int32_t* in_ptr, const int32_t* in_src, const float* hs,
                       float* hf, const float* attn_u, const float* Wvc, const float* bvc, const float* bih,
                       const float* bhh, const float* gh, const float* h_prev, void* stream);
/* backward sweep, levels in reverse.  ghf[N][H] = dL/dhf from the losses; ghs[N][H] is ADDED to;
 * scratch: dzb[N][2H], alpha[E], dsc[E] (in-CSR edge order).  WvcT[T][2H][3H].
 * Written / added to / scratch (both backward entries; tests/test_hip_sweep_reference.py holds them to it):
 *   hf (forward)   every updated row is WRITTEN; no other row is touched (fp32 entry, round 1: the caller zero-fills hf; bf16x3 entry,
 *                  round 1: mgv_sweep_zero_inactive writes the other rows; rounds >= 2: the caller copies h_prev into hf)
 *   ghs            fp32: ADDED to, every row (the caller zero-fills).  bf16x3: WRITTEN, every row (may arrive uninitialised); the rows
 *                  of never-updated nodes with more than skip_inactive_longer_than consumers are written by mgv_sweep_pull_heavy
 *   d_attn_u, dWvc, dbvc, dbih, dbhh   ADDED to (fp32: float atomics per tile; bf16x3: one add per entry after fixed-order slab sums)
 *   d_gh, g_hprev  rows of updated nodes WRITTEN, no other row touched (the caller zero-fills both)
 *   dzb, alpha, dsc   scratch, max(E, 1) / N * 2H floats, may arrive UNINITIALISED: the row / entries of an updated node are written
 *                  before any of its sources reads them; those of a never-updated node (gslot 255) are neither written nor read
 *   scratch, heavy_ws, partial_ws (bf16x3)   may arrive UNINITIALISED: the slab part of scratch is zeroed by the entry itself,
 *                  every other word is written before it is read
 * H outside {16, 32, 64} (bf16x3: {32, 64}) is MGV_EUNSUPPORTED from all four entries before anything else is looked at, also for a
 * sweep without a tile; T > 6 on the bf16x3 entries is MGV_EINVAL (the fp32 entries have no slot cap: ops.FuncSweepFn routes it there). */
int mgv_func_sweep_bwd(int H, int64_t N, int T, int num_levels, const int32_t* level_tile_ptr_host,
                       const int32_t* order, const int32_t* tile_start, const int32_t* tile_count,
                       const int32_t* tile_slot, const int32_t* in_ptr, const int32_t* in_src,
                       const int32_t* out_ptr, const int32_t* out_dst, const int32_t* out_slot,
                       const uint8_t* gslot, const float* hs, const float* hf, const float* attn_u,
                       const float* Wvc, const float* WvcT, const float* bvc, const float* bih, const float* bhh,
                       const float* ghf, float* ghs, float* dzb, float* alpha, float* dsc, float* d_attn_u,
                       float* dWvc, float* dbvc, float* dbih, float* dbhh, const float* gh, const float* h_prev,
                       float* d_gh, float* g_hprev, void* stream);

/* the sweep on bf16x3 split-precision MFMA (H in {32, 64}, T <= 6).  Differences from the fp32 entry points:
 * wpack_bf16[T][4][6H^2] = per slot {Wvc_hi, Wvc_lo, WvcT_hi, WvcT_lo} as bf16 in MFMA fragment order
 * (blocks (row tile, k-step) of 512 elements, lane 16q+r holds W[16 rt + r][32 ks + 8q .. +7]);
 * order_span[n_active][order_span_ints]: order_span_ints = 4: {in_ptr[v], in_ptr[v+1], out_ptr[v], out_ptr[v+1]} of v = order[i] (the CSR
 * spans in sweep order, so a tile reaches its edge lists with one load per row); order_span_ints = 32: the packed rows of
 * mgv_plan_order_rows (spans + the first in-edge sources and consumers: the lists themselves arrive with that one load).
 * Backward: no float atomics per tile.  The level kernels leave their rows' gate gradients and zbar rows in
 * `scratch` (sweep order) and one weight-gradient kernel per slot forms dWvc afterwards from the slot's tile
 * list: slot_tiles[num_tiles] = tile ids grouped by slot, slot_tile_ptr_host = HOST array [T+1] of offsets into
 * it; the small gradients (d_attn_u, dbvc, dbih, dbhh) are summed per workgroup in `scratch` too.
 * scratch_elems >= n_active * 5H + (tiles of the widest level) * T * 11H + 256 * 6H^2 floats, n_active = length of `order`
 * (the last term: per-workgroup rows of the weight-gradient kernel, summed in a fixed order: no float atomics at H = 64).
 * dWvc stays fp32 [T][3H][2H] and is ADDED to; ghs[N][H] is WRITTEN for every node (no zero fill needed). */
/* hf[v] = 0 for the nodes the sweep never updates (gslot[v] == 255; dg_ae_model_aig.py:61 zero-fills the whole state):
 * with it the caller hands the sweep an UNINITIALISED hf instead of a zero-filled one */
int mgv_sweep_zero_inactive(int H, int64_t N, const uint8_t* gslot, float* hf, void* stream);
int mgv_func_sweep_fwd_x3(int H, int64_t N, int T, int num_levels, const int32_t* level_tile_ptr_host,
                          const int32_t* order, const int32_t* order_span, int order_span_ints, const int32_t* tile_start,
                          const int32_t* tile_count, const int32_t* tile_slot, const int32_t* in_ptr,
                          const int32_t* in_src, const float* hs, float* hf, const float* attn_u,
                          const void* wpack_bf16, const float* bvc, const float* bih, const float* bhh,
                          const float* gh, const float* h_prev, void* stream);
int mgv_func_sweep_bwd_x3(int H, int64_t N, int T, int num_levels, const int32_t* level_tile_ptr_host,
                          const int32_t* order, const int32_t* order_span, int order_span_ints, int64_t n_active,
                          const int32_t* tile_start, const int32_t* tile_count, const int32_t* tile_slot,
                          const int32_t* slot_tiles, const int32_t* slot_tile_ptr_host, const int32_t* in_ptr,
                          const int32_t* in_src, const int32_t* out_ptr, const int32_t* out_dst,
                          const int32_t* out_slot, const uint8_t* gslot, const float* hs, const float* hf,
                          const float* attn_u, const void* wpack_bf16, const float* bvc, const float* bih,
                          const float* bhh, const float* ghf, float* ghs, float* dzb, float* alpha, float* dsc,
                          float* d_attn_u, float* dWvc, float* dbvc, float* dbih, float* dbhh, float* scratch,
                          int64_t scratch_elems,
                          int skip_inactive_longer_than /* > 0: never-updated nodes with more consumers are left to mgv_sweep_pull_heavy */,
                          /* updated gates with more than skip_active_longer_than consumers (an inverter of a clock-like input), ordered by
                           * (level, id): nodes[K], node_seg_ptr[K+1], segment bounds, per-level ranges of nodes and segments as HOST arrays
                           * [num_levels + 1] (GraphPlan.heavy_segments(True, active_by_level=True)); heavy_ws: (K + segments) * 2H floats.
                           * Their pulls run per level by whole workgroups in front of the level's kernel.  0 / NULLs: none. */
                          int heavy_active_n, const int32_t* heavy_nodes, const int32_t* heavy_node_seg_ptr, const int32_t* heavy_seg_e0,
                          const int32_t* heavy_seg_e1, const int32_t* heavy_lvl_k_ptr_host, const int32_t* heavy_lvl_seg_ptr_host,
                          float* heavy_ws, int skip_active_longer_than,
                          const float* gh, const float* h_prev, float* d_gh, float* g_hprev, void* stream);

/* ---- stand-alone TFMlpAggr (arch/tfmlp.py:31-46: an edge-list call outside the levelised sweep).  Attention pooling over a CSR by
 * destination: zbar[i][W] = sum_j alpha_ij x[j], alpha = softmax over i's sources of u . x[j] (PyG softmax: exp(s - max) / (sum + 1e-16));
 * the module's message is W_v zbar + b_v [deg > 0] (mgv_linear_*).  W = row width (2 * dim_hidden) in {32, 64, 128};
 * mstat / inv [N]: the softmax statistics the backward re-uses (an empty list: zbar = 0, mstat = 0, inv = 1 / 1e-16); all three are
 * WRITTEN for every node.  Backward: dx [rows of x][W] and du [W] are ADDED to with float atomics
 * (the caller zeroes them; this entry is not on the train step).  Any other W is MGV_EUNSUPPORTED before anything else is looked at. */
int mgv_attn_pool_fwd(int W, int64_t N, const int32_t* in_ptr, const int32_t* in_src, const float* x, const float* u,
                      float* zbar, float* mstat, float* inv, void* stream);
int mgv_attn_pool_bwd(int W, int64_t N, const int32_t* in_ptr, const int32_t* in_src, const float* x, const float* u,
                      const float* zbar, const float* mstat, const float* inv, const float* dzbar, float* dx, float* du,
                      void* stream);

/* ghs rows of the heavy never-updated nodes (primary inputs driving thousands of gates): consumer lists in segments, one workgroup
 * each (GraphPlan.heavy_segments(reverse=True, inactive_only=True)); partial_ws: S * H floats.  H in {32, 64}: any other is
 * MGV_EUNSUPPORTED after the argument checks and after K = 0 or S = 0 returned MGV_OK. */
int mgv_sweep_pull_heavy(int H, int K, const int32_t* nodes, const int32_t* node_seg_ptr, int S, const int32_t* seg_e0,
                         const int32_t* seg_e1, const int32_t* out_dst, const int32_t* out_slot, const uint8_t* gslot,
                         const float* alpha, const float* dsc, const float* dzb, const float* attn_u, float* partial_ws,
                         float* ghs, void* stream);

/* ---- inner-product decoder and reconstruction loss (digae_layer.py:26-29, dg_ae_model_aig.py:108-130).
 * s, t: row pointers with common row stride ld (the two halves of hs_decompose's output);
 * edge lists are int64 like the reference's edge_index rows.
 * Widths of this section (edge_dot, recon_*): H in {16, 32, 64, 128} unless an entry says otherwise.  Every entry checks its
 * arguments first (MGV_EINVAL, ld >= H among them), returns MGV_OK for an empty problem (E = 0; Epos + Eneg = 0; N = 0; K = 0 or
 * S = 0) next, and refuses any other H with MGV_EUNSUPPORTED then: before its workspace size is looked at and before anything is
 * launched. */
int mgv_edge_dot_fwd(int H, int64_t E, const float* s, const float* t, int ld, const int64_t* src,
                     const int64_t* dst, int sigmoid, float* out, void* stream);
int mgv_edge_dot_bwd(int H, int64_t E, const float* s, const float* t, int ld, const int64_t* src,
                     const int64_t* dst, int sigmoid, const float* gout, float* ds, float* dt, void* stream);
/* ---- the decoder over ALL node pairs (digae_layer.py:26-33 forward_all, returned by DirectedGAE.forward, digae_model.py:118-122;
 * csrc/pair_scores.hip).  One arithmetic for the four entries: exact fp32, every pair the chain acc = fmaf(s[i][k], t[j][k], acc) over
 * k = 0 .. H-1 in ascending order from acc = 0 (v_mfma_f32_16x16x4_f32; the listed-pair entry restates it with scalar fmaf), then
 * the sigmoid of mgv_edge_dot_fwd when `sigmoid` is set — a score is the same bits whichever entry reports it.  H in {16, 32, 64, 128}
 * (any other: MGV_EUNSUPPORTED before anything is launched).  s [M][lds], t [N][ldt]: row strides in floats of their own (on the models
 * the two halves of st = hs_decompose(hs), ld = 2H), multiples of 4 and >= H, base pointers 16-byte aligned.
 * fwd (digae_layer.py:31-33, digae_model.py:118-122): out[i][j] = <s_i, t_j>, any M, N >= 0 (0: nothing is launched), ldo >= N; columns of
 * a row past N are not written.  Index arithmetic is 64-bit: M N may pass 2^31. */
int mgv_pair_scores_fwd(int H, int64_t M, int64_t N, const float* s, int lds, const float* t, int ldt, int sigmoid, float* out,
                        int64_t ldo, void* stream);
/* backward of the above (autograd through digae_layer.py:31-33): ds[M][ldds] = G t, dt[N][lddt] = G^T s with G = gout * p (1 - p), p = the
 * saved forward output `out` (G = gout and `out` unused without the sigmoid); gout [M][ldg >= N].  ds / dt are WRITTEN (no zero fill), either
 * may be NULL.  Every output row belongs to one workgroup, which walks the other dimension in tile order: one fmaf chain per entry, no
 * float atomics, bit-identical from call to call. */
int mgv_pair_scores_bwd(int H, int64_t M, int64_t N, const float* s, int lds, const float* t, int ldt, int sigmoid, const float* out,
                        int64_t ldo, const float* gout, int64_t ldg, float* ds, int ldds, float* dt, int lddt, void* stream);
/* out[e] = the score of pair (src[e], dst[e]) (digae_layer.py:26-29 in the arithmetic of forward_all :31-33, digae_model.py:118-122): equal
 * to out[src[e]][dst[e]] of mgv_pair_scores_fwd bit for bit; int64 lists like mgv_edge_dot_fwd */
int mgv_pair_scores_at(int H, int64_t E, const float* s, int lds, const float* t, int ldt, const int64_t* src, const int64_t* dst,
                       int sigmoid, float* out, void* stream);
/* the streaming consumer of forward_all (digae_layer.py:31-33, digae_model.py:118-122) that never writes an N x N array: per row u its k
 * best candidates and the number of candidates the decoder calls an edge.  Candidates of u: the nodes v of u's own graph,
 * graph_ptr[g] <= v < graph_ptr[g+1] (graph_ptr [G+1] int32 on the device, NULL = one graph of all N), without v = u when skip_self.
 * 1 <= k <= 32.  idx[N][k] int32: batch-wide node ids ordered by raw dot product descending, ties by ascending id; -1 past the end when the
 * graph has fewer than k candidates.  score[N][k]: the reported score (sigmoid of the dot product when `sigmoid`), -inf where idx is -1.
 * n_above[N] int32: candidates whose reported score is > threshold (the `>` of pred_bin, trainer.py:240-244).  A NaN score is never
 * selected or counted.  Refused with MGV_EINVAL before anything is launched: k outside [1, 32], a graph_ptr that does not start at 0
 * and end at N (its two ends are read back: the only blocking step, skipped for NULL). */
int mgv_pair_topk(int H, int64_t N, const float* s, int lds, const float* t, int ldt, const int32_t* graph_ptr, int G, int k, int sigmoid,
                  float threshold, int skip_self, int32_t* idx, float* score, int32_t* n_above, void* stream);
/* the reconstructed graph of forward_all (digae_layer.py:31-33, digae_model.py:118-122) as per-row lists, without an N x N array: the
 * candidates of row u (as in mgv_pair_topk: u's own graph, without v = u when skip_self) whose reported score is > threshold, the very
 * decision behind n_above.  A NaN score is never selected.  Two passes around the caller's exclusive scan:
 * count (digae_layer.py:31-33, digae_model.py:118-122): n_sel[N] int32 is written for every row and equals n_above of mgv_pair_topk for
 * the same arguments.  Refused before anything is launched: H outside {16, 32, 64, 128} (MGV_EUNSUPPORTED); a bad row stride or
 * alignment, N > 2^31 - 1, a graph_ptr that does not start at 0 and end at N (read back as in mgv_pair_topk, NULL skips it): MGV_EINVAL.
 * N = 0 launches nothing. */
int mgv_pair_select_count(int H, int64_t N, const float* s, int lds, const float* t, int ldt, const int32_t* graph_ptr, int G, int sigmoid,
                          float threshold, int skip_self, int32_t* n_sel, void* stream);
/* fill (digae_layer.py:31-33, digae_model.py:118-122): row u's selected columns as batch-wide int32 node ids in ascending order at
 * col[row_ptr[u] ..], with score[cap] (or NULL) the reported score beside each.  row_ptr [N+1] int64 on the device (a batch can select more
 * than 2^31 pairs), normally the exclusive scan of n_sel; whatever it holds, a row writes only inside [row_ptr[u], min(row_ptr[u+1], cap)),
 * drops what it has no room for and touches nothing outside [0, cap).  No atomics: positions come from a ballot and a prefix popcount per
 * 16-column block and a cursor the row's lanes carry through the walk, so two calls give the same bytes.  Refusals as for count, and
 * cap < 0: MGV_EINVAL. */
int mgv_pair_select_fill(int H, int64_t N, const float* s, int lds, const float* t, int ldt, const int32_t* graph_ptr, int G, int sigmoid,
                         float threshold, int skip_self, const int64_t* row_ptr, int64_t cap, int32_t* col, float* score, void* stream);
/* ---- functional-similarity search on hf (added functionality; the inference side of the functional loss, trainer.py:158-160:
 * 1 - cosine_similarity(hf[a], hf[b], eps = 1e-8); csrc/pair_scores.hip).  Unit rows first, then the pair entries above on (y, y): a
 * cosine is ONE k-ascending fmaf chain over two unit rows, the same bits whichever entry reports it.  A row's top-k needs all its
 * candidates and is mgv_pair_topk(y, y, sigmoid = 0, skip_self = 1); listed pairs are mgv_pair_scores_at(y, y, sigmoid = 0).
 * unit rows (trainer.py:158-160): y[i] = x[i] / max(|x[i]|, eps) — the clamp is per row, as torch.cosine_similarity applies it and as
 * mgv_func_loss_fwd does — and norm[i] = |x[i]| unclamped when norm is not NULL.  H / 4 lanes per row, float4 loads and stores, the sum of
 * squares in float32 WITHOUT rescaling: the contract is a finite sum of squares (hf is a GRU output in (-1, 1)).  A zero row gives a
 * zero row, a row that holds a NaN a row of NaNs (and a NaN norm).  y may be exactly x (same pointer, same stride); no other overlap
 * is promised.  H in {16, 32, 64, 128}, else MGV_EUNSUPPORTED before anything else is looked at; x [N][ldx], y [N][ldy] under the
 * rule of the pair entries (strides multiples of 4 and >= H, bases 16-byte aligned), else MGV_EINVAL; N < 0: MGV_EINVAL; N = 0
 * launches nothing. */
int mgv_row_unit(int H, int64_t N, const float* x, int ldx, float eps, float* y, int ldy, float* norm, void* stream);
/* the symmetric form of mgv_pair_select_count (trainer.py:158-160 in the arithmetic of digae_layer.py:31-33): s = t = y, raw scores, no
 * sigmoid.  With s = t the score matrix is symmetric bit for bit (every product commutes and k keeps its order), so the candidates of
 * row u are the nodes v of u's own graph with v > u, and a row tile walks the column tiles from its own diagonal tile on.  n_sel[N]
 * int32 is written for every row.  Everything else is the contract of mgv_pair_select_count: `>` is strict and a NaN is never
 * selected; graph_ptr's two ends are read back, NULL is one graph; the same refusals and return codes.  Bit-identical or exactly
 * power-of-two-scaled rows score within (2H + 6) 2^-24 of 1 and are not clamped to it: threshold = 1.0 selects nothing reliably. */
int mgv_sim_select_count(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, float threshold, int32_t* n_sel,
                         void* stream);
/* the symmetric form of mgv_pair_select_fill (trainer.py:158-160, digae_layer.py:31-33): row u's selected v > u as batch-wide int32 ids in
 * ascending order at col[row_ptr[u] ..], score[cap] (or NULL) the cosine beside each — the bits of mgv_pair_scores_fwd(y, y, sigmoid = 0)
 * at [u][v] and at [v][u].  Writes fall only inside [row_ptr[u], min(row_ptr[u+1], cap)); no atomics, a second call gives the same
 * bytes; refusals as for mgv_pair_select_fill (cap < 0: MGV_EINVAL). */
int mgv_sim_select_fill(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, float threshold,
                        const int64_t* row_ptr, int64_t cap, int32_t* col, float* score, void* stream);
/* ---- matching across circuits (added functionality; trainer.py:158-160 in the arithmetic of digae_layer.py:31-33; csrc/pair_scores.hip).
 * The walk of mgv_pair_topk / mgv_pair_select_* on unit rows y (mgv_row_unit), raw scores, where the candidates of a row of graph g are
 * ALL rows of graph peer[g]: a golden design against its revision, a library block against an instance.  graph_ptr [G+1] int32 as
 * above, required; peer [G] int32 on the device: -1 = the rows of g have no candidates; peer[g] = g is allowed and a row is then a
 * candidate of itself (there is no skip_self); peer need not be an involution and several graphs may name one peer.  Range ends read
 * through peer are clamped into [0, N].  A cosine is ONE k-ascending fmaf chain, the bits mgv_pair_scores_at(y, y, sigmoid = 0) reports
 * for the pair.  A row tile walks only the column tiles that hold a candidate of one of its 64 rows, in ascending order.
 * top-k: idx[N][k] int32 batch-wide ids by cosine descending, ties by ascending id, -1 past the end; score[N][k] the cosine, -inf where
 * idx is -1; n_above[N] int32 the number of ALL candidates whose cosine is > threshold; a NaN is nobody's candidate.  1 <= k <= 32.
 * Refused before anything is launched: H outside {16, 32, 64, 128} (MGV_EUNSUPPORTED); k out of range, NULL graph_ptr or peer, a bad
 * row stride or alignment, N out of range, a graph_ptr that does not start at 0 and end at N, an entry of peer outside [-1, G) (peer
 * is read back whole for this, one small blocking copy beside graph_ptr's two ends): MGV_EINVAL.  N = 0 launches nothing. */
int mgv_cross_topk(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, const int32_t* peer, int k, float threshold,
                   int32_t* idx, float* score, int32_t* n_above, void* stream);
/* count (trainer.py:158-160, digae_layer.py:31-33): n_sel[N] int32, written for every row = n_above of mgv_cross_topk for the same
 * arguments.  Refusals as there. */
int mgv_cross_select_count(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, const int32_t* peer, float threshold,
                           int32_t* n_sel, void* stream);
/* fill (trainer.py:158-160, digae_layer.py:31-33): row u's candidates with cosine > threshold as ascending batch-wide int32 ids at
 * col[row_ptr[u] ..], score[cap] (or NULL) the cosine beside each.  The contract of mgv_pair_select_fill: a row writes only inside
 * [row_ptr[u], min(row_ptr[u+1], cap)), no atomics, a second call gives the same bytes; cap < 0: MGV_EINVAL. */
int mgv_cross_select_fill(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, const int32_t* peer, float threshold,
                          const int64_t* row_ptr, int64_t cap, int32_t* col, float* score, void* stream);
/* ---- the distribution of all-pair scores (added functionality; the thresholds of the entries above chosen by count: digae_layer.py:31-33,
 * digae_model.py:118-122 for the decoder, trainer.py:158-160 for the cosine; csrc/pair_scores.hip).  One walk of mgv_pair_select_count —
 * the same candidates (u's own graph, without v = u when skip_self), the same reported score (the sigmoid when `sigmoid`), a NaN counted
 * nowhere — bins every candidate by the number of edges it passes: hist[g][k] = candidates of graph g with #{j : rep > edges[j]} == k, so
 * bin 0 holds rep <= edges[0] and bin B rep > edges[B-1].  edges [B] float32 on the device, strictly ascending, no NaN, 1 <= B <= 256;
 * hist int64 [max(G, 1)][B + 1] is OVERWRITTEN (the launcher zeroes it; NULL graph_ptr: row 0).  The bin comes from the comparisons
 * `rep > edges[j]` themselves (a binary search over the table in LDS), never from an affine map of the score: for every j and g,
 * sum(hist[g][j+1:]) equals the sum over g's rows of n_sel of mgv_pair_select_count at threshold = edges[j] as integers.  Integer atomics
 * only (64-bit counters in LDS, one global add per non-zero (graph, bin) of a workgroup's first and last graph; the graphs between them,
 * at most 62 nodes in all, add directly): exact, the same bytes from call to call, no counter can overflow for any N <= 2^31 - 1.
 * Refused before anything is launched or zeroed: H outside {16, 32, 64, 128} (MGV_EUNSUPPORTED); B outside [1, 256], NULL edges or
 * hist, a bad row stride or alignment, N out of range, a graph_ptr that does not start at 0 and end at N, a table that does not ascend
 * strictly or holds a NaN (edges is read back for this, as graph_ptr's two ends are: one small blocking copy): MGV_EINVAL.  N = 0
 * zeroes hist and launches nothing. */
int mgv_pair_hist(int H, int64_t N, const float* s, int lds, const float* t, int ldt, const int32_t* graph_ptr, int G, int sigmoid,
                  int skip_self, const float* edges, int B, int64_t* hist, void* stream);
/* the symmetric form (trainer.py:158-160 in the arithmetic of digae_layer.py:31-33): the walk, candidates and score of mgv_sim_select_count
 * — unit rows y, v > u only, raw cosine, half the tiles from the diagonal tile on — binned as above; sum(hist[g][j+1:]) equals the
 * total of mgv_sim_select_count at threshold = edges[j].  Zero rows score 0; equal rows score within (2H + 6) 2^-24 of 1 and are not
 * clamped to it.  Arguments and refusals as mgv_pair_hist. */
int mgv_sim_hist(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, const float* edges, int B, int64_t* hist,
                 void* stream);
/* ---- the rank of every true link among ALL candidates of its node (added functionality; exact MRR / Hits@K / mean rank over the full
 * candidate set, where `test` ranks E positives against sampled non-edges: digae_layer.py:31-33, digae_model.py:118-122;
 * csrc/pair_scores.hip).  One walk of mgv_pair_select_count with a LIST of thresholds per row where that entry has one scalar for
 * everybody: for row u and every j in [thr_ptr[u], thr_ptr[u+1])
 *     n_gt[j] = #{candidates v of u : score(u, v) >  thr[j]}        n_eq[j] = #{candidates v of u : score(u, v) == thr[j]}.
 * Candidates are exactly those of mgv_pair_topk / mgv_pair_select_count: the columns of u's own graph (NULL graph_ptr: the whole
 * batch), without v = u when skip_self; a NaN score is nobody's candidate.  The score is the RAW dot product, the order mgv_pair_topk
 * ranks by — a float32 sigmoid saturates and would invent ties, so there is no `sigmoid` argument.  With thr = mgv_pair_scores_at
 * (sigmoid = 0) of row u's links, 1 + n_gt and n_gt + n_eq are the best and the worst rank of each link, and a link always finds
 * itself (n_eq >= 1): both sides of every comparison are the bits of one arithmetic.  A NaN threshold gets (0, 0), both comparisons
 * being false; -inf and +inf are thresholds like any other.
 * thr_ptr [N+1] int32 and thr [T] float32 on the device, T = thr_ptr[N].  EACH ROW'S LIST MUST ASCEND, NaNs last (duplicates allowed;
 * the order torch.sort gives): the kernel searches it.  A list that does not ascend makes only its own counts meaningless.  Whatever
 * thr_ptr holds between its ends, a row's range is clamped into [0, T) and no index outside it is read or written.
 * n_gt, n_eq int32 [T] are WRITTEN for every listed j by exactly one owner (32 entries of a row's list per pass of its tile, int32
 * counters in LDS, plain stores): no global atomics, nothing is zero-filled by the caller, two calls give the same bytes; entries
 * that no row lists are not touched.
 * Refused before anything is launched: H outside {16, 32, 64, 128} (MGV_EUNSUPPORTED); a bad row stride or alignment, N out of range
 * (N < 0 or N > 2^31 - 1), a graph_ptr that does not start at 0 and end at N, a NULL thr_ptr, a thr_ptr whose two ends are not 0 and
 * a T with 0 <= T < 2^31 (its ends are read back in the same small blocking copy as graph_ptr's ends), a NULL thr, n_gt or n_eq with
 * T > 0: MGV_EINVAL.  N = 0 or T = 0 launches nothing. */
int mgv_pair_rank_counts(int H, int64_t N, const float* s, int lds, const float* t, int ldt, const int32_t* graph_ptr, int G, int skip_self,
                         const int32_t* thr_ptr, const float* thr, int32_t* n_gt, int32_t* n_eq, void* stream);
/* ---- decode embeddings into a LEGAL circuit: fan-ins by arity, acyclic (added functionality; the decoder of digae_layer.py:31-33,
 * digae_model.py:118-122 under the constraints of a netlist; csrc/pair_scores.hip).  One more consumer of the walk of mgv_pair_topk.
 * The rows are TARGETS v: x [N][ldx] is the row operand and y [N][ldy] the column operand — on the models x = t and y = s, the
 * by='dst' convention of the selection entries; every product commutes and k keeps its order, so a score is the bits
 * mgv_pair_scores_at(s, t, sigmoid = 0) reports for (u, v).  key [N] int32: an order key per node (a level, a topological position);
 * want [N] int32: how many fan-ins the node takes (its gate's arity); 1 <= K <= 8 the width of the lists.
 * Candidate of row v: a column u of v's own graph (graph_ptr [G+1] int32, NULL = one graph of all N) with key[u] < key[v] whose score
 * is not NaN — strict, so v is never its own candidate and every decoded edge runs from a smaller key to a larger one: the result is
 * a DAG whatever the scores are.  Row v keeps its kk = min(max(want[v], 0), K) best candidates by raw dot product descending, ties by
 * ascending id (the order of mgv_pair_topk).  A row with kk = 0 takes part in nothing: it has no candidates.
 * idx [N][K] int32: batch-wide ids, -1 past the end; score [N][K]: the raw dot product, -inf where idx is -1; n_cand [N] int32: the
 * number of candidates of the row regardless of score (0 where kk = 0): n_cand < want marks a gate that could not be completed.  Every
 * row below N writes all K entries and its n_cand; no atomics, two calls give the same bytes.  A row tile none of whose rows wants
 * anything walks nothing.
 * tile_min int32 [ceil(N / 64)] or NULL, SCRATCH: when given, a small kernel on the same stream first writes the least key of every 64-column
 * tile, and a workgroup steps over a column tile whose least key is not below the greatest key among its rows that want something
 * (uniform per workgroup; such a tile holds nobody's candidate, so the output keeps every byte).  With keys that ascend with the id
 * inside each graph that is half the walk.
 * Refused before anything is launched: H outside {16, 32, 64, 128} (MGV_EUNSUPPORTED); K outside [1, 8], N < 0 or N > (2^31 - 1) / 8,
 * a graph_ptr that does not start at 0 and end at N (its two ends are read back: the only blocking step, skipped for NULL), a bad row
 * stride or alignment, and with N > 0 a NULL key, want, idx, score or n_cand: MGV_EINVAL.  N = 0 launches nothing. */
int mgv_fanin_decode(int H, int64_t N, const float* x, int ldx, const float* y, int ldy, const int32_t* graph_ptr, int G,
                     const int32_t* key, const int32_t* want, int K, int32_t* tile_min, int32_t* idx, float* score, int32_t* n_cand,
                     void* stream);
/* exact gate recovery of decoded lists against the true fan-in sets (added functionality; the strictest form of the reconstruction
 * question of digae_model.py:118-122; csrc/fanin_recovery.hip).  idx [N][K] int32 as mgv_fanin_decode writes it (1 <= K <= 32): the
 * distinct entries of a row other than -1 are its decoded set.  tru_ptr [N+1] int64 and tru_src [T] int32, T = tru_ptr[N] < 2^31: row
 * v's true fan-ins, STRICTLY ascending (a set).  A decoded id is looked up in the row's list by value (binary search) and never used
 * as an address: an id outside [0, N) is a miss.  Whatever tru_ptr holds between its ends, a row's range is clamped into [0, T].
 * n_hit [N] int32 (or NULL): decoded fan-ins found in the row's true list, written for every row.  rec int64 [max(G, 1)][5], zeroed
 * by the launcher: over the rows with a NON-EMPTY true list (the gates; a primary input counts nowhere) of each graph (graph_ptr
 * [G+1] int32, NULL: row 0 for all) {gates, exact, hits, true_total, decoded_total}, exact = the decoded set equals the true set.
 * 64-bit integer atomics only, one per non-zero (graph, field) of a workgroup after a segmented wave reduction: the same bytes from
 * run to run.  Refused before anything is zeroed or launched: K outside [1, 32], N < 0 or N > (2^31 - 1) / 32, a NULL rec, G < 0
 * with a graph_ptr, with N > 0 a NULL idx or tru_ptr, a graph_ptr that does not start at 0 and end at N, a tru_ptr that does not start
 * at 0 or whose end lies outside [0, 2^31) (the four ends are read back in one small blocking step), a NULL tru_src with T > 0:
 * MGV_EINVAL.  N = 0 zeroes rec and launches nothing. */
int mgv_fanin_recovery(int64_t N, int K, const int32_t* idx, const int64_t* tru_ptr, const int32_t* tru_src, const int32_t* graph_ptr,
                       int G, int32_t* n_hit, int64_t* rec, void* stream);
/* ---- connected components on the device (added functionality; csrc/components.hip, csrc/mgv_unionfind.h): candidate classes of the
 * relation "same graph and cosine > threshold" on hf (trainer.py:158-160) and components of decoded link lists (digae_layer.py:31-33).
 * One forest parent[N] int32, N < 2^31, with 0 <= parent[x] <= x at all times: a root is only ever hooked under a smaller root
 * (compare-and-swap), so a finished component's root is its smallest id whatever the schedule, and the labels are the same bits from
 * run to run.  While hooks can happen every access to parent is an agent-scope atomic.  status[4] int32 = {code, a, b, rounds}, all 0
 * when nothing went wrong; the first error wins: 1 = an entry of parent outside [0, x] (parent never went through mgv_cc_init), 2 = a
 * loop reached its cap of 2^20 rounds (no schedule of a sound forest gets there), 3 = a listed id outside [0, N).  The thread that
 * records an error leaves; the host reads status in the read-back it does anyway (mgv_cc_class_count hands it over).
 * init (trainer.py:158-160, digae_layer.py:31-33): parent[i] = i, status = 0.  N = 0 only clears status. */
int mgv_cc_init(int64_t N, int32_t* parent, int32_t* status, void* stream);
/* unites a[e] and b[e] for e < P (trainer.py:158-160, digae_layer.py:31-33): int64 lists like mgv_pair_scores_at's, in any order and
 * orientation, duplicates allowed, a[e] == b[e] does nothing.  Ids are the caller's contract as there, but one outside [0, N) is never
 * dereferenced: the pair is skipped and status records it (code 3).  Grid-stride, one pair per thread.  P = 0 launches nothing. */
int mgv_cc_union_pairs(int64_t N, int64_t P, const int64_t* a, const int64_t* b, int32_t* parent, int32_t* status, void* stream);
/* after the last hook (trainer.py:158-160, digae_layer.py:31-33): label[i] = the root of i = the smallest id of i's component; size[r]
 * (or NULL) = the number of nodes whose root is r, 0 where r is no root (int32 atomic adds: exact, order-free); with size, parent is
 * flattened to the labels.  N = 0 launches nothing. */
int mgv_cc_labels(int64_t N, int32_t* parent, int32_t* label, int32_t* size, void* stream);
/* the classes with at least min_size members as a compact table (trainer.py:158-160, digae_layer.py:31-33): class_ptr int64 [C + 1],
 * members int32 [M]; classes in the order of their labels, members ascending inside a class, so members[class_ptr[c]] is the class's
 * label.  label[N] as mgv_cc_labels writes it (label[i] <= i, label[label[i]] = label[i]; an entry outside [0, N) belongs to nothing).
 * count: sizes from the labels, two flag arrays, two exclusive scans (mgv_scan_exclusive_i32), then counts[6] int32 = {C, M, status[0..3]}
 * (status may be NULL: zeros) — the ONE read-back between sizing and filling.  ws: mgv_cc_class_ws_ints(N) int32s (-1: N out of range),
 * 256-byte aligned, handed unchanged to fill.  min_size < 1: MGV_EINVAL.
 * fill: the selected nodes in id order, a stable sort by label (mgv_sort_pairs; sort_temp of mgv_sort_pairs_temp_ints(4, M) int32s),
 * then members and class_ptr.  C = M = 0 writes class_ptr[0] = 0 only. */
int mgv_cc_class_ws_ints(int64_t N);
int mgv_cc_class_count(int64_t N, const int32_t* label, int min_size, const int32_t* status, int32_t* ws, int64_t ws_ints, int32_t* counts,
                       void* stream);
int mgv_cc_class_fill(int64_t N, const int32_t* label, int64_t C, int64_t M, int32_t* ws, int64_t ws_ints, void* sort_temp,
                      int64_t sort_temp_ints, int64_t* class_ptr, int32_t* members, void* stream);
/* classes straight from the symmetric tile walk (trainer.py:158-160 in the arithmetic of digae_layer.py:31-33): the tiles, scores and
 * decision of mgv_sim_select_fill — v > u, v in u's graph, cosine not NaN and > threshold — but where the fill would store v in row u's
 * list, u and v are united in parent (initialised by mgv_cc_init; several calls may add to one forest).  No pair list ever exists: memory
 * is O(N) whatever the threshold.  A cosine is the same bits whichever entry computes it, so mgv_cc_labels afterwards gives exactly the
 * components of the list mgv_sim_select_fill returns for the same arguments.  Arguments and refusals as mgv_sim_select_count; NULL
 * parent (N > 0) or status: MGV_EINVAL. */
int mgv_sim_union(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, float threshold, int32_t* parent,
                  int32_t* status, void* stream);
/* cross classes straight from the cross walk (trainer.py:158-160 in the arithmetic of digae_layer.py:31-33): the tiles, spans,
 * candidates and decision of mgv_cross_select_fill — v any row of the peer of u's graph, cosine not NaN and > threshold (strict) — but
 * where the fill would store v in row u's list, u and v are united in parent (initialised by mgv_cc_init; several calls may add to
 * one forest: mgv_sim_union followed by mgv_cross_union on one forest gives classes that span a graph and its peer).  u == v (a row of
 * a graph that is its own peer) does nothing, as in mgv_cc_union_pairs.  No pair list ever exists: memory is O(N) whatever the
 * threshold.  CONTRACT: mgv_cc_labels afterwards gives exactly the components of the list mgv_cross_select_fill returns for the same
 * arguments — a cosine is the same bits whichever entry computes it, and a root is only hooked under a smaller root.  Ids reach the
 * union-find only after the walk's clamp of the ranges into [0, N]: no id outside [0, N) is dereferenced whatever graph_ptr and peer
 * hold.  With an involutive peer every pair is met from both sides; the second meeting is two finds and an exit (no rows are skipped).
 * Arguments and refusals as mgv_cross_select_count; in addition a NULL parent (N > 0) or a NULL status: MGV_EINVAL.  N = 0 launches
 * nothing. */
int mgv_cross_union(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, const int32_t* peer, float threshold,
                    int32_t* parent, int32_t* status, void* stream);
/* the distribution of cross scores (trainer.py:158-160 in the arithmetic of digae_layer.py:31-33): the walk, candidates and score of
 * mgv_cross_select_count — unit rows y, every row of the peer of the row's graph, raw cosine — binned as mgv_pair_hist bins:
 * hist[g][k] = number of (row u of graph g, candidate v in graph peer[g]) with #{j : cos > edges[j]} == k.  hist int64 [G][B + 1] is
 * OVERWRITTEN (the launcher zeroes it); the row is the ROW's graph, so with an involutive peer a pair is counted once from each side,
 * in hist[g] and in hist[peer[g]].  A graph with peer = -1 or without rows has a zero row; a NaN is counted nowhere.  Defining
 * property, as integers: for every g and j, sum(hist[g][j+1:]) equals the sum over g's rows of n_sel of mgv_cross_select_count at
 * threshold = edges[j] — the same `>` on the same bits.  Integer atomics only (64-bit LDS counters for a row tile's first and last
 * graph, direct 64-bit adds for the graphs between them, a lane's consecutive candidates of one (graph, bin) merged into one add):
 * exact, the same bytes from call to call.
 * Refused before anything is zeroed or launched: H outside {16, 32, 64, 128} (MGV_EUNSUPPORTED); B outside [1, 256], NULL edges or
 * hist, a table that does not ascend strictly or holds a NaN (read back, as for mgv_pair_hist), and everything mgv_cross_select_count
 * refuses (NULL graph_ptr or peer, a peer entry outside [-1, G), a bad row stride or alignment, N out of range, a graph_ptr that does
 * not start at 0 and end at N): MGV_EINVAL.  N = 0 zeroes hist and launches nothing. */
int mgv_cross_hist(int H, int64_t N, const float* y, int ldy, const int32_t* graph_ptr, int G, const int32_t* peer, const float* edges,
                   int B, int64_t* hist, void* stream);
/* sums[0] += sum_pos -log(sigma+1e-15), sums[1] += sum_neg -log(1-sigma+1e-15); counts += {TP,FP,TN,FN}
 * (trainer.py:240-244); pred_bin[Epos+Eneg] optional */
int mgv_recon_loss_fwd(int H, const float* s, const float* t, int ld, const int64_t* pos_src, const int64_t* pos_dst,
                       int64_t Epos, const int64_t* neg_src, const int64_t* neg_dst, int64_t Eneg,
                       double* sums, uint64_t* counts, int32_t* pred_bin, double* workspace, int64_t workspace_doubles,
                       void* stream);
/* ds/dt += dL/ds, dL/dt for loss = sums[0]/Epos + sums[1]/Eneg scaled by the DEVICE scalar *gscale.
 * When the positive edges are the batch graph's own edges pass its two int32 CSRs (pos_out_* by
 * source, pos_in_* by destination): the positive half then runs as gathers without atomics;
 * NULL CSRs = arbitrary positive list, float atomics (one whole row per wave-instruction).
 * H in {16, 32, 64} (the atomic rows take one float per lane); any other H, 128 included, returns MGV_EUNSUPPORTED with ds / dt
 * untouched — after the argument checks, also when both edge sets are empty. */
int mgv_recon_loss_bwd(int H, int64_t N, const float* s, const float* t, int ld, const int64_t* pos_src, const int64_t* pos_dst,
                       int64_t Epos, const int32_t* pos_out_ptr, const int32_t* pos_out_dst, const int32_t* pos_in_ptr,
                       const int32_t* pos_in_src, const int64_t* neg_src, const int64_t* neg_dst, int64_t Eneg,
                       const float* gscale, float* ds, float* dt, void* stream);
/* the same gradient when BOTH edge sets come as CSR pairs (by source and by destination; the negatives bucketed by
 * mgv_neg_bucket): ds/dt are WRITTEN, every row once, no atomics and no zero fill */
int mgv_recon_loss_bwd_csr(int H, int64_t N, const float* s, const float* t, int ld, const int32_t* pos_out_ptr,
                           const int32_t* pos_out_dst, const int32_t* pos_in_ptr, const int32_t* pos_in_src, int64_t Epos,
                           const int32_t* neg_out_ptr, const int32_t* neg_out_dst, const int32_t* neg_in_ptr,
                           const int32_t* neg_in_src, int64_t Eneg, const float* gscale, float* ds, float* dt,
                           int skip_pos_longer_than /* > 0: positive lists longer than this are left to mgv_recon_heavy_lists */, void* stream);
/* the positive lists mgv_recon_loss_bwd_csr skipped (nodes with thousands of consumers / producers): cut into segments
 * (nodes[K], node_seg_ptr[K+1], seg_node/seg_e0/seg_e1[S]: GraphPlan.heavy_segments), one workgroup per segment, partials
 * [S][H] in partial_ws, added into out (= ds for which 0 with list = pos_out_dst, = dt for which 1 with list = pos_in_src) */
int mgv_recon_heavy_lists(int H, const float* s, const float* t, int ld, int64_t Epos, const float* gscale, int K,
                          const int32_t* nodes, const int32_t* node_seg_ptr, int S, const int32_t* seg_node, const int32_t* seg_e0,
                          const int32_t* seg_e1, const int32_t* list, int which, float* partial_ws, float* out, void* stream);
/* The training step's loss in ONE walk of the lists: mgv_recon_loss_bwd_csr's walk (same ranges, chunks and arithmetic: ds / dt come out
 * bit-identical to it at *gscale == expect_scale, a by-value float here because the upstream gradient is not known yet when the
 * forward runs) which, on the out-list entries — every pair exactly once — also does mgv_recon_loss_fwd's work: sums[0..1] += the
 * two loss sums (that entry's float terms, from a score formed its way — the products of the dot rounded one by one, where the
 * gradient's score is contracted into fmas — added per thread in double, per-workgroup rows in `workspace` (>= 2 * grid doubles,
 * mgv_sum_workspace_doubles() suffices) added in index order: the same bits from run to run), counts[0..3] += {TP, FP, TN, FN},
 * equal to that entry's on every pair.
 * No pair arrays, no pred_bin.  Positive lists longer than skip_pos_longer_than (> 0) are left to mgv_recon_step_heavy_lists. */
int mgv_recon_step_csr(int H, int64_t N, const float* s, const float* t, int ld, const int32_t* pos_out_ptr,
                       const int32_t* pos_out_dst, const int32_t* pos_in_ptr, const int32_t* pos_in_src, int64_t Epos,
                       const int32_t* neg_out_ptr, const int32_t* neg_out_dst, const int32_t* neg_in_ptr,
                       const int32_t* neg_in_src, int64_t Eneg, float expect_scale, double* sums, uint64_t* counts, float* ds,
                       float* dt, int skip_pos_longer_than, double* workspace, int64_t workspace_doubles, void* stream);
/* mgv_recon_heavy_lists for expect_scale by value; with which = 0 (the out lists) the segments' pairs also add their loss terms to
 * sums[0] and their TP / FN to counts[0] / counts[3] (workspace >= min(S, 4096) doubles).  which = 1: sums, counts, workspace unused. */
int mgv_recon_step_heavy_lists(int H, const float* s, const float* t, int ld, int64_t Epos, float expect_scale, int K,
                               const int32_t* nodes, const int32_t* node_seg_ptr, int S, const int32_t* seg_node,
                               const int32_t* seg_e0, const int32_t* seg_e1, const int32_t* list, int which, float* partial_ws,
                               float* out, double* sums, uint64_t* counts, double* workspace, int64_t workspace_doubles,
                               void* stream);
/* rows[0 .. n_floats) *= *g_dev / expect_scale — unless *g_dev == expect_scale: then every workgroup returns after reading the scalar
 * and the rows keep their bits.  The backward of the one-walk loss: the rows were formed for expect_scale in the forward.
 * rows 16-byte aligned; expect_scale 0 or NaN: MGV_EINVAL. */
int mgv_rows_rescale_unless(int64_t n_floats, float* rows, const float* g_dev, float expect_scale, void* stream);
/* ---- link-prediction ranking metrics (digvae_model.py:177-189, digae_model.py:156-168: `test` decodes both edge sets with
 * sigmoid=True, copies every score to the host and calls sklearn's roc_auc_score / average_precision_score).  Here the ranking stays
 * on the device (csrc/link_metrics.hip): keys -> mgv_sort_pairs(4, n, keys, sorted, order, 32, ...) -> rank.
 * link_keys: keys[P + Q] = the decoder's score sigmoid(<s[u], t[v]>) of every pair (positives first; the arithmetic of
 * mgv_edge_dot_fwd) as a 32-bit key whose ASCENDING unsigned order is the DESCENDING score order; scores[P + Q] (nullable): the
 * scores themselves; status[0] += number of NaN scores.  P == 0 or Q == 0: MGV_EINVAL; P + Q >= 2^31: MGV_EUNSUPPORTED.
 * H in {16, 32, 64, 128}: any other is MGV_EUNSUPPORTED after those checks, before anything is launched. */
int mgv_link_keys(int H, const float* s, const float* t, int ld, const int64_t* pos_src, const int64_t* pos_dst, int64_t P,
                  const int64_t* neg_src, const int64_t* neg_dst, int64_t Q, uint32_t* keys, float* scores, int32_t* status,
                  void* stream);
/* link_rank: sorted_keys / order as mgv_sort_pairs left them (element i is a positive iff order[i] < P; both 16-byte aligned).
 * Tie group = maximal run of equal keys; per group g, highest score first: p_g / q_g its positives / negatives, TP_g / FP_g
 * the counts through g.  out (six 8-byte words, written, not added to):
 *   out[0] double AUC = U2 / (2 P Q),  U2 = sum_g p_g (2 (Q - FP_g) + q_g)   (mid-rank Mann-Whitney, an integer)
 *   out[1] double AP  = sum_g p_g TP_g / (TP_g + FP_g) / P                    (sklearn's step-wise definition)
 *   out[2..5] uint64 U2, P, Q, number of tie groups.
 * Deterministic (no float atomics).  work: 8-byte aligned, work_ints >= mgv_link_rank_work_ints(n) (-1: n out of range). */
int mgv_link_rank_work_ints(int64_t n);                                                              /* a size in 4-byte units */
int mgv_link_rank(int64_t n, int64_t P, const uint32_t* sorted_keys, const int32_t* order, double* out, int32_t* work,
                  int64_t work_ints, void* stream);
/* negative sampling of the reconstruction loss (dg_ae_model_aig.py:115-119, torch_geometric negative_sampling): E pairs
 * uniform over {(u, v): u != v, (u, v) not an edge of the CSR}, from a counter-based generator (seed); cnt_out/cnt_in
 * [N] (zeroed by the caller) receive the pairs' per-source / per-destination counts, rank_out/rank_in [E] each pair's place inside
 * its source's / destination's bucket (the count it found).  mgv_neg_bucket then buckets the pairs without atomics: out_ptr/in_ptr =
 * exclusive scans of the counts ([N+1]); outputs the pairs grouped by source (srt_src, srt_dst: int64 like edge_index rows),
 * out_dst[E] and in_src[E] (int32 CSR payloads; order inside a bucket = thread arrival: mgv_sort_lists_i32 fixes it). */
int mgv_neg_sample(int64_t N, int64_t E, uint64_t seed, const int32_t* pos_out_ptr, const int32_t* pos_out_dst,
                   int64_t* neg_src, int64_t* neg_dst, int32_t* cnt_out, int32_t* cnt_in, int32_t* rank_out, int32_t* rank_in,
                   void* stream);
int mgv_neg_bucket(int64_t E, const int64_t* neg_src, const int64_t* neg_dst, const int32_t* out_ptr, const int32_t* in_ptr,
                   const int32_t* rank_out, const int32_t* rank_in, int64_t* srt_src, int64_t* srt_dst, int32_t* out_dst, int32_t* in_src,
                   void* stream);
/* the same draw and the same five arrays as mgv_neg_sample + mgv_neg_bucket + mgv_sort_lists_i32 on both CSRs, integer for integer, in one
 * entry (csrc/neg_partition.hip): the pairs are partitioned by blocks of 2^shift consecutive node ids (chunks of 16,384 slots ordered in
 * LDS, one flat scan of the per-chunk block counts), then every block is finished by one workgroup per side: no global atomic and no
 * scattered store per pair, no list sort of its own, nothing between its kernels.  Written, every entry once: edge_index [2][E] int64
 * (the pairs sorted by (src, dst)), out_ptr / in_ptr [N+1], out_dst / in_src [E] (every list ascending).
 *   shift: 0..12 with ceil(N / 2^shift) <= 2,048 blocks, else MGV_EUNSUPPORTED (the caller then takes the two-entry route); any such
 *   shift gives the same arrays.  A block holding more than 16,384 pairs is finished in several trips over node sub-ranges, a single
 *   list above that in its output rows: slower, never different.
 *   ws: 8-byte aligned, ws_ints >= mgv_neg_partition_ws_ints(N, E) (-1: N < 2, N >= 2^31, E < 0 or E >= 2^28, which the entry answers
 *   with MGV_EINVAL, like a NULL pointer or a short workspace).  ws[0..3] is a status record for tests (written asynchronously, never
 *   read by the product): node blocks, the largest block's pairs, finishing trips summed over both sides (2 x blocks when no block
 *   overflowed), lists finished in their output rows.
 *   E = 0: both ptr arrays zeroed, the payload pointers may be NULL. */
int mgv_neg_partition_ws_ints(int64_t N, int64_t E);                                                 /* a size in 4-byte units */
int mgv_neg_partition(int64_t N, int64_t E, uint64_t seed, int shift, const int32_t* pos_out_ptr, const int32_t* pos_out_dst,
                      int64_t* edge_index, int32_t* out_ptr, int32_t* out_dst, int32_t* in_ptr, int32_t* in_src, int32_t* ws,
                      int64_t ws_ints, void* stream);
/* negative sampling inside each circuit, with a share of reversed links (opt-in; in place of dg_ae_model_aig.py:115-119, whose
 * torch_geometric negative_sampling draws both ends over the whole batch): the candidates every evaluation entry ranks a link against lie
 * in the link's own graph, and the hard negative of a directed link (u, v) is (v, u).  Slot i of a call is a pure function of (seed, i, N,
 * R, graph_ptr, the positive lists) (csrc/mgv_neg_draw.h, neg_draw_slot_local):
 *   ctr = seed ^ (i * 0xD1342543DE82EF95);  attempt a = 0 .. 64:  r = splitmix64(ctr + a),  hi = r >> 32,  lo = r & 0xFFFFFFFF
 *     i <  R:  e = (hi * Epos) >> 32,  s = pos_in_dst[e],  d = pos_in_src[e]
 *     i >= R:  s = (hi * N) >> 32,  g = the largest g < G with graph_ptr[g] <= s,
 *              d = graph_ptr[g] + ((lo * (graph_ptr[g + 1] - graph_ptr[g])) >> 32)
 *   accepted when s != d and (s, d) is not in the positive out-CSR; the pair of attempt 64 is kept whatever it is.
 * graph_ptr [G + 1] int32: non-decreasing from 0 to N, empty graphs allowed; what the kernels read from it is clamped into [0, N], and every
 * drawn id into [0, N): a wrong table gives wrong pairs, never an access outside the arrays.  Up to 4,096 graphs the table is held in LDS.
 * (pos_in_src[e], pos_in_dst[e]), e < Epos: the positive edges in any order (GraphPlan.in_src / in_dst), read only when R > 0.
 * graph_ptr = {0, N} and R = 0 give the draw of mgv_neg_sample / mgv_neg_partition, integer for integer.
 * Refused with MGV_EINVAL, checked in this order, nothing written: G < 1; R < 0 or R > E; R > 0 with Epos < 1 or Epos >= 2^31; a NULL
 * graph_ptr; a NULL pos_in_src or pos_in_dst with R > 0; then
 *   mgv_neg_draw_local: N < 2, N >= 2^31, E < 0, E >= 2^28, a NULL pos_out_ptr; with E > 0 a NULL neg_src or neg_dst.  It writes the
 *     pairs alone, slot by slot (int64 like edge_index rows): the probe of the tests, and with mgv_plan_csr the host's route where
 *     mgv_neg_partition_local answers MGV_EUNSUPPORTED.
 *   mgv_neg_partition_local: everything mgv_neg_partition refuses, the same way (MGV_EINVAL, then MGV_EUNSUPPORTED for the shift).  The
 *     same five arrays, the same ws contract (mgv_neg_partition_ws_ints), status record and shift rule as mgv_neg_partition: only the
 *     draw of its first pass differs.  Reversed slots follow the positive out-degrees: a hub's block may take several finishing trips
 *     and its list the output-row path (slower, never different). */
int mgv_neg_draw_local(int64_t N, int64_t E, uint64_t seed, int64_t R, int G, const int32_t* graph_ptr, const int32_t* pos_out_ptr,
                       const int32_t* pos_out_dst, int64_t Epos, const int32_t* pos_in_src, const int32_t* pos_in_dst, int64_t* neg_src,
                       int64_t* neg_dst, void* stream);
int mgv_neg_partition_local(int64_t N, int64_t E, uint64_t seed, int shift, const int32_t* pos_out_ptr, const int32_t* pos_out_dst,
                            int64_t R, int G, const int32_t* graph_ptr, int64_t Epos, const int32_t* pos_in_src, const int32_t* pos_in_dst,
                            int64_t* edge_index, int32_t* out_ptr, int32_t* out_dst, int32_t* in_ptr, int32_t* in_src, int32_t* ws,
                            int64_t ws_ints, void* stream);

/* ---- functional-similarity loss (trainer.py:158-163, utils/utils.py:32-36): dis = 1 - cos(hf[a], hf[b]),
 * L1 between the z-normalised dis and z-normalised tt.  ws[8] doubles (zeroed by the caller):
 * 0 sum dis, 1 sum dis^2, 2 sum tt, 3 sum tt^2, 4 sum |zd-zt| (loss = ws[4]/P), 5-6 backward sums.
 * fwd: H in {16, 32, 64, 128}; both backwards: H in {16, 32, 64}.  Any other H is MGV_EUNSUPPORTED after the argument checks
 * (P < 2 or a NULL pointer: MGV_EINVAL; bwd_csr: then N = 0: MGV_OK) and before the forward's workspace size is looked at. */
int mgv_func_loss_fwd(int H, int64_t P, const float* hf, const int64_t* pair_a, const int64_t* pair_b,
                      const float* tt, float eps, float* dis, double* ws, double* workspace, int64_t workspace_doubles,
                      void* stream);
/* the same gradient without atomics and without a zero-filled output: every node PULLS over the pairs it belongs to, given
 * the pair lists grouped by first member (a_ptr[N+1], a_pair[P] = pair ids) and by second member (b_ptr, b_pair) — e.g. from
 * mgv_plan_csr over (pair_a, pair_b) with its edge-id outputs; dhf[N][H] is WRITTEN for every node; bit-reproducible.
 * add (nullable, [N][H]): a gradient the same rows receive from another consumer of hf (the readout, trainer.py:155-156), summed
 * into dhf on the way out instead of by a separate N x H add */
int mgv_func_loss_bwd_csr(int H, int64_t N, int64_t P, const float* hf, const int64_t* pair_a, const int64_t* pair_b, const float* tt_sim,
                          const float* dis, float eps, const double* workspace8, const float* grad_loss, const int32_t* a_ptr,
                          const int32_t* a_pair, const int32_t* b_ptr, const int32_t* b_pair, const float* add, float* dhf, void* stream);
int mgv_func_loss_bwd(int H, int64_t P, const float* hf, const int64_t* pair_a, const int64_t* pair_b,
                      const float* tt, const float* dis, float eps, const double* ws, const float* gscale,
                      float* dhf, void* stream);
/* ---- exact functional ordering accuracy (added functionality; utils/utils.py:111-147 get_function_acc on the `dis` of
 * trainer.py:158-160; csrc/concordance.hip).  The reference draws 100 comparisons of two listed truth-table pairs per circuit; this
 * entry counts EVERY unordered comparison {p, q}, p < q, of one segment, as integers.  gt [P] (truth-table distance) and pred [P]
 * (predicted distance, 1 - mgv_pair_scores_at on unit rows) float32 on the device.  With dd = gt[q] - gt[p] and de = pred[q] - pred[p]
 * in float32 a comparison is
 *     eligible at gap j   dd != 0 && fabsf(dd) >= gaps[j]      (the reference's two `continue`s negated; >=, not >)
 *     concordant          (dd > 0 && de > 0) || (dd < 0 && de < 0)
 *     tied                de == 0
 * and out[g][j] = {eligible, eligible and concordant, eligible and tied}.  A NaN in gt makes its comparisons ineligible; a NaN in
 * pred leaves them eligible and neither concordant nor tied (the reference's `succ` stays False).  Comparisons never cross segments
 * and p == q is never counted.  seg_ptr [G+1] int32 on the device: segment g is [seg_ptr[g], seg_ptr[g+1]); NULL is one segment of
 * all P (G is then not looked at beyond its sign, one output row).  Whatever seg_ptr holds, a segment's range is clamped into [0, P)
 * and no index outside it is read; a table that does not ascend makes only the counts meaningless.  gaps_host [B], 1 <= B <= 8,
 * floats in HOST memory, copied into the kernel arguments: the entry reads nothing back and never synchronises.  out int64
 * [max(G, 1)][B][3] is OVERWRITTEN (the launcher zeroes it).  One row of the comparison matrix per thread, column tiles of 256
 * (gt, pred) pairs broadcast from LDS over the upper triangle, int32 counters per lane, 64-bit per workgroup, one global 64-bit
 * integer atomic add per non-zero (segment, gap, kind) of a workgroup's first and last segment (segments wholly inside a tile, fewer
 * than 256 pairs, add once per wave): no floating-point atomics, exact, the same bytes from call to call.
 * Refused with MGV_EINVAL before anything is launched or zeroed: P < 0 or P > 2^31 - 1; G < 0; B outside [1, 8]; a NULL out; a NULL
 * gt, pred or gaps_host with P > 0; a NaN or negative gap.  P = 0 zeroes out and launches nothing. */
int mgv_concord_counts(int64_t P, const float* gt, const float* pred, const int32_t* seg_ptr, int G, const float* gaps_host, int B,
                       int64_t* out, void* stream);

/* ---- reparameterisation sampler + KL (digvae_model.py:134-142, trainer.py:146-147):
 * z = mu + exp(logstd) * eps; eps given, or NULL = drawn from the counter-based generator (seed) and
 * returned in eps_out; klsum += sum(1 + 2 logstd - mu^2 - exp(logstd)^2) */
int mgv_reparam_fwd(int64_t n, const float* mu, const float* logstd, const float* eps, uint64_t seed,
                    float* eps_out, float* z, double* klsum, void* stream);
/* dmu = gz + *gkl*klcoef*(-2mu); dlogstd = gz*eps*exp(logstd) + *gkl*klcoef*(2-2exp(2logstd)); gz/gkl may be NULL */
int mgv_reparam_bwd(int64_t n, const float* mu, const float* logstd, const float* eps, const float* gz,
                    const float* gkl, float klcoef, float* dmu, float* dlogstd, void* stream);
/* ---- the variational link heads in one pass over st = hs_decompose(hs) (digvae_model.py:134-142, trainer.py:145-148; bf16x3,
 * csrc/var_head_x3.hip).  ST [N][ldst >= 2H] = [X_s | X_t].  Per half h: P_h = X_h Wp_h^T + bp_h with Wp_h [2H][H] = fc_h_mu.weight
 * over fc_h_logstd.weight (wpack_h = mgv_wpack_bf16x3(Wp_h, 2H, H, H, 0), bp_h [2H] likewise), the product as mgv_linear_fwd_x3 forms
 * it at (2H, H); mu = P[:, :H], ls = P[:, H:].  eps [N][ldeps >= 2H] = [eps_s | eps_t], or NULL: element (r, c) of half h is the
 * generator of mgv_reparam_fwd at element r*H + c of seed + h.  Z [N][ldz >= 2H]: Z[r][hH + c] = mu + expf(ls) eps (sample = 1) or mu
 * (sample = 0); ls is not clamped.  ML (nullable) [N][ldml >= 4H] = [mu_s | ls_s | mu_t | ls_t].  klsum double[2] is OVERWRITTEN with
 * sum(1 + 2 ls - mu^2 - expf(ls)^2) per half: float32 terms widened at the first addition, per-workgroup sums in rows of `workspace`
 * added in index order — no floating-point atomic, the same bytes from call to call.  workspace: 8-byte aligned, at least
 * mgv_var_head_x3_ws_floats(H, N, 0) floats.
 * Refusals in this order, each before anything is launched or written: H outside {32, 64} MGV_EUNSUPPORTED; N < 0 or a NULL ST, pack,
 * bias, Z, klsum or workspace MGV_EINVAL; a stride below its width or no multiple of 4, or sample outside {0, 1} MGV_EINVAL; a
 * misaligned or short workspace MGV_EINVAL; then N = 0 returns MGV_OK with nothing launched (klsum untouched). */
int mgv_var_head_x3_ws_floats(int H, int64_t N, int backward);                                      /* a size; 0 for a width not served */
int mgv_var_head_fwd_x3(int H, int64_t N, const float* ST, int ldst, const void* wpack_s, const void* wpack_t, const float* b_s,
                        const float* b_t, const float* eps, int ldeps, uint64_t seed, int sample, float* Z, int ldz, float* ML,
                        int ldml, double* klsum, float* workspace, int64_t workspace_floats, void* stream);
/* its whole backward, from ST and the seed alone: P (and eps where it was generated) are recomputed exactly as the forward formed
 * them; with gz = the half's columns of gZ [N][ldg >= 2H] (NULL: zero) and gkl float[2] on the device (NULL: zero), the upstream
 * gradient of each half's sum:  dmu = gz + gkl[h] (-2 mu);  dls = (sample ? gz eps expf(ls) : 0) + gkl[h] (2 - 2 expf(ls)^2);
 * dWp_h [2H][H] += dP^T X_h and dbp_h [2H] += colsum(dP) with dP = [dmu | dls] — both ACCUMULATE, deterministic through workspace rows
 * and a fixed-order second launch as mgv_linear_wgrad_x3 — and dST[r][hH .. (h+1)H) = dP_h Wp_h (WRITTEN, lddst >= 2H) in the same pass.
 * wtpack_h = mgv_wpack_bf16x3(Wp_h, H, 2H, H, 1).  workspace: at least mgv_var_head_x3_ws_floats(H, N, 1) floats.  Refusals as the
 * forward's, in its order (NULL dST / dWp / dbp / transposed pack with the other NULLs); N = 0 returns MGV_OK with nothing launched. */
int mgv_var_head_bwd_x3(int H, int64_t N, const float* ST, int ldst, const void* wpack_s, const void* wpack_t,
                        const void* wtpack_s, const void* wtpack_t, const float* b_s, const float* b_t, const float* eps, int ldeps,
                        uint64_t seed, int sample, const float* gZ, int ldg, const float* gkl, float* dST, int lddst, float* dWp_s,
                        float* dWp_t, float* dbp_s, float* dbp_t, float* workspace, int64_t workspace_floats, void* stream);
/* counts += {TP,FP,TN,FN} of pred_bin vs gt_bin (trainer.py:240-244) */
int mgv_confusion(int64_t n, const int32_t* pred_bin, const int32_t* gt_bin, uint64_t* counts, void* stream);

/* ---- readout MLP pieces (arch/mlp.py:27-47 = Linear, BatchNorm1d, ReLU, Dropout; dg_ae_model_aig.py:102-106)
 * colstats: sums[c] += sum_i Y[i][c], sums[C+c] += sum_i Y[i][c]^2 (BatchNorm batch statistics) */
/* Small sums (column statistics, loss sums, head gradients) are deterministic: every workgroup leaves its partials in its own row of
 * `workspace` (>= mgv_sum_workspace_doubles() doubles, one buffer per stream in flight) and a second launch adds the rows in a fixed
 * order — no floating-point atomics, bit-identical from call to call.  The size covers every served C: at most 2048 workgroup rows of
 * at most 2 * 64 doubles (the launchers themselves insist on workgroups * row only and return MGV_EINVAL below that).
 * Common to the per-layer entries below: C in {4, 8, 16, 32, 64} (else MGV_EINVAL); matrices are contiguous [N][C] (only mgv_colstats
 * takes a row stride) and 16-byte aligned; N = 0 is MGV_OK with nothing written, N < 0 MGV_EINVAL.
 * colstats: sums[2C] (double) is ADDED to; ld >= C and ld % 4 == 0, the columns C .. ld of Y are not read. */
int mgv_sum_workspace_doubles(void);
int mgv_colstats(int64_t N, int C, const float* Y, int ld, double* sums, double* workspace, int64_t workspace_doubles, void* stream);
/* A = dropout_p(relu(gamma*(Y-mean)*invstd+beta)), overwritten; dropout mask from a counter-based hash of (seed, element row * C + col);
 * p_drop in [0, 1) (else MGV_EINVAL); p_drop = 0: no mask, whatever the seed */
int mgv_bn_act_fwd(int64_t N, int C, const float* Y, const float* mean, const float* invstd, const float* gamma,
                   const float* beta, float p_drop, uint64_t seed, float* A, void* stream);
/* dZ = dA * mask * [bn_out > 0] (overwritten); sums[2C] (double) is ADDED to: sums[c] += sum dZ (= dbeta), sums[C+c] += sum dZ*xhat (= dgamma);
 * p_drop in [0, 1) as in the forward (else MGV_EINVAL, nothing written) */
int mgv_bn_act_bwd(int64_t N, int C, const float* Y, const float* mean, const float* invstd, const float* gamma,
                   const float* beta, float p_drop, uint64_t seed, const float* dA, float* dZ, double* sums, double* workspace,
                   int64_t workspace_doubles, void* stream);
/* dY = gamma*invstd*(dZ - [batch_stats](sums[c]/N + xhat*sums[C+c]/N)), overwritten; batch_stats = 0 (eval mode): dY = gamma*invstd*dZ,
 * sums is not read but must not be NULL */
int mgv_bn_bwd_apply(int64_t N, int C, const float* Y, const float* mean, const float* invstd, const float* gamma,
                     const float* dZ, const double* sums, int batch_stats, float* dY, void* stream);
/* prob[N] = A w + b (mlp.py:43, last Linear), clamped to [0,1] when clamp01 != 0 (dg_ae_model_aig.py:105); overwritten */
int mgv_readout_head_fwd(int64_t N, int C, const float* A, const float* w, const float* b, int clamp01, float* prob, void* stream);
/* given dprob[N]: dA = dy w (overwritten); dw[C] and db[1] are ADDED to: dw += sum dy A, db += sum dy; dy = dprob * [clamp inactive],
 * the clamp is inactive for 0 <= A w + b <= 1 (both ends included) and everywhere when clamp01 = 0 */
int mgv_readout_head_bwd(int64_t N, int C, const float* A, const float* w, const float* b, int clamp01, const float* dprob,
                         float* dA, float* dw, float* db, double* workspace, int64_t workspace_doubles, void* stream);
/* ---- fused training-mode readout (arch/mlp.py MLP.forward with dim_in 64, dim_hidden 32, three layers = the pred_prob of
 * dg_ae_model_aig.py:102-106; bf16x3 products).  Passes: hf -> y1, y1 -> y2, y2 -> prob forward; three backward passes that read
 * y1, y2, dprob and hf and recompute activations, dropout masks (the hash of mgv_bn_act_fwd) and BN gradients in registers.
 * wpack: mgv_readout_fused_pack_elems() bf16 = [W1][W2][W2^T][W1^T], each hi/lo planes in fragment order (mgv_wpack_bf16x3).
 * workspace: >= mgv_readout_fused_ws_doubles(N) doubles (per-workgroup slab rows, added in a fixed order: no float atomics). */
int mgv_readout_fused_pack_elems(void);
int mgv_readout_fused_grad_floats(void);
int mgv_readout_fused_ws_doubles(int64_t N);
/* Forward: y1 = hf W1^T + b1, y2 = a1 W2^T + b2 with a_k = dropout(relu(bn_k(y_k))) (batch statistics; running buffers rm/rv
 * updated as nn.BatchNorm1d: running = running * keep + momentum * value, keep = 1 - momentum, unbiased var), prob = clamp(a2 w3 + b3).
 * Out (all overwritten): y1, y2 [N][32]; stats[128] = mean1, invstd1, mean2, invstd2 (kept for the backward); sums[128] (double) scratch;
 * prob [N].  rm / rv are updated in place; momentum, keep and eps are taken as given (keep is not derived from momentum).
 * N >= 1: N = 0 is MGV_EINVAL here (the per-layer entries return MGV_OK).  N = 1: var = 0 and invstd = 1/sqrt(eps) in every column;
 * the unbiased factor is N / max(N - 1, 1) = 1, so running_var = running_var * keep (torch refuses one row in training mode).
 * p1, p2 in [0, 1); workspace_doubles below mgv_readout_fused_ws_doubles(N): MGV_EINVAL. */
int mgv_readout_fused_fwd(int64_t N, const float* hf, const void* wpack, const float* b1, const float* g1, const float* be1,
                          float* rm1, float* rv1, const float* b2, const float* g2, const float* be2, float* rm2, float* rv2,
                          const float* w3, const float* b3, float p1, float p2, uint64_t seed1, uint64_t seed2, float momentum,
                          float keep, float eps, int clamp01, float* y1, float* y2, float* stats, double* sums, float* prob,
                          double* workspace, int64_t workspace_doubles, void* stream);
/* Backward from dprob [N]: dhf [N][64] and grads (mgv_readout_fused_grad_floats() floats: dW1[32][64], db1, dgamma1, dbeta1,
 * dW2[32][32], db2, dgamma2, dbeta2, dw3[32], db3; overwritten); sums[128] (double) scratch. */
int mgv_readout_fused_bwd(int64_t N, const float* hf, const float* y1, const float* y2, const float* stats, const float* dprob,
                          const void* wpack, const float* g1, const float* be1, const float* g2, const float* be2, const float* w3,
                          const float* b3, float p1, float p2, uint64_t seed1, uint64_t seed2, int clamp01, float* dhf,
                          float* grads, double* sums, double* workspace, int64_t workspace_doubles, void* stream);
/* nn.L1Loss, reduction mean (trainer.py:71,156): sum[1] (double) += sum |x - target|;  dx = *gscale/n * sign(x - target), sign(0) = 0,
 * overwritten; gscale is read on the device; n = 0 is MGV_OK with nothing written */
int mgv_l1_loss_fwd(int64_t n, const float* x, const float* target, double* sum, double* workspace, int64_t workspace_doubles,
                    void* stream);
int mgv_l1_loss_bwd(int64_t n, const float* x, const float* target, const float* gscale, float* dx, void* stream);

/* ---- Adam on a flat fp32 buffer (torch.optim.Adam as constructed at trainer.py:73); grad is multiplied
 * by grad_scale first (1/world_size after an all-reduce sum) */
int mgv_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr,
                  float beta1, float beta2, float eps, float weight_decay, float grad_scale, int64_t step, void* stream);

/* ---- on-device batch builder: what the reference recomputes in Python inside every forward —
 * torch.stack([ei[1], ei[0]]) (digae_layer.py:264), the per-level boolean masks (dg_ae_model_aig.py:72-75), the per-node edge
 * scans of `subgraph` (utils/dag_utils.py:91-105) — and at load time the levelisation rounds of top_sort
 * (utils/dag_utils.py:10-37, via return_order_info :80-88).  All index arrays int32; results equal a STABLE sort of the edges by
 * destination / source and of the nodes by (level, slot).  `status` / `done` / `maxlevel` are small DEVICE words written
 * asynchronously (0 = fine): the caller reads them once, after the calls it batches. */
int mgv_scan_exclusive_i32(int64_t n, const int32_t* in, int32_t* out, int32_t* scratch, void* stream);   /* out[n] = total; scratch: n/2048 + 2 */
int mgv_plan_csr_scratch_ints(int64_t N, int64_t E);                                                  /* a size, not a status */
int mgv_plan_csr(int64_t N, int64_t E, const int64_t* src, const int64_t* dst, int32_t* in_ptr, int32_t* in_src, int32_t* in_dst,
                 int32_t* out_ptr, int32_t* out_dst, int32_t* out_slot, int32_t* in_eid /* NULL or [E]: edge id per in-CSR slot */,
                 int32_t* out_eid /* NULL or [E] */, int32_t* scratch, int64_t scratch_ints, int32_t* status, void* stream);
/* every list vals[ptr[n] .. ptr[n+1]) ascending, in place; scratch: N + 1 + E ints.  Applied to the lists mgv_neg_bucket fills in
 * thread-arrival order: their order then no longer depends on it (equal values are interchangeable) */
int mgv_sort_lists_i32(int64_t N, int64_t E, const int32_t* ptr, int32_t* vals, int32_t* scratch, int64_t scratch_ints, void* stream);
/* ASAP levels by frontier relaxation over the out-CSR; `rounds` level steps are enqueued; done[0] == N afterwards iff complete.
 * scratch: 3 N + rounds + 2 ints */
int mgv_plan_levels(int64_t N, const int32_t* in_ptr, const int32_t* out_ptr, const int32_t* out_dst, int32_t* level, int rounds,
                    int32_t* scratch, int64_t scratch_ints, int32_t* done, void* stream);
/* gate id -> aggregator slot (HOST table of 256 bytes, 255 = none), levels to int32, sort key level*T+slot (-1: never updated) */
int mgv_plan_keys(int64_t N, int T, const float* gate, const int64_t* level64, const uint8_t* slot_of_gate_host256, uint8_t* gslot,
                  int32_t* level32, int32_t* key, int32_t* maxlevel, void* stream);
int mgv_plan_check_levels(int64_t E, const int32_t* in_src, const int32_t* in_dst, const uint8_t* gslot, const int32_t* level, int32_t* err,
                          void* stream);
int mgv_count_sort_scratch_ints(int64_t n, int K);                                                    /* a size, not a status */
int mgv_count_sort_i32(int64_t n, const int32_t* key, int K, int32_t* order, int32_t* key_start, int32_t* scratch, int64_t scratch_ints,
                       void* stream);
int mgv_plan_tile_counts(int K, const int32_t* key_start, int32_t* ntile, int32_t* tile_first, int32_t* scan_scratch, void* stream);
int mgv_plan_tiles(int K, int T, int L, int64_t n_active, const int32_t* key_start, const int32_t* tile_first, const int32_t* order,
                   const int32_t* in_ptr, const int32_t* out_ptr, int32_t* tile_start, int32_t* tile_count, int32_t* tile_slot,
                   int32_t* order_span, int32_t* level_tile_ptr, void* stream);
/* packed sweep rows, 32 ints per updated node in sweep order: spans, first 4 in-edge sources, first 8 consumers (node, in-CSR slot) and
 * their gate slots (plan_build.hip k_order_rows); handed to the level sweeps as order_span with order_span_ints = 32 */
int mgv_plan_order_rows(int64_t n_active, const int32_t* order, const int32_t* in_ptr, const int32_t* in_src, const int32_t* out_ptr,
                        const int32_t* out_dst, const int32_t* out_slot, const uint8_t* gslot, int32_t* rows, void* stream);
/* (in-degree, feature class) pairs numbered ascending in degree * 256 + class: cid[N], cls_deg[C] / cls_x[C] (buffers of 65,536; nothing
 * is written behind C), C = rank[65536]; present / rank: 65,537 ints each, scan_scratch: 34.  status[0] = 3 when an in-degree exceeds 255:
 * such a node marks no pair and its cid is the number the pair (255, class) has or would have, in [0, C] — the caller falls back */
int mgv_plan_pairs(int64_t N, const int32_t* in_ptr, const uint8_t* xcls, int32_t* present, int32_t* rank, int32_t* scan_scratch, int32_t* cid,
                   int32_t* cls_deg, uint8_t* cls_x, int32_t* status, void* stream);

/* ---- colour refinement for the quotient stages of the structural encoder (GraphPlan.quotient; digae_layer.py:260: every node starts
 * from ones, so after a half round a node's row depends on (feature class, previous colour, multiset of neighbour colours) only).
 * keys: a 63-bit grouping key per node (f = int64 [3][fstride] random values per previous colour; sums over the list: order
 * independent).  check: exact comparison of every node with its group's representative rep[cid[i]] — class, previous colour, degree,
 * neighbour-colour multiset; flags[0] = 1 on any difference, flags[1] = nodes with lists beyond 48 entries, left to the caller. */
int mgv_colour_keys(int64_t N, const int32_t* nbr_ptr, const int32_t* nbr_idx, const int32_t* prev, const int64_t* f, int64_t fstride,
                    const uint8_t* xcls, int key_bits, int64_t* key, void* stream);
int mgv_colour_check(int64_t N, const int32_t* nbr_ptr, const int32_t* nbr_idx, const int32_t* prev, const uint8_t* xcls, const int32_t* cid,
                     const int32_t* rep, int32_t* flags, void* stream);
/* a refinement stage's tables on the device (csrc/plan_build.hip, GraphPlan._quotient_dev): what GraphPlan.quotient composes from torch
 * sorts / scans / gathers for CPU plans (the reference has no counterpart: it runs every half round on all N rows, digae_layer.py:257-277).
 * sort_pairs: stable radix sort of n keys (key_bytes 4 or 8, unsigned, bits [0, end_bit)), order[] = the sorting permutation (int32). */
int mgv_sort_pairs_temp_ints(int key_bytes, int64_t n);                                             /* a size in 4-byte units (-1: error) */
int mgv_sort_pairs(int key_bytes, int64_t n, const void* keys_in, void* keys_out, int32_t* order, int end_bit, void* temp,
                   int64_t temp_ints, void* stream);
/* runs of equal sorted keys -> colours: cid[N], starts[C + 1] (buffer of N + 1), rep[C] (buffer of N), n_colours[0] = C;
 * scratch_ints >= 2 N + N / 2048 + 66 */
int mgv_colour_groups(int64_t N, const int64_t* skey, const int32_t* by_colour, int32_t* cid, int32_t* starts, int32_t* rep, int32_t* n_colours,
                      int32_t* scratch, int64_t scratch_ints, void* stream);
/* representatives' rows: rptr[C + 1] (rptr[C] = list entries), own[C] previous colour, xrep[C] feature class, n_heavy[0];
 * scratch_ints >= C + C / 2048 + 66; then their lists in previous colours ent[] and the owning colour row[] of every entry */
int mgv_colour_rep_rows(int64_t C, const int32_t* rep, const int32_t* nbr_ptr, const int32_t* prev, const uint8_t* xcls, int heavy_row,
                        int32_t* rptr, int32_t* own, uint8_t* xrep, int32_t* n_heavy, int32_t* scratch, int64_t scratch_ints, void* stream);
int mgv_colour_rep_lists(int64_t C, const int32_t* rep, const int32_t* nbr_ptr, const int32_t* nbr_idx, const int32_t* prev, const int32_t* rptr,
                         int32_t* ent, int32_t* row, void* stream);
int mgv_sorted_key_counts(int64_t n, const int32_t* sorted_keys, int64_t K, int32_t* counts, void* stream);
/* one level of mgv_seg_sum's segment tables: scan leaves work[0..3] = {segments, members, partial rows, colours with > 1 segment},
 * fill writes seg_ptr[n_seg + 1], out_row[n_seg] (nullable) and the next level's colours (nullable pair) */
int mgv_seg_level_work_ints(int64_t G);                                                             /* a size */
int mgv_seg_level_scan(int64_t G, const int32_t* counts, int seg, int32_t* work, int64_t work_ints, void* stream);
int mgv_seg_level_fill(int64_t G, int64_t n_seg, const int32_t* gid, int seg, int base, const int32_t* work, int32_t* seg_ptr, int32_t* out_row,
                       int32_t* gid_next, int32_t* counts_next, void* stream);
/* the flat entry list of mgv_seg_sum_entries for a level-1 table whose members pull their lists: per member position m of items[n_items], in
 * order, items[m] and then ~nbr_idx[e] over items[m]'s list; ent_seg_ptr[s] = entry position of member seg_ptr[s] for s in [0, n_seg]
 * (ent_seg_ptr[n_seg] = entries the tables ask for).  entries[n_entries]: nothing is written behind it (a list of every node once: N + E).
 * Refusals: negative sizes, n_entries < n_items or > 2^31 - 9 (what mgv_seg_sum_entries can walk), NULL seg_ptr / ent_seg_ptr MGV_EINVAL; then n_items == 0 returns MGV_OK with
 * nothing written or launched (every pointer of such a table is 0: the caller's to set); then NULL items / nbr_ptr / nbr_idx / entries /
 * scratch, or scratch_ints below mgv_seg_entries_scratch_ints(n_items) (0 for a size it does not serve) MGV_EINVAL. */
int mgv_seg_entries_scratch_ints(int64_t n_items);                                                  /* a size */
int mgv_seg_entries(int64_t n_items, const int32_t* items, const int32_t* nbr_ptr, const int32_t* nbr_idx, int64_t n_seg, const int32_t* seg_ptr,
                    int64_t n_entries, int32_t* entries, int32_t* ent_seg_ptr, int32_t* scratch, int64_t scratch_ints, void* stream);

/* ---- DiGAE baseline layer, DirectedGCNConv (digae_layer.py:73-114; csrc/digcn_conv.hip).  The lists L(i) a node sums over arrive as a
 * CSR (GraphPlan.csr(reverse): the in-CSR for edge_index as given, the out-CSR for torch.flip(edge_index, [0]), :131,146); with
 * self_loops != 0 every node also sits once in its own list (add_self_loops, :94), without being stored in the CSR.
 * scales (:98-105): r[i] = din(i)^-alpha with din = list length (+1), c[j] = dout(j)^-beta with dout = the opposite CSR's row length (+1);
 * exact for an exponent of 0, 0 for a degree of 0. */
int mgv_digcn_scales(int64_t N, const int32_t* list_ptr, const int32_t* opp_ptr, float alpha, float beta, int self_loops,
                     float* r, float* c, void* stream);
/* the propagate of :107-114 in exact fp32: out[i] = act(outer[i] * (sum_{j in L(i)} inner[j] y[j] [+ inner[i] y[i]])), H in {16,32,64,128}
 * (gather, class_fwd, class_bwd: any other H is MGV_EUNSUPPORTED after the argument checks and before N = 0 returns MGV_OK;
 * class_bwd_ws_floats answers 0),
 * act = ReLU when relu != 0 (F.relu of :127,146).  Forward: outer = r, inner = c.  Backward (the pull that replaces autograd's scatter):
 * the opposite CSR with outer = c, inner = r and mask = the forward's output z[N][H] when it went through the ReLU (a term's columns count
 * where mask[j] > 0; NULL: no mask).  heavy_nodes[heavy_n]: every node whose list is longer than 64 (GraphPlan.heavy), summed by one
 * workgroup each (0 / NULL: every list by its own lane group).  out must not alias y. */
int mgv_digcn_gather(int H, int64_t N, const float* y, const int32_t* nbr_ptr, const int32_t* nbr_idx, const float* outer,
                     const float* inner, const float* mask, int self_loops, int relu, int heavy_n, const int32_t* heavy_nodes,
                     float* out, void* stream);
/* first layer on at most 8 distinct feature rows (xcls[N] = row id, T[C][H] = rows W^T + b formed in weight space): the same sum reading
 * one byte per neighbour, out[i] = act(r[i] * sum_k w_i[k] T[k]) with w_i[k] = sum of c[j] over the list entries of class k.
 * bwd: dT[C][H] += sum_i w_i[k] r[i] [z[i] > 0] dz[i] (z NULL: no ReLU) through workspace rows added in index order
 * (>= mgv_digcn_class_bwd_ws_floats(H, N) floats): no float atomics. */
int mgv_digcn_class_fwd(int H, int64_t N, const uint8_t* xcls, const float* T, int C, const int32_t* nbr_ptr, const int32_t* nbr_idx,
                        const float* outer, const float* inner, int self_loops, int relu, float* out, void* stream);
int mgv_digcn_class_bwd_ws_floats(int H, int64_t N);                                                /* a size */
int mgv_digcn_class_bwd(int H, int64_t N, const uint8_t* xcls, int C, const int32_t* nbr_ptr, const int32_t* nbr_idx, const float* outer,
                        const float* inner, int self_loops, const float* z, const float* dz, float* dT, float* workspace,
                        int64_t workspace_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGVAE_HIP_H */
