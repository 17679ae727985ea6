"""float64 restatements of the functional-similarity entries of csrc/pair_scores.hip (mgv_row_unit, mgv_sim_select_count,
mgv_sim_select_fill; reference: trainer.py:158-160, 1 - cosine_similarity(hf[a], hf[b], eps = 1e-8), in the arithmetic of
digae_layer.py:31-33), with every entry's own error scale, the checkers the device tests use and the seeded case builders.  CPU only;
pinned by tests/test_embed_sim_spec.py.  pair_scores_ref and pair_select_ref are used as they are.

Bounds (u = 2^-24, H = row width; nothing is taken from a device):
  unit row  |err| <= (H/2 + 3) u |y|     sum of H squares in any order: H u relative, halved by the sqrt; the sqrt; the divide; one spare
  norm      |err| <= (H/2 + 2) u |x|     the same without the divide
  cosine    |err| <= (2H + 6) u S,       S[i, j] = sum_k |y_ik y_jk|: two unit rows' errors, (H + 6) u, and one fmaf chain of H terms, H u
The selection is a decision: against the device's own dense scores it is checked exactly, against float64 with each pair's bound, after
the band in which either answer is right has been measured (pair_select_ref's module docstring).
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_scores_ref as PR  # noqa: E402
import pair_select_ref as SR  # noqa: E402

F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64
U24 = PR.U24
TILE, BLOCK = SR.TILE, SR.BLOCK
EPS = 1e-8
THRESHOLDS = (0.999, 0.25, 0.0, -2.0, 1.5)                # of the device tests; 0.0, -2 and 1.5 are exact cases
INF = float('inf')


# ------------------------------------------------------------------------------------------------ launch geometry of mgv_row_unit
# 256 threads, H / 4 lanes per row -> 1024 / H rows per workgroup; at most 2048 workgroups (mgv::grid_for(.., 8)), which then stride.
UNIT_THREADS, UNIT_GRID_CAP = 256, 2048
UNIT_ROWS_PER_BLOCK = {16: 64, 32: 32, 64: 16, 128: 8}    # H -> rows per workgroup
UNIT_CAP_ROWS = {H: UNIT_GRID_CAP * r for H, r in UNIT_ROWS_PER_BLOCK.items()}     # the last N whose rows all have a workgroup position


def unit_grid(H, N):
    r = UNIT_ROWS_PER_BLOCK[H]
    return min(max((N + r - 1) // r, 1), UNIT_GRID_CAP)


def unit_sizes(H):
    """The sizes of the device test: small ones around the 64-row tile, the case size, and one on each side of the grid cap."""
    return (1, 2, 63, 64, 65, 530, UNIT_CAP_ROWS[H], UNIT_CAP_ROWS[H] + 1)


# ------------------------------------------------------------------------------------------------ float64 references
def unit_ref(x, eps=EPS):
    """y = x / max(|x|, eps) per row in float64 -> {'y', 'norm', 'bound' [N, H], 'norm_bound' [N]}."""
    x = x.to(F64)
    H = x.shape[1]
    norm = x.pow(2).sum(1).sqrt()
    y = x / norm.clamp_min(eps)[:, None]                  # clamp_min keeps a NaN
    return {'y': y, 'norm': norm, 'bound': (H / 2 + 3) * U24 * y.abs(), 'norm_bound': (H / 2 + 2) * U24 * norm}


def cos_ref(x, eps=EPS):
    """{'cos', 'S', 'bound'} float64 [N, N] and 'y' = unit_ref's rows."""
    y = unit_ref(x, eps)['y']
    H = y.shape[1]
    S = y.abs() @ y.abs().T
    return {'cos': y @ y.T, 'S': S, 'bound': (2 * H + 6) * U24 * S, 'y': y}


# ------------------------------------------------------------------------------------------------ a float32 stand-in
def unit_f32(x, eps=EPS):
    """What a device may compute: the sum of squares added sequentially in float32, float32 sqrt and divide."""
    x = x.to(F32)
    ss = torch.zeros(x.shape[0], dtype=F32)
    for k in range(x.shape[1]):
        ss = ss + x[:, k] * x[:, k]
    n = ss.sqrt()
    d = torch.where(n < eps, torch.full_like(n, eps), n)
    return x / d[:, None], n


def chain_f32(y):
    """acc = fmaf(y[i][k], y[j][k], acc) over k ascending, for all pairs: the product is exact in float64, the sum rounded to float32."""
    y = y.to(F32)
    acc = torch.zeros((y.shape[0], y.shape[0]), dtype=F32)
    y64 = y.to(F64)
    for k in range(y.shape[1]):
        acc = (acc.to(F64) + y64[:, k, None] * y64[None, :, k]).to(F32)
    return acc


def worst_ratio(val, ref, bound):
    """max |val - ref| / bound over the entries whose reference is a number (inf where a zero bound is missed)."""
    val, ok = val.to(F64), ~torch.isnan(ref)
    e = (val - ref).abs()[ok]
    b = bound[ok]
    if e.numel() == 0:
        return 0.0
    if bool(torch.isnan(e).any()):
        return INF
    r = torch.where(b > 0, e / b.clamp(min=1e-300), torch.where(e > 0, torch.full_like(e, INF), torch.zeros_like(e)))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ the upper selection
def upper_mask(N, graph_ptr):
    """bool [N, N]: the candidates of row u are the nodes v of u's own graph with v > u."""
    return PR.candidate_mask(N, graph_ptr, True) & torch.ones((N, N), dtype=torch.bool).triu(1)


def upper_select_ref(score, graph_ptr, threshold):
    """(row_ptr int64 [N + 1], col int64 [P]): row u lists, ascending, its candidates v > u with score[u, v] > threshold; NaN never."""
    N = score.shape[0]
    keep = (score > threshold) & upper_mask(N, graph_ptr)
    row_ptr = torch.zeros(N + 1, dtype=I64)
    row_ptr[1:] = torch.cumsum(keep.sum(1), 0)
    return row_ptr, torch.nonzero(keep)[:, 1].contiguous()


def _upper_only(x, N, graph_ptr, fill):
    return torch.where(upper_mask(N, graph_ptr) & ~torch.isnan(x), x, torch.full_like(x, fill))


def check_upper(row_ptr, col, score, dense, graph_ptr, threshold):
    """The exact check: SR.check_select on the dense scores with everything that is no upper candidate at -inf (threshold > -inf), so
    the lists must equal nonzero((dense > threshold) & upper_mask) in row-major order and the scores the dense entries' bits."""
    assert threshold > -INF
    N = dense.shape[0]
    return SR.check_select(row_ptr, col, score, _upper_only(dense, N, graph_ptr, -INF), graph_ptr, threshold, True)


def check_upper_band(row_ptr, col, ref, bound, graph_ptr, threshold):
    """Against float64 with no exclusions: SR.check_band with everything that is no upper candidate (a NaN cosine included: it must not
    be selected) at -inf with a zero bound."""
    N = ref.shape[0]
    keep = upper_mask(N, graph_ptr) & ~torch.isnan(ref)
    return SR.check_band(row_ptr, col, torch.where(keep, ref, torch.full_like(ref, -INF)), torch.where(keep, bound, torch.zeros_like(bound)),
                         graph_ptr, threshold, True)


def band_count(ref, bound, threshold, mask):
    """Pairs of `mask` with 0 < |ref - threshold| <= bound: a decision there may go either way."""
    d = (ref - threshold).abs()
    return int(((d > 0) & (d <= bound) & mask).sum())


def band_limit(mask):
    return max(4, int(1e-3 * int(mask.sum())))


def both_sides(row_ptr, col, N):
    """(row_ptr, col) of the upper lists together with their transposes: every pair listed from both of its nodes, rows ascending."""
    m = SR.selected_matrix(row_ptr.to(I64).cpu(), col.to(I64).cpu().flatten(), N)
    m = m | m.T
    out = torch.zeros(N + 1, dtype=I64)
    out[1:] = torch.cumsum(m.sum(1), 0)
    return out, torch.nonzero(m)[:, 1].contiguous()


# ------------------------------------------------------------------------------------------------ the upper fill, restated with defects
DEFECTS = ('diag_ge', 'late_tile', 'graph_start', 'next_graph', 'cursor_reset')


def restated_upper_fill(score, graph_ptr, threshold, defect=None):
    """The symmetric walk as the kernel does it, in Python (SR.restated_fill's style): per row u the 64-column tiles from the row's
    own tile u // 64 (never before its graph's first tile: u lies in its graph) to the end of its graph, in each the four 16-column
    blocks; the decision has the extra term v > u.  -> (row_ptr, col, score); slots never written hold UNWRITTEN / NaN.
      diag_ge      the diagonal is included (v >= u);
      late_tile    the walk starts one tile after the row's own tile;
      graph_start  the walk starts at the graph's first tile and the term v > u is missing: v < u is emitted (and v = u);
      next_graph   the next graph's first node is admitted;
      cursor_reset the row's cursor starts again at every tile."""
    assert defect is None or defect in DEFECTS
    N = score.shape[0]
    lo, hi = (x.tolist() for x in PR.row_range(graph_ptr, N))
    rows = score.tolist()

    def decisions(u, c0):
        bits = []
        for v in range(c0, c0 + BLOCK):
            inside = v < N and (v <= hi[u] if defect == 'next_graph' else v < hi[u])
            if defect == 'graph_start':
                inside = inside and v >= lo[u]
            elif defect == 'diag_ge':
                inside = inside and v >= u
            else:
                inside = inside and v > u
            x = rows[u][v] if inside else 0.0
            bits.append(inside and not math.isnan(x) and x > threshold)
        return bits

    def tiles(u):
        if lo[u] >= hi[u]:
            return range(0)
        first = lo[u] // TILE if defect == 'graph_start' else u // TILE + (1 if defect == 'late_tile' else 0)
        return range(first, (hi[u] + TILE - 1) // TILE)

    n_sel = torch.zeros(N, dtype=I64)
    for u in range(N):
        n_sel[u] = sum(sum(decisions(u, TILE * ct + BLOCK * c)) for ct in tiles(u) for c in range(TILE // BLOCK))
    row_ptr = torch.zeros(N + 1, dtype=I64)
    row_ptr[1:] = torch.cumsum(n_sel, 0)
    total = int(row_ptr[-1])
    col = torch.full((total,), SR.UNWRITTEN, dtype=I64)
    out = torch.full((total,), float('nan'), dtype=score.dtype)
    for u in range(N):
        cursor, room = 0, int(row_ptr[u + 1] - row_ptr[u])
        for ct in tiles(u):
            if defect == 'cursor_reset':
                cursor = 0
            for c in range(TILE // BLOCK):
                c0 = TILE * ct + BLOCK * c
                bits = decisions(u, c0)
                for j, b in enumerate(bits):
                    slot = cursor + sum(bits[:j])
                    if b and slot < room:
                        col[int(row_ptr[u]) + slot] = c0 + j
                        out[int(row_ptr[u]) + slot] = score[u, c0 + j]
                cursor += sum(bits)
    return row_ptr, col, out


# ------------------------------------------------------------------------------------------------ case builders (seeded)
def sim_case(H, seed, sizes=PR.TOPK_SIZES):
    """One batch of graphs of `sizes` nodes, rows PR._rows(N, H, g, 3.0): every row carries its own decade from [-3, 3], because a cosine
    must not care.  Planted, where the batch has a graph of that size:
      200 nodes: a trio across a multiple of 64 — x[b-2], 2 x[b-2] at b+1, x[b-2] / 8 at b+5 (cosine 1 up to rounding, and the SAME unit
                 row in float32: powers of two go through the squares, the sqrt and the divide exactly); a near-duplicate of x[b-2] with
                 noise 1e-2 |x| / sqrt(H) per entry (cosine about 0.99995); the negated row (cosine -1);
      65 nodes : zero rows at its first node and at local index 64 (its last), and one row of entries ~1e-10 whose norm is below eps;
      5 nodes  : its last row times 4 in its first row; and the same last row, bit for bit, in the first node of the next graph: these
                 two must never pair."""
    g = torch.Generator().manual_seed(104729 * seed + H)
    gp = [0]
    for n in sizes:
        gp.append(gp[-1] + n)
    N = gp[-1]
    x = PR._rows(N, H, g, 3.0)
    info = {'trio': None, 'near': None, 'neg': None, 'zeros': [], 'tiny': None, 'scaled': None, 'border': None}
    for i, n in enumerate(sizes):
        lo, hi = gp[i], gp[i + 1]
        if n == 200 and info['trio'] is None:
            b = (lo // TILE + 1) * TILE
            while not (lo + 2 <= b - 2 and b + 30 < hi):
                b += TILE
            x[b + 1] = 2 * x[b - 2]
            x[b + 5] = x[b - 2] / 8
            base = x[b - 2].to(F64)
            x[b + 20] = (base + 1e-2 * base.norm() / math.sqrt(H) * torch.randn(H, generator=g, dtype=F64)).to(F32)
            x[b + 30] = -x[b - 2]
            info['trio'], info['near'], info['neg'] = [b - 2, b + 1, b + 5], b + 20, b + 30
        if n == 65 and not info['zeros']:
            x[lo] = 0
            x[lo + 64] = 0
            x[lo + 10] = (1e-10 * torch.randn(H, generator=g, dtype=F64)).to(F32)
            info['zeros'], info['tiny'] = [lo, lo + 64], lo + 10
    for i, n in enumerate(sizes):                            # after the others: the border copy may land in a graph planted above
        lo, hi = gp[i], gp[i + 1]
        if n == 5 and info['scaled'] is None:
            x[lo] = 4 * x[hi - 1]
            info['scaled'] = (lo, hi - 1)
            if hi < N and hi not in (info['trio'] or []) + info['zeros'] + [info['near'], info['neg'], info['tiny']]:
                x[hi] = x[hi - 1]
                info['border'] = (hi - 1, hi)
    return {'x': x, 'graph_ptr': gp, 'N': N, 'H': H, 'info': info}


def empty_middle_case(H, seed):
    """Graphs without nodes in the middle of graph_ptr (SR.EMPTY_MIDDLE_SIZES), the 5-node graph's plants included."""
    return sim_case(H, seed, sizes=SR.EMPTY_MIDDLE_SIZES)


def nan_case(H, seed):
    """One graph of 200 nodes, graph_ptr None, one row that holds a NaN (it must pair with nothing) and one doubled row."""
    g = torch.Generator().manual_seed(15485863 * seed + H)
    x = PR._rows(200, H, g, 3.0)
    x[77, H // 2] = float('nan')
    x[130] = 2 * x[60]
    return {'x': x, 'graph_ptr': None, 'N': 200, 'H': H, 'info': {'nan': 77, 'pair': (60, 130)}}


CASES = {'sim': sim_case, 'empty_middle': empty_middle_case, 'nan': nan_case}
