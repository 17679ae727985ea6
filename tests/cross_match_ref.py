"""A numpy restatement of the cross-circuit entries of csrc/pair_scores.hip (mgv_cross_topk, mgv_cross_select_count / _fill): who is a
candidate, the `> threshold` decision, the order of a top-k list, its padding, n_above and the ascending per-row lists — from a score
matrix, graph_ptr and peer alone — with the seeded case builders the device tests use.  CPU only; pinned by
tests/test_cross_match_spec.py against a brute-force dense float64 product.

The candidates of a row of graph g are ALL rows of graph peer[g] (peer[g] = -1: none; peer[g] = g: the row's own graph, itself
included).  Everything here is a decision on given scores: applied to the scores mgv_pair_scores_at reports for the device's unit rows it
must give the device's lists EXACTLY, integers as integers and scores as bits.
"""
import numpy as np

TILE, WAVE_ROWS, HEAP = 64, 16, 32       # column / row tile, rows one wave owns, the longest top-k list
GRAPH_SIZES = (70, 1, 64, 129, 0, 63, 5, 33)
PEERS = {
    'involution': (3, 2, 1, 0, -1, 5, 7, 6),        # an involution with a self-peer (5), an empty graph (4: -1) and unequal sizes
    'many_to_one': (3, 3, 3, -1, 0, 0, 2, 2),       # several graphs name one peer; not an involution; far peers inside one row tile
}
KS = (1, 8, 32)
THRESHOLDS = (0.999, 0.25, -2.0)


def graph_ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])


def row_ranges(graph_ptr, peer):
    """(lo, hi) int64 [N]: the candidate columns [lo[u], hi[u]) of every row, lo = hi = 0 where there are none."""
    gp = np.asarray(graph_ptr, dtype=np.int64)
    peer = np.asarray(peer, dtype=np.int64)
    N = int(gp[-1])
    lo, hi = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    for g, p in enumerate(peer.tolist()):
        if p >= 0:
            lo[gp[g]:gp[g + 1]] = gp[p]
            hi[gp[g]:gp[g + 1]] = gp[p + 1]
    return lo, hi


def candidate_mask(graph_ptr, peer):
    """bool [N, N]: entry [u, v] set where v is a candidate of u."""
    lo, hi = row_ranges(graph_ptr, peer)
    col = np.arange(lo.size)
    return (col[None, :] >= lo[:, None]) & (col[None, :] < hi[:, None])


def topk_ref(score, graph_ptr, peer, k, threshold):
    """(idx int32 [N, k], top [N, k] of score's dtype, n_above int32 [N]) from score [N, N] (only candidate entries are looked at):
    per row the k candidates with the largest score, ties to the lower id, a NaN never; -1 / -inf past the end; n_above counts ALL
    candidates with score > threshold."""
    lo, hi = row_ranges(graph_ptr, peer)
    N = lo.size
    idx = np.full((N, k), -1, dtype=np.int32)
    top = np.full((N, k), -np.inf, dtype=score.dtype)
    n_above = np.zeros(N, dtype=np.int32)
    for u in range(N):
        ids = np.arange(lo[u], hi[u])
        s = score[u, lo[u]:hi[u]]
        ok = ~np.isnan(s)
        ids, s = ids[ok], s[ok]
        n_above[u] = int((s > threshold).sum())
        order = np.lexsort((ids, -s))[:k]                  # score descending, then id ascending (-0.0 and 0.0 tie, as `==` has it)
        idx[u, :order.size] = ids[order]
        top[u, :order.size] = s[order]
    return idx, top, n_above


def select_ref(score, graph_ptr, peer, threshold):
    """(row_ptr int64 [N + 1], col int64 [P], val [P]): per row, ascending, the candidates with score > threshold (a NaN never)."""
    keep = candidate_mask(graph_ptr, peer) & (score > threshold)
    row_ptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
    u, v = np.nonzero(keep)                                # row-major: ascending columns inside a row
    return row_ptr, v.astype(np.int64), score[u, v]


def mutual_ref(idx1, top1, graph_ptr, peer, threshold):
    """cross_mutual's definition on top-1 results (idx1, top1 [N]): (pairs int64 [2, M], cos [M]) — v = idx1[u], idx1[v] = u, the
    score > threshold, peer[peer[g]] = g for u's graph g, u in the lower-indexed graph (u <= v inside a self-peer), ordered by u."""
    gp = np.asarray(graph_ptr, dtype=np.int64)
    peer = np.asarray(peer, dtype=np.int64)
    graph_of = np.searchsorted(gp[1:], np.arange(int(gp[-1])), side='right')
    out, cos = [], []
    for u, v in enumerate(np.asarray(idx1).tolist()):
        if v < 0 or int(idx1[v]) != u or not top1[u] > threshold:
            continue
        g, h = int(graph_of[u]), int(graph_of[v])
        if peer[g] < 0 or peer[peer[g]] != g:
            continue
        if g < h or (g == h and u <= v):
            out.append((u, v))
            cos.append(top1[u])
    return np.asarray(out, dtype=np.int64).reshape(-1, 2).T, np.asarray(cos, dtype=np.asarray(top1).dtype)


def tile_spans(graph_ptr, peer, tile_row):
    """The column tiles row tile `tile_row` has to score, as ascending disjoint spans [(first, one past last), ...]: those that hold a
    candidate of one of its 64 rows; overlapping and touching ranges are one span."""
    lo, hi = row_ranges(graph_ptr, peer)
    rows = slice(TILE * tile_row, min(TILE * (tile_row + 1), lo.size))
    rng = sorted({(int(a) // TILE, (int(b) + TILE - 1) // TILE) for a, b in zip(lo[rows], hi[rows]) if a < b})
    spans = []
    for a, b in rng:
        if spans and a <= spans[-1][1]:
            spans[-1][1] = max(spans[-1][1], b)
        else:
            spans.append([a, b])
    return [tuple(s) for s in spans]


# ------------------------------------------------------------------------------------------------ the case (seeded)
def match_case(H, seed=1, sizes=GRAPH_SIZES):
    """x float32 [365, H] for GRAPH_SIZES: normal rows, each times its own power of ten from [-1, 1], and planted in them
      ties    : one direction d as rows 190, 193 and 257 of graph 3 — on both sides of the column-tile borders 192 and 256 — and, times
                0.5, as row 200: four candidates with ONE unit row; the same d as row 5 of graph 0 and, times 4, as row 6 (graph 0
                names graph 3 in both tables): their four best are an exact tie, in id order; and two equal rows, 270 and 300, inside
                the self-peer graph 5;
      zeros   : rows 10 (graph 0), 140 (graph 3) and 280 (graph 5);
      nan     : row 250 (graph 3) holds one NaN: its unit row is all NaN, it is nobody's candidate and has none;
      scaled  : rows 6 and 200 above, and row 100 (graph 2) = 8 x row 75 (graph 2).
    -> {'x', 'graph_ptr', 'N', 'H', 'info'}"""
    rng = np.random.default_rng(9176 * seed + H)
    gp = graph_ptr_of(sizes)
    N = int(gp[-1])
    x = (rng.standard_normal((N, H)) * 10.0 ** rng.uniform(-1, 1, (N, 1))).astype(np.float32)
    d = rng.standard_normal(H).astype(np.float32)
    info = {'trio': (190, 193, 257), 'half': 200, 'copy': 5, 'times4': 6, 'self_pair': (270, 300), 'zeros': (10, 140, 280), 'nan': 250,
            'scaled': (75, 100)}
    for v in info['trio']:
        x[v] = d
    x[info['half']] = np.float32(0.5) * d
    x[info['copy']] = d
    x[info['times4']] = np.float32(4) * d
    x[info['self_pair'][1]] = x[info['self_pair'][0]]
    for z in info['zeros']:
        x[z] = 0
    x[info['nan'], H // 2] = np.nan
    x[info['scaled'][1]] = np.float32(8) * x[info['scaled'][0]]
    return {'x': x, 'graph_ptr': gp, 'N': N, 'H': H, 'info': info}


def unit_rows64(x, eps=1e-8):
    """float64 unit rows, y = x / max(|x|, eps) (a row with a NaN is a row of NaNs)."""
    x = x.astype(np.float64)
    n = np.sqrt((x * x).sum(1))
    return x / np.where(n < eps, eps, n)[:, None]
