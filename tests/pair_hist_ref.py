"""Restatement of the score-distribution entries of csrc/pair_scores.hip (mgv_pair_hist, mgv_sim_hist; the thresholds of
digae_layer.py:31-33 / digae_model.py:118-122 and of trainer.py:158-160 chosen by count): per graph, the candidates of
mgv_pair_select_count / mgv_sim_select_count binned by the number of edges their reported score is > than.  CPU only; pinned by
tests/test_pair_hist_spec.py.  pair_scores_ref, pair_select_ref and embed_sim_ref are used as they are: the candidates are
PR.candidate_mask / ER.upper_mask, a NaN is in no bin, and every comparison is `score > edge` on the float32 edge.

The profile is a set of decisions, like the selection: against the device's own dense scores and against the count entries it is checked
EXACTLY; against float64 the count above an edge may differ by at most the pairs inside their bound of that edge (ER.band_count), after
that band has been held to ER.band_limit.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed_sim_ref as ER  # noqa: E402
import pair_scores_ref as PR  # noqa: E402
import pair_select_ref as SR  # noqa: E402

F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64
TILE = SR.TILE
MAX_EDGES = 256
SLOTS = 2                                                 # LDS histograms of a workgroup: its tile's first and last graph
INF = float('inf')

# ------------------------------------------------------------------------------------------------ the edge tables used everywhere
EDGES = {
    'A': tuple(float(torch.tensor(-1 + (k + 0.5) / 32, dtype=F32)) for k in range(64)),          # 64 even edges across [-1, 1]
    'B': tuple(float(torch.tensor(1 - 2.0 ** -j, dtype=F32)) for j in range(1, 21)),            # 20 edges closing in on 1
    'D': (-2.0, 0.0, 1.5),                                                                        # the exact cases
    'one': (0.999,),
    'wide': tuple(float(torch.tensor(-1.25 + k / 102.0, dtype=F32)) for k in range(256)),        # 256 edges across [-1.25, 1.25]
}


def edges_f32(edges):
    """A table (a name of EDGES or a sequence) as float32 [B]: the values every comparison refers to."""
    e = torch.tensor(EDGES[edges] if isinstance(edges, str) else list(edges), dtype=F32)
    assert 1 <= e.numel() <= MAX_EDGES and bool((e[1:] > e[:-1]).all()) and not bool(torch.isnan(e).any())
    return e


def graph_ids(graph_ptr, N):
    """int64 [N]: the graph of every row (zeros without a graph_ptr), and the number of rows of hist."""
    if graph_ptr is None:
        return torch.zeros(N, dtype=I64), 1
    gp = torch.as_tensor(graph_ptr, dtype=I64)
    return torch.repeat_interleave(torch.arange(gp.numel() - 1), gp[1:] - gp[:-1]), max(gp.numel() - 1, 1)


def mask_of(N, graph_ptr, sym, skip_self=False):
    return ER.upper_mask(N, graph_ptr) if sym else PR.candidate_mask(N, graph_ptr, skip_self)


def passed(score, e):
    """int64, the shape of score: #{j : score > e[j]}, one comparison per edge (a NaN passes none)."""
    sc = score.to(F64)
    k = torch.zeros(sc.shape, dtype=I64)
    for x in e.to(F64).tolist():
        k += (sc > x).to(I64)
    return k


def brute_hist(score, graph_ptr, edges, sym, skip_self=False):
    """int64 [max(G, 1), B + 1] from a score matrix [N, N]: entry [g, k] = candidates of graph g whose score passes exactly k edges."""
    e = edges_f32(edges)
    N, B1 = score.shape[0], e.numel() + 1
    gid, G = graph_ids(graph_ptr, N)
    keep = mask_of(N, graph_ptr, sym, skip_self) & ~torch.isnan(score)
    key = gid[:, None] * B1 + passed(score, e)
    return torch.bincount(key[keep], minlength=G * B1).view(G, B1)


def counts_above(hist):
    """int64 [G, B]: candidates above each edge — the reverse cumulative sum without bin 0."""
    return hist[:, 1:].flip(1).cumsum(1).flip(1)


def select_totals(score, graph_ptr, edges, sym, skip_self=False):
    """int64 [G, B]: the per-graph sums of the count entries' n_sel at threshold = every edge (PR.row_counts / ER.upper_select_ref)."""
    e = edges_f32(edges)
    N = score.shape[0]
    gid, G = graph_ids(graph_ptr, N)
    out = torch.zeros((G, e.numel()), dtype=I64)
    for j, thr in enumerate(e.tolist()):
        if sym:
            row_ptr, _ = ER.upper_select_ref(score, graph_ptr, thr)
            n = row_ptr[1:] - row_ptr[:-1]
        else:
            n = PR.row_counts(score, graph_ptr, thr, skip_self)
        out[:, j] = torch.zeros(G, dtype=I64).index_add_(0, gid, n.to(I64))
    return out


# ------------------------------------------------------------------------------------------------ the walk, restated with defects
DEFECTS = ('ge', 'last_bin', 'diag', 'lower', 'next_graph', 'nan', 'first_graph', 'cursor')
SYM_ONLY = ('diag', 'lower')


def restated_hist(score, graph_ptr, edges, sym, defect=None, skip_self=False):
    """The kernel's walk in Python, a 64 x 64 tile at a time: per row tile the column tiles that meet its rows' graphs (the symmetric
    form from the diagonal tile on), in each the decision `valid` of the count entry, then the branch-free binary search over the table
    padded with +inf to 2^p - 1 entries (pos += score > table[pos + step - 1] ? step : 0 for step = 2^(p-1) .. 1); the tile's first and
    last graph count into their slot, the graphs between them straight into hist, and the slots are flushed at the end.
      ge           `>=` for `>` in the search;
      last_bin     the flush stops one bin early: bin B of the slots is lost;
      diag         the symmetric form counts v = u;
      lower        the symmetric form starts at the graph's first tile and lacks v > u: the lower triangle (and v = u) is counted;
      next_graph   the next graph's first column is admitted;
      nan          a NaN score is a candidate (it passes no edge: bin 0);
      first_graph  every row of a tile is credited to the tile's first graph;
      cursor       the search position is not reset between column tiles."""
    assert defect is None or defect in DEFECTS
    assert sym or defect not in SYM_ONLY
    e = edges_f32(edges)
    N, B = score.shape[0], e.numel()
    B1 = B + 1
    gid, G = graph_ids(graph_ptr, N)
    hist = torch.zeros((G, B1), dtype=I64)
    if N == 0:
        return hist
    lo, hi = PR.row_range(graph_ptr, N)
    top = 1
    while 2 * top <= B:
        top *= 2
    table = torch.cat([e.to(F64), torch.full((2 * top - 1 - B,), INF, dtype=F64)])
    sc = score.to(F64)
    for rt in range((N + TILE - 1) // TILE):
        rows = torch.arange(rt * TILE, min(rt * TILE + TILE, N))
        rlo, rhi, rgi = lo[rows], hi[rows], gid[rows]
        live = rlo < rhi
        if not bool(live.any()):
            continue
        ct0, ct1 = int(rlo[live].min()) // TILE, (int(rhi[live].max()) + TILE - 1) // TILE
        if sym and defect != 'lower':
            ct0 = max(ct0, rt)
        gfirst, glast = int(rgi[0]), int(rgi[-1])
        slots = torch.zeros((SLOTS, B1), dtype=I64)
        pos = None
        for ct in range(ct0, ct1):
            cols = torch.arange(ct * TILE, ct * TILE + TILE)
            inside = cols < N
            blk = torch.zeros((rows.numel(), TILE), dtype=F64)              # zeros past N, as the operand tile holds them
            blk[:, inside] = sc[rows][:, cols[inside]]
            valid = cols[None, :] < (rhi + (1 if defect == 'next_graph' else 0))[:, None]
            if sym and defect == 'lower':
                valid &= cols[None, :] >= rlo[:, None]
            elif sym:
                valid &= (cols[None, :] >= rows[:, None]) if defect == 'diag' else (cols[None, :] > rows[:, None])
            else:
                valid &= cols[None, :] >= rlo[:, None]
                if skip_self:
                    valid &= cols[None, :] != rows[:, None]
            if defect != 'nan':
                valid &= ~torch.isnan(blk)
            if pos is None or defect != 'cursor':
                pos = torch.zeros(blk.shape, dtype=I64)
            step = top
            while step > 0:
                t = table[(pos + step - 1).clamp(max=table.numel() - 1)]
                pos = pos + step * ((blk >= t) if defect == 'ge' else (blk > t)).to(I64)
                step //= 2
            bins = pos.clamp(max=B)
            credit = torch.full_like(rgi, gfirst) if defect == 'first_graph' else rgi
            for g in torch.unique(credit).tolist():
                n = torch.bincount(bins[valid & (credit == g)[:, None]], minlength=B1)
                if g == gfirst:
                    slots[0] += n
                elif g == glast:
                    slots[1] += n
                else:
                    hist[g] += n
        nb = B if defect == 'last_bin' else B1
        hist[gfirst, :nb] += slots[0, :nb]
        hist[glast, :nb] += slots[1, :nb]
    return hist


# ------------------------------------------------------------------------------------------------ case builders (seeded)
def many_graphs_case(H, seed, graphs=64):
    """`graphs` graphs of 1 to 3 nodes: one 64-row tile meets dozens of graphs, most of them between its first and its last.  Rows for
    both forms: x (the cosine; one duplicated row inside a 3-node graph) and s, t (the decoder)."""
    g = torch.Generator().manual_seed(6700417 * seed + H)
    sizes = torch.randint(1, 4, (graphs,), generator=g).tolist()
    gp = [0]
    for n in sizes:
        gp.append(gp[-1] + n)
    N = gp[-1]
    x = PR._rows(N, H, g, 3.0)
    three = [i for i, n in enumerate(sizes) if n == 3]
    if three:
        x[gp[three[0]] + 2] = 2 * x[gp[three[0]]]
    return {'x': x, 's': PR._rows(N, H, g, 1.0), 't': PR._rows(N, H, g, 1.0), 'graph_ptr': gp, 'N': N, 'H': H, 'sizes': sizes}
