"""numpy restatements of the rank entry of csrc/pair_scores.hip (mgv_pair_rank_counts; reference: digae_layer.py:31-33,
digae_model.py:118-122) and of what ops.link_ranks / ops.rank_metrics build on it, each from its definition: counts by plain loops over
a score matrix, filtered ranks by removing a row's other true links from its candidates, metrics by per-graph sums.  CPU only; pinned
by tests/test_pair_rank_spec.py.

A score matrix here is float32 [N, N] with [u, v] = <s_u, t_v>: the device's own dense scores in the device tests, scores_f32 (the
k-ascending fmaf chain tests/embed_sim_ref.py states, on two operands) on the CPU.  Everything compared is an integer."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed_sim_ref as ER  # noqa: E402
import pair_scores_ref as PR  # noqa: E402

F64, F32 = torch.float64, torch.float32
PASS = 32                                                 # thresholds of a row one walk of its tile serves
TILE = PR.TILE


def scores_f32(s, t):
    """[M, N] float32: acc = fmaf(s[i][k], t[j][k], acc) over k ascending — ER.chain_f32 on the stacked rows, its s-by-t block."""
    M = s.shape[0]
    return ER.chain_f32(torch.cat([s.to(F32), t.to(F32)]))[:M, M:].contiguous()


def candidates(N, graph_ptr, skip_self):
    """bool [N, N] numpy: [u, v] = v is a candidate of u (PR.candidate_mask; a NaN score is excluded by the comparisons themselves)."""
    return PR.candidate_mask(N, graph_ptr, skip_self).numpy()


def rank_counts_ref(score, thr_ptr, thr, graph_ptr=None, skip_self=False):
    """(n_gt, n_eq) int64 [T] by plain loops; entries no row lists keep -1."""
    sc = np.asarray(score, dtype=np.float32)
    N = sc.shape[0]
    tp, th = np.asarray(thr_ptr, dtype=np.int64), np.asarray(thr, dtype=np.float32)
    cand = candidates(N, graph_ptr, skip_self)
    n_gt, n_eq = np.full(th.shape[0], -1, dtype=np.int64), np.full(th.shape[0], -1, dtype=np.int64)
    with np.errstate(invalid='ignore'):
        for u in range(N):
            row = sc[u][cand[u]]
            for j in range(tp[u], tp[u + 1]):
                n_gt[j] = int((row > th[j]).sum())
                n_eq[j] = int((row == th[j]).sum())
    return n_gt, n_eq


def sorted_lists(thr_ptr, thr):
    """(thr ascending inside every row, NaNs last — the entry's contract —, order) with sorted = thr[order]."""
    tp, th = np.asarray(thr_ptr, dtype=np.int64), np.asarray(thr, dtype=np.float32)
    order = np.arange(th.shape[0])
    for u in range(tp.shape[0] - 1):
        a, b = tp[u], tp[u + 1]
        order[a:b] = a + np.argsort(th[a:b], kind='stable')
    return th[order], order


def link_ranks_ref(score, edge_index, graph_ptr=None, by='src', skip_self=False, filtered=True):
    """(rank_lo, rank_hi int64 [E], valid bool [E]) from the definition, link by link: the candidates of the link's row, without the
    row's other valid listed links when filtered, compared with the link's own score."""
    sc = np.asarray(score, dtype=np.float32)
    sc = sc if by == 'src' else sc.T
    N = sc.shape[0]
    ei = np.asarray(edge_index, dtype=np.int64)
    rows, cols = (ei[0], ei[1]) if by == 'src' else (ei[1], ei[0])
    E = rows.shape[0]
    cand = candidates(N, graph_ptr, skip_self)
    valid = np.array([bool(cand[rows[e], cols[e]]) and not np.isnan(sc[rows[e], cols[e]]) for e in range(E)], dtype=bool)
    lo, hi = np.zeros(E, dtype=np.int64), np.zeros(E, dtype=np.int64)
    of_row = {}
    for e in range(E):
        of_row.setdefault(int(rows[e]), []).append(e)
    with np.errstate(invalid='ignore'):
        for e in range(E):
            if not valid[e]:
                continue
            keep = cand[rows[e]].copy()
            if filtered:
                for f in of_row[int(rows[e])]:
                    if f != e and valid[f]:
                        keep[cols[f]] = False
            row, x = sc[rows[e]][keep], sc[rows[e], cols[e]]
            gt, eq = int((row > x).sum()), int((row == x).sum())
            lo[e], hi[e] = 1 + gt, gt + eq
    return lo, hi, valid


def rank_metrics_ref(lo, hi, valid, edge_index, graph_ptr, ks, by='src'):
    """dict of numpy arrays per graph: ranked, hits_lo, hits_hi [G, K], sum_lo, sum_hi (int64) and mrr (float64, NaN without a link)."""
    ei = np.asarray(edge_index, dtype=np.int64)
    rows = ei[0] if by == 'src' else ei[1]
    gp = np.asarray(graph_ptr, dtype=np.int64)
    G = gp.shape[0] - 1
    out = {'ranked': np.zeros(G, np.int64), 'hits_lo': np.zeros((G, len(ks)), np.int64), 'hits_hi': np.zeros((G, len(ks)), np.int64),
           'sum_lo': np.zeros(G, np.int64), 'sum_hi': np.zeros(G, np.int64), 'mrr': np.full(G, np.nan)}
    for g in range(G):
        m = valid & (rows >= gp[g]) & (rows < gp[g + 1])
        n = int(m.sum())
        out['ranked'][g] = n
        out['sum_lo'][g], out['sum_hi'][g] = lo[m].sum(), hi[m].sum()
        for j, k in enumerate(ks):
            out['hits_lo'][g, j], out['hits_hi'][g, j] = int((lo[m] <= k).sum()), int((hi[m] <= k).sum())
        if n:
            out['mrr'][g] = float(np.sum((1.0 / lo[m] + 1.0 / hi[m]) / 2)) / n
    return out


# ------------------------------------------------------------------------------------------------ case builders (seeded)
def int_case(N, H, seed, span=3):
    """s, t with small-integer entries in [-span, span]: every product and every partial sum is an integer far below 2^24, so the
    float32 chain and a float64 product agree exactly — and many scores tie."""
    g = torch.Generator().manual_seed(9176 * seed + 13 * N + H)
    s = torch.randint(-span, span + 1, (N, H), generator=g).to(F32)
    t = torch.randint(-span, span + 1, (N, H), generator=g).to(F32)
    return s, t


def float_case(N, H, seed):
    g = torch.Generator().manual_seed(4441 * seed + 17 * N + H)
    return PR._rows(N, H, g, 1.0), PR._rows(N, H, g, 1.0)


def random_edges(N, graph_ptr, per_node, seed):
    """Distinct directed pairs inside the graphs: up to per_node targets per node (self loops allowed)."""
    g = torch.Generator().manual_seed(77 * seed + 3)
    gp = [0, N] if graph_ptr is None else list(graph_ptr)
    pairs = set()
    for i in range(len(gp) - 1):
        n = gp[i + 1] - gp[i]
        for u in range(gp[i], gp[i + 1]):
            for v in torch.randint(0, n, (per_node,), generator=g).tolist():
                pairs.add((u, gp[i] + v))
    pairs = sorted(pairs)
    perm = torch.randperm(len(pairs), generator=g).tolist()
    return torch.tensor([pairs[i] for i in perm], dtype=torch.int64).T.contiguous() if pairs else torch.zeros((2, 0), dtype=torch.int64)


def lists_of_lengths(lengths, values, seed):
    """(thr_ptr int32 [N + 1], thr float32 [T]): row u lists lengths[u] values drawn (with repeats) from `values`."""
    g = torch.Generator().manual_seed(seed)
    tp = np.zeros(len(lengths) + 1, dtype=np.int64)
    tp[1:] = np.cumsum(lengths)
    vals = np.asarray(values, dtype=np.float32)
    idx = torch.randint(0, len(vals), (int(tp[-1]),), generator=g).numpy()
    return tp.astype(np.int32), vals[idx]
