"""A numpy restatement of the two further consumers of the cross walk of csrc/pair_scores.hip — mgv_cross_union (classes without a pair
list) and mgv_cross_hist (the distribution of cross cosines) — on top of tests/cross_match_ref.py: the same candidates, the same strict
`> threshold`, a NaN nobody's candidate.  CPU only; pinned by tests/test_cross_walk_spec.py against a brute-force BFS on the dense
boolean relation and against select_ref's row counts.

Everything here is a decision on given scores: applied to the scores mgv_pair_scores_at reports for the device's unit rows it must give
the device's labels and bins EXACTLY, as integers.
"""
import numpy as np

from cross_match_ref import PEERS, THRESHOLDS, candidate_mask, graph_ptr_of, match_case, row_ranges, select_ref  # noqa: F401

SMALL_GRAPHS, SMALL_NODES = 64, 8        # 64 graphs of 8 nodes: one row tile holds eight graphs whose peers lie in eight column tiles


def random_involution(G, seed):
    """peer int64 [G]: a seeded random involution without fixed points (G even) — peer[peer[g]] = g, peer[g] != g."""
    order = np.random.default_rng(seed).permutation(G)
    peer = np.empty(G, dtype=np.int64)
    peer[order[0::2]] = order[1::2]
    peer[order[1::2]] = order[0::2]
    return peer


def small_case(H, seed=3):
    """x float32 [512, H], 64 graphs of 8 nodes and a random involution: normal rows; graph g's rows 0 and 1 are copied (times a power
    of two) into its peer's rows 0 and 1 from the lower graph of a couple, so every couple has cross links at 0.999, and rows 2 and 3
    of every fourth graph are equal, so own-graph links exist too.  -> {'x', 'graph_ptr', 'peer', 'N', 'H'}"""
    rng = np.random.default_rng(4411 * seed + H)
    gp = graph_ptr_of((SMALL_NODES,) * SMALL_GRAPHS)
    N = int(gp[-1])
    peer = random_involution(SMALL_GRAPHS, seed)
    x = rng.standard_normal((N, H)).astype(np.float32)
    for g in range(SMALL_GRAPHS):
        p = int(peer[g])
        if g < p:
            x[gp[p]] = x[gp[g]]
            x[gp[p] + 1] = np.float32(2) * x[gp[g] + 1]
        if g % 4 == 0:
            x[gp[g] + 3] = x[gp[g] + 2]
    return {'x': x, 'graph_ptr': gp, 'peer': peer, 'N': N, 'H': H}


def own_pairs(score, graph_ptr, threshold):
    """(u, v) int64 arrays: the own-graph pairs v > u with score[u, v] > threshold (a NaN never), the relation of mgv_sim_select_*."""
    gp = np.asarray(graph_ptr, dtype=np.int64)
    N = int(gp[-1])
    graph_of = np.searchsorted(gp[1:], np.arange(N), side='right')
    col = np.arange(N)
    keep = (graph_of[:, None] == graph_of[None, :]) & (col[None, :] > col[:, None]) & (score > threshold)
    return np.nonzero(keep)


def classes_ref(score, graph_ptr, peer, threshold, with_own):
    """label int64 [N], label[i] = the smallest id of i's class: a sequential union-find over select_ref's pairs (row u, listed v), plus
    the own-graph pairs v > u above the threshold when with_own.  `score` [N, N]: cross entries are read at [u, v] for v a candidate of
    u, own entries at [u, v] for v > u in u's graph."""
    gp = np.asarray(graph_ptr, dtype=np.int64)
    N = int(gp[-1])
    row_ptr, col, _ = select_ref(score, gp, peer, threshold)
    us = np.repeat(np.arange(N), np.diff(row_ptr))
    pairs = list(zip(us.tolist(), col.tolist()))
    if with_own:
        a, b = own_pairs(score, gp, threshold)
        pairs += list(zip(a.tolist(), b.tolist()))
    parent = list(range(N))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for u, v in pairs:
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)            # the smaller root wins: a root is its class's smallest id
    return np.asarray([find(i) for i in range(N)], dtype=np.int64)


def hist_ref(score, graph_ptr, peer, edges):
    """int64 [G, B + 1]: hist[g][k] = number of (row u of graph g, candidate v of u) with #{j : score[u, v] > edges[j]} == k, from the
    `>` comparisons themselves (no search, no affine map); a NaN score is counted nowhere."""
    gp = np.asarray(graph_ptr, dtype=np.int64)
    G = gp.size - 1
    e = np.asarray(edges, dtype=np.float32)
    mask = candidate_mask(gp, peer) & ~np.isnan(score)
    hist = np.zeros((G, e.size + 1), dtype=np.int64)
    with np.errstate(invalid='ignore'):
        for g in range(G):
            rows = slice(int(gp[g]), int(gp[g + 1]))
            s, m = score[rows], mask[rows]
            k = np.zeros(s.shape, dtype=np.int64)
            for j in range(e.size):
                k += s > e[j]
            hist[g] = np.bincount(k[m], minlength=e.size + 1)
    return hist


def counts_above_ref(hist):
    """int64 [G, B]: sum(hist[g][j + 1:]) for every j."""
    return hist[:, :0:-1].cumsum(1)[:, ::-1]
