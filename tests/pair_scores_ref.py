"""float64 restatements of the all-pairs decoder entries of csrc/pair_scores.hip (mgv_pair_scores_fwd / _bwd / _at, mgv_pair_topk;
reference: digae_layer.py:26-33 forward_all, digae_model.py:118-122), from exactly the ABI's arguments, with every entry's own error
scale, the checkers the device tests use and the seeded case builders.  CPU only; pinned by tests/test_pair_scores_spec.py.

Bounds (u = 2^-24, H = row width; derived as in tests/test_hip_losses_reference.py:83-85, nothing is taken from a device):
  raw score     |err| <= H u S,            S[i, j] = sum_k |s_ik t_jk|            (one fmaf chain of H terms)
  p = sigma     |err| <= dq = 4 u + p (1 - p) H u S                               (v_exp_f32 + v_rcp_f32 + the add; the raw error through sigma')
  ds_ik         |err| <= max(H, L) u sum_j |g_ij| p (1 - p) |t_jk| + sum_j |g_ij| dq_ij |t_jk|
                L = chain_length(walked dimension): the kernel adds every entry in ONE fmaf chain over the walked dimension in tile
                order, zeros to the end of the last 64-tile included; the second sum is what G = g p (1 - p) inherits from the
                stored float32 p; dt alike with s and the transposes; without the sigmoid p (1 - p) = 1 and dq = 0.
"""
import math

import torch

F64, F32 = torch.float64, torch.float32
U24 = 2.0 ** -24
TILE = 64


def chain_length(n):
    """Sequential float32 additions behind one backward entry whose walked dimension has n terms (k_pair_bwd: one accumulator per
    entry through all 64-wide tiles of the walked dimension)."""
    return TILE * ((int(n) + TILE - 1) // TILE)


# ------------------------------------------------------------------------------------------------ dense scores
def scores_ref(s, t, H=None):
    """raw, S, p, and the two bounds, all float64 [M, N]."""
    s, t = s.to(F64), t.to(F64)
    H = s.shape[1] if H is None else H
    raw = s @ t.T
    S = s.abs() @ t.abs().T
    p = torch.sigmoid(raw)
    raw_bound = H * U24 * S
    dq = 4 * U24 + p * (1 - p) * H * U24 * S
    return {'raw': raw, 'S': S, 'p': p, 'raw_bound': raw_bound, 'dq': dq}


def grads_ref(s, t, g, sigmoid):
    """ds = G t, dt = G^T s with G = g p (1 - p) (sigmoid) or g; with the bound of every entry (module docstring)."""
    s64, t64, g64 = s.to(F64), t.to(F64), g.to(F64)
    H = s64.shape[1]
    M, N = s64.shape[0], t64.shape[0]
    r = scores_ref(s64, t64)
    if sigmoid:
        w = r['p'] * (1 - r['p'])
        dq = r['dq']
    else:
        w = torch.ones_like(r['raw'])
        dq = torch.zeros_like(r['raw'])
    G = g64 * w
    out = {'ds': G @ t64, 'dt': G.T @ s64}
    Ls, Lt = chain_length(N), chain_length(M)
    out['ds_bound'] = max(H, Ls) * U24 * ((g64.abs() * w) @ t64.abs()) + (g64.abs() * dq) @ t64.abs()
    out['dt_bound'] = max(H, Lt) * U24 * ((g64.abs() * w).T @ s64.abs()) + (g64.abs() * dq).T @ s64.abs()
    return out


# ------------------------------------------------------------------------------------------------ top-k and counts
def row_range(graph_ptr, N):
    """(lo, hi) int64 [N]: each row's candidate columns; graph_ptr None = one graph of all N."""
    if graph_ptr is None:
        return torch.zeros(N, dtype=torch.int64), torch.full((N,), N, dtype=torch.int64)
    gp = torch.as_tensor(graph_ptr, dtype=torch.int64)
    sizes = gp[1:] - gp[:-1]
    return torch.repeat_interleave(gp[:-1], sizes), torch.repeat_interleave(gp[1:], sizes)


def candidate_mask(N, graph_ptr, skip_self):
    lo, hi = row_range(graph_ptr, N)
    col = torch.arange(N)
    m = (col[None, :] >= lo[:, None]) & (col[None, :] < hi[:, None])
    if skip_self:
        m &= ~torch.eye(N, dtype=torch.bool)
    return m


def topk_ref(raw, graph_ptr, k, skip_self, sigmoid=True):
    """Brute force: (idx int32 [N, k], score [N, k]) ordered by raw descending, ties by ascending id; -1 / -inf past the end; NaN never."""
    N = raw.shape[0]
    mask = candidate_mask(N, graph_ptr, skip_self) & ~torch.isnan(raw)
    idx = torch.full((N, k), -1, dtype=torch.int32)
    score = torch.full((N, k), -math.inf, dtype=raw.dtype)
    for u in range(N):
        cand = torch.nonzero(mask[u]).flatten().tolist()
        cand.sort(key=lambda v: (-float(raw[u, v]), v))
        for j, v in enumerate(cand[:k]):
            idx[u, j] = v
            score[u, j] = torch.sigmoid(raw[u, v]) if sigmoid else raw[u, v]
    return idx, score


def row_counts(score, graph_ptr, threshold, skip_self=False):
    """n_above: candidates of each row whose reported score is > threshold (strictly, like pred_bin); NaN never counts."""
    mask = candidate_mask(score.shape[0], graph_ptr, skip_self)
    return ((score > threshold) & mask).sum(1)


def graph_sums(per_row, graph_ptr):
    gp = torch.as_tensor(graph_ptr, dtype=torch.int64)
    cs = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(per_row.to(torch.int64), 0)])
    return cs[gp[1:]] - cs[gp[:-1]]


def graph_counts(score, edge_index, graph_ptr, threshold):
    """int64 [G, 4]: true positives, predicted positives over all n_g^2 ordered pairs, edges, ordered pairs."""
    gp = torch.as_tensor(graph_ptr, dtype=torch.int64)
    src, dst = edge_index[0].long(), edge_index[1].long()
    gid = torch.bucketize(src, gp[1:].contiguous(), right=True)
    G = gp.numel() - 1
    hit = (score[src, dst] > threshold).long()
    tp = torch.zeros(G, dtype=torch.int64).index_add_(0, gid, hit)
    ne = torch.zeros(G, dtype=torch.int64).index_add_(0, gid, torch.ones_like(hit))
    n = gp[1:] - gp[:-1]
    return torch.stack([tp, graph_sums(row_counts(score, gp, threshold), gp), ne, n * n], 1)


def band_fraction(score, bound, threshold, mask):
    """Share of the candidate pairs whose float64 score lies within its bound of the threshold (a count there may go either way)."""
    near = ((score - threshold).abs() <= bound) & mask
    return float(near.sum()) / max(int(mask.sum()), 1)


def check_topk(idx, score, r, graph_ptr, k, skip_self, sigmoid):
    """The top-k answer (idx, score) against float64 with NO exclusions; r = scores_ref of the case.  Returns the list of what is wrong.
      - every index is -1 or a valid, distinct candidate of its row; -1 entries only behind all candidates, with score -inf;
      - min(k, candidates) entries are returned;
      - every returned score within its bound (raw_bound, or dq with the sigmoid) of the float64 score;
      - the order: the float64 raw scores of consecutive entries may rise by no more than their two bounds added;
      - no candidate that was NOT returned has a float64 raw score above the row's smallest returned one by more than the two bounds added."""
    raw, rb = r['raw'], r['raw_bound']
    ref = r['p'] if sigmoid else raw
    sb = r['dq'] if sigmoid else rb
    N = raw.shape[0]
    mask = candidate_mask(N, graph_ptr, skip_self) & ~torch.isnan(raw)
    bad = []
    idx, score = idx.long(), score.to(F64)
    for u in range(N):
        ncand = int(mask[u].sum())
        want = min(k, ncand)
        row = idx[u].tolist()
        got = row[:want]
        if any(v != -1 for v in row[want:]) or any(not math.isinf(x) or x > 0 for x in score[u, want:].tolist()):
            bad.append('row %d: padding behind %d candidates is not (-1, -inf): %s' % (u, want, row))
        if any(v < 0 or v >= N or not bool(mask[u, v]) for v in got):
            bad.append('row %d: an index outside the row\'s candidates: %s' % (u, got))
            continue
        if len(set(got)) != len(got):
            bad.append('row %d: repeated index: %s' % (u, got))
            continue
        if not got:
            continue
        gi = torch.tensor(got)
        e = (score[u, :want] - ref[u, gi]).abs()
        if bool((e > sb[u, gi]).any()):
            bad.append('row %d: a returned score is outside its bound (%.3g of it)' % (u, float((e / sb[u, gi]).max())))
        rr, bb = raw[u, gi], rb[u, gi]
        if want > 1 and bool((rr[1:] - rr[:-1] > bb[1:] + bb[:-1]).any()):
            bad.append('row %d: not in descending order beyond the bounds: %s' % (u, got))
        rest = mask[u].clone()
        rest[gi] = False
        if bool(rest.any()):
            j = int(torch.argmin(rr))
            over = (raw[u] - rr[j] > rb[u] + bb[j]) & rest
            if bool(over.any()):
                bad.append('row %d: candidate %d is better than returned %d beyond the bounds' % (u, int(torch.nonzero(over)[0]), got[j]))
    return bad


# ------------------------------------------------------------------------------------------------ case builders (seeded)
def _rows(n, H, g, decades):
    """n rows of standard normal entries, each row times its own power of ten from [-decades, decades]."""
    e = (torch.rand(n, 1, generator=g, dtype=F64) * 2 - 1) * decades
    return (torch.randn(n, H, generator=g, dtype=F64) * 10.0 ** e).to(F32)


def dense_case(M, N, H, seed, sigmoid=True):
    """s [M, H], t [N, H], g [M, N] float32: rows each carry their own power of ten from [-1, 1] ([-3, 3] for the raw-score cases,
    whose outputs are not squashed)."""
    g = torch.Generator().manual_seed(1000003 * seed + 101 * M + 7 * N + H)
    dec = 1.0 if sigmoid else 3.0
    return {'s': _rows(M, H, g, dec), 't': _rows(N, H, g, dec), 'g': _rows(M, N, g, 1.0) if M and N else torch.zeros(M, N), 'H': H,
            'M': M, 'N': N, 'sigmoid': sigmoid}


TOPK_SIZES = (1, 2, 63, 64, 65, 130, 5, 200)


def topk_case(H, seed, sizes=TOPK_SIZES, plant=True):
    """One batch of graphs of `sizes` nodes (graph boundaries inside the 64-row and 64-column tiles), with planted structure:
      ties      : t rows duplicated across a column-tile boundary inside one graph, scaled to rank first for about half its rows;
      edges     : for one row of a small graph the three best columns over ALL nodes are its graph's first node, its last node and the
                  node just past it (the next graph's first: must never appear);
      self      : one row whose own column is its maximum."""
    g = torch.Generator().manual_seed(7919 * seed + H)
    gp = [0]
    for n in sizes:
        gp.append(gp[-1] + n)
    N = gp[-1]
    s, t = _rows(N, H, g, 1.0), _rows(N, H, g, 1.0)
    info = {'ties': [], 'edge_row': None, 'self_row': None}
    if plant:
        big = float(t.abs().max()) * math.sqrt(H)             # above every row's norm
        # ties: the largest graph, three equal rows on both sides of a multiple of 64
        gi = max(range(len(sizes)), key=lambda i: sizes[i])
        lo, hi = gp[gi], gp[gi + 1]
        b = (lo // TILE + 1) * TILE
        while not (lo + 2 <= b - 2 and b + 5 < hi):
            b += TILE
        d = torch.randn(H, generator=g, dtype=F64)
        trio = [b - 2, b + 1, b + 5]
        for v in trio:
            t[v] = (4 * big * d / d.norm()).to(F32)
        info['ties'] = trio
        # self: a row of the last graph whose own column is its maximum
        us = gp[-2] + sizes[-1] // 3
        while us in trio:
            us += 1
        ds_ = s[us].to(F64) / s[us].to(F64).norm()
        t[us] = (50 * big * ds_).to(F32)
        info['self_row'] = us
        # a small graph that has a successor: first, last, one past.  The row is made orthogonal to the self row, so that neither
        # planted direction scores with the other's row
        cand = [i for i in range(len(sizes) - 1) if 3 <= sizes[i] <= 8 and sizes[i + 1] >= 1]
        if cand:
            i = cand[0]
            u = gp[i] + 1
            su = s[u].to(F64)
            s[u] = (su - (su @ ds_) * ds_).to(F32)
            v = s[u].to(F64) / s[u].to(F64).norm()
            v = v - (v @ ds_) * ds_
            t[gp[i + 1]] = (30 * big * v).to(F32)
            t[gp[i + 1] - 1] = (20 * big * v).to(F32)
            t[gp[i]] = (10 * big * v).to(F32)
            info['edge_row'] = (u, gp[i], gp[i + 1] - 1, gp[i + 1])
    return {'s': s, 't': t, 'graph_ptr': gp, 'N': N, 'H': H, 'info': info}


def edges_case(c, per_node, seed):
    """A directed edge list inside the graphs of a topk_case: `per_node` random successors per node (self loops and repeats allowed)."""
    g = torch.Generator().manual_seed(31 * seed + 5)
    gp = c['graph_ptr']
    src, dst = [], []
    for i in range(len(gp) - 1):
        n = gp[i + 1] - gp[i]
        if n == 0:
            continue
        u = torch.arange(gp[i], gp[i + 1]).repeat_interleave(per_node)
        v = gp[i] + torch.randint(0, n, (u.numel(),), generator=g)
        src.append(u)
        dst.append(v)
    return torch.stack([torch.cat(src), torch.cat(dst)])
