"""Ranking and accuracy: the exact rank of every true link among all candidates (MRR / Hits@K), the ROC-AUC / average-precision
record, and the exact functional ordering accuracy over all truth-table pair comparisons.  Added functionality beside the train
step: it depends on _hip, pairs and similarity only (ops re-binds the public names).
"""
from collections import namedtuple

import torch

from . import _hip
from ._hip import F32, I32, HipLibraryError, check, edge_rows, ptr
from .pairs import _graph_of, _graph_ptr64, _pair_graphs, _pair_operands, _pair_width, _same_rows, pair_scores_at
from .similarity import sim_at


# ------------------------------------------------------------------------------------------------
# the rank of every true link among all candidates of its node (added functionality: exact MRR / Hits@K; mgv_pair_rank_counts)
# ------------------------------------------------------------------------------------------------
LinkRanks = namedtuple('LinkRanks', 'rank_lo rank_hi valid')
RankLists = namedtuple('RankLists', 'thr_ptr thr perm valid row')
RankMetrics = namedtuple('RankMetrics', 'ranked hits_lo hits_hi sum_lo sum_hi mrr')


def pair_rank_counts(s, t, thr_ptr, thr, graph_ptr=None, skip_self=False):
    """(n_gt, n_eq) int32 [T], the entry mgv_pair_rank_counts as it is: for row u and every j in [thr_ptr[u], thr_ptr[u + 1]) the
    candidates v of u — pair_select's: v in u's graph, without v = u when skip_self, a NaN score never — whose RAW score <s_u, t_v> is
    > thr[j] and == thr[j].  thr_ptr [N + 1] (int32 on the device, starting at 0), thr [T] float32; EACH ROW'S LIST MUST ASCEND, NaNs
    last (what torch.sort gives; link_ranks sorts).  One all-pairs walk per 32 entries of a tile's longest list; integer counters,
    plain stores, no global atomics: the same bytes from call to call.  A NaN threshold gets (0, 0).  No grad."""
    if s.dim() == 2 and t.dim() == 2 and s.shape[1] == t.shape[1]:
        _pair_width(s, 'pair_rank_counts')
    with torch.no_grad():
        sd, lds, td, ldt, H = _pair_operands(s, t)
        N = _same_rows(sd, td, 'pair_rank_counts ranks inside one batch')
        dev = sd.device
        gp, G = _pair_graphs(graph_ptr, dev)
        tp = torch.as_tensor(thr_ptr).to(device=dev, dtype=I32).contiguous()
        if tp.numel() != N + 1:
            raise HipLibraryError('thr_ptr needs N + 1 = %d entries (got %d)' % (N + 1, tp.numel()))
        th = torch.as_tensor(thr).detach().to(device=dev, dtype=F32).contiguous().flatten()
        n_gt = torch.empty(th.numel(), dtype=I32, device=dev)
        n_eq = torch.empty(th.numel(), dtype=I32, device=dev)
        _hip.call('mgv_pair_rank_counts', H, N, ptr(sd), lds, ptr(td), ldt, ptr(gp), G, int(bool(skip_self)), ptr(tp), ptr(th), ptr(n_gt),
                  ptr(n_eq))
        return n_gt, n_eq


def _rank_by(by, name):
    if by not in ('src', 'dst'):
        raise ValueError("%s: by must be 'src' (a link among its source's targets) or 'dst' (among its target's sources), got %r" % (name, by))


def _rank_rows(edge_index, N, by):
    """(row, col) int64 [E] of a link under `by`; an id outside [0, N) raises ValueError (one read-back)."""
    ei = edge_index.long()
    if ei.dim() != 2 or ei.shape[0] != 2:
        raise ValueError('edge_index must be [2, E] (got shape %s)' % (tuple(edge_index.shape),))
    if ei.shape[1] > 0 and (int(ei.min()) < 0 or int(ei.max()) >= N):
        raise ValueError('edge_index holds node ids outside [0, %d)' % N)
    return (ei[0].contiguous(), ei[1].contiguous()) if by == 'src' else (ei[1].contiguous(), ei[0].contiguous())


def _f32_order_key(x):
    """int64 in [0, 2^32): ascending with the float32 value, every NaN (made one NaN first) behind +inf."""
    x = torch.where(torch.isnan(x), torch.full_like(x, float('nan')), x)
    b = x.contiguous().view(I32).to(torch.int64) & 0xffffffff
    return torch.where(b >= 0x80000000, 0xffffffff - b, b + 0x80000000)


def _run_ends(start):
    """(first, last) index of the run each position belongs to; start[i]: a run begins at i (start[0] is True)."""
    E = start.numel()
    idx = torch.arange(E, device=start.device)
    first = torch.cummax(torch.where(start, idx, torch.zeros_like(idx)), 0).values
    end = torch.ones_like(start)
    end[:-1] = start[1:]
    last = torch.cummin(torch.where(end, idx, torch.full_like(idx, E - 1)).flip(0), 0).values.flip(0)
    return first, last


def link_rank_lists(edge_index, score, N, graph_ptr=None, by='src', skip_self=False, row_ptr=None):
    """The per-row threshold lists mgv_pair_rank_counts takes, from the links' own raw scores (float32 [E], pair_scores_at): plain torch,
    on whatever device the arguments live.  RankLists(thr_ptr int32 [N + 1], thr float32 [E], perm int64 [E], valid bool [E], row int64
    [E]), the last four in LIST order: rows ascending, inside a row the scores ascending; perm[i] is the caller's index of entry i.
    A link is invalid — NaN in thr, behind the row's valid ones, and in no rank, filter or metric — when its other end lies outside
    its row's graph, when its score is NaN, and under skip_self when it is a self loop.  ONE sort, by the key (row, score); row_ptr
    (int [N + 1], a GraphPlan's out_ptr for by='src' / in_ptr for by='dst' when edge_index is the plan's) saves counting the rows.
    The same sort finds a duplicated pair (ValueError): its two copies share row and score bits, so only entries with an equal
    neighbour are looked at by column.  An id outside [0, N): ValueError."""
    _rank_by(by, 'link_rank_lists')
    row, col = _rank_rows(edge_index, N, by)
    dev = row.device
    E = row.numel()
    score = score.detach().to(F32)
    if graph_ptr is None:
        ok = torch.ones(E, dtype=torch.bool, device=dev)
    else:
        gp = _graph_ptr64(graph_ptr, dev).contiguous()
        if gp.numel() < 2:
            ok = torch.zeros(E, dtype=torch.bool, device=dev)
        else:
            ok = torch.bucketize(row, gp[1:].contiguous(), right=True) == torch.bucketize(col, gp[1:].contiguous(), right=True)
    ok = ok & ~torch.isnan(score)
    if skip_self:
        ok = ok & (row != col)
    thr = torch.where(ok, score, torch.full_like(score, float('nan')))
    key, perm = torch.sort(row * (1 << 32) + _f32_order_key(thr), stable=True)
    row_s, col_s, thr_s, ok_s = row[perm], col[perm], thr[perm], ok[perm]
    if E > 1:
        same = key[1:] == key[:-1]
        near = torch.zeros(E, dtype=torch.bool, device=dev)
        near[1:] |= same
        near[:-1] |= same
        pair = torch.sort(row_s[near] * N + col_s[near]).values
        if pair.numel() > 1 and bool((pair[1:] == pair[:-1]).any()):
            raise ValueError('edge_index lists a pair twice: a rank among all candidates is defined for distinct links')
    if row_ptr is None:
        thr_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        thr_ptr[1:] = torch.cumsum(torch.bincount(row, minlength=N), 0)
        thr_ptr = thr_ptr.to(I32)
    else:
        thr_ptr = torch.as_tensor(row_ptr).to(device=dev, dtype=I32).contiguous()
        if thr_ptr.numel() != N + 1:
            raise ValueError('row_ptr needs N + 1 = %d entries (got %d)' % (N + 1, thr_ptr.numel()))
    return RankLists(thr_ptr, thr_s, perm, ok_s, row_s)


def link_rank_filter(lists, n_gt, n_eq, filtered=True):
    """LinkRanks(rank_lo, rank_hi int64 [E], valid bool [E]) in the CALLER's edge order from the counts of mgv_pair_rank_counts over
    link_rank_lists: rank_lo = 1 + n_gt', rank_hi = n_gt' + n_eq'.  filtered: the other true links of the row do not count against a
    link — n_gt' = n_gt - #{other valid listed links of the row with a higher score}, n_eq' = n_eq - #{others with an equal score},
    read off the row's own ascending list (positions and runs of equal values: integers, no second walk).  An invalid link has
    (0, 0, False).  Plain torch on any device."""
    thr_ptr, thr, perm, ok, row = lists
    E = thr.numel()
    gt, eq = n_gt.to(torch.int64), n_eq.to(torch.int64)
    if filtered and E > 0:
        start = torch.ones(E, dtype=torch.bool, device=thr.device)
        start[1:] = (row[1:] != row[:-1]) | (thr[1:] != thr[:-1])          # float equality, the kernel's `==` (-0 == 0); NaN: never
        first, last = _run_ends(start)
        nvalid = torch.zeros(thr_ptr.numel() - 1, dtype=torch.int64, device=thr.device).index_add_(0, row, ok.to(torch.int64))
        vend = thr_ptr[:-1].to(torch.int64) + nvalid                       # the valid links of a row stand first in its list
        gt = gt - (vend[row] - (last + 1))
        eq = eq - (last - first)
    lo = torch.where(ok, 1 + gt, torch.zeros_like(gt))
    hi = torch.where(ok, gt + eq, torch.zeros_like(gt))
    rank_lo, rank_hi = torch.empty_like(lo), torch.empty_like(hi)
    valid = torch.empty_like(ok)
    rank_lo[perm], rank_hi[perm], valid[perm] = lo, hi, ok
    return LinkRanks(rank_lo, rank_hi, valid)


def link_ranks(s, t, edge_index, graph_ptr=None, by='src', skip_self=False, filtered=True, plan=None):
    """LinkRanks(rank_lo, rank_hi int64 [E], valid bool [E]) in the caller's edge order: where every listed link (u, v) stands among ALL
    candidates of its node by raw score <s_u, t_v> — by='src' among the nodes u could point to (its own graph, without u itself when
    skip_self), by='dst' among the nodes that could feed v (the operands change places as in pair_select).  rank_lo = 1 + #{candidates
    scored higher}, rank_hi = #{higher} + #{equal}: the best and the worst place its ties allow (a link counts among its own equals,
    so rank_lo <= rank_hi).  filtered (the default): the row's other true links do not count against a link.
    The thresholds are pair_scores_at(sigmoid=False), the bits the walk computes: a valid link always finds itself.  Lists by
    link_rank_lists (one sort; with `plan` — the batch's GraphPlan, when edge_index is the plan's own edge list — its CSR pointers are
    the rows' ranges), counts by mgv_pair_rank_counts, the filter by link_rank_filter.  Invalid links (other end outside the row's
    graph, NaN score, a self loop under skip_self): valid False, ranks 0.  An id outside [0, N) or a duplicated pair: ValueError.
    E = 0 launches nothing.  No grad."""
    _rank_by(by, 'link_ranks')
    with torch.no_grad():
        N = s.shape[0]
        dev = s.device
        edge_index = edge_index.to(dev)
        _rank_rows(edge_index, N, by)                                      # ids before anything dereferences them
        if edge_index.shape[1] == 0:
            z = torch.zeros(0, dtype=torch.int64, device=dev)
            return LinkRanks(z, z.clone(), torch.zeros(0, dtype=torch.bool, device=dev))
        score = pair_scores_at(s, t, edge_index, sigmoid=False)
        row_ptr = None
        if plan is not None and plan.N == N and plan.E == edge_index.shape[1]:
            row_ptr = plan.out_ptr if by == 'src' else plan.in_ptr
        lists = link_rank_lists(edge_index, score, N, graph_ptr=graph_ptr, by=by, skip_self=skip_self, row_ptr=row_ptr)
        if by == 'dst':
            s, t = t, s
        n_gt, n_eq = pair_rank_counts(s, t, lists.thr_ptr, lists.thr, graph_ptr=graph_ptr, skip_self=skip_self)
        return link_rank_filter(lists, n_gt, n_eq, filtered)


def rank_metrics(ranks, edge_index, graph_ptr, ks=(1, 3, 10, 50), by='src'):
    """RankMetrics per graph of the batch, on the ranks' device: ranked int64 [G] (valid links), hits_lo / hits_hi int64 [G, len(ks)]
    (links with rank_lo <= K / rank_hi <= K), sum_lo / sum_hi int64 [G] (mean rank = sum / ranked) and mrr float64 [G], the mean of
    (1 / rank_lo + 1 / rank_hi) / 2.  A link counts for the graph of its row (its source; its target for by='dst').  Integer sums
    are exact in any order; mrr is summed in ONE fixed order — the links grouped by graph (stable sort), a float64 cumulative sum,
    differences at the graphs' ends — so it is the same bits from run to run.  A graph without a ranked link: mrr NaN, zeros
    elsewhere."""
    _rank_by(by, 'rank_metrics')
    with torch.no_grad():
        lo, hi, valid = ranks
        dev = lo.device
        gp = _graph_ptr64(graph_ptr, dev)
        G = max(gp.numel() - 1, 0)
        K = len(ks)
        i64 = dict(dtype=torch.int64, device=dev)
        if G == 0:
            return RankMetrics(torch.zeros(0, **i64), torch.zeros((0, K), **i64), torch.zeros((0, K), **i64), torch.zeros(0, **i64),
                               torch.zeros(0, **i64), torch.zeros(0, dtype=torch.float64, device=dev))
        row = edge_index.long().to(dev)[0 if by == 'src' else 1]
        gid = _graph_of(row, gp, G)
        v = valid.to(torch.int64)
        kk = torch.tensor([int(k) for k in ks], **i64)
        ranked = torch.zeros(G, **i64).index_add_(0, gid, v)
        hits_lo = torch.zeros((G, K), **i64).index_add_(0, gid, ((lo[:, None] <= kk[None, :]) & valid[:, None]).to(torch.int64))
        hits_hi = torch.zeros((G, K), **i64).index_add_(0, gid, ((hi[:, None] <= kk[None, :]) & valid[:, None]).to(torch.int64))
        sum_lo = torch.zeros(G, **i64).index_add_(0, gid, lo * v)
        sum_hi = torch.zeros(G, **i64).index_add_(0, gid, hi * v)
        one = torch.ones_like(lo)
        term = torch.where(valid, (1.0 / torch.where(valid, lo, one).double() + 1.0 / torch.where(valid, hi, one).double()) / 2,
                           torch.zeros(lo.shape, dtype=torch.float64, device=dev))
        order = torch.sort(gid, stable=True).indices
        cs = torch.zeros(lo.numel() + 1, dtype=torch.float64, device=dev)
        cs[1:] = torch.cumsum(term[order], 0)
        ends = torch.zeros(G + 1, **i64)
        ends[1:] = torch.cumsum(torch.bincount(gid, minlength=G), 0)
        mrr = (cs[ends[1:]] - cs[ends[:-1]]) / ranked.double()             # 0 / 0: NaN for a graph without a ranked link
        return RankMetrics(ranked, hits_lo, hits_hi, sum_lo, sum_hi, mrr)


# ------------------------------------------------------------------------------------------------
# link-prediction ranking metrics (digvae_model.py:177-189: decode, copy to the host, sklearn)
# ------------------------------------------------------------------------------------------------
LINK_RECORD_WORDS = 8       # AUC, AP (float64) | U2, P, Q, tie groups, NaN scores (int64) | spare


def link_record(st_or_s, t=None, pos_edge_index=None, neg_edge_index=None, return_scores=False):
    """One ranking of P positive against Q negative pairs, entirely on the device and without a host synchronisation
    (csrc/link_metrics.hip: score keys -> radix sort -> two streaming passes).  Returns the 64-byte record the kernels wrote, a
    float64[8] tensor: words 0-1 AUC and AP, words 2-6 (read through `.view(torch.int64)`) U2, P, Q, the number of tie groups and
    the number of NaN scores (non-zero: the metrics mean nothing), word 7 unused; with `return_scores` also the fp32 scores that
    were ranked, positives first.  `st_or_s`: the [N, 2H] `st` layout of recon_loss (t=None) or s [N, H] with t [N, H].
    `neg_edge_index`: a [2, Q] tensor or a sampling.NegativeEdges.  No autograd: the metrics are piecewise constant."""
    neg = getattr(neg_edge_index, 'edge_index', neg_edge_index)
    P, Q = int(pos_edge_index.shape[1]), int(neg.shape[1])
    if P == 0 or Q == 0:
        # sklearn's behaviour for y_true with one class; both sizes are host values: nothing is launched
        raise ValueError('Only one class present (%d positive, %d negative pairs): ROC-AUC and average precision are not defined' % (P, Q))
    sd = check(st_or_s.detach().contiguous(), F32, 'st' if t is None else 's')
    if t is None:
        ld = sd.shape[1]
        H = ld // 2
        td = sd[:, H:]
    else:
        td = check(t.detach().contiguous(), F32, 't')
        ld = H = sd.shape[1]
        if td.shape != sd.shape:
            raise HipLibraryError('s and t must have the same shape (got %s and %s)' % (tuple(sd.shape), tuple(td.shape)))
    n = P + Q
    if n >= 1 << 31:
        raise HipLibraryError('mgv_link_keys failed: %s (%d pairs; the ranking holds fewer than 2^31)' % (_hip._ERR[-2], n))
    ps, pd = edge_rows(pos_edge_index)
    ns, nd = edge_rows(neg)
    for name, e in (('pos_edge_index', ps), ('neg_edge_index', ns)):
        if not e.is_cuda:
            raise HipLibraryError('%s must live on the GPU (got %s)' % (name, e.device))
    dev = sd.device
    rec = torch.zeros(LINK_RECORD_WORDS, dtype=torch.float64, device=dev)
    status = rec.view(I32)[12:13]                      # low half of int64 word 6
    buf = torch.empty(3, n + (-n) % 4, dtype=I32, device=dev)      # keys, sorted keys, permutation: each on a 16-byte boundary
    keys, skey, order = buf[0, :n], buf[1, :n], buf[2, :n]
    scores = torch.empty(n, dtype=F32, device=dev) if return_scores else None
    _hip.call('mgv_link_keys', H, ptr(sd), ptr(td), ld, ptr(ps), ptr(pd), P, ptr(ns), ptr(nd), Q, ptr(keys), ptr(scores), ptr(status))
    t_i = _hip.call_value('mgv_sort_pairs_temp_ints', 4, n)
    w_i = _hip.call_value('mgv_link_rank_work_ints', n)
    if t_i < 0 or w_i < 0:
        raise HipLibraryError('link metrics: no workspace size for %d pairs' % n)
    temp = torch.empty(t_i + w_i + 2, dtype=I32, device=dev)
    _hip.call('mgv_sort_pairs', 4, n, ptr(keys), ptr(skey), ptr(order), 32, ptr(temp), t_i)
    work = temp[t_i + (t_i & 1):]                      # 8-byte aligned
    _hip.call('mgv_link_rank', n, P, ptr(skey), ptr(order), ptr(rec), ptr(work), work.numel())
    return (rec, scores) if return_scores else rec


def link_auc_ap(st_or_s, t=None, pos_edge_index=None, neg_edge_index=None, return_scores=False):
    """(metrics, status[, scores, counts]): `metrics` float64[2] = (AUC, AP) and `status` int64[1] = the number of NaN scores, both
    on the device and both views of one link_record (no host synchronisation; a non-zero status means a NaN was ranked and the
    metrics are void).  `return_scores`: also the ranked fp32 scores (positives first) and counts int64[4] = U2, P, Q, tie groups."""
    out = link_record(st_or_s, t, pos_edge_index, neg_edge_index, return_scores)
    rec = out[0] if return_scores else out
    words = rec.view(torch.int64)
    if return_scores:
        return rec[:2], words[6:7], out[1], words[2:6]
    return rec[:2], words[6:7]


def read_link_records(records):
    """[(auc, ap), ...] of link_record tensors as Python floats: ONE host read for all of them; ValueError if any ranked a NaN
    (sklearn: "Input contains NaN")."""
    if not records:
        return []
    host = torch.stack(list(records)).cpu()
    bad = host.view(torch.int64)[:, 6]
    if bool((bad != 0).any()):
        raise ValueError('Input contains NaN: %d of the ranked scores are NaN' % int(bad.sum()))
    return [(float(r[0]), float(r[1])) for r in host]


# ------------------------------------------------------------------------------------------------
# exact functional ordering accuracy (added functionality: every comparison of get_function_acc, utils/utils.py:111-147, counted;
# mgv_concord_counts)
# ------------------------------------------------------------------------------------------------
CONCORD_TILE = 256              # csrc/concordance.hip kConcordTile: rows of a workgroup and columns of an LDS tile
CONCORD_MAX_GAPS = 8
MIN_GAP = 0.05                  # utils/utils.py:112


def segment_table(first, graph_ptr, second=None):
    """(seg_ptr int64 [G + 1], ok bool scalar) in plain torch, on the device of `first`: segment g of the listed pairs are those whose
    first node lies in graph g, found by searchsorted — which is the pairs of graph g exactly when they come grouped by circuit in
    circuit order and neither node leaves the circuit; `ok` says so."""
    gp = _graph_ptr64(graph_ptr, first.device).contiguous()
    G = gp.numel() - 1
    if G < 1:
        return torch.zeros(1, dtype=torch.int64, device=first.device), torch.as_tensor(first.numel() == 0, device=first.device)
    gid = torch.searchsorted(gp[1:].contiguous(), first, right=True)           # the graph of each pair's first node
    ok = ((first >= gp[0]) & (first < gp[-1])).all()
    if first.numel() > 1:
        ok = ok & (gid[1:] >= gid[:-1]).all()
    if second is not None:
        ok = ok & (torch.searchsorted(gp[1:].contiguous(), second, right=True) == gid).all() & (second >= gp[0]).all()
    seg = torch.searchsorted(gid, torch.arange(G + 1, dtype=torch.int64, device=first.device), right=False)
    return seg, ok


def pair_segments(tt_pair_index, graph_ptr, cache=None):
    """int32 seg_ptr [G + 1] on the device: the listed pairs of circuit g are [seg_ptr[g], seg_ptr[g + 1]).  The pairs must come grouped
    by circuit in circuit order (synthetic.collate and the parser deliver them so) with both nodes of a pair in one circuit, else
    ValueError: one small host read when the table is built, which is kept on `cache` (the batch) like pair_lists."""
    pa, pb = edge_rows(tt_pair_index)
    gp = torch.as_tensor(graph_ptr)
    key = (pa.numel(), gp.numel(), pa.device)
    if cache is not None:
        kept = getattr(cache, '_mgv_pair_segments', None)
        if kept is not None and kept[0] == key:
            return kept[1]
    with torch.no_grad():
        seg, ok = segment_table(pa, gp, pb)
        if not bool(ok):
            raise ValueError('tt_pair_index must list its pairs grouped by circuit, in circuit order, both nodes of a pair in one circuit')
        seg = seg.to(I32)
    if cache is not None:
        cache._mgv_pair_segments = (key, seg)
    return seg


def _concord_gaps(gaps):
    """The gaps as the entry takes them: a ctypes float array on the host, converted to float32 ONCE; NaN or negative: ValueError."""
    g = torch.as_tensor(gaps, dtype=torch.float64).flatten().to(F32)
    if not 1 <= g.numel() <= CONCORD_MAX_GAPS:
        raise ValueError('1 to %d gaps (got %d)' % (CONCORD_MAX_GAPS, g.numel()))
    vals = g.tolist()
    if any(not v >= 0.0 for v in vals):
        raise ValueError('a gap must be >= 0 and not NaN (got %r)' % (vals,))
    return (_hip.ctypes.c_float * len(vals))(*vals)


def concord_counts(gt, pred, seg_ptr=None, gaps=(MIN_GAP,)):
    """int64 [G, B, 3] on the device (G = 1 without seg_ptr): {eligible, concordant, tied} over EVERY unordered comparison {p, q} of one
    segment of the listed pairs (mgv_concord_counts).  dd = gt[q] - gt[p], de = pred[q] - pred[p] in float32; eligible at gap j:
    dd != 0 and |dd| >= gaps[j]; concordant: dd and de both > 0 or both < 0; tied: de == 0.  A NaN in gt: not eligible; a NaN in pred:
    eligible, neither concordant nor tied.  Integer atomics: exact, the same bytes from call to call; no host read.  No grad."""
    with torch.no_grad():
        g = check(torch.as_tensor(gt).detach().to(F32).contiguous().flatten(), F32, 'gt')
        p = check(torch.as_tensor(pred).detach().to(device=g.device, dtype=F32).contiguous().flatten(), F32, 'pred')
        if p.numel() != g.numel():
            raise HipLibraryError('gt and pred list the same pairs (got %d and %d)' % (g.numel(), p.numel()))
        hg = _concord_gaps(gaps)
        B = len(hg)
        sp, G = None, 0
        if seg_ptr is not None:
            sp = torch.as_tensor(seg_ptr).to(device=g.device, dtype=I32).contiguous()
            G = sp.numel() - 1
            if G < 0:
                raise HipLibraryError('seg_ptr needs at least one entry')
        out = torch.empty((max(G, 1), B, 3), dtype=torch.int64, device=g.device)
        _hip.call('mgv_concord_counts', g.numel(), ptr(g), ptr(p), ptr(sp), G, hg, B, ptr(out))
        return out if sp is None else out[:G]


def function_accuracy(hf, tt_pair_index, tt_sim, graph_ptr=None, gaps=(MIN_GAP,), cache=None):
    """(acc float64 [G, B], counts int64 [G, B, 3]) on the device: per circuit and gap, concordant / eligible over ALL comparisons of two
    listed truth-table pairs whose distances differ by at least the gap — the quantity get_function_acc (utils/utils.py:111-147)
    estimates from 100 draws — with pred = 1 - sim_at(hf, tt_pair_index) in float32, the bits Model.functional_similarity reports and
    the reference's expression.  acc is -1 where nothing is eligible, the reference's return value for that case.  Without graph_ptr:
    one circuit.  No grad, no host read once the batch's segment table exists (pair_segments, kept on `cache`)."""
    with torch.no_grad():
        pred = 1.0 - sim_at(hf.detach(), tt_pair_index)
        seg = None if graph_ptr is None else pair_segments(tt_pair_index, graph_ptr, cache)
        counts = concord_counts(tt_sim.detach().to(device=pred.device), pred, seg, gaps)
        el, co = counts[..., 0], counts[..., 1]
        acc = torch.where(el > 0, co.double() / el.clamp(min=1).double(), torch.full_like(el, -1, dtype=torch.float64))
        return acc, counts


# ------------------------------------------------------------------------------------------------
# exact gate recovery of a decoded circuit (added functionality: mgv_fanin_recovery against pairs.fanin_decode's lists)
# ------------------------------------------------------------------------------------------------
FaninRecovery = namedtuple('FaninRecovery', 'counts n_hit recovery precision recall')
FANIN_RECORD = ('gates', 'exact', 'hits', 'true_total', 'decoded_total')


def true_fanin_lists(edge_index, N):
    """(tru_ptr int64 [N + 1], tru_src int32 [T]) on edge_index's device: every node's true fan-ins, strictly ascending and without
    repeats — one sort of dst * N + src, unique_consecutive, a bincount and a scan."""
    src, dst = edge_rows(edge_index)
    if src.numel() > 0 and (int(torch.min(torch.minimum(src, dst))) < 0 or int(torch.max(torch.maximum(src, dst))) >= N):
        raise ValueError('edge_index holds node ids outside [0, %d)' % N)
    code = torch.unique_consecutive(torch.sort(dst * N + src).values)
    tru_ptr = torch.zeros(N + 1, dtype=torch.int64, device=src.device)
    if N > 0:
        torch.cumsum(torch.bincount(torch.div(code, N, rounding_mode='floor'), minlength=N), 0, out=tru_ptr[1:])
    return tru_ptr, (code % max(N, 1)).to(I32).contiguous()


def fanin_recovery(idx, edge_index, graph_ptr=None):
    """FaninRecovery(counts int64 [G, 5], n_hit int32 [N], recovery, precision, recall float64 [G]) on the device (G = 1 without
    graph_ptr): decoded fan-in lists idx [N, K] (pairs.fanin_decode; -1: no entry) against the true fan-in sets of `edge_index`
    (repeated edges count once).  counts per graph over the gates — the nodes with at least one true fan-in —: FANIN_RECORD =
    {gates, exact, hits, true_total, decoded_total}, exact: the decoded SET equals the true set.  recovery = exact / gates,
    precision = hits / decoded_total, recall = hits / true_total, -1 where the divisor is 0.  n_hit: decoded fan-ins of each node that
    are true.  Integer atomics: the same bytes from call to call.  One read-back (the range of edge_index).  No grad."""
    with torch.no_grad():
        idx = check(idx.detach().contiguous(), I32, 'idx')
        if idx.dim() != 2 or not 1 <= idx.shape[1] <= 32:
            raise HipLibraryError('idx must be [N, K] with 1 <= K <= 32 (got shape %s)' % (tuple(idx.shape),))
        N, K = idx.shape
        dev = idx.device
        tru_ptr, tru_src = true_fanin_lists(edge_index.to(dev), N)
        gp, G = _pair_graphs(graph_ptr, dev)
        rec = torch.empty((max(G, 1), len(FANIN_RECORD)), dtype=torch.int64, device=dev)
        n_hit = torch.empty(N, dtype=I32, device=dev)
        _hip.call('mgv_fanin_recovery', N, K, ptr(idx), ptr(tru_ptr), ptr(tru_src), ptr(gp), G, ptr(n_hit), ptr(rec))
        rec = rec if gp is None else rec[:G]

        def ratio(a, b):
            return torch.where(b > 0, a.double() / b.clamp(min=1).double(), torch.full_like(b, -1, dtype=torch.float64))
        return FaninRecovery(rec, n_hit, ratio(rec[:, 1], rec[:, 0]), ratio(rec[:, 2], rec[:, 4]), ratio(rec[:, 2], rec[:, 3]))
