"""Restatement of csrc/concordance.hip (mgv_concord_counts; reference: get_function_acc, utils/utils.py:111-147, on the `dis` of
trainer.py:158-160) from its definition: plain Python loops over the float32 values, and a vectorised numpy form that must equal
them.  CPU only; pinned by tests/test_concord_spec.py.

For every unordered pair {p, q}, p < q, of one segment, with dd = gt[q] - gt[p] and de = pred[q] - pred[p] in float32:
    eligible at gap j   dd != 0 and |dd| >= gaps[j]
    concordant          (dd > 0 and de > 0) or (dd < 0 and de < 0)
    tied                de == 0
out[g][j] = (eligible, eligible and concordant, eligible and tied).  Everything compared is an integer.

`defect` plants ONE deviation from the definition (tests show that each changes a count on a designed case):
    'gt_for_ge'   > for >= at the gap                      'no_nonzero'  the dd != 0 test dropped
    'tie_correct' a prediction tie counted as concordant   'diagonal'    p == q included
    'both'        both triangles counted                   'cross'       comparisons across a segment boundary
    'last_row'    the last row of a tile of `tile` rows lost      'last_col'    the last column tile of a row tile's walk lost
'diagonal' alone changes nothing, whatever the input: on the diagonal dd = gt[p] - gt[p] is 0, or NaN for a NaN or infinite gt[p], and
neither is eligible.  It shows only once the dd != 0 test is gone as well ('diagonal+no_nonzero', at gap 0).
"""
import numpy as np

TILE = 256                                                # csrc/concordance.hip kConcordTile = ops.CONCORD_TILE
MIN_GAP = 0.05
F32 = np.float32


def f32_gaps(gaps):
    g = np.asarray(gaps, dtype=np.float64).astype(F32).reshape(-1)
    assert 1 <= g.size <= 8 and not np.isnan(g).any() and (g >= 0).all()
    return g


def clamped_segments(P, seg_ptr):
    """[(lo, hi), ...] per output row: seg_ptr None is one segment of all P; whatever the table holds, a range is clamped into [0, P)."""
    if seg_ptr is None:
        return [(0, int(P))]
    sp = [int(v) for v in np.asarray(seg_ptr).reshape(-1)]
    out = []
    for g in range(len(sp) - 1):
        lo = min(max(sp[g], 0), int(P))
        hi = min(max(sp[g + 1], lo), int(P))
        out.append((lo, hi))
    return out


def counts_loops(gt, pred, seg_ptr=None, gaps=(MIN_GAP,), defect=None, tile=TILE):
    """int64 [max(G, 1), B, 3] by plain loops."""
    gt, pred = np.asarray(gt, dtype=F32).reshape(-1), np.asarray(pred, dtype=F32).reshape(-1)
    P, g32 = gt.size, f32_gaps(gaps)
    segs = clamped_segments(P, seg_ptr)
    out = np.zeros((max(len(segs), 1), g32.size, 3), dtype=np.int64)
    no_nonzero = defect in ('no_nonzero', 'diagonal+no_nonzero')
    defect = 'diagonal' if defect == 'diagonal+no_nonzero' else defect
    for g, (lo, hi) in enumerate(segs):
        for p in range(lo, hi):
            if defect == 'last_row' and p % tile == tile - 1:
                continue
            q_lo = lo if defect == 'both' else (p if defect == 'diagonal' else p + 1)
            q_hi = P if defect == 'cross' else hi
            if defect == 'last_col':                            # the walk of p's row tile stops one column tile early
                last_tile = (q_hi - 1) // tile if q_hi > 0 else 0
                if last_tile > p // tile:
                    q_hi = min(q_hi, last_tile * tile)
            for q in range(q_lo, q_hi):
                if defect == 'both' and q == p:
                    continue
                dd = F32(gt[q] - gt[p])
                de = F32(pred[q] - pred[p])
                for j in range(g32.size):
                    if not no_nonzero and not dd != 0:
                        continue
                    big = abs(dd) > g32[j] if defect == 'gt_for_ge' else abs(dd) >= g32[j]
                    if not big:
                        continue
                    conc = (dd > 0 and de > 0) or (dd < 0 and de < 0)
                    tied = bool(de == 0)
                    if defect == 'tie_correct' and tied:
                        conc = True
                    out[g, j, 0] += 1
                    out[g, j, 1] += int(conc)
                    out[g, j, 2] += int(tied)
    return out


def counts_numpy(gt, pred, seg_ptr=None, gaps=(MIN_GAP,)):
    """The same counts, one segment's upper triangle at a time as float32 difference matrices."""
    gt, pred = np.asarray(gt, dtype=F32).reshape(-1), np.asarray(pred, dtype=F32).reshape(-1)
    P, g32 = gt.size, f32_gaps(gaps)
    segs = clamped_segments(P, seg_ptr)
    out = np.zeros((max(len(segs), 1), g32.size, 3), dtype=np.int64)
    with np.errstate(invalid='ignore'):
        for g, (lo, hi) in enumerate(segs):
            a, b = gt[lo:hi], pred[lo:hi]
            dd = (a[None, :] - a[:, None]).astype(F32)          # [p, q] = gt[q] - gt[p]
            de = (b[None, :] - b[:, None]).astype(F32)
            upper = np.triu(np.ones(dd.shape, dtype=bool), 1)
            conc = ((dd > 0) & (de > 0)) | ((dd < 0) & (de < 0))
            tied = de == 0
            for j in range(g32.size):
                el = upper & (dd != 0) & (np.abs(dd) >= g32[j])
                out[g, j] = (el.sum(), (el & conc).sum(), (el & tied).sum())
    return out


def accuracy(counts):
    """float64 [G, B]: concordant / eligible, -1 where nothing is eligible (get_function_acc's return value for that case)."""
    c = np.asarray(counts, dtype=np.int64)
    el, co = c[..., 0], c[..., 1]
    return np.where(el > 0, co / np.maximum(el, 1), -1.0)


def closed_form(P, k):
    """eligible = concordant for gt[p] = p 2^-17, pred = gt, gap = k 2^-17 (k >= 1): the pairs with q - p >= k."""
    return (P - k) * (P - k + 1) // 2 if P >= k else 0


def ladder(P):
    """gt[p] = p 2^-17: every difference is exact in float32 for P < 2^24."""
    return (np.arange(P, dtype=np.float64) * 2.0 ** -17).astype(F32)


def segments_numpy(first, second, graph_ptr):
    """(seg_ptr int64 [G + 1], ok): ops.segment_table's twin.  Segment g holds the pairs whose first node lies in graph g; ok iff the pairs
    come grouped by circuit in circuit order and both nodes of every pair lie in one circuit."""
    first, second, gp = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (first, second, graph_ptr))
    G = gp.size - 1
    if G < 1:
        return np.zeros(1, dtype=np.int64), first.size == 0
    gid = np.searchsorted(gp[1:], first, side='right')
    gid2 = np.searchsorted(gp[1:], second, side='right')
    ok = bool(((first >= gp[0]) & (first < gp[-1]) & (second >= gp[0]) & (gid2 == gid)).all() and (np.diff(gid) >= 0).all())
    return np.searchsorted(gid, np.arange(G + 1), side='left').astype(np.int64), ok


def random_case(P, seed, levels=7, nan_share=0.0):
    """gt on a coarse grid (many exact ties and many differences exactly at a multiple of the grid step), pred random with planted ties."""
    rng = np.random.RandomState(1000 + seed)
    gt = (rng.randint(0, levels, size=P) * 0.05).astype(F32)
    pred = rng.rand(P).astype(F32)
    if P > 3:
        idx = rng.randint(0, P, size=P)
        pred[idx] = (rng.randint(0, 8, size=P) * 0.125).astype(F32)      # ties in the prediction: about two thirds lie on a grid of 8
    if nan_share > 0 and P > 0:
        gt[rng.rand(P) < nan_share] = np.nan
        pred[rng.rand(P) < nan_share] = np.nan
    return gt, pred
