"""Restatement of the thresholded-link entries of csrc/pair_scores.hip (mgv_pair_select_count / mgv_pair_select_fill; reference:
digae_layer.py:31-33 forward_all, digae_model.py:118-122 — the pairs of the dense matrix above a threshold, as per-node lists), the
checkers the device tests use and the seeded case builders.  CPU only; pinned by tests/test_pair_select_spec.py.

The selection is a decision, not a number: against the device's own dense scores (mgv_pair_scores_fwd, the same bits) it is checked
EXACTLY (check_select); against float64 it is checked with each pair's own bound of pair_scores_ref (check_band): an emitted pair must
have ref + bound > threshold, a candidate that was not emitted ref - bound <= threshold, with no exclusions.  The band in which either
answer is right is measured first (pair_scores_ref.band_fraction), so that it cannot hide a failure.
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_scores_ref as PR  # noqa: E402

F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64
TILE, BLOCK = 64, 16
UNWRITTEN = -77                                          # what an output slot holds before a fill


def select_ref(score, graph_ptr, threshold, skip_self=False, by='src'):
    """(row_ptr int64 [N + 1], col int64 [E']) from a score matrix [N, N] (score[u, v] = the reported score of the pair u -> v): row u
    lists, in ascending order, the candidates v of its own graph (without v = u when skip_self) with score[u, v] > threshold; by='dst':
    row v lists the sources u of the same pairs, i.e. the same on the transpose.  A NaN is never selected (NaN > x is false)."""
    if by not in ('src', 'dst'):
        raise ValueError(by)
    sc = score if by == 'src' else score.T
    N = sc.shape[0]
    keep = (sc > threshold) & PR.candidate_mask(N, graph_ptr, skip_self)
    row_ptr = torch.zeros(N + 1, dtype=I64)
    row_ptr[1:] = torch.cumsum(keep.sum(1), 0)
    return row_ptr, torch.nonzero(keep)[:, 1].contiguous()          # nonzero is row-major: ascending columns inside a row


def selected_matrix(row_ptr, col, N):
    """bool [N, N]: entry [u, v] set where v is in row u's list."""
    rows = torch.repeat_interleave(torch.arange(N), (row_ptr[1:] - row_ptr[:-1]).long())
    m = torch.zeros((N, N), dtype=torch.bool)
    m[rows, col.long()] = True
    return m


def check_select(row_ptr, col, score, dense, graph_ptr, threshold, skip_self, by='src'):
    """The exact check of the device tests: (row_ptr, col, score or None) against nonzero((dense > threshold) & mask) in row-major order,
    `dense` being the [N, N] scores the device reports for the same operands (by='dst': its transpose).  Scores are compared as bits.
    Returns the list of what is wrong."""
    bad = []
    N = dense.shape[0]
    want_ptr, want_col = select_ref(dense, graph_ptr, threshold, skip_self, by)
    row_ptr, col = row_ptr.to(I64).cpu(), col.to(I64).cpu().flatten()
    if row_ptr.shape != want_ptr.shape or not torch.equal(row_ptr, want_ptr):
        n = min(row_ptr.numel(), want_ptr.numel())
        d = torch.nonzero(row_ptr[:n] != want_ptr[:n]).flatten()
        bad.append('row_ptr differs (first at %s; total %s, expected %d)' % (int(d[0]) if d.numel() else 'its length',
                                                                             int(row_ptr[-1]) if row_ptr.numel() else None, int(want_ptr[-1])))
        return bad
    if col.numel() != want_col.numel():
        bad.append('%d columns returned, %d expected' % (col.numel(), want_col.numel()))
        return bad
    if not torch.equal(col, want_col):
        e = int(torch.nonzero(col != want_col)[0])
        u = int(torch.searchsorted(want_ptr, torch.tensor(e), right=True)) - 1
        bad.append('col differs in %d slots, first in row %d at slot %d: %d, expected %d' % (int((col != want_col).sum()), u, e - int(want_ptr[u]),
                                                                                        int(col[e]), int(want_col[e])))
        return bad
    if score is not None:
        sc = dense if by == 'src' else dense.T
        rows = torch.repeat_interleave(torch.arange(N), want_ptr[1:] - want_ptr[:-1])
        want = sc[rows, want_col].to(F32).contiguous().view(I32)
        got = score.to(F32).cpu().flatten().contiguous().view(I32)
        if got.shape != want.shape or not torch.equal(got, want):
            bad.append('%d scores differ in bits from the dense entry' % (int((got != want).sum()) if got.shape == want.shape else -1))
    return bad


def check_band(row_ptr, col, ref, bound, graph_ptr, threshold, skip_self, by='src'):
    """Against float64 with NO exclusions; ref / bound: [N, N] float64 score and its error bound (p and dq with the sigmoid, raw and
    raw_bound without it; by='dst': their transposes are taken here).  Every emitted pair is a candidate of its row, is emitted once,
    in ascending order, and has ref + bound > threshold; every candidate that was not emitted has ref - bound <= threshold."""
    bad = []
    if by == 'dst':
        ref, bound = ref.T, bound.T
    N = ref.shape[0]
    row_ptr, col = row_ptr.to(I64).cpu(), col.to(I64).cpu().flatten()
    if row_ptr.numel() != N + 1 or int(row_ptr[0]) != 0 or bool((row_ptr[1:] < row_ptr[:-1]).any()) or int(row_ptr[-1]) != col.numel():
        return ['row_ptr is not an exclusive scan that ends at the number of columns']
    if col.numel() and (int(col.min()) < 0 or int(col.max()) >= N):
        return ['a column outside [0, N)']
    rows = torch.repeat_interleave(torch.arange(N), row_ptr[1:] - row_ptr[:-1])
    if col.numel() > 1 and bool(((rows[1:] == rows[:-1]) & (col[1:] <= col[:-1])).any()):
        bad.append('a row is not in strictly ascending column order')
    mask = PR.candidate_mask(N, graph_ptr, skip_self)
    if not bool(mask[rows, col].all()):
        bad.append('%d emitted pairs are no candidates of their row' % int((~mask[rows, col]).sum()))
    sel = selected_matrix(row_ptr, col, N)
    wrong_in = sel & ~(ref + bound > threshold)
    wrong_out = mask & ~sel & ~(ref - bound <= threshold)
    if bool(wrong_in.any()):
        u, v = torch.nonzero(wrong_in)[0].tolist()
        bad.append('%d emitted pairs lie below the threshold beyond their bound, first (%d, %d): %.9g' % (int(wrong_in.sum()), u, v, float(ref[u, v])))
    if bool(wrong_out.any()):
        u, v = torch.nonzero(wrong_out)[0].tolist()
        bad.append('%d candidates above the threshold beyond their bound are missing, first (%d, %d): %.9g'
                   % (int(wrong_out.sum()), u, v, float(ref[u, v])))
    return bad


# ------------------------------------------------------------------------------------------------ the fill, restated with its defects
DEFECTS = ('cursor_reset', 'descending_block', 'next_graph', 'self', 'ge', 'nan')


def restated_fill(score, graph_ptr, threshold, skip_self, defect=None, with_scores=True):
    """The two passes as the kernel walks them, in Python: per row the 64-column tiles that meet its graph, in each the four 16-column
    blocks; a block's decisions are one bit mask, a column's slot is the row's cursor plus the popcount of the lower bits, and the cursor
    moves on by the block's popcount.  -> (row_ptr, col, score), slots never written hold UNWRITTEN / NaN.  `defect` plants one of DEFECTS
    in the fill (and, for the defects of the decision, in the count before it, as a kernel with that defect would)."""
    assert defect is None or defect in DEFECTS
    N = score.shape[0]
    lo, hi = (x.tolist() for x in PR.row_range(graph_ptr, N))
    rows = score.tolist()

    def decisions(u, c0):
        bits = []
        for v in range(c0, c0 + BLOCK):
            inside = v < N and lo[u] <= v and (v <= hi[u] if defect == 'next_graph' else v < hi[u])
            x = rows[u][v] if inside else 0.0
            ok = inside and not (skip_self and v == u and defect != 'self')
            if defect != 'nan':
                ok = ok and not math.isnan(x)
            if defect == 'nan':
                take = ok and not (x <= threshold)
            elif defect == 'ge':
                take = ok and x >= threshold
            else:
                take = ok and x > threshold
            bits.append(take)
        return bits

    def tiles(u):
        if lo[u] >= hi[u]:
            return range(0)
        return range(lo[u] // TILE, (hi[u] + TILE - 1) // TILE)

    n_sel = torch.zeros(N, dtype=I64)
    for u in range(N):
        n_sel[u] = sum(sum(decisions(u, TILE * ct + BLOCK * c)) for ct in tiles(u) for c in range(TILE // BLOCK))
    row_ptr = torch.zeros(N + 1, dtype=I64)
    row_ptr[1:] = torch.cumsum(n_sel, 0)
    total = int(row_ptr[-1])
    col = torch.full((total,), UNWRITTEN, dtype=I64)
    out = torch.full((total,), float('nan'), dtype=score.dtype)
    for u in range(N):
        cursor, room = 0, int(row_ptr[u + 1] - row_ptr[u])
        for ct in tiles(u):
            if defect == 'cursor_reset':
                cursor = 0
            for c in range(TILE // BLOCK):
                c0 = TILE * ct + BLOCK * c
                bits = decisions(u, c0)
                n = sum(bits)
                for j, b in enumerate(bits):
                    if not b:
                        continue
                    below = sum(bits[:j])
                    slot = cursor + (n - 1 - below if defect == 'descending_block' else below)
                    if slot < room:
                        col[int(row_ptr[u]) + slot] = c0 + j
                        out[int(row_ptr[u]) + slot] = score[u, c0 + j]
                cursor += n
    return row_ptr, col, (out if with_scores else None)


# ------------------------------------------------------------------------------------------------ case builders (seeded)
SIZES = PR.TOPK_SIZES
EMPTY_MIDDLE_SIZES = (5, 0, 70, 2, 0, 66)               # graphs without nodes in the middle of graph_ptr
CASES = ((True, 0.5), (False, 0.0), (False, -1.0))      # (sigmoid, threshold) of the device tests


def select_case(H, seed, sizes=SIZES):
    """pair_scores_ref.topk_case (graph borders inside the 64-row and 64-column tiles, rows up to four column tiles long, its planted
    ties / edge / self rows) and, in its first 2-node graph, two rows with a known answer at every threshold of CASES and far from all
    of them: `full_row` scores >= 100 with both nodes of its graph (it selects every candidate), `empty_row` <= -100 (it selects
    nothing)."""
    c = PR.topk_case(H, seed, sizes=sizes)
    gp, s, t = c['graph_ptr'], c['s'], c['t']
    c['info']['full_row'] = c['info']['empty_row'] = None
    two = [i for i in range(len(sizes)) if sizes[i] == 2]
    if two:
        a, b = gp[two[0]], gp[two[0]] + 1
        sa, sb = s[a].to(F64), s[b].to(F64)
        d = sa / sa.norm() - sb / sb.norm()                 # <sa, d> = |sa| (1 - cos) > 0 > <sb, d> = -|sb| (1 - cos)
        weakest = min(float(sa @ d), -float(sb @ d))
        assert weakest > 0
        t[a] = (100.0 / weakest * d).to(F32)
        t[b] = (200.0 / weakest * d).to(F32)
        c['info']['full_row'], c['info']['empty_row'] = a, b
    return c


def reported(r, sigmoid):
    """(score, bound) float64 of a pair_scores_ref.scores_ref record, as the entries report them."""
    return (r['p'], r['dq']) if sigmoid else (r['raw'], r['raw_bound'])
