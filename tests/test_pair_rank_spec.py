"""Pins tests/pair_rank_ref.py and the host logic of ops.link_ranks / ops.rank_metrics on the CPU: the restated counts equal a float64
brute force on inputs whose scores are exact in both; ops.link_rank_lists and ops.link_rank_filter — plain torch, driven here by the
restated counts in place of mgv_pair_rank_counts — give the ranks of the definition on designed cases (ties with a true link and with
a non-link, a link that leaves its graph, a self loop, a NaN row, no link at all), keep the caller's edge order and agree between the
plan's row pointers and the counted ones; ops.rank_metrics equals numpy; the header declares the entry and names its refusals."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_rank_ref as RR  # noqa: E402
from conftest import PKG_PARENT  # noqa: E402

F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64
NAN = float('nan')
GP = [0, 5, 70, 129]


def _ops():
    if PKG_PARENT not in sys.path:
        sys.path.insert(0, PKG_PARENT)
    from deepgate import ops
    return ops


def _cpu_link_ranks(score, ei, graph_ptr=None, by='src', skip_self=False, filtered=True, row_ptr=None):
    """ops.link_ranks with the restated counts where the device walks: lists, counts over them, filter."""
    ops = _ops()
    N = score.shape[0]
    lists = ops.link_rank_lists(ei, score[ei[0], ei[1]], N, graph_ptr=graph_ptr, by=by, skip_self=skip_self, row_ptr=row_ptr)
    th = lists.thr.numpy()
    for u in range(N):                                      # the entry's contract: every row ascends, NaNs last
        row = th[int(lists.thr_ptr[u]):int(lists.thr_ptr[u + 1])]
        fin = row[~np.isnan(row)]
        assert (np.diff(fin) >= 0).all() and not np.isnan(row[:fin.size]).any()
    rows = score if by == 'src' else score.T
    n_gt, n_eq = RR.rank_counts_ref(rows, lists.thr_ptr, lists.thr, graph_ptr, skip_self)
    return ops.link_rank_filter(lists, torch.from_numpy(n_gt), torch.from_numpy(n_eq), filtered), lists


def _same(ranks, ref):
    lo, hi, valid = ref
    return (np.array_equal(ranks.rank_lo.numpy(), lo) and np.array_equal(ranks.rank_hi.numpy(), hi)
            and np.array_equal(ranks.valid.numpy(), valid))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('gp,skip', [(None, False), (GP, True), ([0, 5, 5, 129], False)])
def test_the_restated_counts_equal_a_float64_brute_force_where_scores_are_exact(gp, skip):
    N, H = 129, 16
    s, t = RR.int_case(N, H, 1)
    sc = RR.scores_f32(s, t)
    s64 = s.to(F64) @ t.to(F64).T
    assert torch.equal(sc.to(F64), s64) and float(s64.abs().max()) < 2 ** 24          # exact in both
    values = sorted(set(s64.flatten().tolist()))[::3] + [-np.inf, np.inf, NAN, 0.5]
    lengths = [(0, 1, 32, 33, 65)[u % 5] for u in range(N)]
    tp, th = RR.lists_of_lengths(lengths, values, 5)
    n_gt, n_eq = RR.rank_counts_ref(sc, tp, th, gp, skip)
    mask = torch.from_numpy(RR.candidates(N, gp, skip))
    thr = torch.from_numpy(th).to(F64)
    row_of = torch.repeat_interleave(torch.arange(N), torch.tensor(lengths))
    want_gt = ((s64[row_of] > thr[:, None]) & mask[row_of]).sum(1)
    want_eq = ((s64[row_of] == thr[:, None]) & mask[row_of]).sum(1)
    assert np.array_equal(n_gt, want_gt.numpy()) and np.array_equal(n_eq, want_eq.numpy())
    assert int(want_eq.sum()) > 1000 and int((want_eq > 1).sum()) > 100               # the ties are there
    nan = np.isnan(th)
    assert nan.any() and not n_gt[nan].any() and not n_eq[nan].any()                  # a NaN threshold: (0, 0)
    sth, order = RR.sorted_lists(tp, th)                                             # sorting a row permutes its answers
    g2, e2 = RR.rank_counts_ref(sc, tp, sth, gp, skip)
    assert np.array_equal(g2, n_gt[order]) and np.array_equal(e2, n_eq[order])


# ------------------------------------------------------------------------------------------------ designed cases
def _designed():
    """Two graphs [0, 4) and [4, 7) with hand-made scores: row 0 holds a tie between two true links (0 -> 1, 0 -> 2) and a non-link
    (0 -> 3); (1, 5) leaves its graph; (2, 2) is a self loop; row 5 of the score matrix is NaN."""
    sc = torch.tensor([[1., 5., 5., 5., 9., 9., 9.],
                       [2., 0., 3., 1., 9., 9., 9.],
                       [4., 3., 7., 6., 9., 9., 9.],
                       [0., 0., 0., 0., 9., 9., 9.],
                       [9., 9., 9., 9., 1., 2., 3.],
                       [NAN] * 7,
                       [9., 9., 9., 9., 3., 2., 1.]], dtype=F32)
    ei = torch.tensor([[0, 0, 1, 2, 2, 5, 6, 1], [1, 2, 5, 2, 0, 4, 4, 2]])
    return sc, ei, [0, 4, 7]


def test_rank_lo_rank_hi_and_valid_on_designed_cases():
    sc, ei, gp = _designed()
    r, _ = _cpu_link_ranks(sc, ei, gp, filtered=True)
    # (0,1) and (0,2) tie with each other (filtered out) and with the non-link (0,3): ranks 1 .. 2 of {self, 3, 0}
    assert r.rank_lo.tolist() == [1, 1, 0, 1, 2, 0, 1, 1] and r.rank_hi.tolist() == [2, 2, 0, 1, 2, 0, 1, 1]
    assert r.valid.tolist() == [True, True, False, True, True, False, True, True]
    u, _ = _cpu_link_ranks(sc, ei, gp, filtered=False)
    assert u.rank_lo.tolist() == [1, 1, 0, 1, 3, 0, 1, 1] and u.rank_hi.tolist() == [3, 3, 0, 1, 3, 0, 1, 1]
    k, _ = _cpu_link_ranks(sc, ei, gp, skip_self=True)
    assert k.valid.tolist() == [True, True, False, False, True, False, True, True]     # the self loop (2, 2) leaves
    assert k.rank_lo.tolist() == [1, 1, 0, 0, 2, 0, 1, 1]                             # and (2, 0) now stands behind (2, 3) alone
    for by in ('src', 'dst'):
        for skip in (False, True):
            for filt in (False, True):
                got, _ = _cpu_link_ranks(sc, ei, gp, by=by, skip_self=skip, filtered=filt)
                assert _same(got, RR.link_ranks_ref(sc, ei, gp, by, skip, filt)), (by, skip, filt)
    one, _ = _cpu_link_ranks(sc[:4, :4], ei[:, [0, 1, 3, 4, 7]], None)                # no table: one graph
    assert _same(one, RR.link_ranks_ref(sc[:4, :4], ei[:, [0, 1, 3, 4, 7]], None))
    e0, lists = _cpu_link_ranks(sc, ei[:, :0], gp)
    assert e0.rank_lo.shape == (0,) and e0.valid.dtype == torch.bool and lists.thr_ptr.tolist() == [0] * 8
    ops = _ops()
    z = ops.link_ranks(torch.zeros(7, 16), torch.zeros(7, 16), ei[:, :0], gp)        # E = 0: nothing is launched, no library needed
    assert z.rank_lo.shape == z.rank_hi.shape == z.valid.shape == (0,) and z.rank_lo.dtype == I64


def test_a_duplicate_and_an_id_out_of_range_raise_value_error():
    ops = _ops()
    sc, ei, gp = _designed()
    dup = torch.cat([ei, ei[:, 4:5]], 1)
    with pytest.raises(ValueError, match='twice'):
        ops.link_rank_lists(dup, sc[dup[0], dup[1]], 7, gp)
    dup = torch.cat([ei[:, 5:6], ei], 1)                    # a duplicated link whose score is NaN
    with pytest.raises(ValueError, match='twice'):
        ops.link_rank_lists(dup, sc[dup[0], dup[1]], 7, gp, by='dst')
    s = torch.zeros(7, 16)
    for bad in ([[0, 7], [1, 2]], [[0, 1], [-1, 2]]):
        with pytest.raises(ValueError, match='outside'):
            ops.link_ranks(s, s, torch.tensor(bad), gp)      # before any score is asked for
        with pytest.raises(ValueError, match='outside'):
            ops.link_rank_lists(torch.tensor(bad), torch.zeros(2), 7, gp)
    with pytest.raises(ValueError, match='by must be'):
        ops.link_ranks(s, s, ei, gp, by='both')
    # equal scores in one row that are NOT duplicates pass
    ops.link_rank_lists(ei[:, :2], sc[ei[0, :2], ei[1, :2]], 7, gp)


# ------------------------------------------------------------------------------------------------ order and routes
@pytest.mark.parametrize('by', ['src', 'dst'])
def test_the_callers_order_survives_and_the_plan_route_agrees_with_the_counted_one(by):
    from deepgate.graph_plan import GraphPlan
    N, H = 129, 16
    s, t = RR.int_case(N, H, 2, span=2)                     # many ties
    sc = RR.scores_f32(s, t)
    ei = RR.random_edges(N, GP, 3, 1)
    E = ei.shape[1]
    assert E > 300
    for filt in (True, False):
        base, _ = _cpu_link_ranks(sc, ei, GP, by=by, filtered=filt)
        assert _same(base, RR.link_ranks_ref(sc, ei, GP, by, False, filt))
        assert int((base.rank_hi > base.rank_lo).sum()) > 20                       # ties with non-links are there
        perm = torch.randperm(E, generator=torch.Generator().manual_seed(3))
        shuf, _ = _cpu_link_ranks(sc, ei[:, perm], GP, by=by, filtered=filt)
        assert torch.equal(shuf.rank_lo, base.rank_lo[perm]) and torch.equal(shuf.rank_hi, base.rank_hi[perm])
        plan = GraphPlan(ei, N)
        rp = plan.out_ptr if by == 'src' else plan.in_ptr
        routed, lists = _cpu_link_ranks(sc, ei, GP, by=by, filtered=filt, row_ptr=rp)
        assert _same(routed, (base.rank_lo.numpy(), base.rank_hi.numpy(), base.valid.numpy())) and lists.thr_ptr.dtype == I32


# ------------------------------------------------------------------------------------------------ metrics
def test_rank_metrics_against_numpy():
    ops = _ops()
    N, H = 129, 16
    gp = [0, 5, 5, 70, 129]                                 # an empty graph: NaN
    s, t = RR.int_case(N, H, 3)
    sc = RR.scores_f32(s, t)
    sc[60] = NAN                                            # some links without a rank
    ei = RR.random_edges(N, [0, 5, 70, 129], 4, 2)
    ks = (1, 3, 10, 50)
    for by in ('src', 'dst'):
        ranks, _ = _cpu_link_ranks(sc, ei, gp, by=by)
        assert not bool(ranks.valid.all())
        m = ops.rank_metrics(ranks, ei, gp, ks=ks, by=by)
        want = RR.rank_metrics_ref(ranks.rank_lo.numpy(), ranks.rank_hi.numpy(), ranks.valid.numpy(), ei, gp, ks, by)
        for name in ('ranked', 'hits_lo', 'hits_hi', 'sum_lo', 'sum_hi'):
            got = getattr(m, name)
            assert got.dtype == I64 and np.array_equal(got.numpy(), want[name]), name
        assert m.mrr.dtype == F64 and m.hits_lo.shape == (4, 4)
        got, ref = m.mrr.numpy(), want['mrr']
        assert np.isnan(got[1]) and np.isnan(ref[1]) and m.ranked.tolist()[1] == 0 and not m.hits_lo[1].any()
        ok = ~np.isnan(ref)
        assert np.array_equal(np.isnan(got), ~ok) and (np.abs(got[ok] - ref[ok]) <= 1e-12 * np.abs(ref[ok])).all()
        again = ops.rank_metrics(ranks, ei, gp, ks=ks, by=by)
        assert np.array_equal(again.mrr.numpy().view(np.int64), got.view(np.int64))  # the same bits
        assert bool((m.hits_hi <= m.hits_lo).all()) and bool((m.sum_lo <= m.sum_hi).all())
    none = ops.rank_metrics(ops.LinkRanks(torch.zeros(0, dtype=I64), torch.zeros(0, dtype=I64), torch.zeros(0, dtype=torch.bool)),
                            ei[:, :0], gp, ks=(1,))
    assert none.ranked.tolist() == [0] * 4 and bool(torch.isnan(none.mrr).all())
    assert ops.rank_metrics(ranks, ei, [0], ks=ks).mrr.shape == (0,)


# ------------------------------------------------------------------------------------------------ the header
def test_the_header_declares_the_entry_and_names_every_refusal():
    from deepgate import _hip
    sigs = _hip.parse_header()
    assert len(sigs['mgv_pair_rank_counts']) == 14
    with open(_hip.HEADER_PATH) as f:
        text = f.read()
    head = text[:text.index('int mgv_pair_rank_counts(')]
    comment = re.sub(r'\s+', ' ', head[head.rindex('/* ----'):].replace('\n *', ' '))
    assert 'digae_layer.py:31-33' in comment and 'digae_model.py:118-122' in comment
    for words in ('H outside {16, 32, 64, 128} (MGV_EUNSUPPORTED)', 'a bad row stride or alignment', 'N out of range',
                  'a graph_ptr that does not start at 0 and end at N', 'a NULL thr_ptr', 'whose two ends are not 0 and a T',
                  'n_gt or n_eq with T > 0', 'MGV_EINVAL', 'N = 0 or T = 0 launches nothing', 'clamped into [0, T)', 'MUST ASCEND',
                  'A NaN threshold gets (0, 0)', 'no global atomics'):
        assert words in comment, words
