"""The thresholded-link entries of csrc/pair_scores.hip — mgv_pair_select_count, mgv_pair_select_fill — through the C ABI and through the
surface (ops.pair_select, DirectedInnerProductDecoder.select, Model.reconstruct_edges, DirectedGAE.reconstruct_edges,
examples/feature_extract.py --reconstruct), against tests/pair_select_ref.py (pinned on the CPU by tests/test_pair_select_spec.py, which
also asserts the properties of the case builders used here and shows the planted defects of a restated fill to be caught by check_select).

Exact: row_ptr, col and score equal nonzero((dense > thr) & mask) in row-major order, dense = mgv_pair_scores_fwd on the same operands,
scores as bits; by='dst' the same on dense.T; n_sel equals n_above of mgv_pair_topk; two calls give the same bytes.
Against float64, no exclusions: every emitted pair has ref + bound > thr, every other candidate ref - bound <= thr (bound = dq with the
sigmoid, H 2^-24 S without), after the band |ref - thr| <= bound has been measured to hold at most 1e-3 of the candidates.

Conventions of tests/test_hip_pair_scores.py: operands are column slices of wider matrices whose foreign columns hold NaN; every output
has 64 guard rows behind it and is filled before the call (col -77, score NaN).  Every check prints one line `SEL <what> | figures`."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_scores_ref as PR  # noqa: E402
import pair_select_ref as SR  # noqa: E402
import test_hip_pair_scores as TP  # noqa: E402  (Out, the operand slices and the launcher helpers of the pair-score tests)

pytestmark = pytest.mark.gpu

F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64
HS = (16, 32, 64, 128)
INF = float('inf')
MGV_EINVAL, MGV_EUNSUPPORTED = -1, -2
Out, _dev, _ptr, _rc, _call, _bits, _slice = TP.Out, TP._dev, TP._ptr, TP._rc, TP._call, TP._bits, TP._slice


@functools.lru_cache(maxsize=None)
def _case(H, seed=1, sizes=SR.SIZES):
    c = SR.select_case(H, seed, sizes=sizes)
    return c, PR.scores_ref(c['s'], c['t'])


class Run:
    """One count / scan / fill through the raw ABI on strided operands; every output an Out of the test's own."""

    def __init__(self, dev, s, t, gp, sigmoid, thr, skip, with_score=True, row_ptr=None, cap=None, slots=None):
        H, N = s.shape[1], s.shape[0]
        self.sv, lds = _slice(s, dev)
        self.tv, ldt = _slice(t, dev)
        self.gpd = None if gp is None else torch.tensor(gp, dtype=I32, device=dev)
        self.args = (H, N, _ptr(self.sv), lds, _ptr(self.tv), ldt, _ptr(self.gpd), 0 if gp is None else len(gp) - 1, int(sigmoid), float(thr),
                     int(skip))
        self.n_sel = Out(N, 1, dev, dtype=I32)
        _call('mgv_pair_select_count', *self.args, _ptr(self.n_sel.v))
        n = self.n_sel.v.flatten().to(I64)
        self.true_ptr = torch.zeros(N + 1, dtype=I64, device=dev)
        self.true_ptr[1:] = torch.cumsum(n, 0)
        self.total = int(self.true_ptr[-1])
        self.row_ptr = self.true_ptr if row_ptr is None else row_ptr.to(device=dev, dtype=I64).contiguous()
        self.cap = self.total if cap is None else cap
        slots = self.total if slots is None else slots      # the buffers' real size: never below what any row_ptr / cap may reach
        self.col, self.score = Out(slots, 1, dev, dtype=I32), (Out(slots, 1, dev) if with_score else None)
        self.fill()

    def fill(self):
        _call('mgv_pair_select_fill', *self.args, _ptr(self.row_ptr), self.cap, _ptr(self.col.v),
              None if self.score is None else _ptr(self.score.v))

    def intact(self):
        return self.n_sel.intact() and self.col.intact() and (self.score is None or self.score.intact())

    def lists(self):
        """(row_ptr, col, score) of the true lists: the first `total` slots (a test that gives more slots inspects the rest itself)."""
        k = self.total
        return self.row_ptr.cpu(), self.col.v.flatten()[:k].cpu(), None if self.score is None else self.score.v.flatten()[:k].cpu()


def _dense(dev, s, t, sigmoid):
    return TP._fwd(dev, s, t, sigmoid)[0].v.cpu()


def _n_above(dev, c, gp, sigmoid, thr, skip):
    return TP._run_topk(dev, c, 1, gp, sigmoid, thr, skip)[2]


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize('H', HS)
def test_select_equals_the_dense_matrix_above_the_threshold(H):
    """Graphs of (1, 2, 63, 64, 65, 130, 5, 200) nodes and the same nodes as one graph; sigmoid at 0.5, raw at 0.0 and -1.0; with and
    without skip_self; by source and by target; the raw ABI and ops.pair_select."""
    dev = _dev()
    from deepgate import ops
    c, _ = _case(H)
    gp, N, info = c['graph_ptr'], c['N'], c['info']
    sd, td = c['s'].to(dev), c['t'].to(dev)
    bad, totals = [], []
    for sigmoid, thr in SR.CASES:
        dense = _dense(dev, c['s'], c['t'], sigmoid)
        for g in (gp, None):
            for skip in (False, True):
                tag = 'H=%d sigmoid=%s thr=%g graphs=%s skip_self=%s' % (H, sigmoid, thr, g is not None, skip)
                run = Run(dev, c['s'], c['t'], g, sigmoid, thr, skip)
                bad += ['%s ABI: %s' % (tag, b) for b in SR.check_select(*run.lists(), dense, g, thr, skip)]
                if not run.intact():
                    bad.append('%s ABI: guard rows changed' % tag)
                if not torch.equal(run.n_sel.v.flatten().cpu(), _n_above(dev, c, g, sigmoid, thr, skip)):
                    bad.append('%s: n_sel differs from n_above of mgv_pair_topk' % tag)
                totals.append(run.total)
                # two calls give the same bytes
                first = (_bits(run.col.parent), _bits(run.score.parent))
                run.col.parent.fill_(-77)
                run.score.parent.fill_(TP.NAN)
                run.fill()
                if not (torch.equal(first[0], _bits(run.col.parent)) and torch.equal(first[1], _bits(run.score.parent))):
                    bad.append('%s ABI: a second fill gives other bytes' % tag)
                # score = NULL leaves col as before
                bare = Run(dev, c['s'], c['t'], g, sigmoid, thr, skip, with_score=False)
                if not torch.equal(bare.col.parent, run.col.parent):
                    bad.append('%s ABI: col changes when no scores are asked for' % tag)
                # by target through the ABI: the operands change places
                swapped = Run(dev, c['t'], c['s'], g, sigmoid, thr, skip)
                bad += ['%s ABI by dst: %s' % (tag, b) for b in SR.check_select(*swapped.lists(), dense, g, thr, skip, by='dst')]
                for by in ('src', 'dst'):
                    row_ptr, col, score = ops.pair_select(sd, td, graph_ptr=g, sigmoid=sigmoid, threshold=thr, skip_self=skip, by=by,
                                                          with_scores=True)
                    assert row_ptr.dtype == I64 and col.dtype == I32 and score.dtype == F32 and col.is_cuda
                    bad += ['%s ops by %s: %s' % (tag, by, b) for b in SR.check_select(row_ptr, col, score, dense, g, thr, skip, by=by)]
                    assert ops.pair_select(sd, td, graph_ptr=g, sigmoid=sigmoid, threshold=thr, skip_self=skip, by=by)[2] is None
        # the planted rows, in the lists by source with the graphs
        row_ptr, col, _ = ops.pair_select(sd, td, graph_ptr=gp, sigmoid=sigmoid, threshold=thr, skip_self=True)
        row_ptr, col = row_ptr.tolist(), col.tolist()
        row = lambda u: col[row_ptr[u]:row_ptr[u + 1]]  # noqa: E731
        u, v0, v1, vx = info['edge_row']
        if not (v0 in row(u) and v1 in row(u) and vx not in row(u)):
            bad.append('row %d should hold %d and %d and never %d: %s' % (u, v0, v1, vx, row(u)))
        if info['self_row'] in row(info['self_row']):
            bad.append('self row %d lists itself under skip_self' % info['self_row'])
        if row(info['full_row']) != [info['empty_row']] or row(info['empty_row']) != []:
            bad.append('the planted full / empty rows: %s %s' % (row(info['full_row']), row(info['empty_row'])))
    print('SEL exact H=%d N=%d | links per configuration %d .. %d | %d findings' % (H, N, min(totals), max(totals), len(bad)))
    assert not bad, bad[:10]


@pytest.mark.parametrize('H', HS)
def test_infinite_thresholds_and_a_nan_row(H):
    """raw threshold -inf: every candidate of every row (all rows of the 200-node graph are full); +inf: nothing, and nothing is
    written; a row of s that holds a NaN selects nothing."""
    dev = _dev()
    c, _ = _case(H)
    gp, N = c['graph_ptr'], c['N']
    dense = _dense(dev, c['s'], c['t'], False)
    for skip in (False, True):
        run = Run(dev, c['s'], c['t'], gp, False, -INF, skip)
        mask = PR.candidate_mask(N, gp, skip)
        row_ptr, col, score = run.lists()
        assert torch.equal(row_ptr[1:] - row_ptr[:-1], mask.sum(1)) and int((row_ptr[1:] - row_ptr[:-1])[gp[-2]:].min()) == 200 - int(skip)
        assert torch.equal(col.long(), torch.nonzero(mask)[:, 1]) and run.intact()
        assert SR.check_select(row_ptr, col, score, dense, gp, -INF, skip) == []
    slots = int(PR.candidate_mask(N, gp, False).sum())
    run = Run(dev, c['s'], c['t'], gp, False, INF, False, cap=slots, slots=slots)
    assert run.total == 0 and run.col.untouched() and run.score.untouched() and not bool(run.n_sel.v.any())
    s = c['s'].clone()
    poisoned = [gp[5] + 7, gp[7] + 100, gp[7] + 199]
    for u in poisoned:
        s[u, H // 2] = TP.NAN
    for sigmoid, thr in ((True, 0.5), (False, -INF)):
        run = Run(dev, s, c['t'], gp, sigmoid, thr, False)
        n = run.n_sel.v.flatten().cpu()
        assert n[poisoned].tolist() == [0, 0, 0] and run.intact()
        assert SR.check_select(*run.lists(), _dense(dev, s, c['t'], sigmoid), gp, thr, False) == []
        swapped = Run(dev, c['t'], s, gp, sigmoid, thr, False)           # by target: the poisoned nodes appear in no list
        assert not bool(torch.isin(swapped.col.v.flatten().cpu().long(), torch.tensor(poisoned)).any())
    print('SEL infinite thresholds and NaN rows H=%d | ok' % H)


@pytest.mark.parametrize('H', HS)
def test_empty_graphs_one_node_and_no_node(H):
    dev = _dev()
    from deepgate import ops
    c, _ = _case(H, 1, SR.EMPTY_MIDDLE_SIZES)
    gp = c['graph_ptr']
    for sigmoid, thr in SR.CASES:
        dense = _dense(dev, c['s'], c['t'], sigmoid)
        for skip in (False, True):
            run = Run(dev, c['s'], c['t'], gp, sigmoid, thr, skip)
            assert SR.check_select(*run.lists(), dense, gp, thr, skip) == [] and run.intact()
            assert torch.equal(run.n_sel.v.flatten().cpu(), _n_above(dev, c, gp, sigmoid, thr, skip))
            got = ops.pair_select(c['s'].to(dev), c['t'].to(dev), graph_ptr=gp, sigmoid=sigmoid, threshold=thr, skip_self=skip, by='dst',
                                  with_scores=True)
            assert SR.check_select(*got, dense, gp, thr, skip, by='dst') == []
    # N = 1: the node's own score decides, skip_self leaves nothing
    one = PR.topk_case(H, 1, sizes=(1,), plant=False)
    for sign in (1.0, -1.0):
        s, t = one['s'], sign * one['s']
        for g in ([0, 1], None):
            run = Run(dev, s, t, g, True, 0.5, False, slots=1)
            assert run.n_sel.v.flatten().tolist() == [int(sign > 0)] and run.intact()
            assert SR.check_select(*run.lists(), _dense(dev, s, t, True), g, 0.5, False) == []
            assert run.total == 1 or run.col.untouched()
            assert Run(dev, s, t, g, True, 0.5, True, slots=1).total == 0
            row_ptr, col, score = ops.pair_select(s.to(dev), t.to(dev), graph_ptr=g, with_scores=True)
            assert row_ptr.tolist() == [0, int(sign > 0)] and col.tolist() == [0][:int(sign > 0)]
    # N = 0: nothing is launched, nothing is written
    n_sel, col = Out(0, 1, dev, dtype=I32), Out(0, 1, dev, dtype=I32)
    empty = torch.full((1, H), TP.NAN, device=dev)
    zero = torch.zeros(1, dtype=I64, device=dev)
    for gpd, G in ((None, 0), (torch.zeros(1, dtype=I32, device=dev), 0), (torch.zeros(3, dtype=I32, device=dev), 2)):
        common = (H, 0, _ptr(empty), H, _ptr(empty), H, _ptr(gpd), G, 1, 0.5, 0)
        _call('mgv_pair_select_count', *common, _ptr(n_sel.v))
        _call('mgv_pair_select_fill', *common, _ptr(zero), 0, _ptr(col.v), None)
        assert n_sel.untouched() and col.untouched()
    row_ptr, col, score = ops.pair_select(torch.zeros(0, H, device=dev), torch.zeros(0, H, device=dev), graph_ptr=[0], with_scores=True)
    assert row_ptr.tolist() == [0] and col.shape == (0,) and score.shape == (0,) and row_ptr.dtype == I64 and col.dtype == I32
    print('SEL empty graphs, N = 1, N = 0 H=%d | ok' % H)


# ------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize('H', HS)
def test_select_against_float64(H):
    """Seeds 1 - 3, with the graphs and as one graph, the three thresholds, by source and by target: no exclusions."""
    dev = _dev()
    from deepgate import ops
    bad, band, links = [], 0.0, 0
    for seed in (1, 2, 3):
        c, r = _case(H, seed)
        sd, td = c['s'].to(dev), c['t'].to(dev)
        for g in (c['graph_ptr'], None):
            for sigmoid, thr in SR.CASES:
                ref, bound = SR.reported(r, sigmoid)
                skip = seed == 2
                share = PR.band_fraction(ref, bound, thr, PR.candidate_mask(c['N'], g, skip))
                band = max(band, share)
                assert share <= 1e-3, (seed, sigmoid, thr, share)
                for by in ('src', 'dst'):
                    row_ptr, col, _ = ops.pair_select(sd, td, graph_ptr=g, sigmoid=sigmoid, threshold=thr, skip_self=skip, by=by)
                    links += col.numel()
                    bad += ['seed %d graphs=%s sigmoid=%s thr=%g by %s: %s' % (seed, g is not None, sigmoid, thr, by, b)
                            for b in SR.check_band(row_ptr, col, ref, bound, g, thr, skip, by=by)]
    print('SEL float64 H=%d | %d links checked, every candidate on its side of its bound | band holds at most %.3g of the candidates | '
          '%d findings' % (H, links, band, len(bad)))
    assert not bad, bad[:10]


# ------------------------------------------------------------------------------------------------ bounds of the fill
def test_the_fill_stays_inside_the_slots_it_is_given():
    """All buffers are the test's own, at the full size of the true lists: a miswrite would land in memory that is inspected here."""
    dev = _dev()
    c, _ = _case(64)
    gp = c['graph_ptr']
    full = Run(dev, c['s'], c['t'], gp, True, 0.5, False)
    true_ptr, want_col, want_score = full.lists()
    n = true_ptr[1:] - true_ptr[:-1]
    total = full.total
    # one row gets fewer slots than it selects: it writes its first entries only, everything else is where it was
    u = int(torch.argmax(n[:-1] * (n[1:] > 0)))             # the longest list that has a non-empty successor
    short = 5
    assert int(n[u]) > 64 + short
    row_ptr = true_ptr.clone()
    row_ptr[u + 1:] -= int(n[u]) - short
    run = Run(dev, c['s'], c['t'], gp, True, 0.5, False, row_ptr=row_ptr, slots=total)
    keep = torch.ones(total, dtype=torch.bool)
    keep[int(true_ptr[u]) + short:int(true_ptr[u + 1])] = False
    got_col, got_score = run.col.v.flatten().cpu(), run.score.v.flatten().cpu()
    used = int(keep.sum())
    assert torch.equal(got_col[:used], want_col[keep]) and torch.equal(_bits(got_score[:used]), _bits(want_score[keep]))
    assert bool((got_col[used:] == -77).all()) and bool(torch.isnan(got_score[used:]).all()) and run.intact()
    # row_ptr all zero: no row has a slot
    run = Run(dev, c['s'], c['t'], gp, True, 0.5, False, row_ptr=torch.zeros_like(true_ptr), slots=total)
    assert run.col.untouched() and run.score.untouched()
    # only that row's end is pulled in: its successor starts early and keeps its end, every other row keeps its slots
    row_ptr = true_ptr.clone()
    row_ptr[u + 1] = true_ptr[u] + short
    run = Run(dev, c['s'], c['t'], gp, True, 0.5, False, row_ptr=row_ptr, slots=total)
    exp_col, exp_score = want_col.clone(), want_score.clone()
    a, b, e = int(true_ptr[u]) + short, int(true_ptr[u + 1]), int(true_ptr[u + 2])
    exp_col[a:e], exp_score[a:e] = -77, TP.NAN
    exp_col[a:a + e - b], exp_score[a:a + e - b] = want_col[b:e], want_score[b:e]
    assert e - b > 0 and torch.equal(run.col.v.flatten().cpu(), exp_col) and run.intact()
    assert torch.equal(_bits(run.score.v.flatten().cpu()), _bits(exp_score))
    # descending or negative entries: a row never leaves [row_ptr[u], row_ptr[u + 1]) nor [0, cap)
    for odd in (true_ptr.flip(0), true_ptr - total - 7, torch.full_like(true_ptr, total + 1000)):
        run = Run(dev, c['s'], c['t'], gp, True, 0.5, False, row_ptr=odd, slots=total)
        assert run.col.untouched() and run.score.untouched()
    # cap below the total: nothing at or behind cap
    cap = int(true_ptr[u]) + 3                              # ends inside row u's list
    run = Run(dev, c['s'], c['t'], gp, True, 0.5, False, cap=cap, slots=total)
    got_col, got_score = run.col.v.flatten().cpu(), run.score.v.flatten().cpu()
    assert torch.equal(got_col[:cap], want_col[:cap]) and torch.equal(_bits(got_score[:cap]), _bits(want_score[:cap]))
    assert bool((got_col[cap:] == -77).all()) and bool(torch.isnan(got_score[cap:]).all()) and run.intact()
    run = Run(dev, c['s'], c['t'], gp, True, 0.5, False, cap=0, slots=total)
    assert run.col.untouched() and run.score.untouched()
    print('SEL fill bounds | row %d of %d links cut to %d, zero row_ptr, cap %d of %d | ok' % (u, int(n[u]), short, cap, total))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_return_codes_before_anything_is_launched():
    dev = _dev()
    n = 40
    s48, s = torch.randn(n, 48, device=dev), torch.randn(n, 16, device=dev)
    ptr0 = torch.arange(0, 4 * (n + 1), 4, dtype=I64, device=dev)

    def both(H, N, x, ld, gp, cap=None, base=None):
        """(count's code, fill's code, every output untouched)"""
        n_sel, col, score = Out(n, 1, dev, dtype=I32), Out(4 * n, 1, dev, dtype=I32), Out(4 * n, 1, dev)
        gpd = None if gp is None else torch.tensor(gp, dtype=I32, device=dev)
        xp = _ptr(x) if base is None else base
        common = (H, N, xp, ld, xp, ld, _ptr(gpd), 0 if gp is None else len(gp) - 1, 0, -INF, 0)
        a = _rc('mgv_pair_select_count', *common, _ptr(n_sel.v))
        b = _rc('mgv_pair_select_fill', *common, _ptr(ptr0), 4 * n if cap is None else cap, _ptr(col.v), _ptr(score.v))
        return a, b, n_sel.untouched() and col.untouched() and score.untouched()
    assert both(48, n, s48, 48, None) == (MGV_EUNSUPPORTED, MGV_EUNSUPPORTED, True)
    assert both(0, n, s, 16, None) == (MGV_EUNSUPPORTED, MGV_EUNSUPPORTED, True)
    assert both(16, n, s, 12, None) == (MGV_EINVAL, MGV_EINVAL, True)             # row stride below H
    assert both(16, n, s, 18, None) == (MGV_EINVAL, MGV_EINVAL, True)             # row stride no multiple of 4
    assert both(16, n, s, 16, None, base=TP._hip().ptr(s.view(-1)[1:])) == (MGV_EINVAL, MGV_EINVAL, True)      # base not 16-byte aligned
    assert both(16, 2 ** 31, s, 16, None) == (MGV_EINVAL, MGV_EINVAL, True)
    assert both(16, -1, s, 16, None) == (MGV_EINVAL, MGV_EINVAL, True)
    assert both(16, n, s, 16, [0, 10, n - 1]) == (MGV_EINVAL, MGV_EINVAL, True)   # does not end at N
    assert both(16, n, s, 16, [0, 10, n + 1]) == (MGV_EINVAL, MGV_EINVAL, True)
    assert both(16, n, s, 16, [1, 10, n]) == (MGV_EINVAL, MGV_EINVAL, True)       # does not start at 0
    a, b, untouched = both(16, n, s, 16, None, cap=-1)
    assert (a, b, untouched) == (0, MGV_EINVAL, False)                            # (the count ran; the fill wrote nothing:)
    n_sel, col, score = Out(n, 1, dev, dtype=I32), Out(4 * n, 1, dev, dtype=I32), Out(4 * n, 1, dev)
    assert _rc('mgv_pair_select_fill', 16, n, _ptr(s), 16, _ptr(s), 16, None, 0, 0, -INF, 0, _ptr(ptr0), -1, _ptr(col.v), _ptr(score.v)) \
        == MGV_EINVAL and col.untouched() and score.untouched()
    assert both(16, n, s, 16, [0, 10, n]) == (0, 0, False)
    from deepgate import _hip, ops
    with pytest.raises(_hip.HipLibraryError, match='EINVAL'):
        ops.pair_select(s, s, graph_ptr=[0, 10, n - 1])
    with pytest.raises(_hip.HipLibraryError, match='EUNSUPPORTED'):
        ops.pair_select(s48, s48)
    with pytest.raises(_hip.HipLibraryError, match='same number of rows'):
        ops.pair_select(s, s[:7])


# ------------------------------------------------------------------------------------------------ surface
@functools.lru_cache(maxsize=None)
def _model_case():
    dev = _dev()
    import deepgate
    from deepgate import ops
    H = 64
    c, _ = _case(H)
    ei = PR.edges_case(c, 3, 1).to(dev)
    torch.manual_seed(0)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=H, s_rounds=1, t_rounds=1, layernorm=True)
    model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=H).to(dev)
    hs = c['s'].to(dev)
    with torch.no_grad():
        st = ops.linear(hs, model.hs_decompose.weight, model.hs_decompose.bias)
    return c, ei, enc, model, hs, st


def test_reconstruct_edges_on_the_model():
    dev = _dev()
    from deepgate import _hip, ops
    c, ei, enc, model, hs, st = _model_case()
    H, gp, N = 64, c['graph_ptr'], c['N']
    counts = model.reconstruction_counts(hs, ei, gp).cpu()
    edge_index, row_ptr, score = model.reconstruct_edges(hs, graph_ptr=gp)
    assert edge_index.dtype == I64 and edge_index.is_cuda and row_ptr.dtype == I64 and score is None
    assert edge_index.shape == (2, int(counts[:, 1].sum())) and int(row_ptr[-1]) == edge_index.shape[1]
    dense = ops.pair_scores(st[:, :H], st[:, H:]).cpu()
    want_ptr, want_col = SR.select_ref(dense, gp, 0.5)
    rows = torch.repeat_interleave(torch.arange(N), want_ptr[1:] - want_ptr[:-1])
    assert torch.equal(edge_index.cpu(), torch.stack([rows, want_col])) and torch.equal(row_ptr.cpu(), want_ptr)
    # every true edge: in the decoded list exactly when its own score is above the threshold
    sel = SR.selected_matrix(row_ptr.cpu(), edge_index[1].cpu(), N)
    e = ei.cpu()
    above = (ops.pair_scores_at(st[:, :H], st[:, H:], ei) > 0.5).cpu()
    assert torch.equal(sel[e[0], e[1]], above)
    # per graph: the decoded true edges, de-duplicated, against the counts' true positives (which count repeated edges repeatedly)
    gpt = torch.tensor(gp)
    uniq = torch.unique(e, dim=1)
    gid = torch.bucketize(uniq[0].contiguous(), gpt[1:].contiguous(), right=True)
    tp_unique = torch.zeros(len(gp) - 1, dtype=I64).index_add_(0, gid, sel[uniq[0], uniq[1]].long())
    gid_all = torch.bucketize(e[0], gpt[1:].contiguous(), right=True)
    tp_all = torch.zeros(len(gp) - 1, dtype=I64).index_add_(0, gid_all, sel[e[0], e[1]].long())
    assert torch.equal(tp_all, counts[:, 0]) and int(tp_unique.sum()) > 0
    assert torch.equal(tp_unique, model.reconstruction_counts(hs, uniq.to(dev), gp).cpu()[:, 0])
    assert torch.equal(row_ptr.cpu()[gpt[1:]] - row_ptr.cpu()[gpt[:-1]], counts[:, 1])
    # by target: (source, target) rows all the same, listed per target; with scores: the dense entries
    e2, p2, s2 = model.reconstruct_edges(hs, graph_ptr=gp, by='dst', with_scores=True, skip_self=True)
    tptr, tcol = SR.select_ref(dense, gp, 0.5, True, by='dst')
    trows = torch.repeat_interleave(torch.arange(N), tptr[1:] - tptr[:-1])
    assert torch.equal(e2.cpu(), torch.stack([tcol, trows])) and torch.equal(p2.cpu(), tptr)
    assert torch.equal(_bits(s2), _bits(dense[tcol, trows]))
    # the refusal comes before the fill and names the total
    total = edge_index.shape[1]
    calls = []
    real = _hip.call
    try:
        _hip.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
        with pytest.raises(_hip.HipLibraryError, match=str(total)) as err:
            model.reconstruct_edges(hs, graph_ptr=gp, max_edges=total - 1)
    finally:
        _hip.call = real
    assert 'mgv_pair_select_count' in calls and 'mgv_pair_select_fill' not in calls
    assert 'pair_topk' in str(err.value) and 'threshold' in str(err.value)
    assert model.reconstruct_edges(hs, graph_ptr=gp, max_edges=total)[0].shape[1] == total
    print('SEL Model.reconstruct_edges | %d decoded edges, %d of %d true edges among them' % (total, int(tp_all.sum()), e.shape[1]))


def test_directed_gae_and_the_decoder_agree_with_ops():
    _dev()
    import deepgate
    from deepgate import ops
    c, ei, enc, model, hs, st = _model_case()
    H, gp = 64, c['graph_ptr']
    s, t = st[:, :H], st[:, H:]
    gae = deepgate.digae_model.DirectedGAE(enc)
    for by in ('src', 'dst'):
        row_ptr, col, score = ops.pair_select(s, t, graph_ptr=gp, by=by, with_scores=True, threshold=0.6, skip_self=True)
        edge_index, p2, s2 = gae.reconstruct_edges(s, t, graph_ptr=gp, threshold=0.6, skip_self=True, by=by, with_scores=True)
        rows = torch.repeat_interleave(torch.arange(c['N'], device=col.device), row_ptr[1:] - row_ptr[:-1])
        assert torch.equal(edge_index[1 if by == 'src' else 0], col.long()) and torch.equal(edge_index[0 if by == 'src' else 1], rows)
        assert torch.equal(p2, row_ptr) and torch.equal(_bits(s2), _bits(score))
        d = deepgate.digae_layer.DirectedInnerProductDecoder().select(s, t, graph_ptr=gp, threshold=0.6, skip_self=True, by=by, with_scores=True)
        assert torch.equal(d[0], row_ptr) and torch.equal(d[1], col) and torch.equal(_bits(d[2]), _bits(score))
    m1 = gae.reconstruct_edges(s, t, graph_ptr=gp)
    m2 = model.reconstruct_edges(hs, graph_ptr=gp)
    assert torch.equal(m1[0], m2[0]) and torch.equal(m1[1], m2[1])


def test_feature_extract_reconstruct(tmp_path):
    """examples/feature_extract.py --reconstruct THR: name/rec_edge_index with ids local to the graph, name/rec_precision and
    name/rec_recall, beside the embeddings."""
    _dev()
    import importlib

    import numpy as np
    from conftest import PKG_PARENT
    sys.path.insert(0, os.path.join(PKG_PARENT, 'examples'))
    fe = importlib.import_module('feature_extract')
    out = tmp_path / 'emb.npz'
    fe.main(['--type', 'aig', '--synthetic', '2', '--rounds', '1', '--batch_size', '2', '--reconstruct', '0.5', '--out', str(out)])
    emb = np.load(out)
    assert sorted(emb.files) == sorted('graph%d/%s' % (i, k) for i in range(2) for k in ('hs', 'hf', 'rec_edge_index', 'rec_precision',
                                                                                       'rec_recall'))
    for i in range(2):
        ei = emb['graph%d/rec_edge_index' % i]
        n = emb['graph%d/hs' % i].shape[0]
        assert ei.ndim == 2 and ei.shape[0] == 2 and ei.shape[1] > 0 and ei.dtype == np.int32
        assert ei.min() >= 0 and ei.max() < n
        key = ei[0].astype(np.int64) * n + ei[1]
        assert (np.diff(key) > 0).all()                                    # per source, ascending targets, no pair twice
        p, r = float(emb['graph%d/rec_precision' % i]), float(emb['graph%d/rec_recall' % i])
        assert 0.0 <= p <= 1.0 and 0.0 <= r <= 1.0
