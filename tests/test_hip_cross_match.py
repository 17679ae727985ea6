"""The cross-circuit entries of csrc/pair_scores.hip — mgv_cross_topk, mgv_cross_select_count, mgv_cross_select_fill — through the C ABI
and through the surface (ops.cross_topk / cross_pairs / cross_mutual / cross_classes, Model.match_gates / cross_equivalence_candidates /
cross_equivalence_classes, examples/feature_extract.py --match / --cross_equivalences), against tests/cross_match_ref.py (pinned on
the CPU by tests/test_cross_match_spec.py, which also asserts the designed features of the case used here).

Graphs of (70, 1, 64, 129, 0, 63, 5, 33) nodes: tile (64), wave (16) and heap (32) borders fall inside and between graphs; the two peer
tables of cross_match_ref.PEERS; H = 16 / 32 / 64 / 128; k = 1, 8, 32.
Exact, without a tolerance: the restatement applied to the scores the EXISTING mgv_pair_scores_at reports for every (row, candidate)
pair of the device's own unit rows must give the device's idx, score, n_above and lists — integers as integers, scores as bits.  One
float64 check with the project's bound (2H + 6) 2^-24 S (pair_scores_ref.check_topk, pair_select_ref.check_band, after the band has
been measured).  Conventions of tests/test_hip_pair_scores.py: operands are column slices of wider matrices whose foreign columns hold
NaN; every output has 64 guard rows behind it and is filled before the call."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_ref as CC  # noqa: E402
import cross_match_ref as CR  # noqa: E402
import embed_sim_ref as ER  # noqa: E402
import pair_scores_ref as PR  # noqa: E402
import pair_select_ref as SR  # noqa: E402
import test_hip_embed_sim as ES  # noqa: E402  (_unit: mgv_row_unit on a strided operand)
import test_hip_pair_scores as TP  # noqa: E402  (Out, the operand slices and the launcher helpers of the pair-score tests)

pytestmark = pytest.mark.gpu

F64, F32, I32, I64 = torch.float64, torch.float32, torch.int32, torch.int64
HS = (16, 32, 64, 128)
TABLES = sorted(CR.PEERS)
NAN, INF = TP.NAN, float('inf')
MGV_EINVAL, MGV_EUNSUPPORTED = -1, -2
Out, _dev, _ptr, _rc, _call, _bits, _slice = TP.Out, TP._dev, TP._ptr, TP._rc, TP._call, TP._bits, TP._slice
GP = CR.graph_ptr_of(CR.GRAPH_SIZES).tolist()
G, N = len(CR.GRAPH_SIZES), GP[-1]


@functools.lru_cache(maxsize=None)
def _rows(H):
    """The case and the device's own unit rows of it, on the host."""
    c = CR.match_case(H)
    y = ES._unit(_dev(), torch.from_numpy(c['x']), want_norm=False)[0].v.cpu().contiguous()
    return c, y


@functools.lru_cache(maxsize=None)
def _scores(H, table):
    """float32 [N, N]: mgv_pair_scores_at(y, y, sigmoid = 0) at every (row, candidate) pair of the table, NaN elsewhere."""
    dev = _dev()
    _, y = _rows(H)
    u, v = np.nonzero(CR.candidate_mask(GP, CR.PEERS[table]))
    src, dst = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
    yv, ldy = _slice(y, dev)
    out = Out(u.size, 1, dev)
    _call('mgv_pair_scores_at', H, u.size, _ptr(yv), ldy, _ptr(yv), ldy, _ptr(src), _ptr(dst), 0, _ptr(out.v))
    assert out.intact()
    s = np.full((N, N), np.nan, dtype=np.float32)
    s[u, v] = out.v.flatten().cpu().numpy()
    return s


def _tables(dev, peer, gp=GP):
    return torch.tensor(gp, dtype=I32, device=dev), torch.tensor(list(peer), dtype=I32, device=dev)


def _topk(dev, y, peer, k, thr, gp=GP):
    n, H = y.shape
    yv, ldy = _slice(y, dev)
    gpd, prd = _tables(dev, peer, gp)
    idx, score, na = Out(n, k, dev, dtype=I32), Out(n, k, dev), Out(n, 1, dev, dtype=I32)
    _call('mgv_cross_topk', H, n, _ptr(yv), ldy, _ptr(gpd), len(gp) - 1, _ptr(prd), k, float(thr), _ptr(idx.v), _ptr(score.v), _ptr(na.v))
    return idx, score, na


class CrossRun:
    """One count / scan / fill through the raw ABI on a strided operand; every output an Out of the test's own."""

    def __init__(self, dev, y, peer, thr, with_score=True, row_ptr=None, cap=None, slots=None, gp=GP):
        n, H = y.shape
        self.yv, ldy = _slice(y, dev)
        self.gpd, self.prd = _tables(dev, peer, gp)
        self.args = (H, n, _ptr(self.yv), ldy, _ptr(self.gpd), len(gp) - 1, _ptr(self.prd), float(thr))
        self.n_sel = Out(n, 1, dev, dtype=I32)
        _call('mgv_cross_select_count', *self.args, _ptr(self.n_sel.v))
        self.true_ptr = torch.zeros(n + 1, dtype=I64, device=dev)
        self.true_ptr[1:] = torch.cumsum(self.n_sel.v.flatten().to(I64), 0)
        self.total = int(self.true_ptr[-1])
        self.row_ptr = self.true_ptr if row_ptr is None else row_ptr.to(device=dev, dtype=I64).contiguous()
        self.cap = self.total if cap is None else cap
        slots = self.total if slots is None else slots
        self.col, self.score = Out(slots, 1, dev, dtype=I32), (Out(slots, 1, dev) if with_score else None)
        self.rc = self.fill()

    def fill(self):
        return _rc('mgv_cross_select_fill', *self.args, _ptr(self.row_ptr), self.cap, _ptr(self.col.v),
                   None if self.score is None else _ptr(self.score.v))

    def intact(self):
        return self.n_sel.intact() and self.col.intact() and (self.score is None or self.score.intact())

    def lists(self):
        k = self.total
        return self.row_ptr.cpu(), self.col.v.flatten()[:k].cpu(), None if self.score is None else self.score.v.flatten()[:k].cpu()


def _np_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize('table', TABLES)
@pytest.mark.parametrize('H', HS)
def test_topk_equals_the_restatement_on_the_scores_of_pair_scores_at(H, table):
    dev = _dev()
    peer = CR.PEERS[table]
    c, y = _rows(H)
    s = _scores(H, table)
    lo, hi = CR.row_ranges(GP, peer)
    none = torch.from_numpy(lo == hi)
    assert bool(none.any()) == (table == 'many_to_one')      # there graph 3 names nobody; the involution's -1 is the empty graph's
    bad = []
    for k in CR.KS:
        for thr in CR.THRESHOLDS:
            tag = 'H=%d %s k=%d thr=%g' % (H, table, k, thr)
            idx, score, na = _topk(dev, y, peer, k, thr)
            w_idx, w_top, w_above = CR.topk_ref(s, GP, peer, k, thr)
            got_idx, got_top, got_above = idx.v.cpu(), score.v.cpu(), na.v.cpu().flatten()
            if not torch.equal(got_idx, torch.from_numpy(w_idx)):
                d = torch.nonzero((got_idx != torch.from_numpy(w_idx)).any(1)).flatten()
                bad.append('%s: idx differs in %d rows, first %d: %s, expected %s' % (tag, d.numel(), int(d[0]), got_idx[d[0]].tolist(),
                                                                                   w_idx[int(d[0])].tolist()))
            if not np.array_equal(_bits(got_top).numpy(), _np_bits(w_top)):
                bad.append('%s: a reported cosine is not the bits of mgv_pair_scores_at' % tag)
            if not torch.equal(got_above, torch.from_numpy(w_above)):
                bad.append('%s: n_above differs' % tag)
            if not (idx.intact() and score.intact() and na.intact()):
                bad.append('%s: guard rows changed' % tag)
            # rows without candidates (peer -1, a peer without rows): padding only
            if not (bool((got_idx[none] == -1).all()) and bool((got_top[none] == -INF).all()) and bool((got_above[none] == 0).all())):
                bad.append('%s: a row without candidates reports something' % tag)
            again = _topk(dev, y, peer, k, thr)
            if not all(torch.equal(_bits(a.parent) if a.parent.dtype == F32 else a.parent, _bits(b.parent) if b.parent.dtype == F32 else b.parent)
                       for a, b in zip(again, (idx, score, na))):
                bad.append('%s: a second call gives other bytes' % tag)
    # planted: the four equal unit rows of the peer come first, in id order, for the copy and for its multiple
    info = c['info']
    idx = _topk(dev, y, peer, 8, 0.999)[0].v.cpu()
    for u in (info['copy'], info['times4']):
        if idx[u, :4].tolist() != sorted(info['trio'] + (info['half'],)):
            bad.append('%s row %d: the exact ties are not listed in id order: %s' % (table, u, idx[u].tolist()))
    if bool((idx == info['nan']).any()):
        bad.append('%s: the NaN row is somebody\'s candidate' % table)
    print('XM topk H=%d %s | k %s x thresholds %s exact against pair_scores_at | %d findings' % (H, table, CR.KS, CR.THRESHOLDS, len(bad)))
    assert not bad, bad[:10]


@pytest.mark.parametrize('table', TABLES)
@pytest.mark.parametrize('H', HS)
def test_lists_equal_the_scores_of_pair_scores_at_above_the_threshold(H, table):
    dev = _dev()
    peer = CR.PEERS[table]
    _, y = _rows(H)
    s = _scores(H, table)
    bad, totals = [], []
    for thr in CR.THRESHOLDS:
        tag = 'H=%d %s thr=%g' % (H, table, thr)
        run = CrossRun(dev, y, peer, thr)
        assert run.rc == 0
        row_ptr, col, score = run.lists()
        w_ptr, w_col, w_val = CR.select_ref(s, GP, peer, thr)
        totals.append(run.total)
        if not torch.equal(row_ptr, torch.from_numpy(w_ptr)):
            bad.append('%s: row_ptr differs (total %d, expected %d)' % (tag, run.total, int(w_ptr[-1])))
            continue
        if not torch.equal(col.to(I64), torch.from_numpy(w_col)):
            bad.append('%s: the listed ids differ' % tag)
        if not np.array_equal(_bits(score).numpy(), _np_bits(w_val)):
            bad.append('%s: a listed cosine is not the bits of mgv_pair_scores_at' % tag)
        if not run.intact():
            bad.append('%s: guard rows changed' % tag)
        # n_above of the top-k entry is the length of the row's list
        na = _topk(dev, y, peer, 1, thr)[2].v.cpu().flatten().to(I64)
        if not torch.equal(na, row_ptr[1:] - row_ptr[:-1]):
            bad.append('%s: n_above is not row_ptr[u + 1] - row_ptr[u]' % tag)
        if thr == -2.0:
            lo, hi = CR.row_ranges(GP, peer)
            nan_cols = np.isnan(s) & CR.candidate_mask(GP, peer)
            if not np.array_equal(np.diff(w_ptr), (hi - lo) - nan_cols.sum(1)):
                bad.append('%s: below every cosine a row does not list all its candidates' % tag)
        first = (run.col.parent.clone(), _bits(run.score.parent))
        run.col.parent.fill_(-77)
        run.score.parent.fill_(NAN)
        assert run.fill() == 0
        if not (torch.equal(first[0], run.col.parent) and torch.equal(first[1], _bits(run.score.parent))):
            bad.append('%s: a second fill gives other bytes' % tag)
        if not torch.equal(CrossRun(dev, y, peer, thr, with_score=False).col.parent, run.col.parent):
            bad.append('%s: col changes when no scores are asked for' % tag)
    print('XM lists H=%d %s | pairs per threshold %s | %d findings' % (H, table, totals, len(bad)))
    assert not bad, bad[:10]


@pytest.mark.parametrize('H', HS)
def test_topk_and_lists_against_float64(H, monkeypatch):
    """No exclusions: pair_scores_ref.check_topk with the cross mask in place of the own-graph mask, pair_select_ref.check_band with
    everything that is no candidate at -inf; cos and bound (2H + 6) 2^-24 S from embed_sim_ref.cos_ref of the case's float32 rows."""
    dev = _dev()
    c, y = _rows(H)
    cr = ER.cos_ref(torch.from_numpy(c['x']))
    r = {'raw': cr['cos'], 'raw_bound': cr['bound']}
    bad, band = [], 0
    for table in TABLES:
        peer = CR.PEERS[table]
        mask = torch.from_numpy(CR.candidate_mask(GP, peer))
        monkeypatch.setattr(PR, 'candidate_mask', lambda n, gp, skip, m=mask: m.clone())
        keep = mask & ~torch.isnan(cr['cos'])
        ref = torch.where(keep, cr['cos'], torch.full_like(cr['cos'], -INF))
        bound = torch.where(keep, cr['bound'], torch.zeros_like(cr['bound']))
        for k in CR.KS:
            idx, score, _ = _topk(dev, y, peer, k, 0.999)
            bad += ['%s k=%d: %s' % (table, k, b) for b in PR.check_topk(idx.v.cpu(), score.v.cpu(), r, GP, k, False, False)]
        for thr in CR.THRESHOLDS:
            near = ER.band_count(cr['cos'], cr['bound'], thr, keep)
            band = max(band, near)
            assert near <= ER.band_limit(keep), (table, thr, near)
            run = CrossRun(dev, y, peer, thr, with_score=False)
            row_ptr, col, _ = run.lists()
            bad += ['%s thr=%g: %s' % (table, thr, b) for b in SR.check_band(row_ptr, col, ref, bound, None, thr, False)]
    print('XM float64 H=%d | top-k and lists on their side of (2H + 6) 2^-24 S | at most %d pairs inside their bound of a threshold | %d '
          'findings' % (H, band, len(bad)))
    assert not bad, bad[:10]


@pytest.mark.parametrize('H', HS)
def test_a_peer_table_that_names_each_graph_itself_is_the_own_graph_walk(H):
    """ops.cross_topk / cross_pairs with peer[g] = g against ops.pair_topk / pair_select(y, y, skip_self=False) on the same unit rows."""
    dev = _dev()
    from deepgate import ops
    c, _ = _rows(H)
    xd = torch.from_numpy(c['x']).to(dev)
    own = list(range(G))
    y = ops.row_unit(xd)
    for thr in (0.999, 0.25):
        for k in CR.KS:
            a = ops.cross_topk(xd, k, GP, own, threshold=thr)
            b = ops.pair_topk(y, y, k, graph_ptr=GP, sigmoid=False, threshold=thr, skip_self=False)
            assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1])) and torch.equal(a[2], b[2]), (thr, k)
        pi, row_ptr, score = ops.cross_pairs(xd, GP, own, threshold=thr, with_scores=True)
        w_ptr, w_col, w_score = ops.pair_select(y, y, graph_ptr=GP, sigmoid=False, threshold=thr, skip_self=False, with_scores=True)
        assert torch.equal(row_ptr, w_ptr) and torch.equal(pi[1], w_col.to(I64)) and torch.equal(_bits(score), _bits(w_score))
        assert pi.dtype == I64 and row_ptr.dtype == I64 and ops.cross_pairs(xd, GP, own, threshold=thr)[2] is None


# ------------------------------------------------------------------------------------------------ memory safety and refusals
def test_the_fill_stays_inside_the_slots_it_is_given():
    dev = _dev()
    peer = CR.PEERS['involution']
    _, y = _rows(64)
    thr = 0.1
    full = CrossRun(dev, y, peer, thr)
    true_ptr, want_col, want_score = full.lists()
    n = true_ptr[1:] - true_ptr[:-1]
    total = full.total
    u = int(torch.argmax(n[:-1] * (n[1:] > 0)))             # the longest list that has a non-empty successor
    short = 5
    assert int(n[u]) > 16 + short
    row_ptr = true_ptr.clone()
    row_ptr[u + 1:] -= int(n[u]) - short
    run = CrossRun(dev, y, peer, thr, row_ptr=row_ptr, slots=total)
    keep = torch.ones(total, dtype=torch.bool)
    keep[int(true_ptr[u]) + short:int(true_ptr[u + 1])] = False
    got_col, got_score = run.col.v.flatten().cpu(), run.score.v.flatten().cpu()
    used = int(keep.sum())
    assert run.rc == 0 and torch.equal(got_col[:used], want_col[keep]) and torch.equal(_bits(got_score[:used]), _bits(want_score[keep]))
    assert bool((got_col[used:] == -77).all()) and bool(torch.isnan(got_score[used:]).all()) and run.intact()
    for odd in (torch.zeros_like(true_ptr), true_ptr.flip(0), true_ptr - total - 7, torch.full_like(true_ptr, total + 1000)):
        run = CrossRun(dev, y, peer, thr, row_ptr=odd, slots=total)
        assert run.rc == 0 and run.col.untouched() and run.score.untouched()
    cap = int(true_ptr[u]) + 3                              # ends inside row u's list
    run = CrossRun(dev, y, peer, thr, cap=cap, slots=total)
    got_col, got_score = run.col.v.flatten().cpu(), run.score.v.flatten().cpu()
    assert run.rc == 0 and torch.equal(got_col[:cap], want_col[:cap]) and torch.equal(_bits(got_score[:cap]), _bits(want_score[:cap]))
    assert bool((got_col[cap:] == -77).all()) and bool(torch.isnan(got_score[cap:]).all()) and run.intact()
    run = CrossRun(dev, y, peer, thr, cap=0, slots=total)
    assert run.rc == 0 and run.col.untouched() and run.score.untouched()
    run = CrossRun(dev, y, peer, thr, cap=-1, slots=total)  # a cap below zero is refused by return code
    assert run.rc == MGV_EINVAL and run.col.untouched() and run.score.untouched()
    print('XM fill bounds | row %d of %d pairs cut to %d, odd row_ptr, cap %d of %d, cap -1 refused | ok' % (u, int(n[u]), short, cap, total))


def test_refusals_are_return_codes_before_anything_is_launched():
    dev = _dev()
    n = 40
    y48, y = torch.randn(n, 48, device=dev), torch.randn(n, 16, device=dev)
    ptr0 = torch.arange(0, 4 * (n + 1), 4, dtype=I64, device=dev)
    gp, peer = [0, 10, n], [1, 0]

    def all3(H, nn, x, ld, gp, peer, k=4, cap=None, base=None):
        """(top-k's code, count's code, fill's code, every output untouched)"""
        idx, sc, na = Out(n, 32, dev, dtype=I32), Out(n, 32, dev), Out(n, 1, dev, dtype=I32)
        n_sel, col, score = Out(n, 1, dev, dtype=I32), Out(4 * n, 1, dev, dtype=I32), Out(4 * n, 1, dev)
        gpd = None if gp is None else torch.tensor(gp, dtype=I32, device=dev)
        prd = None if peer is None else torch.tensor(peer, dtype=I32, device=dev)
        Gn = 0 if gp is None else len(gp) - 1
        common = (H, nn, _ptr(x) if base is None else base, ld, _ptr(gpd), Gn, _ptr(prd))
        a = _rc('mgv_cross_topk', *common, k, -2.0, _ptr(idx.v), _ptr(sc.v), _ptr(na.v))
        b = _rc('mgv_cross_select_count', *common, -2.0, _ptr(n_sel.v))
        c = _rc('mgv_cross_select_fill', *common, -2.0, _ptr(ptr0), 4 * n if cap is None else cap, _ptr(col.v), _ptr(score.v))
        return a, b, c, all(o.untouched() for o in (idx, sc, na, n_sel, col, score))
    U, E = MGV_EUNSUPPORTED, MGV_EINVAL
    assert all3(48, n, y48, 48, gp, peer) == (U, U, U, True)                      # bad H
    assert all3(0, n, y, 16, gp, peer) == (U, U, U, True)
    assert all3(16, n, y, 16, gp, [1, 2]) == (E, E, E, True)                      # peer out of range: G
    assert all3(16, n, y, 16, gp, [-2, 0]) == (E, E, E, True)                     # below -1
    assert all3(16, n, y, 16, None, peer) == (E, E, E, True)                      # a null graph_ptr with a peer
    assert all3(16, n, y, 16, gp, None) == (E, E, E, True)
    assert all3(16, n, y, 16, gp, peer, k=0) == (E, 0, 0, False)                  # k outside 1 .. 32 (the lists have no k and ran)
    assert all3(16, n, y, 16, gp, peer, k=33)[0] == E
    assert all3(16, n, y, 12, gp, peer) == (E, E, E, True)                        # row stride below H
    assert all3(16, n, y, 18, gp, peer) == (E, E, E, True)                        # row stride no multiple of 4
    assert all3(16, n, y, 16, gp, peer, base=TP._hip().ptr(y.view(-1)[1:])) == (E, E, E, True)
    assert all3(16, n, y, 16, [0, 10, n - 1], peer) == (E, E, E, True)            # graph_ptr does not end at N
    assert all3(16, n, y, 16, [1, 10, n], peer) == (E, E, E, True)
    assert all3(16, -1, y, 16, gp, peer) == (E, E, E, True)
    assert all3(16, n, y, 16, gp, peer, cap=-1) == (0, 0, E, False)
    assert all3(16, n, y, 16, gp, peer) == (0, 0, 0, False)
    assert all3(16, n, y, 16, gp, [-1, -1])[:3] == (0, 0, 0)                      # nobody has candidates: it runs and reports nothing
    # N = 0: nothing is launched, nothing is written
    empty = torch.full((1, 16), NAN, device=dev)
    assert all3(16, 0, empty, 16, [0, 0, 0], [1, 0]) == (0, 0, 0, True)
    from deepgate import _hip, ops
    with pytest.raises(_hip.HipLibraryError, match='EUNSUPPORTED'):
        ops.cross_topk(y48, 4, gp, peer)
    with pytest.raises(_hip.HipLibraryError, match='EINVAL'):
        ops.cross_pairs(y, [0, 10, n - 1], peer)
    with pytest.raises(ValueError):
        ops.cross_topk(y, 4, gp, [1, 2])
    with pytest.raises(_hip.HipLibraryError, match='graph_ptr'):
        ops.cross_topk(y, 4, None, peer)
    pi, row_ptr, score = ops.cross_pairs(torch.zeros(0, 16, device=dev), [0, 0], [0], with_scores=True)
    assert pi.shape == (2, 0) and pi.dtype == I64 and row_ptr.tolist() == [0] and score.shape == (0,)


def test_cross_pairs_refuses_before_the_fill():
    dev = _dev()
    from deepgate import _hip, ops
    c, _ = _rows(64)
    xd, peer = torch.from_numpy(c['x']).to(dev), CR.PEERS['involution']
    total = ops.cross_pairs(xd, GP, peer, threshold=0.25)[0].shape[1]
    calls = []
    real = _hip.call
    try:
        _hip.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
        with pytest.raises(_hip.HipLibraryError, match=str(total)) as err:
            ops.cross_pairs(xd, GP, peer, threshold=0.25, max_pairs=total - 1)
    finally:
        _hip.call = real
    assert 'mgv_cross_select_count' in calls and 'mgv_cross_select_fill' not in calls and 'max_pairs' in str(err.value)
    assert ops.cross_pairs(xd, GP, peer, threshold=0.25, max_pairs=total)[0].shape[1] == total


# ------------------------------------------------------------------------------------------------ derived operators
@pytest.mark.parametrize('table', TABLES)
def test_cross_mutual_is_its_definition_on_the_top_1_results(table):
    dev = _dev()
    from deepgate import ops
    H, peer = 64, CR.PEERS[table]
    c, _ = _rows(H)
    xd = torch.from_numpy(c['x']).to(dev)
    found = 0
    for thr in (0.999, 0.25, -2.0):
        idx, cos, _ = ops.cross_topk(xd, 1, GP, peer, threshold=thr)
        w_pairs, w_cos = CR.mutual_ref(idx[:, 0].cpu().numpy(), cos[:, 0].cpu().numpy(), GP, peer, thr)
        pi, pc = ops.cross_mutual(xd, GP, peer, threshold=thr)
        assert pi.dtype == I64 and pi.shape[0] == 2 and pi.is_cuda
        assert np.array_equal(pi.cpu().numpy(), w_pairs) and np.array_equal(_bits(pc).numpy(), _np_bits(w_cos)), (table, thr)
        found = max(found, pi.shape[1])
    assert (found > 0) == (table == 'involution')           # the many-to-one table has no graph with peer[peer[g]] = g
    print('XM mutual %s | up to %d reciprocal best matches | ok' % (table, found))


@pytest.mark.parametrize('table', TABLES)
def test_cross_classes_are_the_components_of_both_pair_lists(table):
    dev = _dev()
    from deepgate import ops
    H, peer = 64, CR.PEERS[table]
    c, _ = _rows(H)
    xd = torch.from_numpy(c['x']).to(dev)
    graph_of = np.searchsorted(np.asarray(GP[1:]), np.arange(N), side='right')
    for thr in (0.999, 0.3):
        cross = ops.cross_pairs(xd, GP, peer, threshold=thr)[0].cpu()
        own = ops.sim_pairs(xd, graph_ptr=GP, threshold=thr)[0].cpu()
        want = CC.uf_labels(torch.cat([cross, own], 1), N)
        for min_size in (2, 1):
            label, class_ptr, members = ops.cross_classes(xd, GP, peer, threshold=thr, min_size=min_size)
            assert label.dtype == I32 and class_ptr.dtype == I64 and members.dtype == I32
            assert CC.check_components(label, None, want) == [] and CC.check_table(class_ptr, members, want, min_size) == []
        lab = want.numpy()
        spans = 0
        for root in np.unique(lab):
            gs = sorted(set(graph_of[lab == root].tolist()))
            spans += len(gs) > 1
            if table == 'involution':                       # a class lives in one graph, or in a graph and its peer
                assert len(gs) == 1 or (len(gs) == 2 and peer[gs[0]] == gs[1]), (thr, root, gs)
        assert spans >= 1                                   # the planted copies join their peers' ties
    print('XM classes %s | equal to the union-find of cross_pairs + sim_pairs | ok' % table)


# ------------------------------------------------------------------------------------------------ end to end
def test_a_circuit_finds_its_own_copy_through_the_model():
    dev = _dev()
    import deepgate
    from deepgate import ops, synthetic as syn
    H = 64
    torch.manual_seed(0)
    enc = deepgate.digae_layer.DirectMultiGCNEncoder(dim_feature=6, dim_hidden=H, s_rounds=1, t_rounds=1, layernorm=True)
    model = deepgate.dg_ae_model_aig.Model(struct_encoder=enc, dim_hidden=H).to(dev).eval()
    g, other = syn.make_graph('aig', 300, 12, 50, n_inputs=24), syn.make_graph('aig', 200, 10, 51, n_inputs=20)
    batch = deepgate.CircuitBatch.from_arrays(syn.collate([g, dict(g), other]), device=dev)
    with torch.no_grad():
        _, hf = model(batch)
    gp, peer = batch.graph_ptr.tolist(), [1, 0, -1]
    n = gp[1]
    assert gp[2] == 2 * n and hf.shape[0] == gp[3]
    thr = 0.999
    idx, cos, n_above = model.match_gates(hf, 4, batch.graph_ptr, peer, threshold=thr)
    want = ops.cross_topk(hf, 4, gp, peer, threshold=thr)
    assert torch.equal(idx, want[0]) and torch.equal(_bits(cos), _bits(want[1])) and torch.equal(n_above, want[2])
    live = torch.nonzero(hf[:n].abs().sum(1) != 0).flatten()
    assert 0 < live.numel() < n                              # the primary inputs have hf = 0
    mine = ops.sim_at(hf, torch.stack([live, live + n]))      # the cosine of a gate with its own copy
    assert bool((cos[live, 0] >= mine).all()) and bool((idx[live, 0] >= n).all()) and bool((idx[live, 0] < 2 * n).all())
    assert bool((mine > thr).all())                          # the copy is the same circuit: the same function
    pi, row_ptr, pc = model.cross_equivalence_candidates(hf, batch.graph_ptr, peer, threshold=thr, with_scores=True)
    listed = set(zip(pi[0].tolist(), pi[1].tolist()))
    assert all((int(i), int(i) + n) in listed for i, m in zip(live.tolist(), mine.tolist()) if m > thr)
    assert torch.equal(n_above.to(I64), row_ptr[1:] - row_ptr[:-1]) and bool((pc > thr).all())
    # the third graph has no peer: nothing
    assert bool((idx[gp[2]:] == -1).all()) and bool((cos[gp[2]:] == -INF).all()) and int(n_above[gp[2]:].sum()) == 0
    assert int(row_ptr[-1]) == int(row_ptr[gp[2]]) and not bool((pi >= gp[2]).any())
    mp, none, mc = model.cross_equivalence_candidates(hf, batch.graph_ptr, peer, threshold=thr, mutual=True, with_scores=True)
    assert none is None and bool((mp[0] < n).all()) and bool((mp[1] >= n).all()) and bool((mp[1] < 2 * n).all()) and mc.shape == (mp.shape[1],)
    assert mp.shape[1] > 0 and set(zip(mp[0].tolist(), mp[1].tolist())) <= listed
    label, class_ptr, members = model.cross_equivalence_classes(hf, batch.graph_ptr, peer, threshold=thr)
    assert bool((label[live + n] == label[live]).all())      # a gate and its copy share a class
    assert bool((label[gp[2]:] >= gp[2]).all())              # the third circuit's classes stay its own
    print('XM model | %d live gates find their copies, %d pairs above %g, %d reciprocal | ok' % (live.numel(), pi.shape[1], thr, mp.shape[1]))


def test_feature_extract_match_and_cross_equivalences(tmp_path):
    """examples/feature_extract.py --match K --cross_equivalences THR: name/match_idx and name/match_cos with ids local to the PEER graph,
    name/xeq_pairs (row 0 local to the graph, row 1 local to its peer) and name/xeq_cos, beside the embeddings."""
    _dev()
    import importlib

    from conftest import PKG_PARENT
    sys.path.insert(0, os.path.join(PKG_PARENT, 'examples'))
    fe = importlib.import_module('feature_extract')
    out = tmp_path / 'emb.npz'
    fe.main(['--type', 'aig', '--synthetic', '4', '--rounds', '1', '--batch_size', '3', '--match', '4', '--cross_equivalences', '0.999',
             '--out', str(out)])
    emb = np.load(out)
    assert sorted(emb.files) == sorted('graph%d/%s' % (i, k) for i in range(4) for k in ('hs', 'hf', 'match_idx', 'match_cos', 'xeq_pairs',
                                                                                       'xeq_cos'))
    peer = {0: 1, 1: 0, 2: None, 3: None}                    # batches of 3 and 1: graph 2 is an odd last graph, graph 3 is alone
    for i in range(4):
        n = emb['graph%d/hf' % i].shape[0]
        idx, cos = emb['graph%d/match_idx' % i], emb['graph%d/match_cos' % i]
        eq, ec = emb['graph%d/xeq_pairs' % i], emb['graph%d/xeq_cos' % i]
        assert idx.shape == (n, 4) and cos.shape == (n, 4) and idx.dtype == np.int32
        assert eq.ndim == 2 and eq.shape[0] == 2 and eq.dtype == np.int32 and ec.shape == (eq.shape[1],)
        if peer[i] is None:
            assert (idx == -1).all() and np.isneginf(cos).all() and eq.shape[1] == 0
            continue
        m = emb['graph%d/hf' % peer[i]].shape[0]
        assert idx.min() >= -1 and idx.max() < m and (np.diff(cos, axis=1) <= 0).all()
        if eq.shape[1]:
            assert eq[0].min() >= 0 and eq[0].max() < n and eq[1].min() >= 0 and eq[1].max() < m and (ec > 0.999).all()
            key = eq[0].astype(np.int64) * m + eq[1]
            assert (np.diff(key) > 0).all()                  # per gate, ascending, no pair twice
            back = emb['graph%d/xeq_pairs' % peer[i]]
            assert set(zip(eq[0].tolist(), eq[1].tolist())) == set(zip(back[1].tolist(), back[0].tolist()))     # once from each side
